"""GDN / IGDN (third-party compressai definition) stated in float64 on plain dense [P][C]
arrays, and the cases and inputs of tests/test_gpu_gdn_fp32.py.  Imports no product code.

    forward   norm_i = beta_e[i] + sum_j gamma_e[i][j] x_j^2        y = x norm^-1/2 (+ res)     (inverse: norm^+1/2)
    backward  t = dL/dnorm = -1/2 g x norm^-3/2                     (inverse: +1/2 g x norm^-1/2)
              dx_i = g_i f(norm_i) + 2 x_i sum_j t_j gamma_e[j][i]  f = norm^-1/2 (inverse: norm^+1/2)

Every function takes numpy arrays or torch tensors, computes in float64 with torch ops (so torch.autograd can
differentiate `fwd`) and returns float64 torch tensors.  tests/test_gdn_ref64.py pins these functions to the oracle and
to autograd, and proves on the CPU that the exact-input cases do not depend on the order of any sum.
"""
from __future__ import annotations

import numpy as np
import torch

BLOCK = 64                      # pixels per workgroup of the dedicated kernels (lic_gdn_bwd_partial_rows)
WIDTHS = (64, 128, 192)         # lic_gdn_supported
SIZES = (1, 63, 64, 65, 357)    # below one tile, one tile exactly, one pixel more, several ragged tiles
BIG = 65_537                    # 1025 tiles: more than one round of workgroups on 256 CUs at two or three per CU
# (C, inverse, P): every width and direction at every small size; the largest for C = 192 and one other width
CASES = [(C, inv, P) for C in WIDTHS for inv in (0, 1) for P in SIZES] + [(C, inv, BIG) for C in (192, 64) for inv in (0, 1)]
# the cases whose backward reads the forward kernel's own norm instead of a generated one
OWN_NORM_CASES = [(64, 0, 357), (128, 1, 357), (192, 0, 65), (192, 1, 357)]
# the bands (tests/test_gpu_parity.py `close`; tests/test_gpu_latent_ops.py test_gdn_dnorm_vs_float64)
BAND = (1e-4, 1e-6)             # norm, y, t: |err| <= 1e-6 + 1e-4 |ref|
DX_RTOL = 1e-4                  # dx: |err| <= 1e-4 mag, mag = sum of the magnitudes of dx's terms (`bwd`)


def case_id(c):
    return "C%d-%s-P%d" % (c[0], "igdn" if c[1] else "gdn", c[2])


def f64(a):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double() if not a.requires_grad else a.double()
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ---------------------------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------------------------
def fwd(x, beta_e, gamma_e, inverse, res=None):
    """(y, norm) of x [P][C], beta_e [C], gamma_e [C][C] ([norm index][x index])"""
    x, beta_e, gamma_e, res = f64(x), f64(beta_e), f64(gamma_e), f64(res)
    norm = beta_e[None, :] + (x * x) @ gamma_e.t()
    y = x * (norm.sqrt() if inverse else norm.rsqrt())
    if res is not None:
        y = y + res
    return y, norm


def bwd(g, x, norm, gamma_e, inverse):
    """(t, dx, mag) from the output gradient g, the saved input x and the saved pool `norm`; mag_i =
    |g_i f(norm_i)| + 2 |x_i| sum_j |t_j| gamma_e[j][i] is the sum of the magnitudes of dx_i's terms (gamma_e >= 0):
    what a rounding error of dx is measured against"""
    g, x, norm, gamma_e = f64(g), f64(x), f64(norm), f64(gamma_e)
    f = norm.sqrt() if inverse else norm.rsqrt()
    t = 0.5 * (g * x) * norm.rsqrt() if inverse else -0.5 * (g * x) * norm.rsqrt() / norm
    u = g * f
    dx = u + 2.0 * x * (t @ gamma_e)
    mag = u.abs() + 2.0 * x.abs() * (t.abs() @ gamma_e)
    return t, dx, mag


def block_colsums(a, block=BLOCK):
    """[ceil(P / block)][C]: row b is the column sum of pixels block * b ... block * b + block - 1"""
    a = f64(a)
    P, C = a.shape
    rows = (P + block - 1) // block
    pad = torch.zeros((rows * block, C), dtype=torch.float64)
    pad[:P] = a
    return pad.reshape(rows, block, C).sum(1)


# ---------------------------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------------------------
def band_ratio(got, ref, rtol, atol):
    """worst |got - ref| / (atol + rtol |ref|) over EVERY element (a NaN counts as infinite)"""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = (got - ref).abs() / (atol + rtol * ref.abs())
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def mag_ratio(got, ref, mag, rtol=DX_RTOL):
    """worst |got - ref| / (rtol mag) over every element; an element whose magnitude sum is 0 must be exact"""
    got, ref, mag = f64(got), f64(ref), f64(mag)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    err = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    r = torch.where(err == 0, torch.zeros_like(err), err / (rtol * mag))   # (0 / 0 -> 0, e / 0 -> inf)
    return float(r.max())


def canon_bits(a):
    """the int32 bit patterns of `a` as fp32, -0 folded into +0 (the one pair of equal fp32 values with two patterns:
    an exact sum of zeros has either sign depending on where the sum starts)"""
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    a32 = a.to(torch.float32)
    assert torch.equal(a32.double(), a.double()) or bool(torch.isnan(a32).any()), "not representable in fp32"
    return (a32 + 0.0).contiguous().view(torch.int32)


def same_bits(got, ref):
    """True when the fp32 tensor `got` and the (fp32-representable) reference hold the same values bit for bit"""
    got, ref = canon_bits(got), canon_bits(ref)
    return got.shape == ref.shape and bool(torch.equal(got, ref))


# ---------------------------------------------------------------------------------------------
# inputs (fp32 torch tensors on the CPU; the float64 references widen them exactly)
# ---------------------------------------------------------------------------------------------
def _gen(C, inverse, P, salt):
    return torch.Generator().manual_seed(((C * 2 + inverse) * 100_003 + P) * 7 + salt)


def zero_pixels(P):
    """the pixels whose x is all zero in the banded inputs"""
    return [] if P < 8 else sorted({3, P // 2, P - 1})


def banded_inputs(C, inverse, P):
    """x, g: normal, times 10^U(-2, 2) per pixel (four decades of pixel magnitudes), a few all-zero pixels in x;
    gamma_e: asymmetric, non-negative, about 0.05 |N|; beta_e in [1e-6, 1]; res: normal; norm_b in [0.25, 3.25]: the saved
    pool the backward cases read"""
    g_ = _gen(C, inverse, P, 1)
    x = torch.randn(P, C, generator=g_) * 10.0 ** (torch.rand(P, 1, generator=g_) * 4 - 2)
    x[zero_pixels(P)] = 0.0
    g = torch.randn(P, C, generator=g_) * 10.0 ** (torch.rand(P, 1, generator=g_) * 4 - 2)
    gamma_e = 0.05 * torch.randn(C, C, generator=g_).abs()
    beta_e = 1e-6 + (1.0 - 1e-6) * torch.rand(C, generator=g_)
    beta_e[0], beta_e[C - 1] = 1e-6, 1.0
    res = torch.randn(P, C, generator=g_)
    norm_b = 0.25 + 3.0 * torch.rand(P, C, generator=g_)
    return dict(x=x, g=g, gamma_e=gamma_e, beta_e=beta_e, res=res, norm=norm_b)


def _choice(values, shape, g_):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(len(values), shape, generator=g_)]


def exact_fwd_inputs(C, inverse, P):
    """x in {-3..3}, gamma_e in {0, 1/4, .., 1}, beta_e in {1, 2, 3, 4}: every product and every partial sum of the pool is
    a multiple of 1/4 below 2^11, so fp32 forms norm without rounding in any order"""
    g_ = _gen(C, inverse, P, 2)
    return dict(x=_choice([-3, -2, -1, 0, 1, 2, 3], (P, C), g_), gamma_e=_choice([0, 0.25, 0.5, 0.75, 1], (C, C), g_),
                beta_e=_choice([1, 2, 3, 4], (C,), g_))


def exact_bwd_inputs(C, inverse, P):
    """g, x in {-2..2}, gamma_e in {0, 1/2, 1}, norm in {1, 4}: with norm^-1/2 in {1, 1/2} t is a multiple of 1/16 of
    magnitude <= 2, the pool a multiple of 1/32 below 2^9, dx a multiple of 1/16 below 2^11 and a 64-pixel column sum of
    either stays below 2^21 of its unit: fp32 forms all of them without rounding in any order"""
    g_ = _gen(C, inverse, P, 3)
    return dict(g=_choice([-2, -1, 0, 1, 2], (P, C), g_), x=_choice([-2, -1, 0, 1, 2], (P, C), g_),
                gamma_e=_choice([0, 0.5, 1], (C, C), g_), norm=_choice([1, 4], (P, C), g_))


# ---------------------------------------------------------------------------------------------
# the same formulas in fp32, one term at a time in a chosen order (the CPU proof of order independence)
# ---------------------------------------------------------------------------------------------
def fp32_ordered(kind, inp, inverse, descending):
    """the outputs of the exact case `kind` ("fwd": norm; "bwd": t, dx, block sums of t and of dx) evaluated with fp32
    numpy arithmetic only, every sum taken one term at a time in ascending or descending index order"""
    f = {k: v.numpy().astype(np.float32) for k, v in inp.items()}
    C = f["gamma_e"].shape[0]
    order = range(C - 1, -1, -1) if descending else range(C)
    if kind == "fwd":
        x2 = f["x"] * f["x"]
        norm = np.broadcast_to(f["beta_e"][None, :], x2.shape).copy()
        for j in order:
            norm = norm + x2[:, j:j + 1] * f["gamma_e"][None, :, j]
        assert norm.dtype == np.float32
        return dict(norm=norm)
    g, x, n = f["g"], f["x"], f["norm"]
    rs = np.float32(1.0) / np.sqrt(n)
    half = np.float32(0.5)
    t = half * (g * x) * rs if inverse else -half * (g * x) * rs * (rs * rs)
    u = g * (np.sqrt(n) if inverse else rs)
    s = np.zeros_like(t)
    for j in order:
        s = s + t[:, j:j + 1] * f["gamma_e"][j][None, :]
    dx = u + np.float32(2.0) * x * s
    out = dict(t=t, dx=dx)
    P = t.shape[0]
    rows = (P + BLOCK - 1) // BLOCK
    for name, a in (("cs_t", t), ("cs_dx", dx)):
        cs = np.zeros((rows, C), np.float32)
        for b in range(rows):
            blk = a[b * BLOCK:(b + 1) * BLOCK]
            for r in (range(len(blk) - 1, -1, -1) if descending else range(len(blk))):
                cs[b] = cs[b] + blk[r]
        out[name] = cs
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def exact_reference(kind, inp, inverse):
    """the float64 outputs of the exact case `kind`, keyed as fp32_ordered keys them"""
    if kind == "fwd":
        return dict(norm=fwd(inp["x"], inp["beta_e"], inp["gamma_e"], inverse)[1])
    t, dx, _ = bwd(inp["g"], inp["x"], inp["norm"], inp["gamma_e"], inverse)
    return dict(t=t, dx=dx, cs_t=block_colsums(t), cs_dx=block_colsums(dx))
