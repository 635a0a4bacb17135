"""The bf16 latent-side convolutions (lic_igemm_bf16: masked context conv, hyper encoder / decoder, entropy-parameter
MLP) stated in float64, and the layer table, cases, inputs and bands of tests/test_gpu_latent_bf16.py.  Plain torch on
the CPU; no GPU and no product code.  tests/test_conv_bf16_ref.py checks this file.

THE BANDS.  Operands are bf16-exact, so every product is exact in fp32 and the only error of an fp32 output is the
summation's.  An fp32 output is held, element by element, to

    |dev - y64| <= A * S            S = the same convolution of |x| with |w * mask|, plus |b|

(the sum of the magnitudes of the terms).  A is MEASURED against this float64 reference, because neither the bf16 MFMA's
in-instruction summation nor the kernel's chunk order is documented to the bit: the worst err / S over every unsplit
launch of the GPU module, times 4 (inputs not tried), rounded up to a power of two.

    measured worst err / S on the MI355X:   1.934e-07  (A_MEASURED; unsplit: the data gradient of ep1 at M = 192, 512 pixels,
                                            640 products per element; K-split launches: 8.32e-08)
    A = 2^-20 = 9.54e-07                    (A_BAND; 4 x 1.934e-07 = 7.7e-07, rounded up to a power of two)

That is the order of magnitude the f32 MFMA is known for (1e-7 to 3.5e-7 of S) and two orders below n * 2^-23.

Two conditions on A are not measurements (test_conv_bf16_ref.py asserts them for every case):
    A <= n * 2^-23    the worst case of ANY fp32 summation order with at most one ulp per add: a measurement above it is
                      a finding about the kernel, not a reason to widen;
    A * n <= 1 / 8    so that one missing average-sized product (S / n) is at least eight bands wide.
n = live taps times Cin, the number of products summed per (interior) element.

A bf16 output is bit for bit rne_bf16 of the fp32 output of the same forced variant on the same operands (both stores
are a cast of the fp32 value).  The fused LeakyReLU is 1-Lipschitz: leaky_ref(y64) with the same band A * S.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from gdn_bf16_ref import rne_bf16  # noqa: F401  (the one statement of round-to-nearest-even to bf16)

A_MEASURED = 1.934e-07    # worst err / S of an unsplit launch (the GPU module's ERRS lines)
A_BAND = 2.0 ** -20       # the band constant of every fp32 output
SLOPE = 0.01
SLOPE32 = float(np.float32(SLOPE))     # the kernels take the slope as an fp32 argument

GRIDS = ((2, 16, 16), (3, 5, 7), (2, 1, 1), (1, 13, 20))     # y-level (B, h, w)
WIDTHS = (64, 128, 192)


def f64(a):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(torch.float64)


# ---------------------------------------------------------------------------------------------
# tap masks (bit r * kw + s set = tap (r, s) live; 0 = every tap)
# ---------------------------------------------------------------------------------------------
def tap_mask_bits(kind, k):
    """the bit set MaskedConv2d(kind, ...)._tap_mask holds for a k x k kernel"""
    live = 0
    for r in range(k):
        for s in range(k):
            if r < k // 2 or (r == k // 2 and s < k // 2 + (kind == "B")):
                live |= 1 << (r * k + s)
    return live


def mask_array(bits, k):
    """[k, k] float64 0/1 array of a bit set (all ones for 0)"""
    m = torch.ones((k, k), dtype=torch.float64)
    if bits:
        for r in range(k):
            for s in range(k):
                m[r, s] = float((bits >> (r * k + s)) & 1)
    return m


def flip_bits(bits, k):
    """(r, s) -> (k-1-r, k-1-s)"""
    out = 0
    for r in range(k):
        for s in range(k):
            if (bits >> (r * k + s)) & 1:
                out |= 1 << ((k - 1 - r) * k + (k - 1 - s))
    return out


def live_taps(bits, k):
    return k * k if not bits else bin(bits & ((1 << (k * k)) - 1)).count("1")


# ---------------------------------------------------------------------------------------------
# the convolution in float64
# ---------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "y S n")
Grads = namedtuple("Grads", "dx dw db S_dx n_dx")


def _conv(x, w, b, s, p, transposed, op):
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=op)
    return F.conv2d(x, w, b, stride=s, padding=p)


def products_per_element(k, s, p, transposed, op, tap_mask, cin):
    """most products any output element sums: the convolution of ones on a grid with an interior, times cin"""
    one = torch.ones((1, 1, 9, 9), dtype=torch.float64)
    cnt = _conv(one, mask_array(tap_mask, k)[None, None], None, s, p, transposed, op)
    return int(round(float(cnt.max()))) * cin


def conv_ref(x, w, b, k, s, p, transposed=False, op=0, tap_mask=0):
    """x [B, Cin, H, W], w [Cout, Cin, k, k] ([Cin, Cout, k, k] transposed), b [Cout] or None -> Ref(y64, S, n)"""
    x, w = f64(x), f64(w)
    b = None if b is None else f64(b)
    wm = w * mask_array(tap_mask, k)
    y = _conv(x, wm, b, s, p, transposed, op)
    S = _conv(x.abs(), wm.abs(), None if b is None else b.abs(), s, p, transposed, op)
    cin = w.shape[0] if transposed else w.shape[1]
    return Ref(y, S, products_per_element(k, s, p, transposed, op, tap_mask, cin))


def conv_grads(x, w, b, g, k, s, p, transposed=False, op=0, tap_mask=0, dgrad_mask=None):
    """float64 autograd gradients of sum(conv(x, w * mask, b) * g): dx with the masked weights, dw with the mask NOT
    applied (the reference model leaves the weight gradient unmasked), db; S_dx = the data gradient of |g| through
    |w * mask| and n_dx its products per element.  `dgrad_mask`: another bit set for the data gradient only (mutants)."""
    x, w, g = f64(x), f64(w), f64(g)
    m_dx = mask_array(tap_mask if dgrad_mask is None else dgrad_mask, k)
    xr = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(_conv(xr, w * m_dx, None, s, p, transposed, op), xr, g)
    xa = x.abs().clone().requires_grad_(True)
    (S_dx,) = torch.autograd.grad(_conv(xa, (w * m_dx).abs(), None, s, p, transposed, op), xa, g.abs())
    wr = w.clone().requires_grad_(True)       # the unmasked weight: d/dw of the convolution does not depend on w
    (dw,) = torch.autograd.grad(_conv(x, wr, None, s, p, transposed, op), wr, g)
    db = g.sum(dim=(0, 2, 3))
    cout = w.shape[1] if transposed else w.shape[0]
    n_dx = dgrad_products_per_element(k, s, p, transposed, op, tap_mask if dgrad_mask is None else dgrad_mask, cout)
    return Grads(dx.detach(), dw.detach(), db, S_dx.detach(), n_dx)


def dgrad_products_per_element(k, s, p, transposed, op, tap_mask, cout):
    """most products any element of the data gradient sums (the densest phase of a strided layer), times cout"""
    one = torch.ones((1, 1, 9, 9), dtype=torch.float64, requires_grad=True)
    (cnt,) = torch.autograd.grad(_conv(one, mask_array(tap_mask, k)[None, None], None, s, p, transposed, op).sum(), one)
    return int(round(float(cnt.max()))) * cout


def leaky_ref(v, slope=SLOPE32):
    v = f64(v)
    return torch.where(v > 0, v, v * slope)


def leaky_bwd_ref(y_stored, g, slope=SLOPE32):
    """y > 0 ? g : rne_bf16(fp32(g) * fp32(slope)) -- leaky_bwd_bf16_kernel's arithmetic; y_stored and g bf16-exact"""
    y_stored, g = f64(y_stored), f64(g)
    prod = (g.to(torch.float32) * torch.tensor(slope, dtype=torch.float32)).to(torch.float64)   # one fp32 rounding
    return torch.where(y_stored > 0, g, rne_bf16(prod))


# ---------------------------------------------------------------------------------------------
# the latent-side layer table
# ---------------------------------------------------------------------------------------------
Layer = namedtuple("Layer", "role k s p op transposed cin cout leaky mask out level")
# out: "bf16", "f32" or "slice" (bf16 into a channel range of a wider buffer); level: the grid of the layer's INPUT --
# "y" = (h, w), "y2" = ceil(h / 2), "z" = ceil(h / 4)


def LAYERS(M, K):
    """the latent-side layers of a model with M latent channels and K mixture components"""
    M15 = int(1.5 * M)
    ep_out = 2 * M if K == 1 else 3 * K * M
    A5 = tap_mask_bits("A", 5)
    return [
        Layer("ctx", 5, 1, 2, 0, False, M, 2 * M, False, A5, "slice", "y"),
        Layer("he1", 3, 1, 1, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("he2", 5, 2, 2, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("he3", 5, 2, 2, 0, False, M, M, False, 0, "f32", "y2"),
        Layer("he3x3", 3, 2, 1, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("hd1", 5, 2, 2, 1, True, M, M, True, 0, "bf16", "z"),
        Layer("hd2", 5, 2, 2, 1, True, M, M15, True, 0, "bf16", "y2"),
        Layer("hd3", 3, 1, 1, 0, False, M15, 2 * M, False, 0, "slice", "y"),
        Layer("ep1", 1, 1, 0, 0, False, 4 * M, 640, True, 0, "bf16", "y"),
        Layer("ep2", 1, 1, 0, 0, False, 640, 640, True, 0, "bf16", "y"),
        Layer("ep3", 1, 1, 0, 0, False, 640, ep_out, False, 0, "f32", "y"),
    ]


def layer(role, M, K):
    return next(r for r in LAYERS(M, K) if r.role == role)


def npad(c):
    return (c + 63) // 64 * 64


def n_tile(c):
    """the N tile of lic_igemm_bf16 in 64-column units: the widest of 3 / 2 / 1 that divides the padded width"""
    n = npad(c)
    return 3 if n % 192 == 0 else (2 if n % 128 == 0 else 1)


# Which (role, M, K) run.  Every role at M = 192 (ep3 with K = 1 and K = 3); at M = 64 and 128 the roles whose padded
# width or N tile differs from M = 192's, plus the K = 4M inputs of ep1:
#
#   role   M    Cin -> Cout   Npad  TN        role   M    Cin -> Cout   Npad  TN
#   ctx    192  192 -> 384     384   3        ctx    128  128 -> 256     256   2
#   he*    192  192 -> 192     192   3        he3    128  128 -> 128     128   2
#   hd1    192  192 -> 192     192   3        hd2    128  128 -> 192     192   3
#   hd2    192  192 -> 288     320   1        hd3    128  192 -> 256     256   2
#   hd3    192  288 -> 384     384   3        ep1    128  512 -> 640     640   2
#   ep1    192  768 -> 640     640   2        ep3    128  640 -> 256     256   2   (K = 1)
#   ep2    192  640 -> 640     640   2        ep3    128  640 -> 1152   1152   3   (K = 3)
#   ep3    192  640 -> 384     384   3  K=1   ctx     64   64 -> 128     128   2
#   ep3    192  640 -> 1728   1728   3  K=3   he1,2   64   64 -> 64       64   1
#                                             hd2     64   64 -> 96      128   2
#                                             hd3     64   96 -> 128     128   2
#                                             ep1     64  256 -> 640     640   2
#                                             ep3     64  640 -> 576     576   3   (K = 3)
ROLES_192 = ("ctx", "he1", "he2", "he3", "he3x3", "hd1", "hd2", "hd3", "ep1", "ep2")
ROWS = [(r, 192, 1) for r in ROLES_192] + [("ep3", 192, 1), ("ep3", 192, 3)] + \
       [(r, 128, 3) for r in ("ctx", "he3", "hd2", "hd3", "ep1", "ep3")] + [("ep3", 128, 1)] + \
       [(r, 64, 3) for r in ("ctx", "he1", "he2", "hd2", "hd3", "ep1", "ep3")]
REQUIRED_NPAD = (128, 256, 320, 384, 576, 640, 1152, 1728)
REQUIRED_TN = (1, 2, 3)

CASES = [(role, M, K, grid) for (role, M, K) in ROWS for grid in GRIDS]
CTX_CASES = [c for c in CASES if c[0] == "ctx"]
OTHER_CASES = [c for c in CASES if c[0] != "ctx"]


def case_id(case):
    role, M, K, (B, h, w) = case
    return f"{role}-M{M}-K{K}-{B}x{h}x{w}"


def in_grid(lay, grid):
    B, h, w = grid
    d = {"y": 1, "y2": 2, "z": 4}[lay.level]
    return B, -(-h // d), -(-w // d)


def out_size(lay, Hi, Wi):
    if lay.transposed:
        return (Hi - 1) * lay.s - 2 * lay.p + lay.k + lay.op, (Wi - 1) * lay.s - 2 * lay.p + lay.k + lay.op
    return (Hi + 2 * lay.p - lay.k) // lay.s + 1, (Wi + 2 * lay.p - lay.k) // lay.s + 1


# ---------------------------------------------------------------------------------------------
# the planner's K split (csrc/lic_gemm_bf16.hip: igemmh_fill), restated for the tests' expectations
# ---------------------------------------------------------------------------------------------
def max_chunks(k, s, transposed, tap_mask, cin, p=None):
    """K chunks (32 input channels each) of the phase with the most live taps"""
    cpt = (cin + 31) // 32
    if transposed and s > 1:
        p = k // 2 if p is None else p
        best = 0
        for py in range(s):
            for px in range(s):
                best = max(best, sum(1 for r in range(k) for c in range(k)
                                     if (py + p - r) % s == 0 and (px + p - c) % s == 0))
        return best * cpt
    return live_taps(tap_mask, k) * cpt


def expected_ksplit(Ho, Wo, cout, chunks, force_bm=0, force_split=0):
    """the K split functional_bf16._igemm_bf16 + the planner arrive at (1 = one launch, no finishing kernel)"""
    if not (Ho * Wo <= 192 or force_split > 1):      # no workspace offered
        return 1
    t_img = (Ho * Wo + 63) // 64 * (npad(cout) // 64)
    cand = force_split != 1 and ((t_img < 4 and chunks >= 48) or force_split > 1) and chunks >= 2
    if not cand or force_bm == 256:
        return 1
    S = min(-(-24 // t_img), chunks // 8, 32)
    if force_split > 1:
        S = min(force_split, chunks)
    if S <= 1:
        return 1
    cps = -(-chunks // S)
    return -(-chunks // cps)


def expected_kernel(cout, force_bm=0):
    """the igemm_bf16_kernel<BM, TN, SQ, FUSE, RING, NWV> of a plain launch at the tests' sizes (fewer than 512
    workgroups: the automatic tile is 64 rows)"""
    tn = n_tile(cout)
    bm = force_bm or 64
    if bm == 256:
        return f"igemm_bf16_kernel<256, {tn}, false, false, 4, 8>"
    ring = 4 if (bm == 128 and tn <= 2) else 3
    return f"igemm_bf16_kernel<{bm}, {tn}, false, false, {ring}, 4>"


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _rng(key):
    return np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)


def to_bf16_exact(a):
    return torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(lay, x [B,Cin,Hi,Wi], w, b, g [B,Cout,Ho,Wo]): fp32 tensors; x, w, g bf16-exact; w ~ N(0, 1 / n), b ~ N(0, 1),
    for a leaky row shifted by the median pre-activation so that about half of them are negative"""
    role, M, K, grid = case
    lay = layer(role, M, K)
    B, Hi, Wi = in_grid(lay, grid)
    Ho, Wo = out_size(lay, Hi, Wi)
    r = _rng(case_id(case))
    n = products_per_element(lay.k, lay.s, lay.p, lay.transposed, lay.op, lay.mask, lay.cin)
    x = to_bf16_exact(r.standard_normal((B, lay.cin, Hi, Wi)))
    wshape = (lay.cin, lay.cout, lay.k, lay.k) if lay.transposed else (lay.cout, lay.cin, lay.k, lay.k)
    w = to_bf16_exact(r.standard_normal(wshape) / np.sqrt(n))
    b = torch.as_tensor(r.standard_normal((lay.cout,)).astype(np.float32))
    g = to_bf16_exact(r.standard_normal((B, lay.cout, Ho, Wo)))
    if lay.leaky:
        pre = conv_ref(x, w, b, lay.k, lay.s, lay.p, lay.transposed, lay.op, lay.mask).y
        b = (b.double() - pre.median()).to(torch.float32)
    return dict(lay=lay, x=x, w=w, b=b, g=g, n=n, Ho=Ho, Wo=Wo)


@functools.lru_cache(maxsize=None)
def forward_ref(case):
    i = inputs(case)
    lay = i["lay"]
    return conv_ref(i["x"], i["w"], i["b"], lay.k, lay.s, lay.p, lay.transposed, lay.op, lay.mask)


def grads_ref(case, g):
    """gradients of `case` for the output gradient g [B, Cout, Ho, Wo] (bf16-exact)"""
    i = inputs(case)
    lay = i["lay"]
    return conv_grads(i["x"], i["w"], i["b"], g, lay.k, lay.s, lay.p, lay.transposed, lay.op, lay.mask)


def band_ratio(dev, ref64, S, A=None):
    """max |dev - ref| / (A * S); an element with no terms (S = 0) must be exact: inf otherwise"""
    A = A_BAND if A is None else A
    err = (f64(dev) - ref64).abs()
    inf = torch.full_like(err, float("inf"))
    r = torch.where(S > 0, err / (A * S).clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(r.max())


def err_over_S(dev, ref64, S):
    err = (f64(dev) - ref64).abs()
    return float((err / S.clamp_min(1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0


def norm_err(a, b):
    a, b = f64(a), f64(b)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
