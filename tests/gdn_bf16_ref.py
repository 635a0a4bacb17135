"""GDN / IGDN in bf16 storage stated in float64 AT THE KERNELS' OWN ROUNDING POINTS (csrc/lic_epilogue_bf16.h: x and x^2
rounded to bf16, fp32 pool, y from the fp32 norm, the stored norm rounded to bf16; backward: t rounded to bf16, fp32 pool
of bf16 operands), and the cases, inputs and bands of tests/test_gpu_gdn_bf16.py.  Numpy / torch on the CPU only; imports
gdn_ref64 (the unrounded float64 statement) and no product code.  tests/test_gdn_bf16_ref.py checks this file.

Because every stage is compared from the previous stage's DEVICE output (the reference forward starts from the bf16 x
the device read, the backward from the bf16 norm and, for the pool, from the device's own bf16 t), a stage's band holds
only that stage's arithmetic and the bands do not add up.

THE BANDS.  u = 2^-24 is the fp32 unit roundoff (half an fp32 ulp, relative).  An output stored as bf16 is held to

    |got - ref| <= ulp_bf16(ref) / 2 + k u mag

the first term is the one round-to-nearest-even at the store, the second the fp32 arithmetic in front of it (an fp32
output has the second term only).  The constants are DERIVED from the operation counts, first order in u, not measured:

  K_FWD(C) = C + 3, norm against mag = n64 and y against mag = |y64|.  The C products gamma x^2 are products of two bf16
      values (16 significant bits): exact in fp32.  Summed into a zero accumulator in any association they cost at most
      C - 1 roundings of partial sums that never exceed n64 (every term is >= 0), the beta add one more: C u n64 for the
      norm.  y = x * f(n): n^-+1/2 halves the relative error of n (C / 2 u), v_rsq_f32 / v_sqrt_f32 are good to 1 ulp =
      2 u, the multiply adds 1 u: (C / 2 + 3) u.  C + 3 covers both.
  K_T = 16, t against mag = |t64|.  g x is a product of two bf16 values: exact; 0.5 scales.  v_rsq_f32 (2 u) enters to
      the third power in GDN (6 u) and once in IGDN; r * r, gx * r and the last product are three roundings: 9 u.
  K_DX(C) = C + 8, dx against mag = |g f| + 2 |x| sum_j |t_j| gamma_ji (the sum of the magnitudes of its terms).  The
      pool is C exact products in C - 1 fp32 adds, 2 x scales it exactly; g * f is v_rsq / v_sqrt (2 u) and a multiply
      (1 u); the fused multiply-add rounds once: (C + 3) u mag.
  colsum: a sum of n fp32 terms in any association is within (n - 1) u of the sum of their magnitudes.
A measured ratio above 1 is a finding about the kernel (or about a term this derivation missed, to be named from the
kernel's code): the constants are not to be scaled to a measurement.
"""
from __future__ import annotations

import torch

import gdn_ref64 as G
from gdn_ref64 import f64

U = 2.0 ** -24
WIDTHS = (64, 128, 192)
# the sweep's wave owns 32 pixels and its workgroup 128; the igemm tiles are 64 and 128 rows
SIZES = (1, 31, 33, 127, 128, 129, 357)
SWEEP_TILE, SWEEP_MAX_GRID = 128, 2048          # gdn_bwd_bf16_kernel: pixels per tile, the workgroup cap
BIG = SWEEP_TILE * SWEEP_MAX_GRID + 77          # more tiles than workgroups: some workgroups take a second tile
CASES = [(C, inv, P) for C in WIDTHS for inv in (0, 1) for P in SIZES]
BIG_CASES = [(64, 0, BIG), (128, 1, BIG)]
case_id = G.case_id


def K_FWD(C):
    return C + 3


K_T = 16


def K_DX(C):
    return C + 8


# ---------------------------------------------------------------------------------------------
# bf16 in float64
# ---------------------------------------------------------------------------------------------
_DROP = 52 - 7                                             # float64 significand bits bf16 does not keep


def rne_bf16(a):
    """float64 -> the nearest bf16-representable float64, ties to the even 8-bit significand.  Rounded FROM FLOAT64
    DIRECTLY, on its bit pattern (add half of the dropped field, one less at an even kept bit, and clear the field; a
    carry runs into the exponent as it should), never through fp32: a float64 value that lies within fp32 rounding of a
    bf16 tie would otherwise be rounded twice.  Normal bf16 range only (asserted)."""
    a = f64(a).contiguous()
    mag = a.abs()
    hi = float(mag.max()) if a.numel() else 0.0
    lo = float(torch.where(mag == 0, torch.full_like(mag, float("inf")), mag).min()) if a.numel() else float("inf")
    assert hi < 2.0 ** 127 and lo >= 2.0 ** -126, ("outside bf16's normal range (or not finite)", lo, hi)
    b = a.view(torch.int64)
    b = (b + ((1 << (_DROP - 1)) - 1) + ((b >> _DROP) & 1)) & ~((1 << _DROP) - 1)
    return b.view(torch.float64)


def is_bf16(a):
    a = f64(a)
    return bool(torch.equal(rne_bf16(a), a))


def ulp_bf16(v):
    """2^(floor(log2 |v|) - 7): the spacing of bf16 values at v (0 at 0; v normal in float64)"""
    v = f64(v).contiguous()
    p2 = (v.view(torch.int64) & (0x7FF << 52)).view(torch.float64)        # 2^floor(log2 |v|), 0 at 0
    return p2 * 2.0 ** -7


def bf16_bits(a):
    """int16 bit patterns of a bf16 tensor / of bf16-representable values, -0 folded into +0"""
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    if a.dtype != torch.bfloat16:
        assert is_bf16(a), "not representable in bf16"
        a = a.to(torch.bfloat16)
    return (a + 0.0).contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------
# the operation at the kernels' rounding points
# ---------------------------------------------------------------------------------------------
def fwd(x, beta_e, gamma_e, inverse):
    """x [P][C] bf16-exact, beta_e [C] fp32, gamma_e [C][C] fp32 ([norm index][x index]) -> (n64, rne_bf16(n64), y64):
    the pool of the bf16-rounded squares against the bf16-rounded gamma, y from the UNROUNDED norm"""
    x, beta_e = f64(x), f64(beta_e)
    assert is_bf16(x), "x must be bf16-exact"
    gq = rne_bf16(gamma_e)
    sq = rne_bf16(x * x)
    n64 = beta_e[None, :] + sq @ gq.t()
    y64 = x * (n64.sqrt() if inverse else n64.rsqrt())
    return n64, rne_bf16(n64), y64


def t_of(g, x, norm_bf16, inverse):
    g, x, n = f64(g), f64(x), f64(norm_bf16)
    return 0.5 * (g * x) * n.rsqrt() if inverse else -0.5 * (g * x) * n.rsqrt() / n


def bwd(g, x, norm_bf16, gamma_e, inverse, t_dev=None):
    """(t64, dx64, mag) from bf16-exact g, x and the bf16 norm.  t64 is unrounded; the pool contracts the bf16 t --
    the device's own `t_dev` where given, rne_bf16(t64) otherwise -- with rne_bf16(gamma_e); mag as in gdn_ref64.bwd"""
    g, x, n = f64(g), f64(x), f64(norm_bf16)
    gq = rne_bf16(gamma_e)
    t64 = t_of(g, x, n, inverse)
    tq = rne_bf16(t64) if t_dev is None else f64(t_dev)
    u = g * (n.sqrt() if inverse else n.rsqrt())
    dx64 = u + 2.0 * x * (tq @ gq)
    mag = u.abs() + 2.0 * x.abs() * (tq.abs() @ gq)
    return t64, dx64, mag


def reparam_bwd(p, dout, bound):
    """the re-parametrisation's backward (p_eff = max(p, bound)^2 - pedestal) in float64, with the lower bound's
    one-sided rule as oracle.gdn_reparam_bwd states it"""
    p, dout = f64(p), f64(dout)
    bound = float(torch.tensor(bound, dtype=torch.float32))      # (the kernels take the bound as an fp32 argument)
    g = dout * 2.0 * p.clamp_min(bound)
    return torch.where((p >= bound) | (g < 0), g, torch.zeros_like(g))


def tile_colsums(a, grid, tile=SWEEP_TILE):
    """([grid][C] float64, [grid] term counts): row b sums the pixels of tiles b, b + grid, .. of `tile` pixels"""
    a = f64(a)
    P, C = a.shape
    ntile = (P + tile - 1) // tile
    pad = torch.zeros((ntile * tile, C), dtype=torch.float64)
    pad[:P] = a
    per_tile = pad.reshape(ntile, tile, C).sum(1)
    rows = torch.zeros((grid, C), dtype=torch.float64)
    rows.index_add_(0, torch.arange(ntile) % grid, per_tile)
    valid = torch.zeros(ntile * tile)
    valid[:P] = 1
    n = torch.zeros(grid).index_add_(0, torch.arange(ntile) % grid, valid.reshape(ntile, tile).sum(1))
    return rows, n


def sweep_grid(P):
    return min((P + SWEEP_TILE - 1) // SWEEP_TILE, SWEEP_MAX_GRID)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def band_ratios(got, ref, mag, k, half_ulp=True):
    """per element |got - ref| / (ulp_bf16(ref) / 2 + k u mag); a NaN counts as infinite; an element whose bound is 0
    must be exact (0 / 0 -> 0, e / 0 -> inf); `half_ulp=False` for an fp32 output (no bf16 store)"""
    got, ref, mag = f64(got), f64(ref), f64(mag)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    err = (got - ref).abs_()
    bound = mag.abs().mul_(k * U)
    if half_ulp:
        bound.add_(ulp_bf16(ref), alpha=0.5)
    exact = err == 0
    return err.div_(bound).masked_fill_(exact, 0.0).nan_to_num_(nan=float("inf"), posinf=float("inf"))


def band_ratio(got, ref, mag, k, half_ulp=True):
    """the worst of band_ratios over EVERY element"""
    r = band_ratios(got, ref, mag, k, half_ulp)
    return float(r.max()) if r.numel() else 0.0


def with_other_norm(dx64, mag, g, n_main, n_other, inverse):
    """(dx64, mag) of `bwd` re-stated for another norm in the element-wise term g f(norm) (the pool term, which contracts
    the device's own t, stays): the recomputing sweep at an ambiguous element"""
    g, n_main, n_other = f64(g), f64(n_main), f64(n_other)
    u0 = g * (n_main.sqrt() if inverse else n_main.rsqrt())
    u1 = g * (n_other.sqrt() if inverse else n_other.rsqrt())
    return dx64 - u0 + u1, mag - u0.abs() + u1.abs()


def colsum_ratio(part, src, grid):
    """worst error of the [grid][C] fp32 column sums `part` against the float64 sums of the device's own bf16 `src`, over
    the n-term bound (n - 1) u sum |terms|; rows of one term (and of none) must be exact"""
    ref, n = tile_colsums(src, grid)
    mag, _ = tile_colsums(f64(src).abs(), grid)
    part = f64(part)
    assert part.shape == ref.shape, (part.shape, ref.shape)
    err = torch.nan_to_num((part - ref).abs(), nan=float("inf"), posinf=float("inf"))
    bound = (n - 1).clamp_min(0)[:, None] * U * mag
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def bf16_neighbours(n64):
    """the two adjacent bf16 values lo <= n64 < hi (n64 > 0)"""
    n64 = f64(n64)
    u = ulp_bf16(n64)
    lo = torch.floor(n64 / u) * u
    return lo, lo + u


def ambiguous(n64, C):
    """True where the float64 pool lies within K_FWD(C) u n64 of a bf16 rounding boundary (a midpoint of two adjacent
    bf16 values): an fp32 pool inside its band may round to either neighbour there, and to rne_bf16(n64) only elsewhere"""
    n64 = f64(n64)
    lo, hi = bf16_neighbours(n64)
    return (n64 - 0.5 * (lo + hi)).abs() <= K_FWD(C) * U * n64


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def banded_inputs(C, inverse, P):
    """gdn_ref64.banded_inputs with x, g and the generated norm rounded to bf16 (fp32 tensors holding bf16 values);
    gamma_e and beta_e stay fp32: the pack's rounding of gamma is under test too"""
    i = dict(G.banded_inputs(C, inverse, P))
    for k in ("x", "g", "norm"):
        i[k] = rne_bf16(i[k]).float()
    return i


exact_fwd_inputs = G.exact_fwd_inputs
exact_bwd_inputs = G.exact_bwd_inputs


def round_half_up(a):
    """float64 -> bf16 with ties away from zero: the wrong rounding the exact backward case must tell from rne_bf16"""
    a = f64(a)
    m, e = torch.frexp(a)
    s = m.abs() * 256.0
    return torch.ldexp(torch.sign(m) * torch.floor(s + 0.5), e - 8)
