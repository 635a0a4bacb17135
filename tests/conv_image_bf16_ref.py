"""The image-side bf16 convolutions -- the RGB stem (lic_stem_gdn_bf16 / lic_stem_conv_bf16), the RGB head
(lic_head_convt_bf16 and its column-matrix route), the halo-resident 5x5 stride-2 kernels (lic_halo_bf16.h,
lic_halot_bf16.h) and the convolution part of the fused conv -> GDN launches -- stated in float64, with the case tables,
inputs, mutants, exact cases and bands of tests/test_gpu_image_bf16.py.  Plain torch on the CPU; no GPU and no product
code.  The convolution itself is conv_bf16_ref.conv_ref / conv_grads and the rounding gdn_bf16_ref.rne_bf16: nothing is
restated here.  tests/test_conv_image_bf16_ref.py checks this file.

OPERAND ROUNDING.  The kernels multiply bf16 operands and accumulate in fp32.  What is not bf16 yet is rounded to nearest
even on the way in, and the reference says so explicitly:

    stem            x_q = rne_bf16(x)   the fp32 image, in registers (pack2 of csrc/lic_stem_bf16.hip)
    head's dgrad    g_q = rne_bf16(g)   the fp32 image gradient, by the same kernel (its PLAIN instantiation)
    every weight    w_q = rne_bf16(w)   by the packers
    bias            fp32, not rounded

The reference convolves the ROUNDED operands in float64; every product of two bf16 values is exact in fp32, so an fp32
output carries the summation's error only.

THE BANDS.  S is the same convolution of the magnitudes plus |b| (conv_bf16_ref.conv_ref's S).

    fp32 output                     |dev - y64| <= A S                                  (conv_bf16_ref.band_ratio)
    bf16 output without fp32 twin   |dev - y64| <= ulp_bf16(y64) / 2 + A S              (half_ulp_ratio: the half-ulp term
                                    is gdn_bf16_ref.band_ratios', with k u = A)
    bf16 / LeakyReLU output of a template that also stores fp32: bit for bit rne_bf16 of that fp32 output on the same
                                    operands (LeakyReLU: leaky_ref first)
    head, column-matrix route       |dev - y64| <= A S + sum over the <= 9 column terms of ulp_bf16(col64) / 2
                                    (column_route_half_ulps: lic_igemm_bf16 stores the [P][80] per-tap columns as bf16 and
                                    lic_col2im_bf16 sums them in fp32)

THE CONSTANT A.  conv_bf16_ref.A_BAND = 2^-20 was measured on lic_igemm_bf16 (1.934e-07).  The kernels here sum in other
orders (halo: chunk-major; stem and head: the 32x32x16 MFMA with the pixels on the lanes), so the GPU module measures each
family's worst err / S against this reference (its ERRS lines) and a family whose 4 x worst exceeded 2^-20 would get its
own constant: 4 x measured, rounded up to a power of two.

    measured worst err / S on the MI355X (tests/test_gpu_image_bf16.py, ERRS lines), and 4 x it:
        stem    2.827e-08   1.1e-07   bf16 outputs only: the error beyond the store's half ulp (err_beyond_half_ulp); the
                                      head's data gradient at C = 192, 2 x 8 x 31
        head    5.634e-08   2.3e-07   fp32 output; C = 64, the 129-image batch of group e
        halo    1.300e-07   5.2e-07   fp32 data gradient of the transposed layer, Cin = 128, 2 x 19 x 37 (25 x 128 products)
        halot   1.227e-07   4.9e-07   fp32 data gradient of the strided layer, Cin = 128, 2 x 16 x 64
        fused   5.183e-08   2.1e-07   conv_out beyond its half ulp; igemm_t4_igdn_128_192_7x5
    Every family's 4 x worst is below 2^-20 = 9.54e-07, so A = A_BAND for all of them (A below): the chunk-major sum of the
    halo kernels and the pixels-on-lanes MFMA of the stem and head are no worse than lic_igemm_bf16's tap-major sum.
    fp32 RGB route (functional.image_conv2d / image_conv_transpose2d; UNROUNDED operands, fp32 products are rounded):
        rgb32   2.704e-07   1.08e-06  the head's data gradient at C = 64, 2 x 5 x 33
    4 x worst exceeds 2^-20, so the route has its own constant A32 = 2^-19 = 1.907e-06 (<= 75 x 2^-23 = 8.9e-06).

Two conditions on A are asserted on the CPU for every case and are not measurements (conv_bf16_ref.py):
    A <= n 2^-23     and     A n <= 1 / 8
with n the products per interior element: 75 for the stem (and the head's data gradient), 9 C for the head's forward,
25 Cin for the strided halo layer, 9 Cin for the transposed one (its densest phase); data gradients: 9 Cout of the strided
layer, 25 Cout of the transposed one.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import gdn_bf16_ref as G
from conv_bf16_ref import (A_BAND, SLOPE, SLOPE32, Ref, _rng, band_ratio, conv_grads, conv_ref, err_over_S,  # noqa: F401
                           f64, leaky_ref, norm_err, to_bf16_exact)
from gdn_bf16_ref import is_bf16, rne_bf16, round_half_up, ulp_bf16  # noqa: F401

# worst err / S per family, from the ERRS lines of tests/test_gpu_image_bf16.py on the MI355X.  For the families whose only
# output is bf16 (stem) the error left after taking the store's half ulp away is what counts: err_beyond_half_ulp.
A_MEASURED = {"stem": 2.827e-08, "head": 5.634e-08, "halo": 1.300e-07, "halot": 1.227e-07, "fused": 5.183e-08,
              "rgb32": 2.704e-07}
A = {"stem": A_BAND, "head": A_BAND, "halo": A_BAND, "halot": A_BAND, "fused": A_BAND}
A32 = 2.0 ** -19                 # the fp32 RGB route: 4 x 2.704e-07 = 1.08e-06, rounded up to a power of two
WIDTHS = (64, 128, 192)
K5 = dict(k=5, s=2, p=2)         # every layer here is 5x5, stride 2, padding 2 (transposed: output_padding 1)

# ---------------------------------------------------------------------------------------------
# tile constants of the kernels, restated (source line named) for the coverage assertions and group e's bounds
# ---------------------------------------------------------------------------------------------
HD_TH, HD_TW = 4, 32             # csrc/lic_head_bf16.hip: `constexpr int HD_TH = 4, HD_TW = 32` (feature pixels per tile)
HALO_TH, HALO_TW = 8, 32         # csrc/lic_halo_bf16.h: `constexpr int TH = 8, TWD = 32` (output pixels per tile)
HALOT_TH, HALOT_TW = 8, 32       # csrc/lic_halot_bf16.h: `constexpr int TH = 8, TWD = 32` (phase = input pixels per tile)


def stem_tile(C):
    """csrc/lic_stem_bf16.hip: `p.ntiles = (p.P + 255) / 256` at Cout == 192 (8 waves), `(p.P + 127) / 128` otherwise"""
    return 256 if C == 192 else 128


def stem_threads(C):
    """csrc/lic_stem_bf16.hip: dim3(512) at Cout == 192, dim3(256) otherwise"""
    return 512 if C == 192 else 256


def stem_out(H, W):
    return (H + 1) // 2, (W + 1) // 2


def stem_tiles(C, B, H, W):
    Ho, Wo = stem_out(H, W)
    return -(-B * Ho * Wo // stem_tile(C))


def stem_fast_lanes(H, W):
    """how many (output column, lane half) pairs take the two-16-byte-load path of the stem: `colfast = cf0 >= 0 &&
    cf0 + 8 <= rowf` with cf0 = (2 ox - 2) 3 + 8 lh, rowf = 3 W"""
    Wo = (W + 1) // 2
    return sum(1 for ox in range(Wo) for lh in (0, 1) if (2 * ox - 2) * 3 + 8 * lh >= 0 and (2 * ox - 2) * 3 + 8 * lh + 8 <= 3 * W)


def stem_tile_spans_images(C, B, H, W):
    Ho, Wo = stem_out(H, W)
    hw, t = Ho * Wo, stem_tile(C)
    return any((k * t) // hw != min((k + 1) * t - 1, B * hw - 1) // hw for k in range(-(-B * hw // t)))


def stem_seam_inside_row(C, B, H, W):
    """a tile boundary that is not at the start of an output row"""
    Ho, Wo = stem_out(H, W)
    t = stem_tile(C)
    return any((k * t) % Wo for k in range(1, -(-B * Ho * Wo // t)))


def head_tiles(B, Hi, Wi):
    return B * (-(-Hi // HD_TH)) * (-(-Wi // HD_TW))


def halo_tiles(B, Hi, Wi):
    """strided layer: tiles of its OUTPUT ((Hi + 1) // 2 x (Wi + 1) // 2)"""
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    return B * (-(-Ho // HALO_TH)) * (-(-Wo // HALO_TW))


def halot_tiles(B, Hi, Wi):
    """transposed layer: tiles of its INPUT (each output phase of a tile is 8 x 32)"""
    return B * (-(-Hi // HALOT_TH)) * (-(-Wi // HALOT_TW))


# group e: the largest grid the launch code can choose, per CU, from the hardware limits (not from the kernel's own
# occupancy answer) -- a batch with more than twice that many tiles gives some workgroup a third trip
def max_workgroups_per_cu(family, C=0):
    if family in ("halo", "halot"):
        return 1                     # lic_igemm_bf16: `grid = min(nwg, ncu)`, one workgroup per CU
    if family == "head":
        return 2                     # 75 KB of LDS per workgroup (HD_MT * 32 * HD_LD floats) in a 160 KB CU
    if family == "stem":
        return 2048 // stem_threads(C)    # 2048 resident threads per CU: 8 blocks of 256, 4 of 512
    raise KeyError(family)


# ---------------------------------------------------------------------------------------------
# the case tables (shapes are NCHW sizes of the layer's INPUT)
# ---------------------------------------------------------------------------------------------
STEM_SHAPES = ((1, 1, 1), (2, 2, 3), (1, 5, 6), (3, 21, 19), (2, 20, 18), (1, 7, 300), (1, 300, 1))
HEAD_SHAPES = ((3, 1, 1), (2, 4, 32), (2, 5, 33), (1, 3, 65), (1, 9, 40), (2, 8, 31))
HALO_SHAPES = ((2, 1, 1), (2, 16, 64), (2, 17, 65), (1, 37, 45), (1, 15, 63))
HALOT_SHAPES = ((2, 1, 1), (2, 8, 32), (1, 9, 33), (2, 19, 37), (1, 5, 40))
# Even strided shapes for the data gradient only.  halo_convt_bf16_kernel covers Ho = 2 Hi, Wo = 2 Wi (csrc/lic_gemm_bf16.hip:
# `shape_t`), so of HALO_SHAPES only 2 x 16 x 64 -- one aligned tile -- reaches it as a data gradient; these two give it ragged
# 8 x 32 tiles of phase pixels: 9 x 33 (one past in both directions) and 19 x 37.
HALO_DGRAD_SHAPES = ((1, 18, 66), (2, 38, 74))
HALO_COUT = 128
STEM_CASES = [("stem", C, s) for C in WIDTHS for s in STEM_SHAPES]
HEAD_CASES = [("head", C, s) for C in WIDTHS for s in HEAD_SHAPES]
HALO_CASES = [("halo", C, s) for C in WIDTHS for s in HALO_SHAPES]
HALOT_CASES = [("halot", C, s) for C in WIDTHS for s in HALOT_SHAPES]
HALO_DGRAD_CASES = [("halo", 128, s) for s in HALO_DGRAD_SHAPES]
ALL_CASES = STEM_CASES + HEAD_CASES + HALO_CASES + HALOT_CASES
# group e: images per tile count (see max_workgroups_per_cu); one image of each of these has 32 / 8 / 4 / 4 tiles
E_STEM_HW, E_HEAD_HW, E_HALO_HW, E_HALOT_HW = (128, 128), (16, 64), (24, 80), (12, 40)


def case_id(case):
    fam, C, (B, H, W) = case
    return f"{fam}-C{C}-{B}x{H}x{W}"


def transposed(fam):
    return fam in ("head", "halot")


def channels(case):
    """(Cin, Cout) of the layer"""
    fam, C, _ = case
    return {"stem": (3, C), "head": (C, 3), "halo": (C, HALO_COUT), "halot": (C, HALO_COUT)}[fam]


def out_hw(fam, H, W):
    return (2 * H, 2 * W) if transposed(fam) else ((H + 1) // 2, (W + 1) // 2)


def products(case, dgrad=False):
    """n: products per interior element of the forward (or of the data gradient)"""
    fam, C, _ = case
    cin, cout = channels(case)
    if not dgrad:
        return (9 if transposed(fam) else 25) * cin
    return (25 if transposed(fam) else 9) * cout


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(x [B,Cin,H,W], w, b [Cout], g [B,Cout,Ho,Wo]) fp32 tensors.  stem: x uniform in [0, 1) and NOT bf16-exact (the
    kernel rounds it); other families: x bf16-exact (what a bf16 layer hands over).  w ~ N(0, 1 / n) fp32, NOT bf16-exact
    (the packers round it); b ~ N(0, 1) fp32.  g: the head's is fp32 N(0, 1), not bf16-exact (lic_stem_conv_bf16 rounds
    it); the others' are bf16-exact."""
    fam, C, (B, H, W) = case
    cin, cout = channels(case)
    r = _rng("image-" + case_id(case))
    n = products(case)
    Ho, Wo = out_hw(fam, H, W)
    x = _t(r.random_sample((B, cin, H, W))) if fam == "stem" else to_bf16_exact(r.standard_normal((B, cin, H, W)))
    wshape = (cin, cout, 5, 5) if transposed(fam) else (cout, cin, 5, 5)
    w = _t(r.standard_normal(wshape) / np.sqrt(n))
    b = _t(r.standard_normal((cout,)))
    g = r.standard_normal((B, cout, Ho, Wo))
    g = _t(g) if fam == "head" else to_bf16_exact(g)
    if fam == "stem":
        assert not is_bf16(x)
    if fam == "head":
        assert not is_bf16(g)
    assert not is_bf16(w)
    return dict(x=x, w=w, b=b, g=g, Ho=Ho, Wo=Wo)


def layer_ref(fam, x, w, b, round_x=None):
    """float64 reference of one layer on the ROUNDED operands: w_q = rne_bf16(w); x_q = rne_bf16(x) where the kernel
    rounds it (the stem), else x must be bf16-exact already"""
    round_x = (fam == "stem") if round_x is None else round_x
    xq = rne_bf16(x) if round_x else f64(x)
    assert is_bf16(xq)
    return conv_ref(xq, rne_bf16(w), b, 5, 2, 2, transposed(fam), 1 if transposed(fam) else 0)


@functools.lru_cache(maxsize=None)
def forward_ref(case, bias=True):
    i = inputs(case)
    return layer_ref(case[0], i["x"], i["w"], i["b"] if bias else None)


@functools.lru_cache(maxsize=None)
def grads_ref(case):
    """conv_grads on the rounded operands: g_q = rne_bf16(g) (the head's fp32 image gradient is rounded by the kernel; the
    others' are bf16-exact already)"""
    i = inputs(case)
    fam = case[0]
    xq = rne_bf16(i["x"]) if fam == "stem" else f64(i["x"])
    tr = transposed(fam)
    return conv_grads(xq, rne_bf16(i["w"]), i["b"], rne_bf16(i["g"]), 5, 2, 2, tr, 1 if tr else 0)


@functools.lru_cache(maxsize=None)
def forward_ref_fp32(case):
    """the fp32 RGB route: the float64 convolution of the UNROUNDED fp32 operands"""
    i = inputs(case)
    tr = transposed(case[0])
    return conv_ref(i["x"], i["w"], i["b"], 5, 2, 2, tr, 1 if tr else 0)


@functools.lru_cache(maxsize=None)
def grads_ref_fp32(case):
    i = inputs(case)
    tr = transposed(case[0])
    return conv_grads(i["x"], i["w"], i["b"], i["g"], 5, 2, 2, tr, 1 if tr else 0)


# ---------------------------------------------------------------------------------------------
# bands
# ---------------------------------------------------------------------------------------------
def half_ulp_ratio(dev, y64, S, A=A_BAND):
    """worst |dev - y64| / (ulp_bf16(y64) / 2 + A S): gdn_bf16_ref.band_ratios with k u = A"""
    return G.band_ratio(dev, y64, S, A / G.U, half_ulp=True)


def err_beyond_half_ulp(dev, y64, S):
    """worst (|dev - y64| - ulp_bf16(y64) / 2) / S: what the summation must account for behind a bf16 store"""
    e = ((f64(dev) - y64).abs() - 0.5 * ulp_bf16(y64)).clamp_min(0.0)
    return float((e / S.clamp_min(1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0


def column_route_half_ulps(x, w, k=5, s=2, p=2, op=1):
    """[B,3,Ho,Wo]: per output element, the sum of ulp_bf16(col64) / 2 over the column terms it gathers, col64[b, (ky, kx,
    colour), iy, ix] = sum_ci x[b, ci, iy, ix] w_q[ci, colour, ky, kx] -- the bf16 rounding of the [P][Kp] column matrix the
    column-matrix route of the head stores between lic_igemm_bf16 and lic_col2im_bf16 ([P][80] at the default 5x5 stride-2
    geometry; k, s, p, op: another head geometry)"""
    x, wq = f64(x), rne_bf16(w)
    out = None
    for ky in range(k):
        for kx in range(k):
            col = torch.einsum("bchw,cd->bdhw", x, wq[:, :, ky, kx])
            hu = 0.5 * ulp_bf16(col)
            one = torch.zeros((3, 1, k, k), dtype=torch.float64)
            one[:, 0, ky, kx] = 1.0
            t = F.conv_transpose2d(hu, one, None, stride=s, padding=p, output_padding=op, groups=3)
            out = t if out is None else out + t
    return out


def column_route_ratio(dev, y64, S, half_ulps, A=A_BAND):
    err = (f64(dev) - y64).abs()
    bound = A * S + half_ulps
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def check_A(A_, n):
    """the two conditions on a band constant that are not measurements"""
    return A_ <= n * 2.0 ** -23 and A_ * n <= 1.0 / 8.0


# ---------------------------------------------------------------------------------------------
# mutants: what these kernels could actually get wrong, as float64 outputs to hold against the bands
# ---------------------------------------------------------------------------------------------
def _plain(fam, xq, wq, b):
    tr = transposed(fam)
    return conv_ref(xq, wq, b, 5, 2, 2, tr, 1 if tr else 0).y


def mutant_clamp_edge(fam, x, w, b):
    """1. zero padding replaced by clamp-to-edge on the right and bottom border (strided layers)"""
    assert not transposed(fam)
    xq = rne_bf16(x) if fam == "stem" else f64(x)
    xp = F.pad(F.pad(xq, (2, 0, 2, 0)), (0, 2, 0, 2), mode="replicate")
    return F.conv2d(xp, rne_bf16(w), f64(b), stride=2, padding=0)


def mutant_drop_tap(fam, x, w, b, ci=1, r=3, s=1):
    """2. one tap dropped at one input channel"""
    xq = rne_bf16(x) if fam == "stem" else f64(x)
    wq = rne_bf16(w).clone()
    if transposed(fam):
        wq[ci, :, r, s] = 0.0
    else:
        wq[:, ci, r, s] = 0.0
    return _plain(fam, xq, wq, b)


def mutant_stem_slot15(x, w, b):
    """3. the stem's sixteenth K slot live: the lane's eighth float of the upper half is channel 0 of pixel column
    2 ox + 3 of the same image row (zero outside the row); it multiplies a packed zero.  The mutant adds it with the weight
    of slot 14 = (s = 4, c = 2)"""
    xq, wq = rne_bf16(x), rne_bf16(w)
    y = conv_ref(xq, wq, b, 5, 2, 2).y
    we = torch.zeros((wq.shape[0], 3, 5, 6), dtype=torch.float64)
    we[:, 0, :, 5] = wq[:, 2, :, 4]
    return y + F.conv2d(F.pad(xq, (2, 3, 2, 2)), we, None, stride=2, padding=0)


def mutant_head_phase(y64):
    """4. the head's phase rule for odd output columns evaluated with the p_x of the neighbouring (even) column: kx = 2 b'
    at the same feature columns q_x + 1 - b' -- which is the even column's own sum"""
    y = y64.clone()
    y[..., 1::2] = y64[..., 0::2]
    return y


def mutant_head_halo_column(y64):
    """5. the head's gather off by one halo column from feature column 32 on (the second x tile): output column ox >= 64
    holds the value of column ox + 2"""
    y = y64.clone()
    if y.shape[-1] > 66:
        y[..., 64:-2] = y64[..., 66:]
    return y


def mutant_swap_phases(y64):
    """6. the transposed layer with two of its four output phases swapped: (even row, odd column) <-> (odd row, even column)"""
    y = y64.clone()
    y[..., 0::2, 1::2] = y64[..., 1::2, 0::2]
    y[..., 1::2, 0::2] = y64[..., 0::2, 1::2]
    return y


# ---------------------------------------------------------------------------------------------
# exact cases: every partial sum in any order is exact in fp32, so the device must give these bits
# ---------------------------------------------------------------------------------------------
TIE_EVEN_DOWN = 1.0 + 2.0 ** -8            # the tie between 1 and 1 + 2^-7: to even = down
TIE_EVEN_UP = 1.0 + 3.0 * 2.0 ** -8        # the tie between 1 + 2^-7 and 1 + 2^-6: to even = up
_OFF = 2.0 ** -20
TIE_VALUES = (TIE_EVEN_DOWN, TIE_EVEN_UP, TIE_EVEN_DOWN + _OFF, TIE_EVEN_DOWN - _OFF, TIE_EVEN_UP + _OFF,
              TIE_EVEN_UP - _OFF, 1.0, 1.0 + 2.0 ** -7)
TWO_TAP = 10                               # the last channels of the exact stem weight hold two taps (+2, -1)


def trunc_bf16(a):
    """float64 -> bf16 by dropping bits (toward zero): a wrong rounding the exact case must tell from rne_bf16"""
    a = f64(a).contiguous()
    return (a.view(torch.int64) & ~((1 << G._DROP) - 1)).view(torch.float64)


@functools.lru_cache(maxsize=None)
def exact_stem(C, B, H, W):
    """(x fp32 [B,3,H,W], w fp32 [C,3,5,5]): image values on bf16 ties of both parities and just off them (colour 2 with
    either sign); output channel co < C - TWO_TAP has ONE tap, a power of two: y = +-2^e rne_bf16(x) is bf16-exact whatever
    the order.  The last TWO_TAP channels have +2 at colour 0 and -1 at colour 1 of the same tap: 2 a - b with a, b in
    [1, 1 + 2^-5) multiples of 2^-7 is bf16-exact too, and differs from the rounding of the unrounded 2 x0 - x1."""
    r = _rng(f"exact-stem-{C}-{B}-{H}-{W}")
    x = np.asarray(TIE_VALUES)[r.randint(0, len(TIE_VALUES), size=(B, 3, H, W))]
    x[:, 2] *= r.choice([-1.0, 1.0], size=(B, H, W))
    w = np.zeros((C, 3, 5, 5))
    for co in range(C):
        if co < C - TWO_TAP:
            t = (11 * co) % 75
            w[co, t // 25, (t % 25) // 5, t % 5] = (-1.0) ** co * 2.0 ** ((co % 7) - 3)
        else:
            t = (7 * co) % 25
            w[co, 0, t // 5, t % 5], w[co, 1, t // 5, t % 5] = 2.0, -1.0
    xt, wt = _t(x), _t(w)
    assert torch.equal(xt.double(), torch.as_tensor(x)) and is_bf16(wt)
    return xt, wt


def exact_stem_out(x, w, rounding=rne_bf16):
    """the exact stem's output under a rounding of the image: float64, no bias; `rounding=None`: the image not rounded, the
    output rounded at the store only"""
    if rounding is None:
        return rne_bf16(_nz(conv_ref(f64(x), f64(w), None, 5, 2, 2).y))
    return conv_ref(rounding(x), f64(w), None, 5, 2, 2).y


def _nz(a):
    return a + 0.0


@functools.lru_cache(maxsize=None)
def exact_int(fam, C, B, H, W):
    """(x, w, b) integer-valued: |x| <= 3, |w| <= 2, |b| <= 4 -- every partial sum is an integer below 2^24, exact in
    fp32 in any order, so an fp32 output equals the float64 reference bit for bit"""
    case = (fam, C, (B, H, W))
    cin, cout = channels(case)
    r = _rng(f"exact-int-{case_id(case)}")
    x = _t(r.randint(-3, 4, size=(B, cin, H, W)))
    w = _t(r.randint(-2, 3, size=(cin, cout, 5, 5) if transposed(fam) else (cout, cin, 5, 5)))
    b = _t(r.randint(-4, 5, size=(cout,)))
    assert 25 * cin * 6 + 4 < 2 ** 24
    return x, w, b
