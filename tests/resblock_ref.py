"""The layers of the 3x3 residual model (HierarchicalMixtureResidual: Encoder3x3, Decoder3x3, HyperEncoder3x3,
HyperDecoder3x3; LatentSpaceTransform uses the same blocks) stated in float64: the layer table, the cases, inputs, mutants
and bands of tests/test_gpu_resblocks.py.  Plain torch on the CPU; no GPU and no product code.  The convolution is
conv_bf16_ref.conv_ref / conv_grads, the rounding gdn_bf16_ref.rne_bf16, the GDN gdn_bf16_ref.fwd, the column-route band
conv_image_bf16_ref.column_route_half_ulps: nothing of those is restated here.  tests/test_resblock_ref.py checks this file.

WHAT IS NEW HERE (no 5x5 case reaches it): the 3x3 stride-2 transposed convolution with padding 1 and output_padding 1
through lic_igemm_bf16, the 1x1 stride-2 padding-0 convolution (the skip of ResidualBlockWithStride), the RGB stem at
k = 3 (Kp = 32, 27 live columns) and k = 1 (Kp = 8, 3 live columns) through lic_im2col_bf16's generic kernels, its weight
gradient with Mvalid < Kp, the RGB head at k = 3 on the column route ([P][32] columns, lic_col2im_bf16), and the three
residual blocks as modules: the bf16 skip add, the sum of the two branches' data gradients, torch's LeakyReLU behind the
RGB convolution.

DROPPED ROLES.  A role of LAYERS3 that is identical in every field to a layer tests/test_gpu_latent_bf16.py already runs
is not run again (DROPPED, asserted by test_resblock_ref.py):
    rbs1          = he3x3 of conv_bf16_ref.LAYERS  (3x3 s2 p1, M -> M, leaky, bf16): run there at M = 192, here at 64 and 128
    rb1           = he1                            (3x3 s1 p1, M -> M, leaky, bf16): run there at M = 64 and 192, here at 128
    rb2           = rb1 of this table
    hd_up1        = up_l of this table             (the leaky form of `up`; listed once)

ROUNDING POINTS of the blocks (every bf16 store is rne_bf16 of the fp32 value):
    conv (+ fused LeakyReLU)       rne_bf16(leaky(conv64(x_q, w_q) + b))            x_q, w_q bf16, b fp32
    conv + GDN / IGDN              conv_out = rne_bf16(conv64 + b); norm, y: gdn_bf16_ref.fwd(conv_out)
    skip add                       rne_bf16(fp32(a + b))                            a, b bf16: a + b is exact in float64, the
                                                                                    fp32 add rounds once, the store again
    torch LeakyReLU on bf16        y > 0 ? y : rne_bf16(fp32(y * fp32(slope)))      (conv_bf16_ref.leaky_bwd_ref has the same
                                                                                    arithmetic for the gradient)
    gradient of x                  rne_bf16(fp32(dx_main + dx_skip))                both branches' data gradients are bf16
The fp32 blocks are the plain float64 composition.

THE BANDS.  S = the same convolution of the magnitudes plus |b| (conv_bf16_ref.conv_ref).
    fp32 output of a bf16 launch   |dev - y64| <= A S
    bf16 store without fp32 twin   |dev - y64| <= ulp_bf16(y64) / 2 + A S           (conv_image_bf16_ref.half_ulp_ratio; the
                                   inputs of these layers keep the share of elements where the band accepts the neighbouring
                                   bf16 value below 1 %: see SHIFT)
    bf16 store with an fp32 twin   bit for bit rne_bf16 of the fp32 output of the same launch on the same operands
    head, column route             |dev - y64| <= A S + the half ulps of its bf16 column terms (at most 4 per output element:
                                   the odd-row, odd-column phase of 3x3 stride 2 gathers taps (0|2, 0|2); computed by
                                   conv_image_bf16_ref.column_route_half_ulps with k = 3, p = 1, and asserted to be 4)
    weight gradient                (P + splitk + 2) 2^-24 sum |row| |col|            (tests/test_gpu_bf16_reductions.py's bound)
A = conv_bf16_ref.A_BAND = 2^-20 wherever its two conditions hold (A <= n 2^-23, A n <= 1 / 8; n = products per interior
element).  skip_rgb has n = 3 and 3 * 2^-23 < 2^-20: for it, and for any n below 8, the constant is the DERIVED
(n + 1) 2^-23 (n products and the bias, one fp32 rounding each at most), not a measured one: band_A(n).

    measured worst err / S on the MI355X (tests/test_gpu_resblocks.py, ERRS lines), and 4 x it:
        igemm        1.709e-07   6.8e-07   fp32 data gradient of hd_c (3x3, 288 -> 192) at M = 192, 1 x 13 x 20, BM 64, unsplit
        igemm_split  1.168e-07   4.7e-07   fp32 data gradient of rbs1 at M = 128, 1 x 13 x 20, K split forced to 3
        stem3        4.215e-08   1.7e-07   bf16 output only: the error beyond the store's half ulp (err_beyond_half_ulp);
                                           M = 192, 2 x 18 x 14
        skip_rgb     0           0         the same: no element of the three-product layer left its half ulp; band 2^-21
        head3        1.053e-07   4.2e-07   fp32 data gradient at M = 192, 2 x 9 x 7 (27 products of the [P][32] columns)
        fused        1.191e-07   4.8e-07   conv_out of the fused conv -> IGDN launch beyond its half ulp, M = 128, 2 x 9 x 7
    Every family's 4 x worst is below 2^-20 = 9.54e-07 (skip_rgb's below its derived 2^-21 = 4.77e-07), so no family has a
    constant of its own, and no measurement comes near n 2^-23.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_bf16_ref as CB
import gdn_bf16_ref as G
from conv_bf16_ref import (A_BAND, SLOPE, SLOPE32, Layer, Ref, _rng, band_ratio, conv_grads, conv_ref, err_over_S,  # noqa: F401
                           f64, leaky_bwd_ref, leaky_ref, n_tile, norm_err, npad, out_size, to_bf16_exact)
from conv_image_bf16_ref import column_route_half_ulps, column_route_ratio, err_beyond_half_ulp, half_ulp_ratio  # noqa: F401
from gdn_bf16_ref import is_bf16, rne_bf16, ulp_bf16  # noqa: F401

# worst err / S per family from the ERRS lines of tests/test_gpu_resblocks.py on the MI355X (bf16-only outputs: the error
# beyond the store's half ulp).
A_MEASURED = {"igemm": 1.709e-07, "igemm_split": 1.168e-07, "stem3": 4.215e-08, "skip_rgb": 0.0, "head3": 1.053e-07,
              "fused": 1.191e-07}
WIDTHS = (64, 128, 192)
GRIDS = ((2, 9, 7), (3, 5, 6), (2, 1, 1), (1, 13, 20))          # (B, h, w) at the layer's INPUT
RGB_SIZES = ((2, 18, 14), (1, 17, 13), (3, 2, 2))               # image sizes of the stem's cases (odd sides among them)


def band_A(n):
    """the band constant of a sum of n products: A_BAND where A_BAND <= n 2^-23, else the derived (n + 1) 2^-23"""
    return A_BAND if A_BAND <= n * 2.0 ** -23 else (n + 1) * 2.0 ** -23


def check_A(A, n):
    """the two conditions of conv_bf16_ref; where the first cannot hold (n < 8) the constant must be the derived one"""
    if A_BAND <= n * 2.0 ** -23:
        return A == A_BAND and A * n <= 1.0 / 8.0
    return A == (n + 1) * 2.0 ** -23 and A * n <= 1.0 / 8.0


# ---------------------------------------------------------------------------------------------
# the layer table of the 3x3 model (fields of conv_bf16_ref.Layer; level "y": the grid is the layer's input)
# ---------------------------------------------------------------------------------------------
def LAYERS3(M):
    M15 = int(1.5 * M)
    return [
        # image side
        Layer("stem3", 3, 2, 1, 0, False, 3, M, False, 0, "bf16", "y"),        # LeakyReLU applied by torch afterwards
        Layer("skip_rgb", 1, 2, 0, 0, False, 3, M, False, 0, "bf16", "y"),
        Layer("rbs1", 3, 2, 1, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("skip", 1, 2, 0, 0, False, M, M, False, 0, "bf16", "y"),
        Layer("rb1", 3, 1, 1, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("rb2", 3, 1, 1, 0, False, M, M, True, 0, "bf16", "y"),
        Layer("up", 3, 2, 1, 1, True, M, M, False, 0, "bf16", "y"),
        Layer("up_l", 3, 2, 1, 1, True, M, M, True, 0, "bf16", "y"),
        Layer("enc_last", 3, 2, 1, 0, False, M, M, False, 0, "f32", "y"),
        Layer("head3", 3, 2, 1, 1, True, M, 3, False, 0, "f32", "y"),
        # hyper side
        Layer("hd_up1", 3, 2, 1, 1, True, M, M, True, 0, "bf16", "y"),
        Layer("hd_c", 3, 1, 1, 0, False, M, M15, True, 0, "bf16", "y"),
        Layer("hd_up2", 3, 2, 1, 1, True, M15, M15, True, 0, "bf16", "y"),
    ]


def layer(role, M):
    return next(r for r in LAYERS3(M) if r.role == role)


# role -> (table, role) of the identical layer: "latent" = conv_bf16_ref.LAYERS, dropped at the widths M at which
# conv_bf16_ref.ROWS runs that layer (he3x3 at 192 only, he1 at 64 and 192); "here" = another role of this table
DROPPED = {"rbs1": ("latent", "he3x3"), "rb1": ("latent", "he1"), "rb2": ("here", "rb1"), "hd_up1": ("here", "up_l")}
IGEMM_ROLES = ("skip", "up", "up_l", "enc_last", "hd_c", "hd_up2", "rbs1", "rb1")
RGB_ROLES = ("stem3", "skip_rgb", "head3")


def dropped(role, M):
    if role not in DROPPED:
        return False
    table, other = DROPPED[role]
    return table == "here" or any(r == other and m == M for (r, m, _) in CB.ROWS)


def _tile_of(role, M):
    c = layer(role, M).cout
    return npad(c), n_tile(c)


# Which (role, M) run: every role at M = 192; at M = 64 and 128 the roles whose padded width or N tile differs from
# M = 192's (conv_bf16_ref.ROWS' rule) -- every role's does -- less what the latent file runs already:
#
#   role      M    Cin -> Cout   Npad  TN        role      M    Cin -> Cout   Npad  TN
#   skip      192  192 -> 192     192   3        skip..    128  128 -> 128     128   2    (skip, up, up_l, enc_last, rbs1, rb1)
#   up, up_l  192  192 -> 192     192   3        hd_c      128  128 -> 192     192   3
#   enc_last  192  192 -> 192     192   3        hd_up2    128  192 -> 192     192   3
#   hd_c      192  192 -> 288     320   1        skip..     64   64 -> 64       64   1    (skip, up, up_l, enc_last, rbs1)
#   hd_up2    192  288 -> 288     320   1        hd_c       64   64 -> 96      128   2
#   (rbs1, rb1 at 192: the latent file's)        hd_up2     64   96 -> 96      128   2
#   stem3, skip_rgb: 3 -> M through a [P][Kp] column matrix, N = M; head3: M -> 3 through [P][32] columns, N = 32 (Npad 64)
ROWS = [(r, M) for M in (192, 128, 64) for r in IGEMM_ROLES
        if not dropped(r, M) and (M == 192 or _tile_of(r, M) != _tile_of(r, 192))]
REQUIRED_NPAD = (64, 128, 192, 320)
REQUIRED_TN = (1, 2, 3)

# a case is conv_bf16_ref's 4-tuple (role, M, K, grid) with K = 0 (no mixture here), so that conv_bf16_ref.case_id and the
# launch helpers of tests/test_gpu_latent_bf16.py take it
CASES = [(role, M, 0, grid) for (role, M) in ROWS for grid in GRIDS]
STEM_CASES = [(role, M, 0, size) for role in ("stem3", "skip_rgb") for M in WIDTHS for size in RGB_SIZES]
HEAD_CASES = [("head3", M, 0, grid) for M in WIDTHS for grid in GRIDS]
case_id = CB.case_id


def products(lay, dgrad=False):
    """n: the most products any element of the forward (of the data gradient) sums"""
    if dgrad:
        return CB.dgrad_products_per_element(lay.k, lay.s, lay.p, lay.transposed, lay.op, 0, lay.cout)
    return CB.products_per_element(lay.k, lay.s, lay.p, lay.transposed, lay.op, 0, lay.cin)


def kpad8(k, c):
    """functional_bf16._kpad8: the column matrix' width"""
    return (k * k * c + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


# A bf16 store WITHOUT an fp32 twin (the stem's output, the fused conv_out, the blocks' stored intermediates) is held to
# half a bf16 ulp + A S, which accepts the neighbouring bf16 value where y64 lies within A S of a rounding boundary.  The
# share of such elements is about 2 A S / ulp_bf16(y) = 2^-11 S / |y|: zero-mean operands (S / |y| of 10 to 30, |y| often
# near zero) put it at 1 to 3 %.  The inputs of those layers are therefore NOT zero-mean: non-negative activations (an
# image; |N(0, 1)| features) against weights whose mean is SHIFT standard deviations, with the sign alternating from one
# output channel to the next -- |y| stays within a small factor of S, both signs occur, every product still differs, and
# tests/test_resblock_ref.py asserts the share at most 1 % for every such output.
SHIFT = 1.0


def shifted_w(r, shape, n, out_axis):
    """fp32 weights (N(0, 1) + SHIFT sign(co)) / sqrt(n), sign(co) = +1, -1, +1, .. along `out_axis`"""
    sign = np.where(np.arange(shape[out_axis]) % 2 == 0, 1.0, -1.0)
    sign = sign.reshape([-1 if a == out_axis else 1 for a in range(len(shape))])
    return _t((r.standard_normal(shape) + SHIFT * sign) / np.sqrt(n))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(lay, x [B,Cin,Hi,Wi], w, b, g [B,Cout,Ho,Wo], n, Ho, Wo) of fp32 tensors.
    igemm roles (conv_bf16_ref.inputs' recipe): x, w, g bf16-exact, w ~ N(0, 1 / n), b ~ N(0, 1) shifted by the median
    pre-activation of a leaky row.  stem3 / skip_rgb: x uniform in [0, 1) and NOT bf16-exact (lic_im2col_bf16 rounds it), w
    NOT bf16-exact (the packer rounds it), g bf16-exact.  head3: x bf16-exact, w and g NOT bf16-exact."""
    role, M, _, (B, Hi, Wi) = case
    lay = layer(role, M)
    Ho, Wo = out_size(lay, Hi, Wi)
    r = _rng("res3-" + case_id(case))
    n = products(lay)
    wshape = (lay.cin, lay.cout, lay.k, lay.k) if lay.transposed else (lay.cout, lay.cin, lay.k, lay.k)
    if role in RGB_ROLES:
        x = to_bf16_exact(r.standard_normal((B, lay.cin, Hi, Wi))) if role == "head3" else _t(r.random_sample((B, 3, Hi, Wi)))
        w = _t(r.standard_normal(wshape) / np.sqrt(n)) if role == "head3" else shifted_w(r, wshape, n, 0)
        b = _t(r.standard_normal((lay.cout,)) * (1.0 if role == "head3" else 0.1))
        g = r.standard_normal((B, lay.cout, Ho, Wo))
        g = _t(g) if role == "head3" else to_bf16_exact(g)
        assert not is_bf16(w) and (is_bf16(x) if role == "head3" else not is_bf16(x) or x.numel() < 4)
        return dict(lay=lay, x=x, w=w, b=b, g=g, n=n, Ho=Ho, Wo=Wo)
    x = to_bf16_exact(r.standard_normal((B, lay.cin, Hi, Wi)))
    w = to_bf16_exact(r.standard_normal(wshape) / np.sqrt(n))
    b = _t(r.standard_normal((lay.cout,)))
    g = to_bf16_exact(r.standard_normal((B, lay.cout, Ho, Wo)))
    if lay.leaky:
        pre = conv_ref(x, w, b, lay.k, lay.s, lay.p, lay.transposed, lay.op).y
        b = (b.double() - pre.median()).to(torch.float32)
    return dict(lay=lay, x=x, w=w, b=b, g=g, n=n, Ho=Ho, Wo=Wo)


def rounded_operands(case):
    """(x_q, w_q, g_q) in float64 as the kernels multiply them"""
    i = inputs(case)
    return rne_bf16(i["x"]), rne_bf16(i["w"]), rne_bf16(i["g"])


@functools.lru_cache(maxsize=None)
def forward_ref(case, bias=True):
    i = inputs(case)
    lay = i["lay"]
    xq, wq, _ = rounded_operands(case)
    return conv_ref(xq, wq, i["b"] if bias else None, lay.k, lay.s, lay.p, lay.transposed, lay.op)


def grads_ref(case, g=None):
    """conv_grads on the rounded operands; `g`: another (bf16-exact) output gradient, e.g. behind a LeakyReLU's backward"""
    i = inputs(case)
    lay = i["lay"]
    xq, wq, gq = rounded_operands(case)
    return conv_grads(xq, wq, i["b"], gq if g is None else g, lay.k, lay.s, lay.p, lay.transposed, lay.op)


# ---------------------------------------------------------------------------------------------
# the column matrices of the RGB layers
# ---------------------------------------------------------------------------------------------
def im2col_ref(x, k, s, p, Kp):
    """x [B,C,H,W] -> float64 [P][Kp]: col[(b, oh, ow)][(r k + t) C + c] = rne_bf16(x[b, c, oh s - p + r, ow s - p + t]),
    zero outside the image and in columns k k C .. Kp - 1"""
    xq = rne_bf16(x)
    B, C, H, W = xq.shape
    u = F.unfold(xq, k, padding=p, stride=s)                      # [B, C k k, L], rows ordered (c, r, t)
    L = u.shape[2]
    u = u.reshape(B, C, k * k, L).permute(0, 3, 2, 1).reshape(B * L, k * k * C)
    out = torch.zeros((B * L, Kp), dtype=torch.float64)
    out[:, :k * k * C] = u
    return out


def col2im_ref(col, bias, B, Hi, Wi, C, k, s, p, op):
    """col [P][Kp] (P = B Hi Wi, column (r k + t) C + c) -> (out64 [B,C,Ho,Wo], S): out[b, c, ih s - p + r, iw s - p + t]
    += col; S sums the magnitudes (and |bias|)"""
    col = f64(col)
    Ho, Wo = (Hi - 1) * s - 2 * p + k + op, (Wi - 1) * s - 2 * p + k + op
    u = col[:, :k * k * C].reshape(B, Hi * Wi, k * k, C).permute(0, 3, 2, 1).reshape(B, C * k * k, Hi * Wi)
    out = F.fold(u, (Ho, Wo), k, padding=p, stride=s)
    S = F.fold(u.abs(), (Ho, Wo), k, padding=p, stride=s)
    if bias is not None:
        out = out + f64(bias)[None, :, None, None]
        S = S + f64(bias).abs()[None, :, None, None]
    return out, S


def stem_matrix_weight(w, Kp):
    """[Kp][Cout]: row (r k + t) Cin + c = w_q[co, c, r, t]; rows k k Cin .. Kp - 1 zero (functional_bf16._stem_columns_bf16)"""
    wq = rne_bf16(w)
    Cout, Cin, k, _ = wq.shape
    m = torch.zeros((Kp, Cout), dtype=torch.float64)
    m[:k * k * Cin] = wq.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout)
    return m


def column_terms(k=3, s=2, p=1, op=1):
    """most column terms any output element of the head's col2im gathers (the densest phase)"""
    one = torch.ones((1, 1, 5, 5), dtype=torch.float64)
    return int(round(float(F.conv_transpose2d(one, torch.ones((1, 1, k, k), dtype=torch.float64), None, s, p, op).max())))


# ---------------------------------------------------------------------------------------------
# weight gradient band
# ---------------------------------------------------------------------------------------------
def wgrad_weight(x, g, lay):
    """sum |row| |col| of every element of the weight gradient: conv_grads of the magnitudes"""
    return conv_grads(f64(x).abs(), torch.ones(_wshape(lay), dtype=torch.float64), None, f64(g).abs(), lay.k, lay.s, lay.p,
                      lay.transposed, lay.op).dw


def _wshape(lay):
    return (lay.cin, lay.cout, lay.k, lay.k) if lay.transposed else (lay.cout, lay.cin, lay.k, lay.k)


def wgrad_ratio(dw, dw64, weight, P, splitk):
    """worst |dw - dw64| / ((P + splitk + 2) 2^-24 sum |row| |col|); an element without terms must be exact"""
    err = (f64(dw) - dw64).abs()
    bound = (P + splitk + 2) * 2.0 ** -24 * weight
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def colsum_ratio(db, g64):
    """the column-sum band of tests/test_gpu_latent_bf16.py: |db - sum g| <= 1e-5 sum |g| + 1e-6"""
    g64 = f64(g64)
    ref = g64.sum(dim=(0, 2, 3))
    tol = 1e-5 * g64.abs().sum(dim=(0, 2, 3)) + 1e-6
    return float(((f64(db) - ref).abs() / tol).max())


# ---------------------------------------------------------------------------------------------
# the element-wise rounding points of the blocks
# ---------------------------------------------------------------------------------------------
def _fp32(a):
    return f64(a).to(torch.float32).to(torch.float64)


def add_bf16_ref(a, b):
    """torch's bf16 add (the skip add, the sum of two branches' gradients): rne_bf16(fp32(a + b)), a and b bf16-exact"""
    a, b = f64(a), f64(b)
    assert is_bf16(a) and is_bf16(b)
    return rne_bf16(_fp32(a + b))


def torch_leaky_bf16_ref(y, slope=SLOPE32):
    """torch's LeakyReLU on a bf16 tensor: y > 0 ? y : rne_bf16(fp32(y * fp32(slope)))"""
    y = f64(y)
    assert is_bf16(y)
    prod = _fp32(y * slope)
    return torch.where(y > 0, y, rne_bf16(prod))


def torch_leaky_bf16_bwd_ref(y_in, g, slope=SLOPE32):
    """its backward: y_in > 0 ? g : rne_bf16(fp32(g * fp32(slope))), the mask from the LeakyReLU's INPUT"""
    return leaky_bwd_ref(y_in, g, slope)


def rows(t):
    """[B,C,H,W] -> [P][C] (gdn_bf16_ref's layout)"""
    t = f64(t)
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unrows(r, B, H, W):
    return r.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------
# the blocks, layer by layer, at the device's rounding points (bf16 storage)
# ---------------------------------------------------------------------------------------------
def conv_store(x, w, b, lay_or_geo, leaky=False, round_x=False):
    """one bf16-storage conv launch: (y64 before the store -- LeakyReLU applied when fused --, S).  x bf16-exact unless
    round_x (the stem rounds the image); w is rounded by the packer"""
    k, s, p, tr, op = lay_or_geo
    xq = rne_bf16(x) if round_x else f64(x)
    assert is_bf16(xq)
    ref = conv_ref(xq, rne_bf16(w), b, k, s, p, tr, op)
    return (leaky_ref(ref.y) if leaky else ref.y), ref.S


C3S2 = (3, 2, 1, False, 0)
C3S1 = (3, 1, 1, False, 0)
C1S2 = (1, 2, 0, False, 0)
T3S2 = (3, 2, 1, True, 1)


_store = rne_bf16      # every bf16 store


def block_forward(kind, x, P, mutant=None):
    """the bf16-storage forward of a block in float64 -> dict of the stored tensors, `out` the block's result.
    kind: "rbs_rgb" (ResidualBlockWithStride(3, M)), "rbs" (M -> M), "rb" (ResidualBlock), "rbu" (ResidualBlockUpsample).
    P: dict of fp32 parameters (w1 b1 w2 b2 [ws bs] [beta_e gamma_e]).  mutant: "no_skip", "skip_offset", "leaky_positive",
    or None"""
    x = f64(x)
    B = x.shape[0]
    st = {}

    def leaky_stage(v):
        return torch.where(v > 0, v * SLOPE32, v) if mutant == "leaky_positive" else leaky_ref(v)

    if kind == "rbs_rgb":
        c1, _ = conv_store(x, P["w1"], P["b1"], C3S2, round_x=True)
        st["c1"] = _store(c1)
        if mutant == "leaky_positive":
            st["h1"] = torch.where(st["c1"] > 0, _store(_fp32(st["c1"] * SLOPE32)), st["c1"])
        else:
            st["h1"] = torch_leaky_bf16_ref(st["c1"])
    elif kind == "rbs":
        c1, _ = conv_store(x, P["w1"], P["b1"], C3S2)
        st["h1"] = _store(leaky_stage(c1))
    elif kind == "rb":
        c1, _ = conv_store(x, P["w1"], P["b1"], C3S1)
        st["h1"] = _store(leaky_stage(c1))
    elif kind == "rbu":
        c1, _ = conv_store(x, P["w1"], P["b1"], T3S2)
        st["h1"] = _store(leaky_stage(c1))
    else:
        raise KeyError(kind)
    c2, _ = conv_store(st["h1"], P["w2"], P["b2"], C3S1)
    if kind == "rb":
        st["main"] = _store(leaky_stage(c2))
        identity = st["identity"] = x
    else:
        st["conv_out"] = _store(c2)
        _, H2, W2 = st["conv_out"].shape[1:]
        n64, nq, y64 = G.fwd(rows(st["conv_out"]), P["beta_e"], P["gamma_e"], kind == "rbu")
        st["norm"], st["main"] = unrows(nq, B, H2, W2), _store(unrows(y64, B, H2, W2))
        if kind == "rbu":
            idn, _ = conv_store(x, P["ws"], P["bs"], T3S2)
        elif mutant == "skip_offset":
            xs = F.pad(rne_bf16(x) if kind == "rbs_rgb" else x, (0, 1, 0, 1))[..., 1:, 1:]
            idn = conv_ref(xs, rne_bf16(P["ws"]), P["bs"], 1, 2, 0).y
        else:
            idn, _ = conv_store(x, P["ws"], P["bs"], C1S2, round_x=(kind == "rbs_rgb"))
        identity = st["identity"] = _store(idn)
    st["out"] = st["main"] if mutant == "no_skip" else add_bf16_ref(st["main"], identity)
    return st


def block_forward_fp32(kind, x, P):
    """the fp32 blocks: the plain float64 composition (no rounding anywhere) -> out64"""
    x = f64(x)
    p = {k: f64(v) for k, v in P.items()}
    geo = {"rbs_rgb": C3S2, "rbs": C3S2, "rb": C3S1, "rbu": T3S2}[kind]
    h1 = leaky_ref(conv_ref(x, p["w1"], p["b1"], *geo).y)
    c2 = conv_ref(h1, p["w2"], p["b2"], *C3S1).y
    if kind == "rb":
        return leaky_ref(c2) + x
    B, _, H2, W2 = c2.shape
    r = rows(c2)
    n = p["beta_e"][None, :] + (r * r) @ p["gamma_e"].t()
    y = unrows(r * (n.sqrt() if kind == "rbu" else n.rsqrt()), B, H2, W2)
    idn = conv_ref(x, p["ws"], p["bs"], *(T3S2 if kind == "rbu" else C1S2)).y
    return y + idn


def block_params(kind, M, seed="p", shifted=True):
    """fp32 parameters of a block, NOT bf16-exact (the packers round them); GDN operands as a trained layer has them.
    shifted: the weights in front of a bf16 store WITHOUT an fp32 twin (the RGB conv1, conv2 in front of a GDN, the skip) are
    shifted_w; the layers with a fused LeakyReLU, whose stores the GPU test holds through an fp32 twin, keep zero-mean
    weights, as does every layer of the fp32 blocks (shifted=False): conv_ref64's constants were measured on cancelling
    sums.  (With same-sign terms the fp32 accumulation error grows with the partial sums: the fp32 twin of
    ResidualBlockUpsample's first layer at M = 192, 768 products, measured err / S = 5.14e-07 on such weights, the fp32
    conv2 + residual of ResidualBlock(192) 2.2e-06 -- three and a half and two orders below n 2^-23.)"""
    r = _rng(f"block-{kind}-{M}-{seed}")
    cin = 3 if kind == "rbs_rgb" else M

    def w(shape, n, out_axis=0, shift=True):
        if shifted and shift:
            return shifted_w(r, shape, n, out_axis)
        return _t(r.standard_normal(shape) / np.sqrt(n))
    P = {}
    if kind == "rbu":
        P["w1"], P["ws"] = w((M, M, 3, 3), 4 * M, 1, shift=False), w((M, M, 3, 3), 4 * M, 1)
    else:
        P["w1"] = w((M, cin, 3, 3), 9 * cin, shift=(kind == "rbs_rgb"))
        if kind != "rb":
            P["ws"] = w((M, cin, 1, 1), cin)
    P["w2"] = w((M, M, 3, 3), 9 * M, shift=(kind != "rb"))
    P["b1"], P["b2"] = _t(0.1 * r.standard_normal(M)), _t(0.1 * r.standard_normal(M))
    if kind != "rb":
        P["bs"] = _t(0.1 * r.standard_normal(M))
        P["beta_e"] = _t(1.0 + 0.2 * r.random_sample(M))
        P["gamma_e"] = _t(0.1 * np.eye(M) + 0.02 * r.random_sample((M, M)) / np.sqrt(M))
    return P


def block_input(kind, M, grid):
    B, h, w = grid
    r = _rng(f"block-x-{kind}-{M}-{B}x{h}x{w}")
    if kind == "rbs_rgb":
        return _t(r.random_sample((B, 3, h, w)))
    return to_bf16_exact(np.abs(r.standard_normal((B, M, h, w))))


BLOCK_KINDS = ("rbs_rgb", "rbs", "rb", "rbu")
BLOCK_GRIDS = {"rbs_rgb": (2, 18, 14), "rbs": (2, 9, 7), "rb": (2, 9, 7), "rbu": (2, 5, 6)}
BLOCK_WIDTHS = (64, 192)
FUSED_GRIDS = ((2, 9, 7), (1, 13, 20))


@functools.lru_cache(maxsize=None)
def fused_inputs(M, inverse, grid):
    """the fused conv -> GDN / IGDN launch at 3x3 s1 p1: dict(x bf16-exact and non-negative, w (shifted, not bf16-exact), b, g)"""
    B, H, W = grid
    r = _rng(f"fused3-M{M}-{int(inverse)}-{B}x{H}x{W}")
    x = to_bf16_exact(np.abs(r.standard_normal((B, M, H, W))))
    w = shifted_w(r, (M, M, 3, 3), 9 * M, 0)
    b = _t(0.1 * r.standard_normal(M))
    g = to_bf16_exact(r.standard_normal((B, M, H, W)))
    return dict(x=x, w=w, b=b, g=g)


def block_stage_refs(kind, x, P):
    """[(name, y64, S, n)] of every conv output a block stores as bf16 without an fp32 twin, along the reference's own
    chain.  The stores behind a fused LeakyReLU (h1; ResidualBlock's main) are not among them: their negative half is a
    hundred times smaller against the same A S, so the GPU test launches an fp32 twin of those layers instead and holds
    the bf16 store bit for bit to its rounding."""
    st = block_forward(kind, x, P)
    rgb = kind == "rbs_rgb"
    M = P["w2"].shape[0]
    out = []
    if rgb:
        out.append(("c1",) + conv_store(x, P["w1"], P["b1"], C3S2, round_x=True) + (27,))
    if kind != "rb":
        out.append(("conv_out",) + conv_store(st["h1"], P["w2"], P["b2"], C3S1) + (9 * M,))
    if kind != "rb":
        geo_s, n_s = (T3S2, 4 * M) if kind == "rbu" else (C1S2, 3 if rgb else M)
        out.append(("identity",) + conv_store(x, P["ws"], P["bs"], geo_s, round_x=rgb) + (n_s,))
    return out


def no_twin_outputs():
    """yields (tag, y64, S, A) of EVERY bf16 output tests/test_gpu_resblocks.py holds at half a bf16 ulp + A S because no fp32
    twin of the launch exists: the stem's outputs (b), the fused conv_out (d), the blocks' stored conv outputs (e)"""
    for case in STEM_CASES:
        ref = forward_ref(case)
        yield case_id(case), ref.y, ref.S, band_A(ref.n)
    for M in WIDTHS:
        for inverse in (False, True):
            for grid in FUSED_GRIDS:
                i = fused_inputs(M, inverse, grid)
                ref = conv_ref(i["x"], rne_bf16(i["w"]), i["b"], 3, 1, 1)
                yield f"fused-M{M}-{int(inverse)}-{'x'.join(map(str, grid))}", ref.y, ref.S, band_A(ref.n)
    for kind in BLOCK_KINDS:
        for M in BLOCK_WIDTHS:
            for name, y64, S, n in block_stage_refs(kind, block_input(kind, M, BLOCK_GRIDS[kind]), block_params(kind, M)):
                yield f"{kind}-M{M}-{name}", y64, S, band_A(n)


# ---------------------------------------------------------------------------------------------
# mutants: what these layers could actually get wrong, as float64 outputs to hold against the bands
# ---------------------------------------------------------------------------------------------
def mutant_drop_tap(case, ci=1, r=None, t=None):
    """1. one tap dropped at one input channel"""
    i = inputs(case)
    lay = i["lay"]
    xq, wq, _ = rounded_operands(case)
    r = lay.k - 1 if r is None else r
    t = 0 if t is None else t
    wq = wq.clone()
    if lay.transposed:
        wq[ci, :, r, t] = 0.0
    else:
        wq[:, ci, r, t] = 0.0
    return conv_ref(xq, wq, i["b"], lay.k, lay.s, lay.p, lay.transposed, lay.op).y


def mutant_no_output_padding(case):
    """2. output_padding ignored: the last output row and column hold the bias only"""
    i = inputs(case)
    y = forward_ref(case).y.clone()
    b = f64(i["b"])[None, :, None]
    y[:, :, -1, :] = b
    y[:, :, :, -1] = b
    return y


def mutant_skip_offset(case):
    """3. the stride-2 1x1 convolution sampled at offset 1: pixel (2 oy + 1, 2 ox + 1), zero outside"""
    i = inputs(case)
    lay = i["lay"]
    assert (lay.k, lay.s, lay.p) == (1, 2, 0)
    xq, wq, _ = rounded_operands(case)
    return conv_ref(F.pad(xq, (0, 1, 0, 1))[..., 1:, 1:], wq, i["b"], 1, 2, 0).y


def mutant_leaky_positive(y64):
    """5. LeakyReLU applied on the positive side"""
    return torch.where(y64 > 0, y64 * SLOPE32, y64)


def mutant_not_flipped(case):
    """6. the transposed convolution with the weight's taps not flipped: tap (r, t) used as (k - 1 - r, k - 1 - t)"""
    i = inputs(case)
    lay = i["lay"]
    assert lay.transposed
    xq, wq, _ = rounded_operands(case)
    return conv_ref(xq, wq.flip(2, 3), i["b"], lay.k, lay.s, lay.p, True, lay.op).y


def mutant_live_padding_columns(case):
    """7. columns K .. Kp - 1 of the stem's matrix live: they hold the next floats of the NHWC image row behind the last
    tap's pixel (channel c of pixel column ow s - p + k + j // 3, zero outside the row) and meet the weight of the last
    live row instead of a packed zero -> (column matrix, output)"""
    i = inputs(case)
    lay = i["lay"]
    k, s, p, C = lay.k, lay.s, lay.p, lay.cin
    K, Kp = k * k * C, kpad8(k, C)
    xq, wq, _ = rounded_operands(case)
    col = im2col_ref(i["x"], k, s, p, Kp)
    B, _, H, W = xq.shape
    Ho, Wo = i["Ho"], i["Wo"]
    xh = xq.permute(0, 2, 3, 1)
    extra = torch.zeros((B, Ho, Wo, Kp - K), dtype=torch.float64)
    for j in range(Kp - K):
        for oh in range(Ho):
            for ow in range(Wo):
                ih, iw, c = oh * s - p + k - 1, ow * s - p + k + j // C, j % C
                if 0 <= ih < H and 0 <= iw < W:
                    extra[:, oh, ow, j] = xh[:, ih, iw, c]
    col[:, K:] = extra.reshape(-1, Kp - K)
    m = stem_matrix_weight(i["w"], Kp)
    m[K:] = m[K - 1]
    y = (col @ m).reshape(B, Ho, Wo, lay.cout).permute(0, 3, 1, 2) + f64(i["b"])[None, :, None, None]
    return col, y


def mutant_wgrad_rows(dw):
    """8. the stem's weight-gradient row (tap, c) sent to tap Cin + c instead of tap + c taps: dw [Cout][Cin][k][k]"""
    Cout, Cin, k, _ = dw.shape
    return dw.reshape(Cout, Cin, k * k).permute(0, 2, 1).reshape(Cout, Cin, k, k).clone()


def out_of_band(y_mut, y64, S, A, half_ulp):
    """how many elements of a mutant lie outside the band of the reference"""
    bound = A * S + (0.5 * ulp_bf16(y64) if half_ulp else 0.0)
    return int(((f64(y_mut) - y64).abs() > bound).sum())


def near_boundary_share(y64, S, A):
    """the share of elements whose float64 value lies within A S of a bf16 rounding boundary (the midpoint of two adjacent
    bf16 values): there a store may round to either neighbour, and the half-ulp band accepts both"""
    y64 = f64(y64)
    u = ulp_bf16(y64)
    lo = torch.floor(y64 / u.clamp_min(1e-300)) * u
    return float(((y64 - (lo + 0.5 * u)).abs() <= A * S).double().mean())
