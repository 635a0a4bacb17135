"""The bf16 image-side convolutions -- the RGB stem (stem_gdn_bf16_kernel, pooled and PLAIN), the RGB head
(head_convt_bf16_kernel and the column-matrix route), the halo-resident 5x5 stride-2 kernels (halo_conv_bf16_kernel,
halo_convt_bf16_kernel, plain and fused) and the convolution part of the fused igemm variants -- against
tests/conv_image_bf16_ref.py, the float64 statement of the same convolutions on the operands as the kernels round them.
The bands and their constants are derived / measured there.

  a. stem, direct launches of lic_stem_gdn_bf16 (with conv_out) and lic_stem_conv_bf16 at C = 64 / 128 / 192 on fp32
     images that are NOT bf16-exact: conv_out and the PLAIN output to half a bf16 ulp + A S; exact cases (bf16 ties of
     both parities, single power-of-two taps) bit for bit;
  b. head, direct launches of lic_head_convt_bf16 with and without bias: fp32 output to A S; exact integer cases bit for
     bit; the data gradient (lic_stem_conv_bf16 on an fp32 gradient that is not bf16-exact) to half an ulp + A S; dw / db
     at the existing bands; the column-matrix route to A S + the half ulps of its <= 9 bf16 column terms;
  c. halo kernels forced with FORCE_IGEMM = (512, 0, 1): fp32 output to A S, bf16 and LeakyReLU outputs bit for bit the
     rounded fp32 output, fused launches' conv_out to half an ulp + A S, data gradients (each runs the other kernel);
  d. the five igemm_* geometries of test_gpu_bf16_epilogue_bits.FUSED: conv_out to half an ulp + A S;
  e. every persistent loop takes a second and a third trip: a batch of many small images, bit for bit the concatenation of
     its single-image launches (one trip each); first, middle and last image to the float64 bands;
  f. refusals launch nothing;
  g. the fp32 RGB route (functional.image_conv2d / image_conv_transpose2d) to A32 S against the float64 convolution of
     the UNROUNDED operands, forward and data gradient.

Every output of a direct launch is a view inside a NaN-filled allocation whose guard rows are checked afterwards
(test_gpu_gdn_bf16.Guarded).  Launches through functional_bf16 assert their kernel variant through KERNEL_TRACE; the C
entry points of the stem and the head launch one kernel template each and put no name into the trace themselves (the
Python wrapper does), so every direct launch of a and b is paired with the traced wrapper launch of the same operands
and must give the same bits.  Every figure is printed as `RATIO <group> <case> <what> <value>` before it is asserted;
`ERRS` lines carry the raw err / S per family.

Measured on the MI355X (256 CUs), worst err / S per family against the float64 reference: stem 2.827e-08 (beyond the
store's half ulp; the head's data gradient, C = 192, 2 x 8 x 31), head 5.634e-08 (C = 64, the 129-image batch of e), halo
1.300e-07 (the transposed layer's fp32 data gradient, Cin = 128, 2 x 19 x 37), halot 1.227e-07 (the strided layer's fp32
data gradient, Cin = 128, 2 x 16 x 64), fused conv_out 5.183e-08 beyond its half ulp (igemm_t4_igdn_128_192_7x5).  4 x each
is below 2^-20, so every bf16 family keeps A = conv_bf16_ref.A_BAND = 2^-20 = 9.54e-07.  The fp32 RGB route measured
2.704e-07 (the head's data gradient, C = 64, 2 x 5 x 33): 4 x that is 1.08e-06 > 2^-20, so A32 = 2^-19 (n 2^-23 = 8.9e-06
at n = 75).  Worst RATIO per group, each against a bound of 1:

    a  stem              conv_out, PLAIN 0.9996 of half a bf16 ulp + A S (the rounding itself uses the half ulp); PLAIN and
                         the wrapper's conv_out / y / norm bit for bit the direct launch; exact cases bit for bit
    b  head              y 0.051 (C128 2x5x33)   y without bias 0.048   dx 0.9994 of half an ulp + A S   dw 0.003   db 0.003
                         column route: y 0.996 of A S + its column half ulps, dx 0.9994; exact cases bit for bit
    c  halo kernels      y, leaky 0.113 (halot C64 1x9x33)   dx 0.136 (halot C128 2x19x37, run by halo_conv_bf16_kernel)
                         fused conv_out 0.9992 of half an ulp + A S; every bf16 / LeakyReLU store bit for bit
    d  fused igemm       conv_out 0.9984 of half an ulp + A S   plain fp32 0.098
    e  many tiles        every batch bit for bit its single-image launches; y 0.118 (halot C128), stem 0.9995 of its band
    g  fp32 RGB route    y 0.135 (stem C192 1x7x300)   dx 0.142 (head C64 2x5x33) of A32 S

The fused launches' conv_out is bit for bit rne_bf16 of the plain fp32 output in every case of c and d (35 of 35), and is
asserted: the FUSE instantiation is the same kernel template as the plain one, sums K in the same order, and
gdn_fwd_square_tile rounds x = acc + bias to bf16 once (lic_epilogue_bf16.h), which is what the plain bf16 store does.

Kernel variants and grids (workgroups) a trace of this module shows:
(rocprofv3 --kernel-trace alone, in a run of its own; 204 tests; rocprofv3 prints the PLAIN template argument as
`true`; e = the 129-image batch of group e, its tile count behind the grid)
    stem_gdn_bf16_kernel<2, 4, false>   grids 1, 2, 3, 5, 32    e: 768 workgroups for 4128 tiles
    stem_gdn_bf16_kernel<2, 4, true>    grids 1 .. 5, 32        e: 1280 for 4128        (PLAIN)
    stem_gdn_bf16_kernel<4, 4, false>   grids 1, 2, 3, 5, 32    e: 512 for 4128
    stem_gdn_bf16_kernel<4, 4, true>    grids 1 .. 5, 32        e: 1024 for 4128        (PLAIN)
    stem_gdn_bf16_kernel<6, 8, false>   grids 1, 2, 3, 16       e: 256 for 2064
    stem_gdn_bf16_kernel<6, 8, true>    grids 1, 2, 3, 16       e: 256 for 2064         (PLAIN)
    head_convt_bf16_kernel<4>           grids 2, 3, 4, 6, 8     e: 512 for 1032
    head_convt_bf16_kernel<8>           grids 2, 3, 4, 6, 8     e: 512 for 1032
    head_convt_bf16_kernel<12>          grids 2, 3, 4, 6, 8     e: 256 for 1032
    halo_conv_bf16_kernel<2, false, 0>  grids 1, 2, 3, 4, 8, 12 e: 256 for 516
    halo_conv_bf16_kernel<2, true, 0>   grids 1, 2, 3, 8
    halo_convt_bf16_kernel<2, false>    grids 2, 4, 12          e: 256 for 516
    halo_convt_bf16_kernel<2, true>     grids 2, 4, 12
Every batch of e runs on a grid smaller than a third of its tile count (the stem at C = 192: an eighth), so every
persistent loop there takes at least three trips; the single-image launches (32, 16, 8 and 4 tiles) take one.
The module takes 7 s on the MI355X; its slowest test 0.7 s (the first head launch), a group e test 0.1 to 0.5 s.

What did not hold as the issue words it, and what is asserted instead:
  * the strided layer's data gradient runs halo_convt_bf16_kernel only where the layer's input is even in both directions
    (the transposed kernel covers Ho = 2 Hi, i.e. output_padding 1): of the issue's strided cases that is 2 x 16 x 64, one
    aligned tile.  HALO_DGRAD_SHAPES adds 1 x 18 x 66 and 2 x 38 x 74, whose gradients are ragged for the transposed kernel
    (9 x 33 and 19 x 37 phase pixels).  The odd cases assert the implicit-GEMM kernel's name and hold its fp32 dx to
    conv_bf16_ref's band; the transposed layer's data gradient runs halo_conv_bf16_kernel in every case.  Data gradients
    need Cin = 128 (the halo kernels write 128 channels).
  * lic_stem_gdn_bf16 / lic_stem_conv_bf16 / lic_head_convt_bf16 put no name into KERNEL_TRACE (functional_bf16 does): each
    direct launch of a, b and e (exact cases included) is paired with the traced wrapper launch of the same operands, bit
    for bit.  The wrapper reaches the PLAIN stem only as the head's data gradient (test_b_head asserts that name); the
    direct PLAIN launches of a and e are held bit for bit to the conv_out of the pooled launch they are paired with.  The
    single-image launches of e and the refused / accepted calls of f are the same entry points with no wrapper beside them.
  * the head has no 16-byte aligned output (fp32, 4-byte aligned): its refusals are a misaligned x and w_packed.
  * behind ONE power-of-two tap a forgotten rounding of the image gives the same bits as the store's rounding: the exact
    stem weight has ten two-tap channels (+2, -1) that tell it apart (test_conv_image_bf16_ref.py).
No kernel, packing or Python error was found.

Run on the MI355X box:  python -m pytest tests/test_gpu_image_bf16.py -m gpu -q -s"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_image_bf16_ref as R
from test_gpu_bf16_epilogue_bits import FUSED
from test_gpu_gdn_bf16 import ERR_INVALID, ERR_UNSUPPORTED, Guarded
from test_gpu_latent_bf16 import close_norm, colsum_ratio

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HALO_FORCE = (512, 0, 1)
ERRS = {k: 0.0 for k in R.A_MEASURED}
FUSED_EQUALS_ROUNDED_PLAIN = {}      # case -> whether a fused launch's conv_out is bit for bit rne_bf16 of the plain fp32 output
# What the code says and the device confirmed for every case of c and d: the FUSE instantiation is the same kernel template
# as the plain one, sums K in the same order and rounds x = acc + bias to bf16 once for conv_out (lic_epilogue_bf16.h).
FUSED_CONV_IS_ROUNDED_PLAIN = True


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic  # noqa: F401
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd import functional_bf16 as FB
    L.load()  # must be the in-tree HIP extension; raises if missing
    yield F_, FB, L, torch.device("cuda:0")
    print("\nMEASURED " + " ".join(f"{k} {v:.4e}" for k, v in ERRS.items()) + f" A_BAND {R.A_BAND:.4e}")
    print("FUSED conv_out == rne_bf16(plain fp32): " + " ".join(f"{k}={v}" for k, v in sorted(FUSED_EQUALS_ROUNDED_PLAIN.items())))


@pytest.fixture(autouse=True)
def stop_after_a_device_error(env):
    """a HIP error (an illegal access, a failed launch) ends the module: nothing more is started on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def ratio(group, tag, what, value):
    print(f"RATIO {group} {tag} {what} {value:.4f}")
    return value


def note(fam, group, tag, what, e):
    ERRS[fam] = max(ERRS[fam], e)
    print(f"ERRS {group} {tag} {what} {fam} {e:.3e}")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw64(t):
    """a device NHWC tensor -> float64 NCHW on the CPU"""
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def bf(a, dev):
    t = a.to(BF)
    assert torch.equal(t.float(), a.float()), "the input is not bf16-exact"
    return t.to(dev)


def ptr(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def same(a, b, what):
    """two device tensors hold the same bits"""
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    v = torch.int16 if a.dtype == BF else torch.int32
    assert torch.equal(a.view(v), b.view(v)), f"{what}: {int((a.view(v) != b.view(v)).sum())} of {a.numel()} elements differ"


def banded32(fam, group, tag, what, dev64, ref64, S):
    """an fp32 output: |dev - y64| <= A S"""
    assert not bool(torch.isnan(dev64).any()), f"{tag} {what}: an element kept its NaN"
    note(fam, group, tag, what, R.err_over_S(dev64, ref64, S))
    r = ratio(group, tag, what, R.band_ratio(dev64, ref64, S, R.A[fam]))
    assert r <= 1.0, (tag, what, r)


def banded16(fam, group, tag, what, dev64, ref64, S, measure=True):
    """a bf16 output without an fp32 twin: |dev - y64| <= ulp_bf16(y64) / 2 + A S"""
    assert not bool(torch.isnan(dev64).any()), f"{tag} {what}: an element kept its NaN"
    if measure:
        note(fam, group, tag, what, R.err_beyond_half_ulp(dev64, ref64, S))
    r = ratio(group, tag, what, R.half_ulp_ratio(dev64, ref64, S, R.A[fam]))
    assert r <= 1.0, (tag, what, r)


def traced(env, fn, force=None):
    F_ = env[0]
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = force, names
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    return out, names


def gdn_layer(env, C, inverse=False):
    from neural_image_compression_amd.layers import GDN
    g = GDN(C, inverse=inverse).to(env[3])
    return g, (g.beta_reparam.bound_value, g.gamma_reparam.bound_value, g.beta_reparam.pedestal_value)


# =============================================================================================
# a. stem
# =============================================================================================
def stem_name(C, plain=False):
    return f"stem_gdn_bf16_kernel<{C // 32}, plain>" if plain else f"stem_gdn_bf16_kernel<{C // 32}, {8 if C == 192 else 4}>"


def pack_stem(env, w, C):
    F_, FB, L, dev = env
    lib = L.load()
    wp = torch.empty((lib.lic_stem_weight_bf16_elems(C),), device=dev, dtype=BF)
    L.check(lib.lic_pack_stem_weight_bf16(ptr(w.contiguous()), ptr(wp), C, F_._stream()), "lic_pack_stem_weight_bf16")
    return wp


_GDN = {}


def gdn_operands(env, C):
    """(beta_eff, gamma_eff^T packed) of a fresh GDN(C): the pool behind the stem's convolution (not under test here)"""
    cache = _GDN.setdefault(C, {})
    if not cache:
        g, (bb, gb, pd) = gdn_layer(env, C)
        cache["ops"] = env[1]._gdn_operands_bf16(g.beta.detach(), g.gamma.detach(), bb, gb, pd, kperm=True)
        cache["layer"] = (g, (bb, gb, pd))
    return cache["ops"], cache["layer"]


def stem_direct(env, xh, wp, b, C, plain, outs=None):
    """one direct launch of lic_stem_conv_bf16 (plain) or lic_stem_gdn_bf16 into guarded NaN-filled outputs (or into the
    given [B, Ho, Wo, C] tensors) -> dict of device tensors [B, Ho, Wo, C]"""
    F_, FB, L, dev = env
    lib = L.load()
    B, H, W, _ = xh.shape
    Ho, Wo = R.stem_out(H, W)
    P = B * Ho * Wo
    keys = ("y",) if plain else ("y", "conv", "norm")
    guards = None
    if outs is None:
        guards = {k: Guarded(P, C, dev) for k in keys}
        outs = {k: g.t.view(B, Ho, Wo, C) for k, g in guards.items()}
    if plain:
        rc = lib.lic_stem_conv_bf16(ptr(xh), ptr(wp), ptr(b), ptr(outs["y"]), B, H, W, C, F_._stream())
    else:
        (beta_e, gT), _ = gdn_operands(env, C)
        rc = lib.lic_stem_gdn_bf16(ptr(xh), ptr(wp), ptr(b), ptr(gT), ptr(beta_e), ptr(outs["y"]), ptr(outs["conv"]),
                                   ptr(outs["norm"]), B, H, W, C, 0, F_._stream())
    L.check(rc, "stem launch")
    torch.cuda.synchronize()
    if guards is not None:
        for k, g in guards.items():
            g.check(f"stem {'plain' if plain else 'pooled'} {k}")
    return outs


def stem_wrapper(env, x_nchw, w, b, C):
    """FB.conv_gdn_bf16 on the same operands with a kernel trace -> (y, conv_out, norm) NHWC"""
    F_, FB, L, dev = env
    _, (g, (bb, gb, pd)) = gdn_operands(env, C)
    wr = w.clone().requires_grad_(True)

    def run():
        y = FB.conv_gdn_bf16(x_nchw, wr, b, g.beta, g.gamma, 2, 2, False, bb, gb, pd)
        _, _, conv_out, norm, _, _ = y.grad_fn.saved_tensors
        return y.detach().permute(0, 2, 3, 1), conv_out, norm
    (y, conv_out, norm), names = traced(env, run)
    assert stem_name(C) in names, names
    return y, conv_out, norm


@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_a_stem(env, case):
    F_, FB, L, dev = env
    _, C, (B, H, W) = case
    i, ref = R.inputs(case), R.forward_ref(case)
    tag = R.case_id(case)
    xh = nhwc(i["x"]).to(dev)
    w, b = i["w"].to(dev), i["b"].to(dev)
    wp = pack_stem(env, w, C)
    pooled = stem_direct(env, xh, wp, b, C, False)
    banded16("stem", "a", tag, "conv_out", nchw64(pooled["conv"]), ref.y, ref.S)
    for k in ("y", "norm"):      # the GDN half has its own tests: here only that it was written and stayed in its rows
        assert not bool(torch.isnan(pooled[k].float()).any()), f"{tag}: {k} kept a NaN"
    plain = stem_direct(env, xh, wp, b, C, True)
    banded16("stem", "a", tag, "plain", nchw64(plain["y"]), ref.y, ref.S)
    # the same template, the same K order, the same rounding of x = acc + bias: PLAIN's output is the pooled launch's conv_out
    same(plain["y"], pooled["conv"], f"{tag}: PLAIN against conv_out")
    # the traced wrapper launch of the same operands: the same bits
    y, conv_out, norm = stem_wrapper(env, xh.permute(0, 3, 1, 2), w, b, C)
    same(conv_out, pooled["conv"], f"{tag}: wrapper conv_out")
    same(y, pooled["y"], f"{tag}: wrapper y")
    if norm is not None:
        same(norm, pooled["norm"], f"{tag}: wrapper norm")


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("B,H,W", [(2, 9, 14), (3, 21, 19), (1, 7, 300), (1, 300, 1)])
def test_a_stem_exact(env, C, B, H, W):
    """bf16 ties of both parities and values just off them behind single power-of-two taps (and two-tap channels that show a
    forgotten rounding): the bits of round-to-nearest-even, whatever the summation order"""
    F_, FB, L, dev = env
    x, w = R.exact_stem(C, B, H, W)
    want = R.exact_stem_out(x, w)
    assert R.is_bf16(want)
    for wrong in (R.trunc_bf16, R.round_half_up, None):
        assert not torch.equal(want, R.exact_stem_out(x, w, wrong))
    xh, wp = nhwc(x).to(dev), pack_stem(env, w.to(dev), C)
    pooled = stem_direct(env, xh, wp, None, C, False)
    plain = stem_direct(env, xh, wp, None, C, True)
    for what, got in (("conv_out", pooled["conv"]), ("plain", plain["y"])):
        got = nchw64(got)
        bad = int((got != want).sum())
        assert bad == 0, f"stem exact C{C} {B}x{H}x{W} {what}: {bad} of {want.numel()} elements differ from rne_bf16's"
    # the traced wrapper launch of the same operands (the pooled kernel by name; PLAIN is reached by name through the head's
    # backward only, in test_b_head -- here it must equal the pooled launch's conv_out, as in test_a_stem)
    same(stem_wrapper(env, xh.permute(0, 3, 1, 2), w.to(dev), None, C)[1], pooled["conv"], f"stem exact C{C}: wrapper conv_out")
    same(plain["y"], pooled["conv"], f"stem exact C{C}: PLAIN against conv_out")


# =============================================================================================
# b. head
# =============================================================================================
def pack_head(env, w):
    """the [Cin][80] forward operand of the head (functional_bf16._ImageConvTBF16Fn.forward)"""
    F_, FB, L, dev = env
    Cin = w.shape[0]
    wd = torch.zeros((Cin, 80), device=dev, dtype=torch.float32)
    F_._permute3(w.contiguous(), wd, (Cin, 3, 25), (75, 25, 1), (80, 1, 3))
    return FB._pack_bf16(wd, 1, Cin, 80, 0, 80, 1)


def head_traced(env, xh, w, b, direct, what):
    """the traced wrapper launch of the same operands: head_convt_bf16_kernel<C / 16> by name, the direct launch's bits"""
    out, _, _, _, names = head_wrapper(env, xh, w, b, None)
    assert names == {f"head_convt_bf16_kernel<{xh.shape[3] // 16}>"}, names
    same(out, direct, f"{what}: wrapper out")


def head_direct(env, xh, wpk, b, out=None):
    F_, FB, L, dev = env
    B, Hi, Wi, C = xh.shape
    guard = None
    if out is None:
        guard = Guarded(B * Hi * Wi, 12, dev, torch.float32)          # 2 x 2 output pixels x 3 colours per feature pixel
        out = guard.t.view(B, 2 * Hi, 2 * Wi, 3)
    L.check(L.load().lic_head_convt_bf16(ptr(xh), ptr(wpk), ptr(b), ptr(out), B, Hi, Wi, C, F_._stream()), "lic_head_convt_bf16")
    torch.cuda.synchronize()
    if guard is not None:
        guard.check("head out")
    return out


def head_wrapper(env, xh, w, b, g):
    """FB.image_conv_transpose2d_bf16 forward and backward (forward only where g is None) with a kernel trace ->
    (out NHWC, dx NHWC, dw, db, names)"""
    F_, FB, L, dev = env
    tx = xh.permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), (None if b is None else b.clone().requires_grad_(True))

    def run():
        out = FB.image_conv_transpose2d_bf16(tx, wr, br, 2, 2, 1)
        if g is not None:
            out.backward(g.permute(0, 3, 1, 2))
        return out.detach().permute(0, 2, 3, 1)
    out, names = traced(env, run)
    if g is None:
        return out, None, None, None, names
    return out, tx.grad.permute(0, 2, 3, 1), wr.grad, (None if br is None else br.grad), names


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.case_id)
def test_b_head(env, case):
    F_, FB, L, dev = env
    _, C, (B, Hi, Wi) = case
    i, ref, ref0, gr = R.inputs(case), R.forward_ref(case), R.forward_ref(case, False), R.grads_ref(case)
    tag = R.case_id(case)
    xh = bf(nhwc(i["x"]), dev)
    w, b, g = i["w"].to(dev), i["b"].to(dev), nhwc(i["g"]).to(dev)
    wpk = pack_head(env, w)
    out = head_direct(env, xh, wpk, b)
    banded32("head", "b", tag, "y", nchw64(out), ref.y, ref.S)
    banded32("head", "b", tag, "y-nobias", nchw64(head_direct(env, xh, wpk, None)), ref0.y, ref0.S)
    wout, dx, dw, db, names = head_wrapper(env, xh, w, b, g)
    assert f"head_convt_bf16_kernel<{C // 16}>" in names and stem_name(C, plain=True) in names, names
    same(wout, out, f"{tag}: wrapper out")
    assert dx.dtype == BF
    banded16("stem", "b", tag, "dx", nchw64(dx), gr.dx, gr.S_dx)
    ratio("b", tag, "dw", close_norm(dw.cpu(), gr.dw, 1e-4, f"{tag} dw"))
    assert ratio("b", tag, "db", colsum_ratio(db, R.f64(i["g"]))) <= 1.0


@pytest.mark.parametrize("fam,C,B,H,W", [("head", 64, 2, 5, 33), ("head", 128, 2, 8, 31), ("head", 192, 1, 3, 65)])
def test_b_head_exact(env, fam, C, B, H, W):
    F_, FB, L, dev = env
    x, w, b = R.exact_int(fam, C, B, H, W)
    want = R.layer_ref(fam, x, w, b).y
    xh, wd, bd = bf(nhwc(x), dev), w.to(dev), b.to(dev)
    out = head_direct(env, xh, pack_head(env, wd), bd)
    got = nchw64(out)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
    head_traced(env, xh, wd, bd, out, f"head exact C{C}")


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.case_id)
def test_b_head_column_route(env, monkeypatch, case):
    """LIC_BF16_HEAD_DIRECT=0: lic_igemm_bf16 writes the [P][80] per-tap columns as bf16, lic_col2im_bf16 sums them in fp32"""
    F_, FB, L, dev = env
    _, C, (B, Hi, Wi) = case
    i, ref, gr = R.inputs(case), R.forward_ref(case), R.grads_ref(case)
    tag = R.case_id(case)
    monkeypatch.setenv("LIC_BF16_HEAD_DIRECT", "0")
    out, dx, dw, db, names = head_wrapper(env, bf(nhwc(i["x"]), dev), i["w"].to(dev), i["b"].to(dev), nhwc(i["g"]).to(dev))
    assert names and not any("head_convt" in n or "plain" in n for n in names), names
    assert all(n.startswith(("igemm_bf16_kernel", "wgrad_bf16_kernel")) for n in names), names
    got = nchw64(out)
    assert not bool(torch.isnan(got).any())
    hu = R.column_route_half_ulps(i["x"], i["w"])
    r = ratio("b", tag, "y-columns", R.column_route_ratio(got, ref.y, ref.S, hu))
    assert r <= 1.0, (tag, r)
    # its data gradient: bf16 columns of rne_bf16(g) (lic_im2col_bf16) through the implicit GEMM into a bf16 tensor
    banded16("stem", "b", tag, "dx-columns", nchw64(dx), gr.dx, gr.S_dx, measure=False)


# =============================================================================================
# c. halo kernels
# =============================================================================================
def halo_name(tr, fuse=False):
    f = "true" if fuse else "false"
    return f"halo_convt_bf16_kernel<2, {f}>" if tr else f"halo_conv_bf16_kernel<2, {f}, 0>"


class Conv:
    """device operands and geometry of a halo / halot case"""

    def __init__(self, env, case, x=None, w=None, b=None):
        F_, FB, L, dev = env
        fam, C, (B, Hi, Wi) = case
        i = R.inputs(case) if x is None else dict(x=x, w=w, b=b)
        self.fam, self.tr, self.case = fam, R.transposed(fam), case
        self.x, self.w, self.b = bf(nhwc(i["x"]), dev), i["w"].to(dev), i["b"].to(dev)
        self.B, self.Hi, self.Wi, self.Cin = self.x.shape
        self.Cout = R.HALO_COUT
        self.Ho, self.Wo = R.out_hw(fam, Hi, Wi)
        assert (self.Ho, self.Wo) == tuple(F_.conv_out_size(Hi, Wi, 5, 2, 2, self.tr, 1 if self.tr else 0))
        self.geo = dict(B=self.B, Hi=Hi, Wi=Wi, Cin=self.Cin, Ho=self.Ho, Wo=self.Wo, Cout=self.Cout, kh=5, kw=5, stride=2,
                        pad=2, transposed=self.tr)
        self.P = self.B * self.Ho * self.Wo
        self.wp = FB._pack_conv_weight_bf16(self.w, self.tr, False)


def halo_forward(env, o, out_f32, leaky=False, want=None, out=None, x=None, B=None):
    """one forward launch through FB._igemm_bf16 under HALO_FORCE into a guarded NaN-filled tensor -> device NHWC tensor"""
    F_, FB, L, dev = env
    guard = None
    geo = dict(o.geo)
    if B is not None:
        geo["B"] = B
    if out is None:
        guard = Guarded(o.P, o.Cout, dev, torch.float32 if out_f32 else BF)
        out = guard.t.view(o.B, o.Ho, o.Wo, o.Cout)
    _, names = traced(env, lambda: FB._igemm_bf16(o.x if x is None else x, o.wp, out, bias=o.b,
                                                  epilogue=L.EPI_LEAKY if leaky else L.EPI_NONE, slope=R.SLOPE, **geo), HALO_FORCE)
    assert names == {halo_name(o.tr) if want is None else want}, (R.case_id(o.case), names)
    if guard is not None:
        guard.check(R.case_id(o.case))
    return out


@pytest.mark.parametrize("case", R.HALO_CASES + R.HALOT_CASES, ids=R.case_id)
def test_c_halo_forward(env, case):
    o = Conv(env, case)
    ref = R.forward_ref(case)
    tag = R.case_id(case)
    y32 = halo_forward(env, o, True)
    banded32(o.fam, "c", tag, "y", nchw64(y32), ref.y, ref.S)
    y16 = halo_forward(env, o, False)
    assert torch.equal(nchw64(y16), R.rne_bf16(nchw64(y32))), f"{tag}: the bf16 store is not the rounded fp32 value"
    l32 = halo_forward(env, o, True, leaky=True)       # (fp32 + LEAKY: the C ABI allows it)
    banded32(o.fam, "c", tag, "leaky", nchw64(l32), R.leaky_ref(ref.y), ref.S)
    l16 = halo_forward(env, o, False, leaky=True)
    assert torch.equal(nchw64(l16), R.rne_bf16(nchw64(l32))), f"{tag}: the bf16 LeakyReLU store is not the rounded fp32 value"
    neg = float((nchw64(l32) < 0).double().mean())
    assert o.P * o.Cout < 1024 or 0.2 < neg < 0.8, neg


@pytest.mark.parametrize("fam,C,B,H,W", [("halo", 192, 2, 17, 65), ("halo", 64, 2, 1, 1), ("halot", 192, 1, 9, 33),
                                          ("halot", 128, 2, 8, 32)])
def test_c_halo_exact(env, fam, C, B, H, W):
    x, w, b = R.exact_int(fam, C, B, H, W)
    want = R.layer_ref(fam, x, w, b).y
    o = Conv(env, (fam, C, (B, H, W)), x, w, b)
    got = nchw64(halo_forward(env, o, True))
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
    assert torch.equal(nchw64(halo_forward(env, o, False)), R.rne_bf16(want))


def fused_conv_out(env, x_nchw, w, b, C, s, p, tr, op, inverse, force):
    """FB.conv_gdn_bf16 under `force` -> (conv_out NHWC bf16, names)"""
    F_, FB, L, dev = env
    g, (bb, gb, pd) = gdn_layer(env, C, inverse)
    wr = w.clone().requires_grad_(True)

    def run():
        y = FB.conv_gdn_bf16(x_nchw, wr, b, g.beta, g.gamma, s, p, inverse, bb, gb, pd, transposed=tr, output_padding=op)
        assert not bool(torch.isnan(y.float()).any())
        return y.grad_fn.saved_tensors[2]
    return traced(env, run, force)


def record_fused_equality(tag, conv_out, plain32):
    eq = bool(torch.equal(nchw64(conv_out), R.rne_bf16(nchw64(plain32))))
    FUSED_EQUALS_ROUNDED_PLAIN[tag] = eq
    print(f"BITS {tag} fused conv_out == rne_bf16(plain fp32): {eq}")
    if FUSED_CONV_IS_ROUNDED_PLAIN is not None:
        assert eq == FUSED_CONV_IS_ROUNDED_PLAIN, tag


@pytest.mark.parametrize("case", R.HALO_CASES + R.HALOT_CASES, ids=R.case_id)
def test_c_halo_fused_conv_out(env, case):
    o = Conv(env, case)
    ref = R.forward_ref(case)
    tag = R.case_id(case)
    conv_out, names = fused_conv_out(env, o.x.permute(0, 3, 1, 2), o.w, o.b, o.Cout, 2, 2, o.tr, 1 if o.tr else 0, o.tr, (512, 0, 0))
    assert halo_name(o.tr, fuse=True) in names, names
    banded16("fused", "c", tag, "conv_out", nchw64(conv_out), ref.y, ref.S)
    record_fused_equality(tag, conv_out, halo_forward(env, o, True))


@pytest.mark.parametrize("case", [c for c in R.HALO_CASES + R.HALO_DGRAD_CASES + R.HALOT_CASES if c[1] == 128], ids=R.case_id)
def test_c_halo_data_gradient(env, case):
    """FB._conv_backward_bf16 under the forced 512: the strided layer's data gradient runs halo_convt_bf16_kernel (where the
    layer's input is 2 Ho x 2 Wo, i.e. even: the transposed kernel covers output_padding 1 only), the transposed layer's
    runs halo_conv_bf16_kernel"""
    F_, FB, L, dev = env
    o = Conv(env, case)
    i, gr = R.inputs(case), R.grads_ref(case)
    tag = R.case_id(case)
    g = bf(nhwc(i["g"]), dev)
    covered = o.tr or (o.Hi % 2 == 0 and o.Wi % 2 == 0)
    want = halo_name(not o.tr) if covered else "igemm_bf16_kernel<64, 2, false, false, 3, 4>"
    dxs = {}
    for dt in (torch.float32, BF):
        (dx, _, _), names = traced(env, lambda: FB._conv_backward_bf16(o.x, o.w, g, 2, 2, o.tr, dt, 0, True, False, False), HALO_FORCE)
        assert names == {want}, (tag, names)
        assert dx.dtype == dt
        dxs[dt] = dx.detach().cpu().double()
    dfam = ("halo" if o.tr else "halot") if covered else None
    if dfam:
        banded32(dfam, "c", tag, "dx", dxs[torch.float32], gr.dx, gr.S_dx)
    else:       # the implicit GEMM: conv_bf16_ref's family, its constant
        r = ratio("c", tag, "dx-igemm", R.band_ratio(dxs[torch.float32], gr.dx, gr.S_dx))
        assert r <= 1.0
    assert torch.equal(dxs[BF], R.rne_bf16(dxs[torch.float32])), f"{tag}: the bf16 dx is not the rounded fp32 dx"


# =============================================================================================
# d. fused igemm variants, convolution part
# =============================================================================================
IGEMM_FUSED = sorted(k for k in FUSED if k.startswith("igemm_"))


@functools.lru_cache(maxsize=None)
def fused_inputs(key):
    k, s, p, ci, co, H, W, B, tr, op, inverse, bm = FUSED[key]
    r = R._rng("fused-" + key)
    x = R.to_bf16_exact(r.standard_normal((B, ci, H, W)))
    n = (9 if tr else k * k) * ci
    w = R._t(r.standard_normal((ci, co, k, k) if tr else (co, ci, k, k)) / np.sqrt(n))
    b = R._t(r.standard_normal((co,)))
    ref = R.conv_ref(x, R.rne_bf16(w), b, k, s, p, tr, op)
    assert R.check_A(R.A["fused"], ref.n)
    return x, w, b, ref


@pytest.mark.parametrize("key", IGEMM_FUSED)
def test_d_fused_igemm_conv_out(env, key):
    F_, FB, L, dev = env
    assert len(IGEMM_FUSED) == 5
    k, s, p, ci, co, H, W, B, tr, op, inverse, bm = FUSED[key]
    x, w, b, ref = fused_inputs(key)
    xd, wd, bd = bf(nhwc(x), dev).permute(0, 3, 1, 2), w.to(dev), b.to(dev)
    conv_out, names = fused_conv_out(env, xd, wd, bd, co, s, p, tr, op, inverse, (bm, 0, 0))
    bm_run = 256 if bm == 256 else 128            # (igemmh_fill: `if (fuse) BM = 128` unless 256 is forced)
    assert any(n.startswith(f"igemm_bf16_kernel<{bm_run}, {co // 64}, false, true") for n in names), names
    banded16("fused", "d", key, "conv_out", nchw64(conv_out), ref.y, ref.S)
    fn = (lambda: FB.conv_transpose2d_bf16(xd, wd, bd, s, p, op, out_f32=True)) if tr else \
        (lambda: FB.conv2d_bf16(xd, wd, bd, s, p, out_f32=True))
    with torch.no_grad():
        plain, pnames = traced(env, fn, (bm_run, 0, 1))
    assert all(n.startswith(f"igemm_bf16_kernel<{bm_run}, {co // 64}, false, false") for n in pnames) and pnames, pnames
    plain = plain.permute(0, 2, 3, 1)
    r = ratio("d", key, "plain", R.band_ratio(nchw64(plain), ref.y, ref.S))
    assert r <= 1.0
    record_fused_equality(key, conv_out, plain)


# =============================================================================================
# e. every persistent loop takes a second and a third trip
# =============================================================================================
def batch_for(env, family, tiles_per_image, C=0):
    """(B, bound): the smallest batch whose tile count exceeds twice the largest grid the launch code can choose"""
    cus = torch.cuda.get_device_properties(env[3]).multi_processor_count
    bound = 2 * R.max_workgroups_per_cu(family, C) * cus
    B = bound // tiles_per_image + 1
    assert B * tiles_per_image > bound
    return B, bound


def three(B):
    return (0, B // 2, B - 1)


@pytest.mark.parametrize("C", R.WIDTHS)
def test_e_stem_many_tiles(env, C):
    """stem: 256-thread blocks -> at most 2048 / 256 = 8 per CU, tiles > 16 CUs at 128 pixels per tile (C = 64, 128);
    512-thread blocks -> at most 4 per CU, tiles > 8 CUs at 256 pixels per tile (C = 192); PLAIN: the same bounds"""
    F_, FB, L, dev = env
    H, W = R.E_STEM_HW
    per = R.stem_tiles(C, 1, H, W)
    B, bound = batch_for(env, "stem", per, C)
    assert R.stem_tiles(C, B, H, W) == B * per > bound
    Ho, Wo = R.stem_out(H, W)
    r = R._rng(f"e-stem-{C}")
    xh = torch.as_tensor(r.random_sample((B, H, W, 3)).astype(np.float32)).to(dev)
    w = R._t(r.standard_normal((C, 3, 5, 5)) / np.sqrt(75))
    b = R._t(r.standard_normal((C,)))
    wd, bd = w.to(dev), b.to(dev)
    wp = pack_stem(env, wd, C)
    batch = {}
    for plain in (False, True):
        whole = batch[plain] = stem_direct(env, xh, wp, bd, C, plain)
        parts = {k: torch.full_like(v, float("nan")) for k, v in whole.items()}
        for n in range(B):
            stem_direct(env, xh[n:n + 1], wp, bd, C, plain, outs={k: v[n:n + 1] for k, v in parts.items()})
        for k in whole:
            same(whole[k], parts[k], f"stem C{C} {'plain' if plain else 'pooled'} {k}: the batch against its single images")
        idx = list(three(B))
        ref = R.layer_ref("stem", xh[idx].cpu().permute(0, 3, 1, 2), w, b)
        got = whole["y" if plain else "conv"][idx]
        banded16("stem", "e", f"stem-C{C}-B{B}", "plain" if plain else "conv_out", nchw64(got), ref.y, ref.S)
    # the traced wrapper launch of the batch: the pooled kernel by name, the same bits; PLAIN (reached by name through the
    # head's backward only, test_b_head) must equal the pooled launch's conv_out
    same(stem_wrapper(env, xh.permute(0, 3, 1, 2), wd, bd, C)[1], batch[False]["conv"], f"stem C{C}: wrapper conv_out")
    same(batch[True]["y"], batch[False]["conv"], f"stem C{C}: PLAIN against conv_out")


@pytest.mark.parametrize("C", R.WIDTHS)
def test_e_head_many_tiles(env, C):
    """head: 75 KB of LDS per workgroup -> at most 2 workgroups per CU, tiles > 4 CUs"""
    F_, FB, L, dev = env
    Hi, Wi = R.E_HEAD_HW
    per = R.head_tiles(1, Hi, Wi)
    B, bound = batch_for(env, "head", per)
    assert R.head_tiles(B, Hi, Wi) == B * per > bound
    r = R._rng(f"e-head-{C}")
    x = R.to_bf16_exact(r.standard_normal((B, Hi, Wi, C)))
    w = R._t(r.standard_normal((C, 3, 5, 5)) / np.sqrt(9 * C))
    b = R._t(r.standard_normal((3,)))
    xh, bd = bf(x, dev), b.to(dev)
    wpk = pack_head(env, w.to(dev))
    whole = head_direct(env, xh, wpk, bd)
    parts = torch.full_like(whole, float("nan"))
    for n in range(B):
        head_direct(env, xh[n:n + 1], wpk, bd, out=parts[n:n + 1])
    same(whole, parts, f"head C{C}: the batch against its single images")
    idx = list(three(B))
    ref = R.layer_ref("head", x[idx].permute(0, 3, 1, 2), w, b)
    banded32("head", "e", f"head-C{C}-B{B}", "y", nchw64(whole[idx]), ref.y, ref.S)
    head_traced(env, xh, w.to(dev), bd, whole, f"head C{C} batch")


@pytest.mark.parametrize("fam,C", [("halo", 128), ("halo", 64), ("halot", 64), ("halot", 128)])
def test_e_halo_many_tiles(env, fam, C):
    """halo kernels: one workgroup per CU, tiles > 2 CUs; the last chunk of a tile prefetches the next tile's first chunk
    and the weight pointer wraps"""
    F_, FB, L, dev = env
    Hi, Wi = R.E_HALO_HW if fam == "halo" else R.E_HALOT_HW
    per = (R.halo_tiles if fam == "halo" else R.halot_tiles)(1, Hi, Wi)
    B, bound = batch_for(env, fam, per)
    assert per == 4 and B * per > bound
    r = R._rng(f"e-{fam}-{C}")
    x = R.to_bf16_exact(r.standard_normal((B, C, Hi, Wi)))
    w = R._t(r.standard_normal((C, 128, 5, 5) if fam == "halot" else (128, C, 5, 5)) / np.sqrt((9 if fam == "halot" else 25) * C))
    b = R._t(r.standard_normal((128,)))
    o = Conv(env, (fam, C, (B, Hi, Wi)), x, w, b)
    whole = halo_forward(env, o, True)
    parts = torch.full_like(whole, float("nan"))
    for n in range(B):
        halo_forward(env, o, True, out=parts[n:n + 1], x=o.x[n:n + 1], B=1)
    same(whole, parts, f"{fam} C{C}: the batch against its single images")
    idx = list(three(B))
    ref = R.layer_ref(fam, x[idx], w, b)
    banded32(fam, "e", f"{fam}-C{C}-B{B}", "y", nchw64(whole[idx]), ref.y, ref.S)
    # the bf16 store on the later trips too
    assert torch.equal(halo_forward(env, o, False).float(), whole.to(BF).float())


# =============================================================================================
# f. refusals launch nothing
# =============================================================================================
def test_f_stem_and_head_refusals(env):
    F_, FB, L, dev = env
    lib = L.load()
    st = F_._stream()
    B, H, W, C = 2, 6, 8, 64
    x = torch.rand((B, H, W, 3), device=dev)
    wp = pack_stem(env, torch.randn((C, 3, 5, 5), device=dev), C)
    wp96 = torch.zeros((lib.lic_stem_weight_bf16_elems(96),), device=dev, dtype=BF)
    (beta_e, gT), _ = gdn_operands(env, C)
    out = Guarded(B * 3 * 4, 192, dev)                 # room for every width tried here
    y = out.t

    def stem_gdn(xp=ptr(x), wq=ptr(wp), yp=ptr(y), cp=ptr(y), b=B, h=H, w=W, c=C):
        return lib.lic_stem_gdn_bf16(xp, wq, None, ptr(gT), ptr(beta_e), yp, cp, None, b, h, w, c, 0, st)

    def stem_conv(xp=ptr(x), wq=ptr(wp), yp=ptr(y), b=B, h=H, w=W, c=C):
        return lib.lic_stem_conv_bf16(xp, wq, None, yp, b, h, w, c, st)
    for fn in (stem_gdn, stem_conv):
        assert fn(c=96, wq=ptr(wp96)) == ERR_UNSUPPORTED
        assert fn(yp=ptr(y, 2)) == ERR_INVALID and fn(yp=ptr(y, 8)) == ERR_INVALID
        assert fn(wq=ptr(wp, 2)) == ERR_INVALID
        assert fn(b=0) == ERR_INVALID and fn(h=0) == ERR_INVALID and fn(w=0) == ERR_INVALID
        assert fn(xp=None) == ERR_INVALID and fn(yp=None) == ERR_INVALID
    assert stem_gdn(cp=ptr(y, 2)) == ERR_INVALID
    assert not bool(lib.lic_stem_gdn_bf16_supported(3, 96, 5, 5, 2, 2))
    # head: x and w_packed must be 16-byte aligned (its fp32 output only 4-byte)
    Hi, Wi = 3, 5
    xh = torch.randn((B, Hi, Wi, C), device=dev).to(BF)
    wpk = pack_head(env, torch.randn((C, 3, 5, 5), device=dev))
    ho = Guarded(B * Hi * Wi, 12, dev, torch.float32)

    def head(xp=ptr(xh), wq=ptr(wpk), op=ptr(ho.t), b=B, h=Hi, w=Wi, c=C):
        return lib.lic_head_convt_bf16(xp, wq, None, op, b, h, w, c, st)
    assert head(c=96) == ERR_UNSUPPORTED
    assert head(xp=ptr(xh, 2)) == ERR_INVALID and head(wq=ptr(wpk, 2)) == ERR_INVALID and head(op=ptr(ho.t, 2)) == ERR_INVALID
    assert head(b=0) == ERR_INVALID and head(h=0) == ERR_INVALID and head(w=0) == ERR_INVALID
    assert head(op=None) == ERR_INVALID
    assert not bool(lib.lic_head_convt_bf16_supported(96, 3, 5, 5, 2, 2, 1))
    torch.cuda.synchronize()
    assert out.untouched() and ho.untouched(), "a refused launch wrote its output"
    # (and the calls that are accepted, so that the refusals above are not refusals of everything)
    assert stem_conv() == 0 and head() == 0
    torch.cuda.synchronize()
    out.check("accepted stem")
    ho.check("accepted head")
    assert not out.untouched() and not bool(torch.isnan(ho.t).any())


def test_f_forced_halo_on_a_shape_it_does_not_cover(env):
    """FORCE_IGEMM = (512, 0, 1) at Cout = 64: the halo kernels cover 128 output channels only, the launch keeps its
    automatic implicit-GEMM tile"""
    F_, FB, L, dev = env
    r = R._rng("f-halo-64")
    B, Cin, Hi, Wi, Cout = 2, 64, 17, 21, 64
    x = R.to_bf16_exact(r.standard_normal((B, Cin, Hi, Wi)))
    w = R._t(r.standard_normal((Cout, Cin, 5, 5)) / 40.0)
    b = R._t(r.standard_normal((Cout,)))
    ref = R.conv_ref(x, R.rne_bf16(w), b, 5, 2, 2)
    Ho, Wo = R.out_hw("halo", Hi, Wi)
    out = Guarded(B * Ho * Wo, Cout, dev, torch.float32)
    view = out.t.view(B, Ho, Wo, Cout)
    wp = FB._pack_conv_weight_bf16(w.to(dev), False, False)
    _, names = traced(env, lambda: FB._igemm_bf16(bf(nhwc(x), dev), wp, view, bias=b.to(dev), B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho,
                                                  Wo=Wo, Cout=Cout, kh=5, kw=5, stride=2, pad=2, transposed=False), HALO_FORCE)
    assert names == {"igemm_bf16_kernel<64, 1, false, false, 3, 4>"}, names
    out.check("forced 512 at Cout = 64")
    r_ = ratio("f", "halo-Cout64", "y", R.band_ratio(nchw64(view), ref.y, ref.S))
    assert r_ <= 1.0


# =============================================================================================
# g. the fp32 RGB route
# =============================================================================================
def banded_rgb32(tag, what, dev64, ref64, S):
    assert not bool(torch.isnan(dev64).any())
    note("rgb32", "g", tag, what, R.err_over_S(dev64, ref64, S))
    r = ratio("g", tag, what, R.band_ratio(dev64, ref64, S, R.A32))
    assert r <= 1.0, (tag, what, r)


@pytest.mark.parametrize("case", R.STEM_CASES + R.HEAD_CASES, ids=R.case_id)
def test_g_fp32_rgb_route(env, case):
    """im2col + igemm (+ col2im) in fp32 on the UNROUNDED operands"""
    F_, FB, L, dev = env
    fam = case[0]
    i, ref, gr = R.inputs(case), R.forward_ref_fp32(case), R.grads_ref_fp32(case)
    tag = R.case_id(case)
    x = nhwc(i["x"]).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    w, b, g = i["w"].to(dev), i["b"].to(dev), nhwc(i["g"]).to(dev).permute(0, 3, 1, 2)

    def run():
        y = F_.image_conv2d(x, w, b, 2, 2) if fam == "stem" else F_.image_conv_transpose2d(x, w, b, 2, 2, 1)
        y.backward(g)
        return y.detach()
    y, names = traced(env, run)
    assert y.dtype == torch.float32 and x.grad.dtype == torch.float32
    assert not any("bf16" in n for n in names), names
    banded_rgb32(tag, "y", y.cpu().double(), ref.y, ref.S)
    banded_rgb32(tag, "dx", x.grad.cpu().double(), gr.dx, gr.S_dx)
