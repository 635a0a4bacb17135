"""The layers of the 3x3 residual model (HierarchicalMixtureResidual's Encoder3x3 / Decoder3x3 / HyperEncoder3x3 /
HyperDecoder3x3) in bf16 storage and in fp32 against tests/resblock_ref.py, the float64 statement of the same layers at
the device's rounding points.  The bands and their constants are derived in resblock_ref.py.

  a. the bf16 implicit-GEMM layers no 5x5 case reaches (3x3 stride-2 transposed with output_padding 1 at M -> M and
     1.5M -> 1.5M, plain and with the fused LeakyReLU; the 1x1 stride-2 skip; the 3x3 stride-2 layer with an fp32 output;
     3x3 M -> 1.5M), with the automatic plan, BM forced to 64 / 128 / 256 and the K split forced off and to 3: forward fp32
     banded and bf16 bit for bit its rounding; the LeakyReLU's backward bit for bit from the device's own stored output;
     data gradient, weight gradient per tap, bias gradient; the kernel variant and K split of every launch asserted;
  b. the RGB stem at k = 3 s = 2 p = 1 (Kp = 32) and k = 1 s = 2 p = 0 (Kp = 8): lic_im2col_bf16's column matrix bit for bit
     (im2col_vec_kernel<bf16_t, 8>, and im2col_bf16_kernel behind a column pointer that is not 16-byte aligned), the
     output banded on images that are not bf16-exact, the weight gradient on the immediate and the deferred route bit-equal
     and held to float64, the bias gradient;
  c. the RGB head at k = 3 s = 2 p = 1 op = 1: always the column route ([P][32] bf16 columns, col2im_fast_kernel<bf16_t>):
     forward banded and bit for bit on small integers, data gradient into bf16 and fp32 inputs, weight gradient immediate
     and deferred, bias gradient, lic_col2im_bf16 alone;
  d. the fused conv -> GDN / IGDN launch at 3x3 s1 p1, M = 64 / 128 / 192: conv_out, y and the stored norm from the kernel's
     own conv output; the backward bit for bit the explicit GDN-backward + conv-backward composition;
  e. the residual blocks as modules in bf16: every intermediate of the explicit composition held to the reference applied
     to the device's own previous tensor, the skip add and the two-branch gradient sum bit for bit their stated rounding,
     the module bit for bit the composition, FUSE_CONV_GDN on and off;
  f. the blocks in fp32, TransposedDeconv3x3(M, 3) among them: every intermediate against float64 from the device's
     previous tensor, the module bit for bit the composition, gradients against float64 autograd;
  g. the four stacks at M = 64 on one 64 x 64 image in bf16: bit for bit the block-by-block composition
     (LatentSpaceTransform has no bf16 route: it is held in fp32, against float64 and its own blocks);
  h. refusals launch nothing.

Every output of a direct launch is a view inside a NaN-filled allocation whose neighbouring rows are checked.  Every
figure is printed as `RATIO <group> <case> <what> <value>` before it is asserted; `ERRS` lines carry the raw err / S.

Kernel variants a trace of this module shows: igemm_bf16_kernel<64, 1 | 2 | 3, false, false, 3, 4>,
<128, 1 | 2, false, false, 4, 4>, <128, 3, false, false, 3, 4>, <256, 1 | 2 | 3, false, false, 4, 8>, the fused
<128, 1 | 2, false, true, 4, 4> and <128, 3, false, true, 3, 4>, the GDN pool <64, 1 | 3, true, false, 3, 4>,
wgrad_bf16_kernel<1 | 2 | 3, 1 | 2 | 3, false> and <1, 1, true>, <2, 2, true>, <3, 3, true>, gdn_bwd_bf16_kernel<2 | 4>; in fp32 igemm_kernel<64 | 128, 1, true, true, false, true> and gdn_kernel<1 | 3, 0 | 1>.  No
head_convt_bf16_kernel and no halo kernel: the 3x3 head always takes the column route.

Measured on the MI355X: worst err / S  igemm 1.709e-07 (a, data gradient of hd_c at M = 192, 1 x 13 x 20)
igemm_split 1.168e-07   stem3 4.215e-08   skip_rgb 0   head3 1.053e-07   fused 1.191e-07 (bf16-only outputs: beyond the
store's half ulp); A = 2^-20 = 9.54e-07 for all but skip_rgb (n = 3: the derived 2^-21).  Worst RATIO per group, each
against a bound of 1:

    a  igemm layers   y 0.114 (up_l M192 2x9x7)   dx 0.179 (hd_c M192 1x13x20)   dx split 0.122   dw element-wise 0.388
                      (hd_up2 M192 2x1x1)   db 0.005   every bf16 output and masked gradient bit for bit
    b  RGB stem       columns bit for bit, both kernels   y 0.9998 of half a bf16 ulp + A S   dw 0.158   db 0.001
                      immediate and deferred weight gradients bit-equal
    c  RGB head       y 0.997 of the column-route band   dx32 0.110, dx16 bit for bit its rounding   dw 0.197   db 0.004
                      col2im alone 0.100   exact integer cases bit for bit
    d  fused 3x3      conv_out 0.9997   y 0.999   norm 0.997   dx (fp32 twin) 0.122, bf16 bit for bit its rounding
                      dw 0.015   backward bit for bit the composition
    e  blocks, bf16   stores without an fp32 twin (c1, conv_out, identity) <= 0.9997 of half a bf16 ulp + A S; stores
                      behind a fused LeakyReLU and the skip's data gradient through their fp32 twins: h1 0.085, main
                      0.138, dx-skip 0.080, bf16 bit for bit the rounding; skip add, gradient sum, module against
                      composition: bit for bit
    f  blocks, fp32   stages <= 0.237 of A S   head y 0.120, dx 0.213, dw 0.141   gradients <= 0.009 of the 1e-4 band
                      module against composition bit for bit
    g  stacks         bit for bit their blocks

ONE BUG FOUND, in the Python route (reductions.can_defer), by group e: torch.autograd.grad(y, [x]) on a block left the
weight-gradient reductions of its layers pending although the engine drops those gradients at once; at the end of the
pass lic_reduce_batch wrote conv2's weight gradient into freed memory that by then held conv1's data gradient (NaNs and
1e19s in x's gradient).  can_defer now asks the engine whether the parameter's AccumulateGrad node will run.  No kernel
error was found: no bf16 store differed from its rounded fp32 value in any variant.

Run on the MI355X box:  python -m pytest tests/test_gpu_resblocks.py -m gpu -q -s"""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16_reduce_ref as RR
import conv_ref64 as C64
import gdn_bf16_ref as G
import gdn_ref64 as G64
import golden_recipe as GR
import resblock_ref as R
from test_gpu_gdn_bf16 import CANARY16, Guarded, bits
from test_gpu_latent_bf16 import (Ops, backward, bf, check_dw_db, colsum_ratio, forward, nchw64, nhwc,
                                  same_bits_as_rounded, traced)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FORCES = (None, (64, 0, 1), (128, 0, 1), (256, 0, 1), (0, 0, 3))
ERRS = {k: 0.0 for k in R.A_MEASURED}
WORST = {}
VARIANTS = set()


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
    key = (group, what)
    if value > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (value, tag)
    return value


def note(fam, group, tag, what, e):
    ERRS[fam] = max(ERRS[fam], e)
    print(f"ERRS {group} {tag} {what} {fam} {e:.3e}")


def ptr(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def banded32(fam, group, tag, what, dev64, ref64, S, A):
    assert not bool(torch.isnan(dev64).any()), f"{tag} {what}: an element kept its NaN"
    note(fam, group, tag, what, R.err_over_S(dev64, ref64, S))
    r = ratio(group, tag, what, R.band_ratio(dev64, ref64, S, A))
    assert r <= 1.0, (tag, what, r)


def banded16(fam, group, tag, what, dev64, ref64, S, A, measure=True):
    assert not bool(torch.isnan(dev64).any()), f"{tag} {what}: an element kept its NaN"
    if measure:
        note(fam, group, tag, what, R.err_beyond_half_ulp(dev64, ref64, S))
    r = ratio(group, tag, what, R.half_ulp_ratio(dev64, ref64, S, A))
    assert r <= 1.0, (tag, what, r)


def to64(t):
    """an NCHW-logical device tensor -> float64 NCHW on the CPU"""
    return t.detach().float().cpu().double().contiguous()


def same(a, b, what):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    n = int((bits(a) != bits(b)).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ"


def is_ref(dev, ref64, what):
    """a bf16 device tensor holds exactly these float64 (bf16-exact) values"""
    got = to64(dev)
    n = int((got != ref64).sum())
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ from the stated rounding"


class Ops3(Ops):
    """test_gpu_latent_bf16.Ops on a case of resblock_ref"""

    def __init__(self, env, case):
        F_, FB, L, dev = env
        i = R.inputs(case)
        self.case, self.lay, self.i = case, i["lay"], i
        lay = self.lay
        self.x = bf(nhwc(i["x"]), dev)
        self.g = bf(nhwc(i["g"]), dev)
        self.w, self.b = i["w"].to(dev), i["b"].to(dev)
        self.B, self.Hi, self.Wi, _ = self.x.shape
        self.Ho, self.Wo = i["Ho"], i["Wo"]
        assert (self.Ho, self.Wo) == tuple(F_.conv_out_size(self.Hi, self.Wi, lay.k, lay.s, lay.p, lay.transposed, lay.op))
        self.geo = dict(B=self.B, Hi=self.Hi, Wi=self.Wi, Cin=lay.cin, Ho=self.Ho, Wo=self.Wo, Cout=lay.cout, kh=lay.k,
                        kw=lay.k, stride=lay.s, pad=lay.p, transposed=lay.transposed)
        self.chunks = R.CB.max_chunks(lay.k, lay.s, lay.transposed, 0, lay.cin, lay.p)
        self.chunks_dx = R.CB.max_chunks(lay.k, lay.s, not lay.transposed, 0, lay.cout, lay.p)
        self.P = self.B * self.Ho * self.Wo


def ftag(case, force):
    return R.case_id(case) + ("-auto" if force is None else f"-bm{force[0]}-s{force[2]}")


def layer_wgrad_plan(o):
    """(pixels summed, K split) of the layer's weight gradient as functional_bf16._conv_backward_bf16 launches it"""
    lay = o.lay
    if lay.transposed:
        d = SimpleNamespace(B=o.B, Hs=o.Hi, Ws=o.Wi, Cp=lay.cin, Cg=lay.cout, kh=lay.k, kw=lay.k, g_is_row=0)
    else:
        d = SimpleNamespace(B=o.B, Hs=o.Ho, Ws=o.Wo, Cp=lay.cout, Cg=lay.cin, kh=lay.k, kw=lay.k, g_is_row=1)
    return d.B * d.Hs * d.Ws, RR.plan_ref(d)[2]


# =============================================================================================
# a. the bf16 implicit-GEMM layers
# =============================================================================================
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_a_forward(env, case):
    o = Ops3(env, case)
    lay = o.lay
    ref = R.forward_ref(case)
    want = R.leaky_ref(ref.y) if lay.leaky else ref.y
    A = R.band_A(ref.n)
    splits = set()
    for force in FORCES:
        tag = ftag(case, force)
        y32, ks = forward(env, o, force, True, lay.leaky)
        splits.add(ks)
        banded32("igemm" if ks == 1 else "igemm_split", "a", tag, "y" if ks == 1 else "y-split", y32, want, ref.S, A)
        y16, ks16 = forward(env, o, force, False, lay.leaky)
        assert ks16 == ks
        same_bits_as_rounded(y16, y32, tag)
    VARIANTS.update(R.CB.expected_kernel(lay.cout, f[0] if f else 0) for f in FORCES)
    if o.chunks >= 2:
        assert max(splits) > 1, (splits, o.chunks)      # (the forced split ran as a split)
    if lay.transposed:      # the four output phases gather 1, 2, 2 and 4 taps: every one of them has elements here
        assert (o.Ho, o.Wo) == (2 * o.Hi, 2 * o.Wi)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_a_backward(env, case):
    F_, FB, L, dev = env
    from neural_image_compression_amd.reductions import _leaky_bwd_colsum_bf16
    o = Ops3(env, case)
    lay = o.lay
    tag = R.case_id(case)
    y_dev = None
    g64 = R.f64(o.i["g"])
    if lay.leaky:
        wp = FB._pack_conv_weight_bf16(o.w, lay.transposed, False)
        y_dev = torch.empty((o.B, o.Ho, o.Wo, lay.cout), device=dev, dtype=BF)
        FB._igemm_bf16(o.x, wp, y_dev, bias=o.b, epilogue=L.EPI_LEAKY, slope=R.SLOPE, **o.geo)
        g1, db1 = _leaky_bwd_colsum_bf16(y_dev, o.g, R.SLOPE, o.P, lay.cout)
        g2 = FB._leaky_bwd_bf16(y_dev, o.g, R.SLOPE)
        torch.cuda.synchronize()
        gq = R.leaky_bwd_ref(nchw64(y_dev), g64)
        assert torch.equal(nchw64(g1), gq), f"{tag}: the one-pass route's masked gradient"
        assert torch.equal(nchw64(g2), gq), f"{tag}: leaky_bwd_bf16_kernel's masked gradient"
        assert ratio("a", tag, "db-onepass", colsum_ratio(db1, gq)) <= 1.0
        g64 = gq
    gr = R.grads_ref(case, g64)
    A = R.band_A(gr.n_dx)
    first = None
    for force in FORCES:
        t = ftag(case, force)
        dx32, dw, db, ks = backward(env, o, force, torch.float32, (True, True, True), leaky_y=y_dev)
        banded32("igemm" if ks == 1 else "igemm_split", "a", t, "dx" if ks == 1 else "dx-split", dx32, gr.dx, gr.S_dx, A)
        dx16, _, _, _ = backward(env, o, force, BF, (True, False, False), leaky_y=y_dev)
        same_bits_as_rounded(dx16, dx32, t + " dx")
        if first is None:
            first = dw
            check_dw_db("a", t, case, dw, db, gr, g64)
            # and element by element at the contraction's own bound
            P, sk = layer_wgrad_plan(o)
            r = ratio("a", t, "dw-elementwise", R.wgrad_ratio(dw, gr.dw, R.wgrad_weight(o.i["x"], g64, lay), P, sk))
            assert r <= 1.0, (t, r)
        else:
            assert torch.equal(first, dw), "the weight gradient does not depend on the data gradient's plan"


# =============================================================================================
# b. the RGB stem
# =============================================================================================
def run_im2col(env, x_nhwc, lay, Ho, Wo, Kp, misalign=False):
    """lic_im2col_bf16 called directly into a canary-filled buffer -> [P][Kp] bf16 (a copy), the surroundings checked.
    misalign: the column pointer 2 bytes past a 16-byte boundary (im2col_bf16_kernel)"""
    F_, FB, L, dev = env
    B, H, W, C = x_nhwc.shape
    P = B * Ho * Wo
    lead = 64 + (1 if misalign else 0)
    raw = torch.full((lead + P * Kp + 64,), CANARY16, dtype=torch.int16, device=dev)
    col = raw[lead:lead + P * Kp]
    assert (col.data_ptr() % 16 != 0) == misalign
    L.check(L.load().lic_im2col_bf16(ptr(x_nhwc), ptr(col), B, H, W, C, Ho, Wo, lay.k, lay.k, lay.s, lay.p, Kp, F_._stream()),
            "lic_im2col_bf16")
    torch.cuda.synchronize()
    assert bool((raw[:lead] == CANARY16).all()) and bool((raw[lead + P * Kp:] == CANARY16).all()), "wrote outside the columns"
    return col.view(BF).view(P, Kp).clone()


def defer_calls(env, fn):
    """run fn() counting the reductions it leaves pending (functional.defer)"""
    F_ = env[0]
    n = [0]
    orig = F_.defer

    def counting(*a, **k):
        n[0] += 1
        return orig(*a, **k)
    F_.defer = counting
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        F_.defer = orig
    return out, n[0]


def both_routes(env, run):
    """run(): a forward + backward through autograd returning its gradients -> (deferred result, immediate result); the
    deferred run must have left reductions pending and the immediate one none"""
    from neural_image_compression_amd import reductions as RD
    assert RD.DEFER_REDUCTIONS is True
    d, nd = defer_calls(env, run)
    RD.DEFER_REDUCTIONS = False
    try:
        i, ni = defer_calls(env, run)
    finally:
        RD.DEFER_REDUCTIONS = True
    assert nd > 0 and ni == 0, (nd, ni)
    return d, i


def wgrad_splitk(Cp, Cg, P):
    d = SimpleNamespace(B=1, Hs=1, Ws=P, Cp=Cp, Cg=Cg, kh=1, kw=1, g_is_row=0)
    return RR.plan_ref(d)[2]


@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_b_stem(env, case):
    F_, FB, L, dev = env
    role, M, _, (B, H, W) = case
    i, ref, gr = R.inputs(case), R.forward_ref(case), R.grads_ref(case)
    lay = i["lay"]
    tag = R.case_id(case)
    Kp, K = R.kpad8(lay.k, 3), lay.k * lay.k * 3
    assert (Kp, K) == ((32, 27) if role == "stem3" else (8, 3))
    Ho, Wo = i["Ho"], i["Wo"]
    xh = nhwc(i["x"]).to(dev)
    # the column matrix itself
    want = R.im2col_ref(i["x"], lay.k, lay.s, lay.p, Kp)
    for misalign in (False, True):
        col = run_im2col(env, xh, lay, Ho, Wo, Kp, misalign)
        got = col.float().cpu().double()
        bad = int((got != want).sum())
        assert bad == 0, f"{tag} im2col misalign={misalign}: {bad} of {want.numel()} elements differ"
        assert not bool(got[:, K:].any()) and not bool(torch.signbit(col[:, K:].float()).any()), "padding columns not +0"
    # the layer
    x = xh.permute(0, 3, 1, 2)
    g = bf(nhwc(i["g"]), dev).permute(0, 3, 1, 2)
    A = R.band_A(ref.n)

    def run():
        w, b = i["w"].to(dev).requires_grad_(True), i["b"].to(dev).requires_grad_(True)
        y = FB.image_conv2d_bf16(x, w, b, lay.s, lay.p)
        y.backward(g)
        return y.detach(), w.grad, b.grad
    ((y, dw, db), (y2, dw2, db2)), names = traced(env, None, lambda: both_routes(env, run))
    VARIANTS.update(names)
    assert R.CB.expected_kernel(lay.cout) in names and any(n.startswith("wgrad_bf16_kernel") for n in names), names
    assert y.dtype == BF and tuple(y.shape) == (B, M, Ho, Wo)
    banded16(role, "b", tag, "y", to64(y), ref.y, ref.S, A)
    same(y, y2, f"{tag} y of the two runs")
    same(dw, dw2, f"{tag} dw deferred against immediate")
    same(db, db2, f"{tag} db deferred against immediate")
    P = B * Ho * Wo
    xq, _, gq = R.rounded_operands(case)
    r = ratio("b", tag, "dw", R.wgrad_ratio(dw.cpu(), gr.dw, R.wgrad_weight(xq, gq, lay), P, wgrad_splitk(Kp, M, P)))
    assert r <= 1.0, (tag, r)
    assert ratio("b", tag, "db", colsum_ratio(db, gq)) <= 1.0


# =============================================================================================
# c. the RGB head
# =============================================================================================
def head_run(env, x, w, b, g=None, x_dtype=BF):
    """FB.image_conv_transpose2d_bf16 (3x3 s2 p1 op1) forward (and backward) -> (out, dx, dw, db)"""
    F_, FB, L, dev = env
    tx = (x if x_dtype == BF else x.float()).detach().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = FB.image_conv_transpose2d_bf16(tx, wr, br, 2, 1, 1)
    if g is None:
        return out.detach(), None, None, None
    out.backward(g)
    return out.detach(), tx.grad, wr.grad, br.grad


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.case_id)
def test_c_head(env, case):
    F_, FB, L, dev = env
    _, M, _, (B, Hi, Wi) = case
    i, ref, gr = R.inputs(case), R.forward_ref(case), R.grads_ref(case)
    lay = i["lay"]
    tag = R.case_id(case)
    assert L.load().lic_head_convt_bf16_supported(M, 3, 3, 3, 2, 1, 1) == 0 and not FB._head_direct(M, 3, 3, 3, 2, 1, 1)
    x = bf(nhwc(i["x"]), dev).permute(0, 3, 1, 2)
    w, b = i["w"].to(dev), i["b"].to(dev)
    g = nhwc(i["g"]).to(dev).permute(0, 3, 1, 2)
    ((out, dx, dw, db), (out2, dx2, dw2, db2)), names = traced(env, None, lambda: both_routes(env, lambda: head_run(env, x, w, b, g)))
    VARIANTS.update(names)
    assert names and not any("head_convt" in n or "plain" in n for n in names), names
    assert all(n.startswith(("igemm_bf16_kernel", "wgrad_bf16_kernel")) for n in names), names
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, 2 * Hi, 2 * Wi)
    got = to64(out)
    assert not bool(torch.isnan(got).any())
    hu = R.column_route_half_ulps(i["x"], i["w"], 3, 2, 1, 1)
    note("head3", "c", tag, "y-columns", float((((got - ref.y).abs() - hu).clamp_min(0) / ref.S.clamp_min(1e-300)).max()))
    r = ratio("c", tag, "y-columns", R.column_route_ratio(got, ref.y, ref.S, hu))
    assert r <= 1.0, (tag, r)
    # data gradient: bf16 columns of rne_bf16(g) through the implicit GEMM, into a bf16 and into an fp32 input
    A = R.band_A(gr.n_dx)
    assert dx.dtype == BF
    _, dx32, dw32, _ = head_run(env, x, w, b, g, torch.float32)
    torch.cuda.synchronize()
    assert dx32.dtype == torch.float32
    banded32("head3", "c", tag, "dx32", to64(dx32), gr.dx, gr.S_dx, A)
    same(dx.float(), R.rne_bf16(to64(dx32)).float().to(dx.device), f"{tag} dx16 against the rounded dx32")
    same(dw32, dw, f"{tag} dw does not depend on the input's type")
    # weight gradient: immediate and deferred bit-equal, one of them held to float64; bias gradient
    same(out, out2, f"{tag} out of the two runs")
    same(dx, dx2, f"{tag} dx of the two runs")
    same(dw, dw2, f"{tag} dw deferred against immediate")
    same(db, db2, f"{tag} db deferred against immediate")
    P = B * Hi * Wi
    xq, _, gq = R.rounded_operands(case)
    r = ratio("c", tag, "dw", R.wgrad_ratio(dw.cpu(), gr.dw, R.wgrad_weight(xq, gq, lay), P, wgrad_splitk(M, 32, P)))
    assert r <= 1.0, (tag, r)
    assert ratio("c", tag, "db", colsum_ratio(db, R.f64(i["g"]))) <= 1.0


@pytest.mark.parametrize("M,B,H,W", [(64, 2, 5, 7), (128, 1, 9, 6), (192, 2, 3, 5)])
def test_c_head_exact(env, M, B, H, W):
    """small integers, eight live input channels per (tap, colour): every column value is an integer of at most 48 -- exact
    in bf16 -- and every sum exact in fp32, so the column route must give the float64 result bit for bit"""
    F_, FB, L, dev = env
    r = R._rng(f"head3-exact-{M}-{B}-{H}-{W}")
    x = torch.as_tensor(r.randint(-3, 4, size=(B, M, H, W)).astype(np.float32))
    w = np.zeros((M, 3, 3, 3), np.float32)
    for c in range(3):
        for t in range(9):
            ci = r.choice(M, 8, replace=False)
            w[ci, c, t // 3, t % 3] = r.randint(-2, 3, size=8)
    w = torch.as_tensor(w)
    b = torch.as_tensor(r.randint(-4, 5, size=3).astype(np.float32))
    want = R.conv_ref(x, w, b, 3, 2, 1, True, 1).y
    (out, _, _, _), names = traced(env, None, lambda: head_run(env, bf(nhwc(x), dev).permute(0, 3, 1, 2), w.to(dev), b.to(dev)))
    assert not any("head_convt" in n for n in names), names
    got = to64(out)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("B,Hi,Wi", [(2, 9, 7), (1, 1, 1), (1, 13, 20)])
def test_c_col2im_alone(env, B, Hi, Wi):
    """lic_col2im_bf16 on a given bf16 [P][32] column matrix (the five padding columns hold NaN: they must not be read)
    against the float64 scatter, with bias and without; at most 4 terms and the bias per element"""
    F_, FB, L, dev = env
    r = R._rng(f"col2im-{B}-{Hi}-{Wi}")
    P, Kp = B * Hi * Wi, 32
    colv = R.to_bf16_exact(r.standard_normal((P, Kp)))
    bias = torch.as_tensor(r.standard_normal(3).astype(np.float32))
    cold = colv.to(BF).to(dev)
    cold[:, 27:] = float("nan")
    Ho, Wo = 2 * Hi, 2 * Wi
    for bz in (None, bias):
        out = Guarded(B * Hi * Wi, 12, dev, torch.float32)      # 2 x 2 output pixels x 3 colours per feature pixel
        bd = None if bz is None else bz.to(dev)
        L.check(L.load().lic_col2im_bf16(ptr(cold), ptr(bd), ptr(out.t), B, Hi, Wi, 3, Ho, Wo, 3, 3, 2, 1, Kp, F_._stream()),
                "lic_col2im_bf16")
        torch.cuda.synchronize()
        out.check("col2im out")
        ref, S = R.col2im_ref(colv, bz, B, Hi, Wi, 3, 3, 2, 1, 1)
        got = out.t.reshape(B, Ho, Wo, 3).cpu().permute(0, 3, 1, 2).double()
        tag = f"{B}x{Hi}x{Wi}-{'bias' if bz is not None else 'nobias'}"
        r_ = ratio("c", tag, "col2im", R.band_ratio(got, ref, S, R.band_A(4)))
        assert r_ <= 1.0, (tag, r_)


# =============================================================================================
# d. the fused conv -> GDN / IGDN launch at 3x3 stride 1 padding 1
# =============================================================================================
def gdn_module(env, C, inverse, seed):
    from neural_image_compression_amd.layers import GDN
    m = GDN(C, inverse=inverse).to(env[3])
    with torch.no_grad():
        m.beta.copy_(torch.from_numpy(GR.make_param(f"{seed}.beta", (C,), 3)))
        m.gamma.copy_(torch.from_numpy(GR.make_param(f"{seed}.gamma", (C, C), 3)))
    return m, (m.beta_reparam.bound_value, m.gamma_reparam.bound_value, m.beta_reparam.pedestal_value)


def gdn_effective(env, m, gp):
    """the re-parametrised operands as the device formed them (the re-parametrisation has its own tests)"""
    FB = env[1]
    return FB._gamma_eff(m.beta.detach(), gp[0], gp[2]).cpu(), FB._gamma_eff(m.gamma.detach(), gp[1], gp[2]).cpu()


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("M", R.WIDTHS)
@pytest.mark.parametrize("grid", R.FUSED_GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_d_fused_conv_gdn(env, M, inverse, grid):
    F_, FB, L, dev = env
    B, H, W = grid
    tag = f"M{M}-{'igdn' if inverse else 'gdn'}-{B}x{H}x{W}"
    i = R.fused_inputs(M, inverse, grid)
    x, w, b, g = i["x"], i["w"], i["b"], i["g"]
    m, gp = gdn_module(env, M, inverse, "fused3")
    assert FB.fused_gdn_supported_bf16(M, M)
    xd = bf(nhwc(x), dev).permute(0, 3, 1, 2).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    gd = bf(nhwc(g), dev).permute(0, 3, 1, 2)

    def run():
        y = FB.conv_gdn_bf16(xd, wd, bd, m.beta, m.gamma, 1, 1, inverse, *gp)
        _, _, conv_out, norm, _, _ = y.grad_fn.saved_tensors
        y.backward(gd)
        return y.detach(), conv_out, norm
    (y, conv_out, norm), names = traced(env, None, run)
    VARIANTS.update(names)
    assert any(n.startswith("igemm_bf16_kernel<") and n.split(", ")[3] == "true" for n in names), names
    assert conv_out is not None and conv_out.dtype == BF and (norm is not None) == (not FB.norm_recomputed_bf16(M))
    ref = R.conv_ref(x, R.rne_bf16(w), b, 3, 1, 1)
    banded16("fused", "d", tag, "conv_out", nchw64(conv_out), ref.y, ref.S, R.band_A(ref.n))
    beta_e, gamma_e = gdn_effective(env, m, gp)
    xc = conv_out.detach().reshape(-1, M).cpu().float()
    n64, nq, y64 = G.fwd(xc, beta_e, gamma_e, inverse)
    rs = [ratio("d", tag, "y", G.band_ratio(R.rows(to64(y)), y64, y64.abs(), G.K_FWD(M)))]
    if norm is not None:
        rs.append(ratio("d", tag, "norm", G.band_ratio(norm.detach().reshape(-1, M).cpu(), n64, n64, G.K_FWD(M))))
    assert max(rs) <= 1.0, rs
    # backward: bit for bit the explicit composition of the GDN's backward and the convolution's (each held elsewhere:
    # tests/test_gpu_gdn_bf16.py and group a / tests/test_gpu_latent_bf16.py)
    with torch.no_grad():
        g_conv, dbeta, dgamma, db_pre = FB._gdn_backward_bf16(conv_out, norm, m.beta.detach(), m.gamma.detach(), nhwc(gd),
                                                               inverse, *gp, True, True, True, bias_from_dx=True)
        dx, dw, db = FB._conv_backward_bf16(nhwc(xd.detach()), wd.detach(), g_conv, 1, 1, False, BF, 0, True, True,
                                            db_pre is None)
        dx32, _, _ = FB._conv_backward_bf16(nhwc(xd.detach()), wd.detach(), g_conv, 1, 1, False, torch.float32, 0, True,
                                            False, False)
        torch.cuda.synchronize()
    same(xd.grad, dx, f"{tag} dx")
    same(wd.grad, dw, f"{tag} dw")
    same(bd.grad, db_pre if db_pre is not None else db, f"{tag} db")
    same(m.beta.grad, dbeta.view_as(m.beta.grad), f"{tag} dbeta")
    same(m.gamma.grad, dgamma, f"{tag} dgamma")
    # the convolution's data and weight gradient of the device's own g_conv against float64
    gc64 = nchw64(g_conv)
    gr = R.conv_grads(x, R.rne_bf16(w), b, gc64, 3, 1, 1)
    banded32("fused", "d", tag, "dx", to64(dx32), gr.dx, gr.S_dx, R.band_A(gr.n_dx))
    is_ref(dx, R.rne_bf16(to64(dx32)), f"{tag} dx against its rounded fp32 twin")
    lay = R.layer("rb1", M)
    sk = RR.plan_ref(SimpleNamespace(B=B, Hs=H, Ws=W, Cp=M, Cg=M, kh=3, kw=3, g_is_row=1))[2]
    r_ = ratio("d", tag, "dw", R.wgrad_ratio(dw.cpu(), gr.dw, R.wgrad_weight(x, gc64, lay), B * H * W, sk))
    assert r_ <= 1.0, (tag, r_)


# =============================================================================================
# e. the blocks as modules, bf16
# =============================================================================================
BLOCK_GRIDS = R.BLOCK_GRIDS


def make_block(env, kind, M, shifted=True):
    """the layers module of a block with resblock_ref.block_params as its parameters -> (module, P, (beta_e, gamma_e))"""
    from neural_image_compression_amd import layers as LY
    dev = env[3]
    P = R.block_params(kind, M, shifted=shifted)
    if kind in ("rbs_rgb", "rbs"):
        m = LY.ResidualBlockWithStride(3 if kind == "rbs_rgb" else M, M)
        convs = {"w1": m.conv1, "w2": m.conv2, "ws": m.skip}
        gdn = m.gdn
    elif kind == "rb":
        m = LY.ResidualBlock(M, M)
        convs = {"w1": m.conv1, "w2": m.conv2}
        gdn = None
    else:
        m = LY.ResidualBlockUpsample(M, M)
        convs = {"w1": m.subpel_conv.deconv, "w2": m.conv, "ws": m.upsample.deconv}
        gdn = m.igdn
    m = m.to(dev)
    with torch.no_grad():
        for k, c in convs.items():
            c.weight.copy_(P[k])
            c.bias.copy_(P["b" + k[1:]])
        if gdn is not None:
            ped = gdn.beta_reparam.pedestal_value
            gdn.beta.copy_((P["beta_e"].double() + ped).sqrt().float())
            gdn.gamma.copy_((P["gamma_e"].double() + ped).sqrt().float())
    eff = None
    if gdn is not None:
        gp = (gdn.beta_reparam.bound_value, gdn.gamma_reparam.bound_value, gdn.beta_reparam.pedestal_value)
        eff = gdn_effective(env, gdn, gp)
    return m, P, eff


def compose_bf16(env, kind, m, x, fuse):
    """the block layer by layer through functional_bf16 -> dict of every intermediate (NCHW-logical)"""
    F_, FB, L, dev = env
    s = 0.01
    cap = {}
    if kind == "rbs_rgb":
        cap["c1"] = FB.image_conv2d_bf16(x, m.conv1.weight, m.conv1.bias, 2, 1)
        cap["h1"] = torch.nn.functional.leaky_relu(cap["c1"], s)
    elif kind == "rbs":
        cap["h1"] = FB.conv2d_bf16(x, m.conv1.weight, m.conv1.bias, 2, 1, False, True, s)
    elif kind == "rb":
        cap["h1"] = FB.conv2d_bf16(x, m.conv1.weight, m.conv1.bias, 1, 1, False, True, s)
    else:
        d = m.subpel_conv.deconv
        cap["h1"] = FB.conv_transpose2d_bf16(x, d.weight, d.bias, 2, 1, 1, False, True, s)
    if kind == "rb":
        cap["main"] = FB.conv2d_bf16(cap["h1"], m.conv2.weight, m.conv2.bias, 1, 1, False, True, s)
        cap["identity"] = FB.as_bf16(x)
    else:
        conv, g = (m.conv, m.igdn) if kind == "rbu" else (m.conv2, m.gdn)
        gp = (g.beta_reparam.bound_value, g.gamma_reparam.bound_value, g.beta_reparam.pedestal_value)
        if fuse:
            cap["main"] = FB.conv_gdn_bf16(cap["h1"], conv.weight, conv.bias, g.beta, g.gamma, 1, 1, g.inverse, *gp)
            cap["conv_out"] = cap["main"].grad_fn.saved_tensors[2].permute(0, 3, 1, 2)
        else:
            cap["conv_out"] = FB.conv2d_bf16(cap["h1"], conv.weight, conv.bias, 1, 1)
            cap["main"] = FB.gdn_bf16(cap["conv_out"], g.beta, g.gamma, g.inverse, *gp)
        if kind == "rbs_rgb":
            cap["identity"] = FB.image_conv2d_bf16(x, m.skip.weight, m.skip.bias, 2, 0)
        elif kind == "rbs":
            cap["identity"] = FB.conv2d_bf16(x, m.skip.weight, m.skip.bias, 2, 0)
        else:
            d = m.upsample.deconv
            cap["identity"] = FB.conv_transpose2d_bf16(x, d.weight, d.bias, 2, 1, 1)
    cap["out"] = cap["main"] + cap["identity"]
    return cap


def block_x(env, kind, M):
    dev = env[3]
    x = R.block_input(kind, M, BLOCK_GRIDS[kind])
    if kind == "rbs_rgb":
        return x, nhwc(x).to(dev).permute(0, 3, 1, 2)
    return x, bf(nhwc(x), dev).permute(0, 3, 1, 2)


def named_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def twin32(env, x, weight, bias, geo, leaky):
    """the fp32 twin of a bf16 conv launch: the same layer on the same device operands through FB._igemm_bf16 into a guarded
    fp32 tensor (the plan depends on the geometry only; group a holds bf16 = rne_bf16(fp32) for every variant)"""
    F_, FB, L, dev = env
    k, s, p, tr, op = geo
    xh = x.detach().permute(0, 2, 3, 1).contiguous()
    assert xh.dtype == BF
    B, Hi, Wi, Cin = xh.shape
    Cout = weight.shape[1] if tr else weight.shape[0]
    Ho, Wo = F_.conv_out_size(Hi, Wi, k, s, p, tr, op)
    out = Guarded(B * Ho * Wo, Cout, dev, torch.float32)
    view = out.t.view(B, Ho, Wo, Cout)
    FB._igemm_bf16(xh, FB._pack_conv_weight_bf16(weight.detach(), tr, False), view, B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo,
                   Cout=Cout, kh=k, kw=k, stride=s, pad=p, transposed=tr, bias=bias.detach(),
                   epilogue=L.EPI_LEAKY if leaky else L.EPI_NONE, slope=0.01)
    torch.cuda.synchronize()
    out.check("fp32 twin")
    return nchw64(view)


def check_block_forward(env, kind, M, cap, x64, P, eff, tag, xdev=None, mod=None):
    """every intermediate against the reference applied to the device's own previous stored tensor; the stores behind a
    fused LeakyReLU through the fp32 twin of their launch (xdev, mod: the device input and the module with the weights)"""
    rgb = kind == "rbs_rgb"
    geo1 = {"rbs_rgb": R.C3S2, "rbs": R.C3S2, "rb": R.C3S1, "rbu": R.T3S2}[kind]
    n1 = {"rbs_rgb": 27, "rbs": 9 * M, "rb": 9 * M, "rbu": 4 * M}[kind]
    if rgb:
        y64, S = R.conv_store(x64, P["w1"], P["b1"], geo1, round_x=True)
        banded16("stem3", "e", tag, "c1", to64(cap["c1"]), y64, S, R.band_A(n1))
        is_ref(cap["h1"], R.torch_leaky_bf16_ref(to64(cap["c1"])), f"{tag} torch LeakyReLU behind the RGB conv")
    else:
        y64, S = R.conv_store(x64, P["w1"], P["b1"], geo1, leaky=True)
        c1 = mod.subpel_conv.deconv if kind == "rbu" else mod.conv1
        y32 = twin32(env, xdev, c1.weight, c1.bias, geo1, True)
        banded32("igemm", "e", tag, "h1", y32, y64, S, R.band_A(n1))
        is_ref(cap["h1"], R.rne_bf16(y32), f"{tag} h1 against its rounded fp32 twin")
    h1 = to64(cap["h1"])
    y64, S = R.conv_store(h1, P["w2"], P["b2"], R.C3S1, leaky=(kind == "rb"))
    if kind == "rb":
        y32 = twin32(env, cap["h1"], mod.conv2.weight, mod.conv2.bias, R.C3S1, True)
        banded32("igemm", "e", tag, "main", y32, y64, S, R.band_A(9 * M))
        is_ref(cap["main"], R.rne_bf16(y32), f"{tag} main against its rounded fp32 twin")
    else:
        banded16("fused", "e", tag, "conv_out", to64(cap["conv_out"]), y64, S, R.band_A(9 * M))
        n64, nq, g64 = G.fwd(R.rows(to64(cap["conv_out"])), eff[0], eff[1], kind == "rbu")
        r = ratio("e", tag, "gdn-y", G.band_ratio(R.rows(to64(cap["main"])), g64, g64.abs(), G.K_FWD(M)))
        assert r <= 1.0, (tag, r)
        geo_s, n_s = (R.T3S2, 4 * M) if kind == "rbu" else (R.C1S2, 3 if rgb else M)
        y64, S = R.conv_store(x64, P["ws"], P["bs"], geo_s, round_x=rgb)
        banded16("skip_rgb" if rgb else "igemm", "e", tag, "identity", to64(cap["identity"]), y64, S, R.band_A(n_s))
    is_ref(cap["out"], R.add_bf16_ref(to64(cap["main"]), to64(cap["identity"])), f"{tag} skip add")


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("kind", ["rbs_rgb", "rbs", "rb", "rbu"])
def test_e_block_bf16(env, kind, M, fuse):
    F_, FB, L, dev = env
    from neural_image_compression_amd import layers as LY
    tag = f"{kind}-M{M}-{'fused' if fuse else 'unfused'}"
    m, P, eff = make_block(env, kind, M)
    m2 = copy.deepcopy(m)
    x_cpu, xd = block_x(env, kind, M)
    rgb = kind == "rbs_rgb"
    xa = xd.clone() if rgb else xd.clone().requires_grad_(True)
    xb = xd.clone() if rgb else xd.clone().requires_grad_(True)
    # the explicit composition, every intermediate captured
    cap, names_c = traced(env, None, lambda: compose_bf16(env, kind, m2, xa, fuse))
    VARIANTS.update(names_c)
    if kind != "rb":
        assert any(n.startswith("igemm_bf16_kernel<") and n.split(", ")[3] == "true" for n in names_c) == fuse, names_c
    check_block_forward(env, kind, M, cap, x_cpu.double(), P, eff, tag, xa, m2)
    r = R._rng("block-g-" + tag)
    g = bf(nhwc(R.to_bf16_exact(r.standard_normal(tuple(cap["out"].shape)))), dev).permute(0, 3, 1, 2)
    if not rgb:
        # the two branches' data gradients, then their sum as autograd forms it
        (dx_main,) = torch.autograd.grad(cap["main"], xa, g, retain_graph=True)
        dx_skip = g if kind == "rb" else torch.autograd.grad(cap["identity"], xa, g, retain_graph=True)[0]
        torch.cuda.synchronize()
        if kind != "rb":
            geo_s, n_s = (R.T3S2, 9 * M) if kind == "rbu" else (R.C1S2, M)
            k_, s_, p_, tr_, op_ = geo_s
            gs = R.conv_grads(x_cpu, R.rne_bf16(P["ws"]), P["bs"], to64(g), k_, s_, p_, tr_, op_)
            assert gs.n_dx == n_s
            cs = m2.upsample.deconv if kind == "rbu" else m2.skip
            with torch.no_grad():
                ds32, _, _ = FB._conv_backward_bf16(nhwc(xa.detach()), cs.weight.detach(), nhwc(g), s_, p_, tr_, torch.float32, 0,
                                                    True, False, False)
                torch.cuda.synchronize()
            banded32("igemm", "e", tag, "dx-skip", to64(ds32), gs.dx, gs.S_dx, R.band_A(n_s))
            is_ref(dx_skip, R.rne_bf16(to64(ds32)), f"{tag} dx-skip against its rounded fp32 twin")
    cap["out"].backward(g)
    torch.cuda.synchronize()
    if not rgb:
        is_ref(xa.grad, R.add_bf16_ref(to64(dx_main), to64(dx_skip)), f"{tag} the two branches' gradients summed")
    # the module: bit for bit the composition
    old = LY.FUSE_CONV_GDN
    LY.FUSE_CONV_GDN = fuse
    try:
        out, names_m = traced(env, None, lambda: m(xb, bf16=True))
        out.backward(g)
        torch.cuda.synchronize()
    finally:
        LY.FUSE_CONV_GDN = old
    assert names_m == names_c, (names_m, names_c)
    same(out, cap["out"], f"{tag} module out")
    if not rgb:
        same(xb.grad, xa.grad, f"{tag} module x.grad")
    else:
        assert xb.grad is None
    ga, gb = named_grads(m2), named_grads(m)
    assert set(ga) == set(gb) == {n for n, _ in m.named_parameters()}, sorted(set(ga) ^ set(gb))
    for n in sorted(ga):
        same(gb[n], ga[n], f"{tag} {n}.grad")


def test_e_a_backward_pass_for_the_input_alone_leaves_nothing_pending(env):
    """torch.autograd.grad(y, [x]) -- what test_e_block_bf16 uses to see one branch's data gradient -- still asks every layer
    for its weight gradient (ctx.needs_input_grad does not know the pass is restricted) and drops it at once.  A reduction
    left pending for such a gradient would write, at the end of the pass, into memory the allocator has already handed to
    another tensor (it did: the weight-gradient slabs of conv2 landed in conv1's data gradient).  reductions.can_defer
    must refuse there, and keep deferring in a full backward pass."""
    F_, FB, L, dev = env
    M = 64
    m, P, _ = make_block(env, "rb", M)
    _, xd = block_x(env, "rb", M)
    g = torch.ones_like(xd)

    def partial():
        x = xd.clone().requires_grad_(True)
        return torch.autograd.grad(m(x, bf16=True), x, g)[0]

    def restricted():
        x = xd.clone().requires_grad_(True)
        m(x, bf16=True).backward(g, inputs=[x])
        return x.grad

    def full():
        x = xd.clone().requires_grad_(True)
        m(x, bf16=True).backward(g)
        return x.grad
    dx_p, n_p = defer_calls(env, partial)
    dx_r, n_r = defer_calls(env, restricted)
    assert all(p.grad is None for p in m.parameters())
    dx_f, n_f = defer_calls(env, full)
    assert n_p == 0 and n_r == 0 and n_f > 0, (n_p, n_r, n_f)
    same(dx_p, dx_f, "x.grad of the restricted pass (autograd.grad)")
    same(dx_r, dx_f, "x.grad of the restricted pass (backward(inputs=))")
    # the captured form: the gradients come back to the caller, reduced before autograd.grad returns
    x = xd.clone().requires_grad_(True)
    ws = [p for p in m.parameters()]
    got, n_c = defer_calls(env, lambda: torch.autograd.grad(m(x, bf16=True), ws, g))
    assert n_c == 0
    for p, gw in zip(ws, got):
        same(gw, p.grad, "a captured parameter gradient against the full pass's")
    # a pass for one weight alone: its bias sum must not wait either (the engine drops the bias gradient at once)
    full_w = m.conv1.weight.grad.clone()
    for p in m.parameters():
        p.grad = None
    x = xd.clone().requires_grad_(True)
    _, n_w = defer_calls(env, lambda: m(x, bf16=True).backward(g, inputs=[m.conv1.weight]))
    assert n_w == 0 and m.conv1.bias.grad is None and x.grad is None
    same(m.conv1.weight.grad, full_w, "the weight gradient of a pass restricted to that weight")


@pytest.mark.parametrize("M", [64, 192])
def test_e_head_block_bf16(env, M):
    """TransposedDeconv3x3(M, 3) as run_bf16 runs it: the column-route head of group c, bit for bit"""
    F_, FB, L, dev = env
    from neural_image_compression_amd import layers as LY
    torch.manual_seed(7 + M)
    m = LY.TransposedDeconv3x3(M, 3).to(dev)
    case = ("head3", M, 0, (2, 9, 7))
    i = R.inputs(case)
    xa = bf(nhwc(i["x"]), dev).permute(0, 3, 1, 2).requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = nhwc(i["g"]).to(dev).permute(0, 3, 1, 2)
    m2 = copy.deepcopy(m)
    ya = FB.image_conv_transpose2d_bf16(xa, m2.deconv.weight, m2.deconv.bias, 2, 1, 1)
    ya.backward(g)
    yb, names = traced(env, None, lambda: LY.run_bf16(nn.Sequential(m), xb, out_f32=True))
    yb.backward(g)
    torch.cuda.synchronize()
    assert not any("head_convt" in n for n in names), names
    assert yb.dtype == torch.float32
    same(yb, ya, f"head M{M} out")
    same(xb.grad, xa.grad, f"head M{M} x.grad")
    for n in ("weight", "bias"):
        same(getattr(m.deconv, n).grad, getattr(m2.deconv, n).grad, f"head M{M} {n}.grad")
    # float64, with the module's own parameters
    ref = R.conv_ref(i["x"], R.rne_bf16(m.deconv.weight.detach().cpu()), m.deconv.bias.detach().cpu(), 3, 2, 1, True, 1)
    hu = R.column_route_half_ulps(i["x"], m.deconv.weight.detach().cpu(), 3, 2, 1, 1)
    assert ratio("e", f"head-M{M}", "y-columns", R.column_route_ratio(to64(yb), ref.y, ref.S, hu)) <= 1.0


# =============================================================================================
# f. the blocks in fp32
# =============================================================================================
def compose_fp32(env, kind, m, x):
    F_ = env[0]
    s = 0.01
    cap = {}
    if kind == "rbs_rgb":
        cap["h1"] = F_.image_conv2d(x, m.conv1.weight, m.conv1.bias, 2, 1, True, s)
    elif kind in ("rbs", "rb"):
        cap["h1"] = F_.conv2d(x, m.conv1.weight, m.conv1.bias, 2 if kind == "rbs" else 1, 1, True, s)
    else:
        d = m.subpel_conv.deconv
        cap["h1"] = F_.conv_transpose2d(x, d.weight, d.bias, 2, 1, 1, True, s)
    if kind == "rb":
        cap["out"] = F_.conv2d(cap["h1"], m.conv2.weight, m.conv2.bias, 1, 1, True, s, 0, x)
        return cap
    conv, g = (m.conv, m.igdn) if kind == "rbu" else (m.conv2, m.gdn)
    cap["c2"] = F_.conv2d(cap["h1"], conv.weight, conv.bias, 1, 1)
    if kind == "rbs_rgb":
        cap["identity"] = F_.image_conv2d(x, m.skip.weight, m.skip.bias, 2, 0)
    elif kind == "rbs":
        cap["identity"] = F_.conv2d(x, m.skip.weight, m.skip.bias, 2, 0)
    else:
        d = m.upsample.deconv
        cap["identity"] = F_.conv_transpose2d(x, d.weight, d.bias, 2, 1, 1)
    cap["out"] = F_.gdn(cap["c2"], g.beta, g.gamma, g.inverse, g.beta_reparam.bound_value, g.gamma_reparam.bound_value,
                        g.beta_reparam.pedestal_value, cap["identity"])
    return cap


def fp32_stage(tag, what, dev, x64, w, b, geo, A, leaky=False, res64=None):
    """an fp32 conv launch: |dev - y64| <= A S (+ one fp32 add of the residual: 2^-24 |y64|)"""
    k, s, p, tr, op = geo
    ref = R.conv_ref(x64, w, b, k, s, p, tr, op)
    y64 = R.leaky_ref(ref.y) if leaky else ref.y
    bound = A * ref.S
    if res64 is not None:
        y64 = y64 + res64
        bound = bound + 2.0 ** -24 * y64.abs()
    err = (to64(dev) - y64).abs()
    r = ratio("f", tag, what, float(torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)),
                                                     nan=float("inf")).max()))
    assert r <= 1.0, (tag, what, r)


@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("kind", ["rbs_rgb", "rbs", "rb", "rbu"])
def test_f_block_fp32(env, kind, M):
    F_, FB, L, dev = env
    tag = f"{kind}-M{M}"
    m, P, _ = make_block(env, kind, M, shifted=False)
    m2 = copy.deepcopy(m)
    r = R._rng("f-" + tag)
    B, h, w = BLOCK_GRIDS[kind]
    x_cpu = torch.as_tensor(r.standard_normal((B, 3 if kind == "rbs_rgb" else M, h, w)).astype(np.float32))
    xd = nhwc(x_cpu).to(dev).permute(0, 3, 1, 2)
    xa, xb = xd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    cap, names_c = traced(env, None, lambda: compose_fp32(env, kind, m2, xa))
    VARIANTS.update(names_c)
    rgb = kind == "rbs_rgb"
    x64 = x_cpu.double()
    geo1 = {"rbs_rgb": R.C3S2, "rbs": R.C3S2, "rb": R.C3S1, "rbu": R.T3S2}[kind]
    fp32_stage(tag, "h1", cap["h1"], x64, P["w1"], P["b1"], geo1, C64.A_RGB if rgb else C64.A_IGEMM, leaky=True)
    h1 = to64(cap["h1"])
    if kind == "rb":
        fp32_stage(tag, "out", cap["out"], h1, P["w2"], P["b2"], R.C3S1, C64.A_IGEMM, leaky=True, res64=x64)
    else:
        fp32_stage(tag, "c2", cap["c2"], h1, P["w2"], P["b2"], R.C3S1, C64.A_IGEMM)
        fp32_stage(tag, "identity", cap["identity"], x64, P["ws"], P["bs"], R.T3S2 if kind == "rbu" else R.C1S2,
                   C64.A_RGB if rgb else C64.A_IGEMM)
        g = m2.igdn if kind == "rbu" else m2.gdn
        gp = (g.beta_reparam.bound_value, g.gamma_reparam.bound_value, g.beta_reparam.pedestal_value)
        be = torch.clamp(g.beta.detach().cpu().double(), min=gp[0]) ** 2 - gp[2]
        ge = torch.clamp(g.gamma.detach().cpu().double(), min=gp[1]) ** 2 - gp[2]
        y64, _ = G64.fwd(R.rows(to64(cap["c2"])), be, ge, kind == "rbu", R.rows(to64(cap["identity"])))
        rr = ratio("f", tag, "out", G64.band_ratio(R.rows(to64(cap["out"])), y64, *G64.BAND))
        assert rr <= 1.0, (tag, rr)
    gcpu = torch.as_tensor(r.standard_normal(tuple(cap["out"].shape)).astype(np.float32))
    g_d = nhwc(gcpu).to(dev).permute(0, 3, 1, 2)
    cap["out"].backward(g_d)
    out, names_m = traced(env, None, lambda: m(xb))
    out.backward(g_d)
    torch.cuda.synchronize()
    same(out, cap["out"], f"{tag} module out")
    same(xb.grad, xa.grad, f"{tag} module x.grad")
    ga, gb = named_grads(m2), named_grads(m)
    assert set(ga) == set(gb) == {n for n, _ in m.named_parameters()}
    for n in sorted(ga):
        same(gb[n], ga[n], f"{tag} {n}.grad")
    # every gradient against float64 autograd of the plain composition, at 1e-4 of the tensor's maximum (the fp32 suites'
    # gradient band)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items() if not k.endswith("_e")}
    if kind != "rb":
        gmod = m.igdn if kind == "rbu" else m.gdn
        bp = gmod.beta.detach().cpu().double().requires_grad_(True)
        gpp = gmod.gamma.detach().cpu().double().requires_grad_(True)
        P64["beta_e"] = torch.clamp(bp, min=gp[0]) ** 2 - gp[2]
        P64["gamma_e"] = torch.clamp(gpp, min=gp[1]) ** 2 - gp[2]
    xr = x64.clone().requires_grad_(True)
    out64 = R.block_forward_fp32(kind, xr, P64)
    leaves = {"x": xr, **{k: v for k, v in P64.items() if not k.endswith("_e")}}
    if kind != "rb":
        leaves.update(beta=bp, gamma=gpp)
    grads = dict(zip(leaves, torch.autograd.grad(out64, list(leaves.values()), gcpu.double())))
    rr = ratio("f", tag, "out-vs-float64", R.norm_err(to64(out), out64.detach()) / 1e-4)
    assert rr <= 1.0
    names = {"rbs_rgb": dict(w1="conv1.weight", b1="conv1.bias", w2="conv2.weight", b2="conv2.bias", ws="skip.weight",
                             bs="skip.bias", beta="gdn.beta", gamma="gdn.gamma"),
             "rb": dict(w1="conv1.weight", b1="conv1.bias", w2="conv2.weight", b2="conv2.bias"),
             "rbu": dict(w1="subpel_conv.deconv.weight", b1="subpel_conv.deconv.bias", w2="conv.weight", b2="conv.bias",
                         ws="upsample.deconv.weight", bs="upsample.deconv.bias", beta="igdn.beta", gamma="igdn.gamma")}
    names["rbs"] = names["rbs_rgb"]
    worst = R.norm_err(to64(xb.grad), grads["x"]) / 1e-4
    ratio("f", tag, "dx", worst)
    assert worst <= 1.0, (tag, "dx", worst)
    for k, n in names[kind].items():
        e = R.norm_err(gb[n].cpu(), grads[k]) / 1e-4
        ratio("f", tag, "d" + k, e)
        assert e <= 1.0, (tag, k, e)


@pytest.mark.parametrize("M", [64, 192])
def test_f_head_fp32(env, M):
    """TransposedDeconv3x3(M, 3) in fp32: layers.ConvTranspose2d -> functional.image_conv_transpose2d (dense launch into
    [P][28] columns + lic_col2im), output and every gradient against float64 of the UNROUNDED operands"""
    F_, FB, L, dev = env
    from neural_image_compression_amd import layers as LY
    tag = f"head-M{M}"
    torch.manual_seed(11 + M)
    m = LY.TransposedDeconv3x3(M, 3).to(dev)
    i = R.inputs(("head3", M, 0, (2, 9, 7)))
    r = R._rng("f-" + tag)
    x_cpu = i["x"] + torch.as_tensor(r.standard_normal(tuple(i["x"].shape)).astype(np.float32)) * 2.0 ** -10   # not bf16-exact
    x = nhwc(x_cpu).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    g = nhwc(i["g"]).to(dev).permute(0, 3, 1, 2)
    y, names = traced(env, None, lambda: m(x))
    y.backward(g)
    torch.cuda.synchronize()
    VARIANTS.update(names)
    assert y.dtype == torch.float32 and names and not any("bf16" in n for n in names), names
    w, b = m.deconv.weight.detach().cpu(), m.deconv.bias.detach().cpu()
    ref = R.conv_ref(x_cpu, w, b, 3, 2, 1, True, 1)
    gr = R.conv_grads(x_cpu, w, b, i["g"], 3, 2, 1, True, 1)
    for what, dev64, ref64, S in (("y", to64(y), ref.y, ref.S), ("dx", to64(x.grad), gr.dx, gr.S_dx)):
        print(f"ERRS f {tag} {what} rgb32 {R.err_over_S(dev64, ref64, S):.3e}")
        rr = ratio("f", tag, what, R.band_ratio(dev64, ref64, S, C64.A_RGB))
        assert rr <= 1.0, (tag, what, rr)
    weight = R.wgrad_weight(x_cpu, i["g"], i["lay"])
    err = (m.deconv.weight.grad.cpu().double() - gr.dw).abs()
    rr = ratio("f", tag, "dw", float((err / (C64.A_WGRAD * weight).clamp_min(1e-300)).max()))
    assert rr <= 1.0, (tag, "dw", rr)
    assert ratio("f", tag, "db", colsum_ratio(m.deconv.bias.grad, R.f64(i["g"]))) <= 1.0


# =============================================================================================
# g. whole stacks in bf16
# =============================================================================================
def by_blocks(env, net, x):
    """the stack block by block, as layers.run_bf16 pairs it: Conv -> LeakyReLU as one launch, the last layer in fp32"""
    from neural_image_compression_amd import layers as LY
    mods = list(net)
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        last = i == len(mods) - 1
        if isinstance(m, (LY.ResidualBlock, LY.ResidualBlockWithStride, LY.ResidualBlockUpsample)):
            x = m(x, bf16=True)
        elif isinstance(m, LY.TransposedDeconv3x3):
            if isinstance(nxt, LY.LeakyReLU):
                x = m.deconv(x, bf16=True, leaky=True, slope=nxt.negative_slope)
                i += 1
            else:
                x = m.deconv(x, bf16=True) if m.deconv.out_channels < 4 else m.deconv(x, bf16=True, out_f32=last)
        elif isinstance(m, LY.Conv2d):
            if isinstance(nxt, LY.LeakyReLU):
                x = m(x, bf16=True, leaky=True, slope=nxt.negative_slope)
                i += 1
            else:
                x = m(x, bf16=True, out_f32=last)
        else:
            raise AssertionError(type(m).__name__)
        i += 1
    return x


@pytest.mark.parametrize("name", ["Encoder3x3", "Decoder3x3", "HyperEncoder3x3", "HyperDecoder3x3"])
def test_g_stack_is_its_blocks(env, name):
    F_, FB, L, dev = env
    from neural_image_compression_amd import components as CP
    M = 64
    torch.manual_seed(100 + len(name))
    st = getattr(CP, name)(M).to(dev)
    st.precision = "bf16"
    r = R._rng("stack-" + name)
    shape = {"Encoder3x3": (1, 3, 64, 64), "Decoder3x3": (1, M, 4, 4), "HyperEncoder3x3": (1, M, 4, 4),
             "HyperDecoder3x3": (1, M, 1, 1)}[name]
    x_cpu = torch.as_tensor((r.random_sample(shape) if name == "Encoder3x3" else r.standard_normal(shape)).astype(np.float32))
    xd = nhwc(x_cpu).to(dev).permute(0, 3, 1, 2)
    rgb = name == "Encoder3x3"
    xa = xd.clone() if rgb else xd.clone().requires_grad_(True)
    xb = xd.clone() if rgb else xd.clone().requires_grad_(True)
    ya, names_a = traced(env, None, lambda: st(xa))
    assert ya.dtype == torch.float32
    g = torch.as_tensor(r.standard_normal(tuple(ya.shape)).astype(np.float32)).to(dev)
    ya.backward(g)
    torch.cuda.synchronize()
    ga = named_grads(st)
    assert set(ga) == {n for n, _ in st.named_parameters()}
    for p in st.parameters():
        p.grad = None
    yb, names_b = traced(env, None, lambda: by_blocks(env, st.net, xb))
    yb.backward(g)
    torch.cuda.synchronize()
    VARIANTS.update(names_a)
    assert names_a == names_b, (names_a ^ names_b)
    same(ya, yb, f"{name} out")
    if not rgb:
        same(xa.grad, xb.grad, f"{name} x.grad")
    gb = named_grads(st)
    for n in sorted(ga):
        same(ga[n], gb[n], f"{name} {n}.grad")
    if name == "Decoder3x3":
        assert not any("head_convt" in n for n in names_a), names_a


def _lst64(m, x):
    """components.LatentSpaceTransform in float64 plain torch, from the module's own parameters"""
    import torch.nn.functional as TF

    def d(t):
        return t.detach().cpu().double()

    def conv(c, v):
        return TF.conv2d(v, d(c.weight), d(c.bias), stride=c.stride, padding=c.padding)

    def deconv(c, v):
        return TF.conv_transpose2d(v, d(c.weight), d(c.bias), stride=c.stride, padding=c.padding, output_padding=c.output_padding)

    def rb(b, v):
        return TF.leaky_relu(conv(b.conv2, TF.leaky_relu(conv(b.conv1, v), 0.01)), 0.01) + v

    def urb(b, v):
        c2 = conv(b.conv, TF.leaky_relu(deconv(b.subpel_conv.deconv, v), 0.01))
        g = b.igdn
        be = torch.clamp(d(g.beta), min=g.beta_reparam.bound_value) ** 2 - g.beta_reparam.pedestal_value
        ge = torch.clamp(d(g.gamma), min=g.gamma_reparam.bound_value) ** 2 - g.gamma_reparam.pedestal_value
        n = be[None, :, None, None] + torch.einsum("ij,bjhw->bihw", ge, c2 * c2)
        return c2 * n.sqrt() + deconv(b.upsample.deconv, v)
    for blk in (m.RB1, m.URB1, m.RB2, m.URB2, m.RB3, m.URB3, m.RB4):
        x = rb(blk, x) if type(blk).__name__ == "ResidualBlock" else urb(blk, x)
    return conv(m.conv, x)


def test_g_latent_space_transform_fp32(env):
    """LatentSpaceTransform(64) has no bf16 route: its forward is the fp32 loop over the same blocks (two of its three
    upsampling blocks have factor 1: a 3x3 stride-1 transposed convolution).  Output and the input's gradient against
    float64 at 1e-4 of the tensor's maximum, the fp32 suites' whole-tensor band; bit for bit the loop over its blocks"""
    F_, FB, L, dev = env
    from neural_image_compression_amd import components as CP
    torch.manual_seed(64)
    m = CP.LatentSpaceTransform(64).to(dev)
    r = R._rng("lst")
    x_cpu = torch.as_tensor(r.standard_normal((1, 64, 5, 4)).astype(np.float32))
    xa = nhwc(x_cpu).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    ya = m(xa)
    g_cpu = torch.as_tensor(r.standard_normal(tuple(ya.shape)).astype(np.float32))
    g = nhwc(g_cpu).to(dev).permute(0, 3, 1, 2)
    ya.backward(g)
    ga = named_grads(m)
    for p in m.parameters():
        p.grad = None
    yb = xb
    for blk in (m.RB1, m.URB1, m.RB2, m.URB2, m.RB3, m.URB3, m.RB4, m.conv):
        yb = blk(yb)
    yb.backward(g)
    torch.cuda.synchronize()
    same(ya, yb, "LatentSpaceTransform out")
    same(xa.grad, xb.grad, "LatentSpaceTransform x.grad")
    gb = named_grads(m)
    for n in sorted(ga):
        same(ga[n], gb[n], f"LatentSpaceTransform {n}.grad")
    xr = x_cpu.double().requires_grad_(True)
    y64 = _lst64(m, xr)
    (dx64,) = torch.autograd.grad(y64, xr, g_cpu.double())
    assert tuple(y64.shape) == tuple(ya.shape) == (1, 64, 10, 8)
    ry = ratio("g", "lst", "y", R.norm_err(to64(ya), y64.detach()) / 1e-4)
    rdx = ratio("g", "lst", "dx", R.norm_err(to64(xa.grad), dx64) / 1e-4)
    assert ry <= 1.0 and rdx <= 1.0, (ry, rdx)


# =============================================================================================
# h. refusals launch nothing
# =============================================================================================
def test_h_refusals_launch_nothing(env):
    F_, FB, L, dev = env
    from neural_image_compression_amd import layers as LY
    M = 64
    conv = LY.Conv2d(M, M, 3, 1, 1).to(dev)
    stem = LY.Conv2d(3, M, 3, 2, 1).to(dev)
    head = LY.TransposedDeconv3x3(M, 3).to(dev)
    up = LY.TransposedDeconv3x3(M, M).to(dev)
    xb = torch.zeros((1, 4, 4, M), device=dev, dtype=BF).permute(0, 3, 1, 2)
    img = torch.rand((1, 8, 8, 3), device=dev).permute(0, 3, 1, 2)
    bad = [
        ("residual= with bf16=True", lambda: conv(xb, bf16=True, residual=xb)),
        ("residual= on the bf16 transposed layer", lambda: up.deconv(xb, bf16=True, residual=xb)),
        ("leaky on the bf16 RGB head", lambda: head.deconv(xb, bf16=True, leaky=True)),
        ("the bf16 stem with an image that requires grad", lambda: stem(img.clone().requires_grad_(True), bf16=True)),
    ]
    for what, fn in bad:
        names = set()
        F_.KERNEL_TRACE = names
        try:
            with pytest.raises(NotImplementedError):
                fn()
        finally:
            F_.KERNEL_TRACE = None
        torch.cuda.synchronize()
        assert not names, (what, names)
    # (and the forms that are accepted, so that the refusals above are not refusals of everything)
    _, names = traced(env, None, lambda: (conv(xb, bf16=True), head.deconv(xb, bf16=True), stem(img, bf16=True, leaky=True)))
    assert names, names


def test_z_summary():
    """the figures the docstrings quote: worst RATIO per group and the raw err / S per family"""
    if not WORST:      # (run alone: nothing to report)
        return
    print("\nMEASURED " + " ".join(f"{k} {v:.4e}" for k, v in ERRS.items()) + f" A_BAND {R.A_BAND:.4e}")
    for (group, what), (v, tag) in sorted(WORST.items()):
        print(f"WORST {group} {what} {v:.4f} ({tag})")
    print("VARIANTS " + " | ".join(sorted(VARIANTS)))
    for fam, e in ERRS.items():
        assert 4 * e <= R.A_BAND, f"{fam}: 4 x {e:.3e} exceeds A_BAND -- record it in resblock_ref.A_MEASURED and give the family its own constant"
