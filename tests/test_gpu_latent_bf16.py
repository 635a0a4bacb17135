"""The bf16 latent-side convolutions (lic_igemm_bf16 with a tap mask, a pitched output slice, the fused LeakyReLU and
its backward, at the widths of the hyper stacks and the entropy-parameter MLP) against tests/conv_bf16_ref.py, the
float64 statement of the same convolutions.  The bands and their constant A are derived / measured in conv_bf16_ref.py.

  a. masked context conv, M = 64 / 128 / 192, four grids, BM forced to 64 / 128 / 256 and the K split to 1 / 3 / 5:
     forward fp32 banded and bf16 bit for bit; data gradient into an fp32 and a bf16 tensor; weight gradient per tap
     (dead taps included: it is not masked); bias gradient;
  b. the context conv and the hyper decoder's last conv written into the two channel ranges of one NaN-filled
     [B, h, w, 4M] bf16 buffer with guard rows, every forced tile, with and without the finishing kernel; refusals;
  c. every other latent-side layer (LAYERS of conv_bf16_ref.py) forward and backward, with the automatic K split and
     with the split forced off; the LeakyReLU's backward bit for bit from the device's own stored output, on the
     one-pass column-sum route and the plain one;
  d. JointAutoregressiveHierarchical(M, K) in bf16 precision, latent side only: phi, psi, combined, the raw entropy
     parameters and every gradient bit for bit the explicit composition of the same launches; the torch.cat route gives
     the same bits as the slice route;
  e. the fp32 masked conv into a slice (what the fp32 model runs), forward and backward against the oracle.

Every output of a direct launch is a view inside a larger NaN-filled allocation whose neighbouring rows are checked
afterwards.  Every launch asserts through KERNEL_TRACE which igemm_bf16_kernel<BM, TN, SQ, FUSE, RING, NWV> ran and, from
the workspace the planner asked for, its K split; a split launch's main kernel writes fp32 slabs only, so a finite
output in the NaN-filled tensor is igemm_bf16_finish_kernel's.  Every figure is printed as
`RATIO <group> <case> <what> <value>` before it is asserted; `ERRS` lines carry the raw err / S the constant A is
chosen from.

Kernel variants a trace of this module shows: igemm_bf16_kernel<64, 1 | 2 | 3, false, false, 3, 4>,
<128, 1 | 2, false, false, 4, 4>, <128, 3, false, false, 3, 4>, <256, 1 | 2 | 3, false, false, 4, 8>,
igemm_bf16_finish_kernel, wgrad_bf16_kernel, the bf16 column-sum kernels and leaky_bwd_bf16_kernel; no halo kernel.

Measured on the MI355X: worst err / S of an unsplit launch 1.934e-07 (c, the data gradient of ep1 at M = 192 on the
2 x 16 x 16 grid), of a K-split launch 8.32e-08 (a, the data gradient at M = 192, BM 128, 5 splits); A = 2^-20 =
9.54e-07 (4 x the unsplit figure, rounded up to a power of two; conv_bf16_ref.py).  Worst RATIO per group, each against
a bound of 1:

    a  context conv      y 0.117 (M192 1x13x20 bm256)   y split 0.079   dx 0.104 (M64 1x13x20 bm256)   dx split 0.087
                         dw 0.004   db 0.001            every bf16 output bit for bit
    b  slices            0.99 of half a bf16 ulp + A S (the rounding itself uses the half ulp); slices and the
                         untouched rest bit for bit
    c  other layers      y 0.129 (hd3 M128 1x13x20)     y split 0.058   dx 0.203 (ep1 M192 2x16x16)    dx split 0.076
                         dw 0.006   db 0.010            masked gradients and every bf16 output bit for bit
    d  module            every tensor and gradient bit for bit, slice route and torch.cat route
    e  fp32 into a slice y, dx 0.014, dw 0.004, db 0.000 of the 1e-4 band

No kernel, packing or Python error was found: no bf16 store differed from its rounded fp32 value in any variant, so the
fall-back band of half a bf16 ulp is used nowhere but in b's float64 cross-check.

Run on the MI355X box:  python -m pytest tests/test_gpu_latent_bf16.py -m gpu -q -s"""
import functools

import numpy as np
import pytest
import torch

import conv_bf16_ref as R
from test_gpu_gdn_bf16 import CANARY16, CANARY32, Guarded, bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FORCED_BM = (64, 128, 256)
FORCED_SPLIT = (1, 3, 5)


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
    # what A is chosen from: the worst err / S of the unsplit and of the K-split launches of this run
    print(f"\nMEASURED unsplit {ERRS['unsplit']:.4e} split {ERRS['split']:.4e} A_BAND {R.A_BAND:.4e}")


def ratio(group, tag, what, value):
    print(f"RATIO {group} {tag} {what} {value:.4f}")
    return value


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw64(t):
    """a device NHWC tensor -> float64 NCHW on the CPU"""
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def bf(a, dev):
    t = a.to(BF)
    assert torch.equal(t.float(), a.float()), "the input is not bf16-exact"
    return t.to(dev)


def close_norm(a, b, rtol=1e-4, what=""):
    e = R.norm_err(a, b)
    assert e <= rtol, f"{what}: {e:.3e} of the tensor's maximum (allowed {rtol:.3e})"
    return e / rtol


def colsum_ratio(db, g64):
    """the existing column-sum band: |db - sum g| <= 1e-5 sum |g| + 1e-6, as a ratio"""
    ref = g64.sum(dim=(0, 2, 3))
    tol = 1e-5 * g64.abs().sum(dim=(0, 2, 3)) + 1e-6
    return float(((R.f64(db.detach().cpu()) - ref).abs() / tol).max())


@functools.lru_cache(maxsize=None)
def _grads_cached(case):
    return R.grads_ref(case, R.inputs(case)["g"])


class Ops:
    """the device operands of a case (NHWC bf16 activations, the fp32 weight and bias) and its geometry"""

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
        self.chunks = R.max_chunks(lay.k, lay.s, lay.transposed, lay.mask, lay.cin, lay.p)
        self.chunks_dx = R.max_chunks(lay.k, lay.s, not lay.transposed, lay.mask, lay.cout, lay.p)
        self.P = self.B * self.Ho * self.Wo


def traced(env, force, fn):
    """run fn() under FORCE_IGEMM = force with a kernel trace -> (result, names)"""
    F_ = env[0]
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = force, names
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    return out, names


def planned_ksplit(env, geo, tap_mask, force):
    """the K split of the launch that just ran, from the workspace _igemm_bf16 asked the planner for"""
    FB = env[1]
    fb, fs = (force[0], force[2]) if force else (0, 0)
    key = (geo["B"], geo["Hi"], geo["Wi"], geo["Cin"], geo["Ho"], geo["Wo"], geo["Cout"], geo["kh"], geo["kw"],
           geo["stride"], geo["pad"], bool(geo["transposed"]), tap_mask, fs, fb)
    nbytes = FB._SPLIT_WS.get(key, 0)
    per = 4 * geo["B"] * geo["Ho"] * geo["Wo"] * geo["Cout"]
    assert nbytes % per == 0
    return max(nbytes // per, 1)


def check_plan(env, names, geo, tap_mask, force, chunks, what):
    fb, fs = (force[0], force[2]) if force else (0, 0)
    want = R.expected_kernel(geo["Cout"], fb)
    assert names == {want}, (what, names, want)
    ks = planned_ksplit(env, geo, tap_mask, force)
    assert ks == R.expected_ksplit(geo["Ho"], geo["Wo"], geo["Cout"], chunks, fb, fs), (what, ks, force)
    return ks


def forward(env, o, force, out_f32, leaky=False):
    """one forward launch of the case through FB._igemm_bf16 into a guarded NaN-filled tensor -> (NCHW float64, ksplit)"""
    F_, FB, L, dev = env
    lay = o.lay
    wp = FB._pack_conv_weight_bf16(o.w, lay.transposed, False)
    out = Guarded(o.P, lay.cout, dev, torch.float32 if out_f32 else BF)
    view = out.t.view(o.B, o.Ho, o.Wo, lay.cout)
    _, names = traced(env, force, lambda: FB._igemm_bf16(
        o.x, wp, view, bias=o.b, epilogue=L.EPI_LEAKY if leaky else L.EPI_NONE, slope=R.SLOPE, tap_mask=lay.mask, **o.geo))
    what = f"{R.case_id(o.case)} forward {force}"
    ks = check_plan(env, names, o.geo, lay.mask, force, o.chunks, what)
    out.check(what)
    y = nchw64(view)
    assert not bool(torch.isnan(y).any()), f"{what}: an element kept its NaN (ksplit {ks}: the finishing launch writes it)"
    return y, ks


def backward(env, o, force, in_dtype, need=(True, True, True), leaky_y=None, g=None):
    """FB._conv_backward_bf16 of the case -> (dx NCHW float64 or None, dw, db, ksplit of the data gradient)"""
    F_, FB, L, dev = env
    lay = o.lay
    g = o.g if g is None else g
    (dx, dw, db), names = traced(env, force, lambda: FB._conv_backward_bf16(
        o.x, o.w, g, lay.s, lay.p, lay.transposed, in_dtype, lay.mask, need[0], need[1], need[2], leaky_y=leaky_y,
        slope=R.SLOPE))
    ks = 1
    if need[0]:
        geo = dict(B=o.B, Hi=o.Ho, Wi=o.Wo, Cin=lay.cout, Ho=o.Hi, Wo=o.Wi, Cout=lay.cin, kh=lay.k, kw=lay.k,
                   stride=lay.s, pad=lay.p, transposed=not lay.transposed)
        ig = {n for n in names if n.startswith("igemm_bf16_kernel")}
        ks = check_plan(env, ig, geo, lay.mask, force, o.chunks_dx, f"{R.case_id(o.case)} dgrad {force}")
        assert dx.dtype == in_dtype
        dx = dx.detach().cpu().double()
        assert not bool(torch.isnan(dx).any())
    assert not any("halo" in n for n in names), names
    return dx, (None if dw is None else dw.detach().cpu().double()), db, ks


def same_bits_as_rounded(y16, y32, what):
    """a bf16 output is rne_bf16 of the fp32 output of the same variant"""
    assert torch.equal(y16, R.rne_bf16(y32)), f"{what}: the bf16 store is not the rounded fp32 value"


ERRS = {"unsplit": 0.0, "split": 0.0}


def banded(group, tag, what, dev64, ref64, S, ks):
    e = R.err_over_S(dev64, ref64, S)
    key = "unsplit" if ks == 1 else "split"
    ERRS[key] = max(ERRS[key], e)
    print(f"ERRS {group} {tag} {what} {key} {e:.3e}")
    r = ratio(group, tag, what + ("" if ks == 1 else "-split"), R.band_ratio(dev64, ref64, S))
    assert r <= 1.0, (tag, what, r)
    return r


def check_dw_db(group, tag, case, dw, db, gr, g64):
    """weight gradient per tap at 1e-4 of that tap's own scale (dead taps too: the gradient is not masked), bias
    gradient at the column-sum band"""
    k = dw.shape[2]
    worst = 0.0
    for r in range(k):
        for s in range(k):
            worst = max(worst, close_norm(dw[:, :, r, s], gr.dw[:, :, r, s], 1e-4, f"{tag} dw tap ({r},{s})"))
    ratio(group, tag, "dw", worst)
    rb = ratio(group, tag, "db", colsum_ratio(db, g64))
    assert rb <= 1.0, (tag, rb)


# ---------------------------------------------------------------------------------------------
# a. masked context conv
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CTX_CASES, ids=R.case_id)
def test_a_ctx_forward(env, case):
    o = Ops(env, case)
    ref = R.forward_ref(case)
    assert R.live_taps(o.lay.mask, 5) == 12 and o.chunks == 12 * (o.lay.cin // 32)
    seen = set()
    for bm in FORCED_BM:
        for sp in FORCED_SPLIT:
            force, tag = (bm, 0, sp), f"{R.case_id(case)}-bm{bm}-s{sp}"
            y32, ks = forward(env, o, force, True)
            seen.add(ks)
            banded("a", tag, "y", y32, ref.y, ref.S, ks)
            y16, ks16 = forward(env, o, force, False)
            assert ks16 == ks
            same_bits_as_rounded(y16, y32, tag)
    assert seen == {1, 3, 5}, seen      # (1: the forced 1 and every 256-row launch, which has no split)


@pytest.mark.parametrize("case", R.CTX_CASES, ids=R.case_id)
def test_a_ctx_backward(env, case):
    o = Ops(env, case)
    gr = _grads_cached(case)
    g64 = R.f64(o.i["g"])
    for bm in FORCED_BM:
        for sp in FORCED_SPLIT:
            force, tag = (bm, 0, sp), f"{R.case_id(case)}-bm{bm}-s{sp}"
            dx32, _, _, ks = backward(env, o, force, torch.float32, (True, False, False))
            banded("a", tag, "dx", dx32, gr.dx, gr.S_dx, ks)
            dx16, _, _, _ = backward(env, o, force, BF, (True, False, False))
            same_bits_as_rounded(dx16, dx32, tag + " dx")
    _, dw, db, _ = backward(env, o, None, torch.float32, (False, True, True))
    check_dw_db("a", R.case_id(case), case, dw, db, gr, g64)
    live = R.mask_array(o.lay.mask, 5)
    assert float(gr.dw[:, :, live == 0].abs().max()) > 0      # (the dead taps' gradients are there to be got wrong)


# ---------------------------------------------------------------------------------------------
# b. channel slices
# ---------------------------------------------------------------------------------------------
SLICE_FORCES = [(64, 0, 1), (128, 0, 1), (256, 0, 1), (64, 0, 3), (128, 0, 5)]


def conv2d_call(env, o, out=None, **kw):
    FB = env[1]
    lay = o.lay
    args = dict(out_f32=False, leaky=False, slope=R.SLOPE, tap_mask=lay.mask, out=out)
    args.update(kw)
    return FB.conv2d_bf16(o.x.permute(0, 3, 1, 2), o.w, o.b, lay.s, lay.p, **args)


@pytest.mark.parametrize("M,K,grid", [(M, K, grid) for (r, M, K) in R.ROWS if r == "ctx" for grid in R.GRIDS],
                         ids=lambda v: str(v).replace(" ", ""))
def test_b_two_producers_one_buffer(env, M, K, grid):
    F_, FB, L, dev = env
    ctx, hd3 = Ops(env, ("ctx", M, K, grid)), Ops(env, ("hd3", M, K, grid))
    B, h, w = grid
    c_phi, c_psi = ctx.lay.cout, hd3.lay.cout
    C = c_phi + c_psi
    assert C == 4 * M and (ctx.Ho, ctx.Wo, hd3.Ho, hd3.Wo) == (h, w, h, w)
    for force in SLICE_FORCES:
        tag = f"M{M}-{B}x{h}x{w}-bm{force[0]}-s{force[2]}"
        buf = Guarded(B * h * w, C, dev)
        comb = buf.t.view(B, h, w, C)
        raw = buf.t.view(torch.int16)
        fresh = {}
        for o, lo, hi in ((ctx, 0, c_phi), (hd3, c_phi, C)):
            fresh[lo], names_f = traced(env, force, lambda: conv2d_call(env, o))
            before = raw.clone()
            res, names = traced(env, force, lambda: conv2d_call(env, o, out=comb[..., lo:hi]))
            assert names == names_f == {R.expected_kernel(o.lay.cout, force[0])}, (tag, names, names_f)
            geo = dict(o.geo)
            ks = planned_ksplit(env, geo, o.lay.mask, force)
            assert ks == R.expected_ksplit(h, w, o.lay.cout, o.chunks, force[0], force[2]), (tag, ks)
            assert res.data_ptr() == comb[..., lo:hi].data_ptr() and tuple(res.shape) == (B, hi - lo, h, w)
            # the slice: the same launch into a fresh tensor, bit for bit
            assert torch.equal(bits(comb[..., lo:hi]), bits(fresh[lo].permute(0, 2, 3, 1))), f"{tag}: slice {lo}:{hi}"
            assert not bool(torch.isnan(comb[..., lo:hi].float()).any())
            # everything outside it: untouched (the canary, or what the other producer wrote before)
            keep = torch.ones(C, dtype=torch.bool, device=dev)
            keep[lo:hi] = False
            assert torch.equal(raw[:, keep], before[:, keep]), f"{tag}: wrote outside channels {lo}:{hi}"
            if lo == 0:
                assert bool((raw[:, hi:] == CANARY16).all())
            buf.check(tag)
        # against the reference too: the slices hold the layers' outputs (fp32 band + the bf16 store's half ulp)
        for o, lo, hi in ((ctx, 0, c_phi), (hd3, c_phi, C)):
            ref = R.forward_ref(o.case)
            got = nchw64(comb[..., lo:hi])
            tol = R.A_BAND * ref.S + 2.0 ** -8 * ref.y.abs()
            r = ratio("b", f"{tag}-{o.lay.role}", "y16", float(((got - ref.y).abs() / tol.clamp_min(1e-300)).max()))
            assert r <= 1.0


def test_b_refusals_launch_nothing(env):
    F_, FB, L, dev = env
    case = ("ctx", 64, 3, (3, 5, 7))
    o = Ops(env, case)
    B, h, w, Co = o.B, o.Ho, o.Wo, o.lay.cout
    buf = Guarded(B * h * w, 2 * Co, dev)
    comb = buf.t.view(B, h, w, 2 * Co)
    f32 = torch.zeros((B, h, w, 2 * Co), device=dev)
    bad = [
        ("a slice starting at channel 4", dict(out=comb[..., 4:4 + Co])),
        ("leaky with out", dict(out=comb[..., :Co], leaky=True)),
        ("out_f32 with out", dict(out=comb[..., :Co], out_f32=True)),
        ("one channel short", dict(out=comb[..., :Co - 8])),
        ("one row short", dict(out=comb[:, :h - 1, :, :Co])),
        ("a transposed view", dict(out=comb[..., :Co].permute(0, 2, 1, 3))),
        ("an fp32 buffer", dict(out=f32[..., :Co])),
    ]
    for what, kw in bad:
        names = set()
        F_.KERNEL_TRACE = names
        try:
            with pytest.raises(ValueError):
                conv2d_call(env, o, **kw)
        finally:
            F_.KERNEL_TRACE = None
        torch.cuda.synchronize()
        assert not names, (what, names)
        assert buf.untouched() and not bool(f32.any()), what
    # (and the slice that is accepted, so that the refusals above are not refusals of everything)
    conv2d_call(env, o, out=comb[..., 8:8 + Co])
    torch.cuda.synchronize()
    buf.check("accepted slice")
    assert not bool(torch.isnan(comb[..., 8:8 + Co].float()).any()) and bool(torch.isnan(comb[..., :8].float()).all())


# ---------------------------------------------------------------------------------------------
# c. every other layer
# ---------------------------------------------------------------------------------------------
SPLITS_C = (None, (0, 0, 1))        # what training dispatches (the automatic split) and the split forced off


@pytest.mark.parametrize("case", R.OTHER_CASES, ids=R.case_id)
def test_c_forward(env, case):
    F_, FB, L, dev = env
    o = Ops(env, case)
    lay = o.lay
    ref = R.forward_ref(case)
    want = R.leaky_ref(ref.y) if lay.leaky else ref.y
    auto_ks = None
    for force in SPLITS_C:
        tag = f"{R.case_id(case)}-{'auto' if force is None else 'nosplit'}"
        y32, ks = forward(env, o, force, True, lay.leaky)      # (fp32 + LEAKY: the C ABI allows it)
        banded("c", tag, "y", y32, want, ref.S, ks)
        y16, ks16 = forward(env, o, force, False, lay.leaky)
        assert ks16 == ks
        same_bits_as_rounded(y16, y32, tag)
        if force is None:
            auto_ks = ks
        else:
            assert ks == 1
    if lay.role in ("he2", "he3", "hd1") and case[1] == 192 and case[3] == (2, 16, 16):
        assert auto_ks > 1, "the z-level 5x5 layers of the training shape split K on their own"
    if lay.leaky and lay.out == "bf16":      # the autograd wrapper refuses the form launched directly above
        fn = FB.conv_transpose2d_bf16 if lay.transposed else FB.conv2d_bf16
        extra = (lay.op,) if lay.transposed else ()
        with pytest.raises(NotImplementedError):
            fn(o.x.permute(0, 3, 1, 2), o.w, o.b, lay.s, lay.p, *extra, out_f32=True, leaky=True)


@pytest.mark.parametrize("case", R.OTHER_CASES, ids=R.case_id)
def test_c_backward(env, case):
    F_, FB, L, dev = env
    from neural_image_compression_amd.reductions import _leaky_bwd_colsum_bf16
    o = Ops(env, case)
    lay = o.lay
    tag = R.case_id(case)
    y_dev = g1 = None
    g64 = R.f64(o.i["g"])
    if lay.leaky:
        # the device's own stored y is the mask: the kernel's rounding point, no element is ambiguous
        wp = FB._pack_conv_weight_bf16(o.w, lay.transposed, False)
        y_dev = torch.empty((o.B, o.Ho, o.Wo, lay.cout), device=dev, dtype=BF)
        FB._igemm_bf16(o.x, wp, y_dev, bias=o.b, epilogue=L.EPI_LEAKY, slope=R.SLOPE, **o.geo)
        g1, db1 = _leaky_bwd_colsum_bf16(y_dev, o.g, R.SLOPE, o.P, lay.cout)
        g2 = FB._leaky_bwd_bf16(y_dev, o.g, R.SLOPE)
        torch.cuda.synchronize()
        gq = R.leaky_bwd_ref(nchw64(y_dev), g64)
        assert torch.equal(nchw64(g1), gq), f"{tag}: the one-pass route's masked gradient"
        assert torch.equal(nchw64(g2), gq), f"{tag}: leaky_bwd_bf16_kernel's masked gradient"
        share = float((nchw64(y_dev) <= 0).double().mean())
        assert 0.35 <= share <= 0.65, share
        assert ratio("c", tag, "db-onepass", colsum_ratio(db1, gq)) <= 1.0
        g64 = gq
        gr = R.grads_ref(case, gq)
    else:
        gr = _grads_cached(case)
    first = None
    for force in SPLITS_C:
        ftag = f"{tag}-{'auto' if force is None else 'nosplit'}"
        dx32, dw, db, ks = backward(env, o, force, torch.float32, (True, True, True), leaky_y=y_dev)
        banded("c", ftag, "dx", dx32, gr.dx, gr.S_dx, ks)
        check_dw_db("c", ftag, case, dw, db, gr, g64)
        dx16, _, _, _ = backward(env, o, force, BF, (True, False, False), leaky_y=y_dev)
        same_bits_as_rounded(dx16, dx32, ftag + " dx")
        # the need_db = False route (leaky rows: lic_leaky_bwd_bf16 instead of the one-pass kernel): the same bits
        dx_b, dw_b, db_b, _ = backward(env, o, force, torch.float32, (True, True, False), leaky_y=y_dev)
        assert db_b is None and torch.equal(dx_b, dx32) and torch.equal(dw_b, dw), ftag
        if force is not None:
            assert ks == 1
        if first is None:
            first = dw
        else:
            assert torch.equal(first, dw), "the weight gradient does not depend on the data gradient's split"


# ---------------------------------------------------------------------------------------------
# d. module level
# ---------------------------------------------------------------------------------------------
def _module_setup(env, M, K):
    F_, FB, L, dev = env
    import neural_image_compression_amd as nic
    torch.manual_seed(1000 + M + K)
    model = nic.JointAutoregressiveHierarchical(M, K).to(dev).set_precision("bf16")
    r = R._rng(f"module-{M}-{K}")
    B, h, w = 2, 16, 16
    hz = wz = 4

    def t(shape, scale=1.0, uniform=False):
        a = r.random_sample(shape) if uniform else r.standard_normal(shape) * scale
        return torch.as_tensor(a.astype(np.float32)).to(dev)
    y = t((B, h, w, M), 3.0).permute(0, 3, 1, 2).requires_grad_(True)
    uy = t((B, h, w, M), uniform=True).permute(0, 3, 1, 2)
    uz = t((B, hz, wz, M), uniform=True).permute(0, 3, 1, 2)
    cout = 2 * M if K == 1 else 3 * K * M
    G = t((B, h, w, cout)).permute(0, 3, 1, 2)
    x = torch.zeros((B, 3, 256, 256), device=dev)
    model.encoder.forward = lambda _x: y       # latent side only: y given, no analysis stack
    return model, x, y, (uz, uy), G


LATENT_MODULES = ("hyper_encoder", "hyper_decoder", "context_model", "entropy_parameters")


def _latent_grads(model):
    out = {}
    for name in LATENT_MODULES:
        for pn, p in getattr(model, name).named_parameters():
            assert p.grad is not None, (name, pn)
            out[f"{name}.{pn}"] = p.grad.detach().clone()
    return out


def _zero_grads(model, *ts):
    for p in model.parameters():
        p.grad = None
    for t in ts:
        t.grad = None


def _run_model(model, x, noise, G):
    """analysis_hyperprior with hooks on the latent side -> dict of phi, psi, combined, raw and the gradients"""
    cap, hooks = {}, []
    hooks.append(model.context_model.register_forward_hook(lambda m, a, out: cap.__setitem__("phi", out)))
    hooks.append(model.hyper_decoder.register_forward_hook(lambda m, a, out: cap.__setitem__("psi", out)))
    ep = model.entropy_parameters.net
    hooks.append(ep[0].register_forward_pre_hook(lambda m, a: cap.__setitem__("combined", a[0])))
    hooks.append(ep[-1].register_forward_hook(lambda m, a, out: cap.__setitem__("raw", out)))
    try:
        out = model.analysis_hyperprior(x, True, noise)
    finally:
        for hk in hooks:
            hk.remove()
    for k in ("y_in", "z_in", "z"):
        out[k].retain_grad()
    cap["raw"].backward(G)
    torch.cuda.synchronize()
    cap.update(y_in=out["y_in"], z_in=out["z_in"], z=out["z"])
    return cap


def _explicit(env, model, y, noise, G):
    """the same latent side as direct launches: FB._igemm_bf16 forward, FB._conv_backward_bf16 backward"""
    F_, FB, L, dev = env
    uz, uy = noise
    he, hd, ep, mc = model.hyper_encoder.net, model.hyper_decoder.net, model.entropy_parameters.net, model.context_model.masked

    def fwd(xh, m, leaky=False, f32=False, out=None, tap_mask=0):
        tr = type(m).__name__ == "ConvTranspose2d"
        k, s, p = m.weight.shape[2], m.stride[0], m.padding[0]
        B, Hi, Wi, Cin = xh.shape
        Cout = m.weight.shape[1] if tr else m.weight.shape[0]
        Ho, Wo = F_.conv_out_size(Hi, Wi, k, s, p, tr, m.output_padding[0] if tr else 0)
        o = out if out is not None else torch.empty((B, Ho, Wo, Cout), device=dev, dtype=torch.float32 if f32 else BF)
        FB._igemm_bf16(xh, FB._pack_conv_weight_bf16(m.weight, tr, False), o, B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo,
                       Cout=Cout, kh=k, kw=k, stride=s, pad=p, transposed=tr, bias=m.bias.detach(),
                       epilogue=L.EPI_LEAKY if leaky else L.EPI_NONE, slope=0.01, tap_mask=tap_mask,
                       out_ld=None if out is None else out.stride(2))
        return o

    grads = {}

    def bwd(name, xh, m, g16, in_dtype, leaky_y=None, tap_mask=0):
        tr = type(m).__name__ == "ConvTranspose2d"
        dx, dw, db = FB._conv_backward_bf16(xh, m.weight.detach(), g16, m.stride[0], m.padding[0], tr, in_dtype, tap_mask,
                                            True, True, True, leaky_y=leaky_y, slope=0.01)
        grads[name + ".weight"], grads[name + ".bias"] = dw, db
        return dx.permute(0, 2, 3, 1)        # NHWC (the memory layout)

    with torch.no_grad():
        yd = y.detach()
        y16 = nhwc(yd).to(BF)
        y_in = F_.quantize(yd, uy, True)
        h1 = fwd(y16, he[0], leaky=True)
        h2 = fwd(h1, he[2], leaky=True)
        z = fwd(h2, he[4], f32=True)
        z_in = F_.quantize(z.permute(0, 3, 1, 2), uz, True)
        z16, yin16 = nhwc(z_in).to(BF), nhwc(y_in).to(BF)
        B, h, w, M = y16.shape
        c_phi = mc.out_channels
        comb = torch.empty((B, h, w, c_phi + hd[4].out_channels), device=dev, dtype=BF)
        d1 = fwd(z16, hd[0], leaky=True)
        d2 = fwd(d1, hd[2], leaky=True)
        psi = fwd(d2, hd[4], out=comb[..., c_phi:])
        phi = fwd(yin16, mc, out=comb[..., :c_phi], tap_mask=mc._tap_mask)
        e1 = fwd(comb, ep[0], leaky=True)
        e2 = fwd(e1, ep[2], leaky=True)
        raw = fwd(e2, ep[4], f32=True)
        # backward
        g = nhwc(G).to(BF)
        g = bwd("entropy_parameters.net.4", e2, ep[4], g, BF)
        g = bwd("entropy_parameters.net.2", e1, ep[2], g.contiguous(), BF, leaky_y=e2)
        dcomb = bwd("entropy_parameters.net.0", comb, ep[0], g.contiguous(), BF, leaky_y=e1)
        dy_in = bwd("context_model.masked", yin16, mc, dcomb[..., :c_phi].contiguous(), torch.float32, tap_mask=mc._tap_mask)
        g = bwd("hyper_decoder.net.4", d2, hd[4], dcomb[..., c_phi:].contiguous(), BF)
        g = bwd("hyper_decoder.net.2", d1, hd[2], g.contiguous(), BF, leaky_y=d2)
        dz_in = bwd("hyper_decoder.net.0", z16, hd[0], g.contiguous(), torch.float32, leaky_y=d1)
        g = bwd("hyper_encoder.net.4", h2, he[4], dz_in.contiguous().to(BF), BF)
        g = bwd("hyper_encoder.net.2", h1, he[2], g.contiguous(), BF, leaky_y=h2)
        dy = bwd("hyper_encoder.net.0", y16, he[0], g.contiguous(), torch.float32, leaky_y=h1)
        torch.cuda.synchronize()
    return dict(phi=phi, psi=psi, combined=comb, raw=raw, y_in=nhwc(y_in), z_in=nhwc(z_in), z=z, dy_in=dy_in, dz_in=dz_in,
                dy=dy + dy_in, grads=grads)


def _eq(a, b, what):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("M,K", [(128, 3), (192, 1)])
def test_d_module_latent_side(env, M, K):
    F_, FB, L, dev = env
    from neural_image_compression_amd.layers import run_bf16
    model, x, y, noise, G = _module_setup(env, M, K)
    names = set()
    F_.KERNEL_TRACE = names
    try:
        cap = _run_model(model, x, noise, G)
    finally:
        F_.KERNEL_TRACE = None
    assert not any("halo" in n for n in names), names
    assert cap["combined"].dtype == BF and cap["phi"].data_ptr() == cap["combined"].data_ptr(), "the slice route ran"
    mgrads = _latent_grads(model)
    m_dy, m_dyin, m_dzin = y.grad.clone(), cap["y_in"].grad.clone(), cap["z_in"].grad.clone()
    ex = _explicit(env, model, y, noise, G)
    tag = f"M{M}-K{K}"
    for k in ("y_in", "z_in", "z", "phi", "psi", "combined", "raw"):
        _eq(nhwc(cap[k]), ex[k].contiguous(), f"{tag} {k}")
    _eq(nhwc(m_dyin), ex["dy_in"].contiguous(), f"{tag} y_in.grad")
    _eq(nhwc(m_dzin), ex["dz_in"].contiguous(), f"{tag} z_in.grad")
    _eq(nhwc(m_dy), ex["dy"].contiguous(), f"{tag} y.grad")
    assert set(mgrads) == set(ex["grads"]), sorted(set(mgrads) ^ set(ex["grads"]))
    for k in sorted(mgrads):
        _eq(mgrads[k], ex["grads"][k].view_as(mgrads[k]), f"{tag} {k}.grad")
    # the dead taps of the context conv: the parameter is zeroed there, its gradient is not
    dead = R.mask_array(model.context_model.masked._tap_mask, 5) == 0
    wm = model.context_model.masked.weight.detach().cpu()
    assert float(wm[:, :, dead].abs().max()) == 0 and float(mgrads["context_model.masked.weight"].cpu()[:, :, dead].abs().max()) > 0
    # (the explicit composition is what groups a-c hold to float64 layer by layer)
    # the torch.cat route of models.py: the same kernels on the same operands -> the same bits
    _zero_grads(model, y)
    y_in = F_.quantize(y, noise[1], True, cast_in=True, cast_out=True)
    z_in = F_.quantize(model.hyper_encoder(y), noise[0], True, cast_out=True)
    y_in.retain_grad()
    z_in.retain_grad()
    psi = model.hyper_decoder(z_in)
    phi = model.context_model(y_in)
    combined = torch.cat([phi, psi], dim=1)
    raw = run_bf16(model.entropy_parameters.net, combined, out_f32=True)
    raw.backward(G)
    torch.cuda.synchronize()
    assert phi.data_ptr() != combined.data_ptr()
    for k, v in (("phi", phi), ("psi", psi), ("combined", combined), ("raw", raw)):
        _eq(nhwc(v), nhwc(cap[k]), f"{tag} cat route {k}")
    _eq(nhwc(y_in.grad), nhwc(m_dyin), f"{tag} cat route y_in.grad")
    _eq(nhwc(z_in.grad), nhwc(m_dzin), f"{tag} cat route z_in.grad")
    _eq(nhwc(y.grad), nhwc(m_dy), f"{tag} cat route y.grad")
    cgrads = _latent_grads(model)
    for k in sorted(mgrads):
        _eq(cgrads[k], mgrads[k], f"{tag} cat route {k}.grad")


# ---------------------------------------------------------------------------------------------
# e. the fp32 masked conv into a slice
# ---------------------------------------------------------------------------------------------
def test_e_fp32_masked_conv_into_slice(env):
    F_, FB, L, dev = env
    from oracle import oracle as O
    case = ("ctx", 64, 3, (3, 5, 7))
    i = R.inputs(case)
    lay = i["lay"]
    r = R._rng("e-fp32")
    x = (i["x"] + torch.as_tensor(r.standard_normal(tuple(i["x"].shape)).astype(np.float32)) * 2.0 ** -10)   # not bf16-exact
    w, b, g = i["w"] * 1.0009765625, i["b"], i["g"]
    B, Cin, h, wd = x.shape
    Co = lay.cout
    buf = Guarded(B * h * wd, 2 * Co, dev, torch.float32)
    comb = buf.t.view(B, h, wd, 2 * Co)
    xd = nhwc(x).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    wdv, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    names = set()
    F_.KERNEL_TRACE = names
    try:
        y = F_.conv2d(xd, wdv, bd, 1, 2, tap_mask=lay.mask, out=comb[..., Co:])
        torch.cuda.synchronize()
        buf.check("fp32 slice forward")
        assert bool((buf.buf.view(B * h * wd + 2, 2 * Co)[1:-1, :Co] == CANARY32).all()), "wrote outside its channels"
        y.backward(nhwc(g).to(dev).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
    finally:
        F_.KERNEL_TRACE = None
    assert y.data_ptr() == comb[..., Co:].data_ptr() and names
    wm = w.numpy() * O.mask_a(tuple(w.shape))
    ratio("e", R.case_id(case), "y", close_norm(nchw64(comb[..., Co:]), O.conv2d_fwd(x.numpy(), wm, b.numpy(), 1, 2), 1e-4, "y"))
    dx, dw, db = O.conv2d_bwd(x.numpy(), wm, g.numpy(), 1, 2)
    ratio("e", R.case_id(case), "dx", close_norm(xd.grad.cpu(), dx, 1e-4, "dx"))
    ratio("e", R.case_id(case), "dw", close_norm(wdv.grad.cpu(), dw, 1e-4, "dw (unmasked)"))
    ratio("e", R.case_id(case), "db", close_norm(bd.grad.cpu(), db, 1e-4, "db"))
    dead = R.mask_array(lay.mask, 5) == 0
    assert float(wdv.grad.cpu()[:, :, dead].abs().max()) > 0
    buf.check("fp32 slice backward")
