"""The bf16-storage GDN / IGDN kernels against tests/gdn_bf16_ref.py, the float64 statement of the operation at the
rounding points csrc/lic_epilogue_bf16.h defines.  Every bf16 output is held, element by element, to half a bf16 ulp
plus a derived fp32 term (the constants and their derivation are in gdn_bf16_ref.py); small exact-integer cases are
compared bit for bit, ties of the bf16 store among them.

  a. stand-alone forward: igemm_bf16_kernel<BM, TN, SQ = true> with the GDN / IGDN epilogue, BM 64 and 128 forced, at
     C = 64, 128, 192: stored norm and y banded; exact inputs: the stored norm bit for bit rne_bf16(n64);
  b. pool and finish of every fused conv -> GDN kernel (the geometries of test_gpu_bf16_epilogue_bits.FUSED): y and the
     stored norm against the reference forward of the kernel's own conv output;
  c. two-launch backward (lic_gdn_dnorm_bf16, then lic_igemm_bf16 with GDN_BWD / IGDN_BWD) at three widths;
  d. one-sweep backward reading the norm (lic_gdn_bwd_bf16), with and without the column sums, BIG included;
  e. one-sweep backward recomputing the norm (lic_gdn_bwd_bf16_recompute), with and without the column sums: at an
     element whose float64 pool lies within the norm band of a bf16 rounding boundary t and dx may come from either
     neighbouring bf16 norm, everywhere else from rne_bf16(n64);
  f. exact backward through c and d: t, dx and every column-sum row bit for bit (premise: v_rsq_f32 / v_sqrt_f32 are
     exact at 1 and 4, asserted on its own);
  g. a transposed panel misses the bands;
  h. layers.GDN(bf16=True) reaches these kernels: y and x.grad bit for bit the C-ABI launches', d beta and d gamma
     against float64 sums of the device's own t;
  i. refusals launch nothing.

Every output of a C-ABI launch is a view inside a larger allocation pre-filled with a NaN pattern; the row in front of
it and the row behind it are checked afterwards (b and h take the tensors the functional layer allocates).  Every
figure is printed as `RATIO <group> <case> <what> <value>` before it is asserted.  Which gdn_bwd_bf16_kernel<NT4, CS,
RN> a sweep launch runs is a function of (C, a column-sum buffer, the entry point) alone (gdn_bwd_bf16_run); igemm
launches assert their variant through KERNEL_TRACE.  A rocprofv3 kernel trace of this module lists all eight
gdn_bwd_bf16_kernel<2 | 4, false | true, false | true>, the six igemm_bf16_kernel<64 | 128, 1 | 2 | 3, true, false, 3, 4>,
the fused igemm <128, 1 | 2 | 3, false, true> and <256, 2, false, true, 4, 8>, both halo kernels, stem_gdn_bf16_kernel<2 | 4 |
6> and the two-launch route's igemm_bf16_kernel<64, 1 | 2 | 3, false, false, 3, 4> with gdn_dnorm_bf16_kernel.

Worst RATIO per group on the MI355X, each against a bound of 1 (no band's derivation had to be amended):

    a  stand-alone forward        norm 0.9988   y 0.9989                      (C64-igdn-P127, BM 64)
    b  fused pool and finish      norm 0.9968   y 0.9988                      (stem_192_12x12_igdn, stem_64_21x19)
    c  two-launch backward        t 0.9998      dx 0.9987                     (C64-gdn-P128)
    d  sweep, reading             t 0.9998      dx 0.9989   colsums 0.1489    (C64-gdn-P128, C64-gdn-BIG, C128-igdn-P33)
    e  sweep, recomputing         t 0.9998      dx 0.9989   colsums 0.1119    (C128-igdn-P129, C64-gdn-BIG, C128-gdn-P33)
    h  module                     d beta 0.0056 d gamma 0.0248                (C192-gdn-P357, C192-igdn-P357)

The bf16 figures sit just under 1 because over thousands of elements some exact value always lies next to a rounding
boundary, where round-to-nearest-even itself uses the whole half ulp; the fp32 term is what is left for the kernel.
Ambiguous elements of e: 0.52 % of a case at the most.

Run on the MI355X box:  python -m pytest tests/test_gpu_gdn_bf16.py -m gpu -q -s"""
import ctypes
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import gdn_bf16_ref as R
import gdn_ref64 as G
import golden_recipe as GR
import test_gpu_bf16_epilogue_bits as EB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CANARY16 = 0x7FC1            # a bf16 quiet NaN with a payload
CANARY32 = 0x7FC0BEEF        # an fp32 quiet NaN with a payload no arithmetic produces
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
SWEEP_WIDTHS = (64, 128)
SWEEP_CASES = [c for c in R.CASES if c[0] in SWEEP_WIDTHS]
EXACT_SIZES = (1, 33, 129, 357)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic  # noqa: F401
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd import functional_bf16 as FB
    L.load()  # must be the in-tree HIP extension; raises if missing
    return F_, FB, L, torch.device("cuda:0")


class Guarded:
    """a [rows][C] bf16 or fp32 output pre-filled with a NaN pattern, one canary row in front of it and one behind"""

    def __init__(self, rows, C, dev, dtype=BF):
        self.pat = CANARY16 if dtype == BF else CANARY32
        self.buf = torch.full(((rows + 2) * C,), self.pat, dtype=torch.int16 if dtype == BF else torch.int32, device=dev)
        self.rows, self.C = rows, C
        self.t = self.buf.view(dtype)[C:(rows + 1) * C].view(rows, C)
        assert self.t.data_ptr() % 16 == 0

    def check(self, what=""):
        assert bool((self.buf[:self.C] == self.pat).all()), f"{what}: the row in front of the output was written"
        assert bool((self.buf[-self.C:] == self.pat).all()), f"{what}: the row behind the output was written"

    def untouched(self):
        return bool((self.buf == self.pat).all())

    def cpu(self):
        return self.t.detach().cpu().contiguous()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bf(a, dev):
    """bf16-exact fp32 values -> a bf16 device tensor"""
    t = a.to(BF)
    assert torch.equal(t.float(), a.float()), "the input is not bf16-exact"
    return t.to(dev)


def ratio(group, tag, what, value):
    print(f"RATIO {group} {tag} {what} {value:.4f}")
    return value


_small = functools.lru_cache(maxsize=None)(R.banded_inputs)
_big = functools.lru_cache(maxsize=len(R.BIG_CASES))(R.banded_inputs)      # (0.6 GB of fp32: d and e share them)


def banded(case):
    return (_big if case[2] == R.BIG else _small)(*case)


@functools.lru_cache(maxsize=None)
def _fwd_ref_small(case):
    C, inverse, P = case
    i = banded(case)
    return R.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)


def fwd_ref(case):
    """(n64, rne_bf16(n64), y64) of the banded inputs; computed once per small case and left unchanged"""
    return _fwd_ref_small.__wrapped__(case) if case[2] == R.BIG else _fwd_ref_small(case)


# ---------------------------------------------------------------------------------------------
# launches (operands packed exactly as functional_bf16.py packs them)
# ---------------------------------------------------------------------------------------------
def launch_fwd(env, case, inp, bm=0, want_norm=True):
    """the stand-alone forward as _GDNBF16Fn.forward launches it -> (y, norm) bf16 on the CPU"""
    F_, FB, L, dev = env
    C, inverse, P = case
    x = bf(inp["x"], dev)
    beta_e = inp["beta_e"].to(dev)
    gT = FB._pack_bf16(inp["gamma_e"].to(dev).contiguous(), 1, C, C, 0, 1, C)
    y, norm = Guarded(P, C, dev), Guarded(P, C, dev)
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = ((bm, 0, 0) if bm else None), names
    try:
        FB._igemm_bf16(x, gT, y.t, B=1, Hi=1, Wi=P, Cin=C, Ho=1, Wo=P, Cout=C, kh=1, kw=1, stride=1, pad=0,
                       transposed=False, bias=beta_e, prologue=1, epilogue=L.EPI_IGDN if inverse else L.EPI_GDN,
                       out2=norm.t if want_norm else None, aux=x)
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    want = f"igemm_bf16_kernel<{bm if bm else 64}, {C // 64}, true, false"
    assert len(names) == 1 and all(n.startswith(want) for n in names), (names, want)
    y.check("y")
    norm.check("norm")
    if not want_norm:
        assert norm.untouched()
    return y.cpu(), norm.cpu()


def launch_dnorm(env, case, inp, norm=None):
    F_, FB, L, dev = env
    C, inverse, P = case
    g, x, n = bf(inp["g"], dev), bf(inp["x"], dev), bf(inp["norm"] if norm is None else norm, dev)
    t = Guarded(P, C, dev)
    L.check(L.load().lic_gdn_dnorm_bf16(_ptr(g), _ptr(x), _ptr(n), _ptr(t.t), P * C, inverse, F_._stream()), "dnorm")
    torch.cuda.synchronize()
    t.check("dnorm t")
    return t.cpu()


def launch_igemm_bwd(env, case, inp, t_dev, norm=None, out_f32=False):
    """dx of the two-launch route from the device's t, as _gdn_backward_bf16's `else` branch launches it"""
    F_, FB, L, dev = env
    C, inverse, P = case
    g, x, n = bf(inp["g"], dev), bf(inp["x"], dev), bf(inp["norm"] if norm is None else norm, dev)
    gp = FB._pack_bf16(inp["gamma_e"].to(dev).contiguous(), 1, C, C, 0, C, 1)
    dx = Guarded(P, C, dev, torch.float32 if out_f32 else BF)
    names = set()
    F_.KERNEL_TRACE = names
    try:
        FB._igemm_bf16(t_dev.to(dev), gp, dx.t, B=1, Hi=1, Wi=P, Cin=C, Ho=1, Wo=P, Cout=C, kh=1, kw=1, stride=1, pad=0,
                       transposed=False, epilogue=L.EPI_IGDN_BWD if inverse else L.EPI_GDN_BWD, aux=g, aux2=x, aux3=n)
        torch.cuda.synchronize()
    finally:
        F_.KERNEL_TRACE = None
    want = f"igemm_bf16_kernel<64, {C // 64}, false, false"
    assert len(names) == 1 and all(nm.startswith(want) for nm in names), (names, want)
    dx.check("two-launch dx")
    return dx.cpu()


def launch_sweep(env, case, inp, cs, norm=None, recompute=False, gamma_for_panel=None):
    """lic_gdn_bwd_bf16 (gdn_bwd_bf16_kernel<C / 32, cs, false>) or lic_gdn_bwd_bf16_recompute (<C / 32, cs, true>) ->
    (t, dx, colsum_t_partial, colsum_dx_partial) on the CPU (the partials None without `cs`)"""
    F_, FB, L, dev = env
    C, inverse, P = case
    lib = L.load()
    g, x = bf(inp["g"], dev), bf(inp["x"], dev)
    gamma_e = (inp["gamma_e"] if gamma_for_panel is None else gamma_for_panel).to(dev).contiguous()
    gp = FB._pack_bf16(gamma_e, 1, C, C, 0, C, 1, kperm=True)
    rows = lib.lic_gdn_bwd_bf16_partial_rows(P)
    assert rows == R.sweep_grid(P)
    t, dx = Guarded(P, C, dev), Guarded(P, C, dev)
    pt, pdx = Guarded(rows, C, dev, torch.float32), Guarded(rows, C, dev, torch.float32)
    if recompute:
        gTp = FB._pack_bf16(inp["gamma_e"].to(dev).contiguous(), 1, C, C, 0, 1, C, kperm=True)
        beta_e = inp["beta_e"].to(dev)
        L.check(lib.lic_gdn_bwd_bf16_recompute(_ptr(g), _ptr(x), _ptr(gp), _ptr(gTp), _ptr(beta_e), _ptr(dx.t), _ptr(t.t),
                                               _ptr(pt.t) if cs else None, _ptr(pdx.t) if cs else None, P, C, inverse,
                                               F_._stream()), "lic_gdn_bwd_bf16_recompute")
    else:
        n = bf(inp["norm"] if norm is None else norm, dev)
        L.check(lib.lic_gdn_bwd_bf16(_ptr(g), _ptr(x), _ptr(n), _ptr(gp), _ptr(dx.t), _ptr(t.t), _ptr(pt.t) if cs else None,
                                     _ptr(pdx.t) if cs else None, P, C, inverse, F_._stream()), "lic_gdn_bwd_bf16")
    torch.cuda.synchronize()
    for o, what in ((t, "t"), (dx, "dx"), (pt, "colsum_t_partial"), (pdx, "colsum_dx_partial")):
        o.check(what)
    if not cs:
        assert pt.untouched() and pdx.untouched()
        return t.cpu(), dx.cpu(), None, None
    return t.cpu(), dx.cpu(), pt.cpu(), pdx.cpu()


def check_colsums(group, tag, pt, pdx, t, dx, P):
    """every row of both partial buffers against the float64 sums of the device's own bf16 t / dx"""
    worst = 0.0
    for part, src, what in ((pt, t, "cs_t"), (pdx, dx, "cs_dx")):
        assert not bool(torch.isnan(part).any()), f"{what}: a row kept its NaN"
        worst = max(worst, ratio(group, tag, what, R.colsum_ratio(part, src.double(), R.sweep_grid(P))))
    return worst


# ---------------------------------------------------------------------------------------------
# a. stand-alone forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_a_forward_banded(env, case):
    C, inverse, P = case
    inp = banded(case)
    n64, nq, y64 = fwd_ref(case)
    rs = []
    for bm in (64, 128):
        tag = f"{R.case_id(case)}-bm{bm}"
        y, norm = launch_fwd(env, case, inp, bm)
        rs.append(ratio("a", tag, "norm", R.band_ratio(norm, n64, n64, R.K_FWD(C))))
        rs.append(ratio("a", tag, "y", R.band_ratio(y, y64, y64.abs(), R.K_FWD(C))))
        y2, _ = launch_fwd(env, case, inp, bm, want_norm=False)      # as the layer runs it where the norm is recomputed
        assert torch.equal(bits(y2), bits(y))
    assert max(rs) <= 1.0, rs


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_a_forward_exact(env, case):
    """the pool of the exact inputs is exact in fp32 in any order: the stored norm is rne_bf16(n64) bit for bit, ties
    among it; y is banded (v_rsq_f32 is not exact in general)"""
    C, inverse, P = case
    inp = R.exact_fwd_inputs(*case)
    n64, nq, y64 = R.fwd(inp["x"], inp["beta_e"], inp["gamma_e"], inverse)
    rs = []
    for bm in (64, 128):
        y, norm = launch_fwd(env, case, inp, bm)
        bad = R.bf16_bits(norm) != R.bf16_bits(nq)
        assert not bool(bad.any()), f"norm: {int(bad.sum())} values differ, first in row {int(bad.any(1).nonzero()[0])}"
        rs.append(ratio("a", f"exact-{R.case_id(case)}-bm{bm}", "y", R.band_ratio(y, y64, y64.abs(), R.K_FWD(C))))
    assert max(rs) <= 1.0, rs


# ---------------------------------------------------------------------------------------------
# b. pool and finish of the fused conv -> GDN kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(EB.FUSED))
def test_b_fused_pool_and_finish(env, key):
    """FB.conv_gdn_bf16 with gradients enabled on the geometries of test_gpu_bf16_epilogue_bits.FUSED (its inputs too);
    the convolution is not under test: its bf16 output, saved for the backward pass, is the reference's input"""
    F_, FB, L, dev = env
    from neural_image_compression_amd.layers import GDN
    k, s, p, ci, co, H, W, B, tr, op, inverse, bm = EB.FUSED[key]
    r = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    stem = ci < 4
    x = EB.rb(r.randn(B, ci, H, W).astype(np.float32))
    wshape = (ci, co, k, k) if tr else (co, ci, k, k)
    w = torch.from_numpy(EB.rb(r.randn(*wshape).astype(np.float32) / math.sqrt(ci * k * k))).to(dev).requires_grad_(True)
    b = torch.from_numpy(EB.rb(0.1 * r.randn(co).astype(np.float32))).to(dev).requires_grad_(True)
    m = GDN(co, inverse=inverse).to(dev)
    with torch.no_grad():
        m.beta.copy_(torch.from_numpy(GR.make_param("g.beta", (co,), 3)))
        m.gamma.copy_(torch.from_numpy(GR.make_param("g.gamma", (co, co), 3)))
    bb, gb, pd = m.beta_reparam.bound_value, m.gamma_reparam.bound_value, m.beta_reparam.pedestal_value
    tx = EB.nhwc(x, dev, None if stem else BF)
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = (bm, 0, 0), names
    try:
        y = FB.conv_gdn_bf16(tx, w, b, m.beta, m.gamma, s, p, inverse, bb, gb, pd, transposed=tr, output_padding=op)
        _, _, conv_out, norm, _, _ = y.grad_fn.saved_tensors
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    if stem:
        assert f"stem_gdn_bf16_kernel<{co // 32}, {8 if co == 192 else 4}>" in names, names
    elif bm == 512:
        assert ("halo_convt_bf16_kernel<2, true>" if tr else "halo_conv_bf16_kernel<2, true, 0>") in names, names
    else:
        assert any(n.startswith(f"igemm_bf16_kernel<{256 if bm == 256 else 128}, {co // 64}, false, true") for n in names), names
    assert conv_out is not None and conv_out.dtype == BF and (norm is not None) == (co == 192)
    # the re-parametrised operands as the device formed them (the re-parametrisation has its own tests)
    beta_e, gamma_e = FB._gamma_eff(m.beta.detach(), bb, pd).cpu(), FB._gamma_eff(m.gamma.detach(), gb, pd).cpu()
    xc = conv_out.detach().reshape(-1, co).cpu()
    n64, nq, y64 = R.fwd(xc.float(), beta_e, gamma_e, inverse)
    yd = y.detach().permute(0, 2, 3, 1).reshape(-1, co).cpu()
    assert yd.shape == xc.shape
    rs = [ratio("b", key, "y", R.band_ratio(yd, y64, y64.abs(), R.K_FWD(co)))]
    if norm is not None:
        rs.append(ratio("b", key, "norm", R.band_ratio(norm.detach().reshape(-1, co).cpu(), n64, n64, R.K_FWD(co))))
    assert max(rs) <= 1.0, rs


# ---------------------------------------------------------------------------------------------
# c. two-launch backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_c_two_launch_backward(env, case):
    C, inverse, P = case
    inp = banded(case)
    tag = R.case_id(case)
    t = launch_dnorm(env, case, inp)
    t64, dx64, mag = R.bwd(inp["g"], inp["x"], inp["norm"], inp["gamma_e"], inverse, t_dev=t)
    rt = ratio("c", tag, "t", R.band_ratio(t, t64, t64.abs(), R.K_T))
    dx = launch_igemm_bwd(env, case, inp, t)
    rdx = ratio("c", tag, "dx", R.band_ratio(dx, dx64, mag, R.K_DX(C)))
    assert rt <= 1.0 and rdx <= 1.0, (rt, rdx)


# ---------------------------------------------------------------------------------------------
# d. one-sweep backward, reading the norm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP_CASES + R.BIG_CASES, ids=R.case_id)
def test_d_sweep_reading(env, case):
    C, inverse, P = case
    inp = banded(case)
    tag = R.case_id(case)
    t, dx, _, _ = launch_sweep(env, case, inp, cs=False)
    t2, dx2, pt, pdx = launch_sweep(env, case, inp, cs=True)
    assert torch.equal(bits(t2), bits(t)) and torch.equal(bits(dx2), bits(dx)), "the column sums changed t or dx"
    tn = launch_dnorm(env, case, inp)
    assert torch.equal(bits(t), bits(tn)), int((bits(t) != bits(tn)).sum())
    t64, dx64, mag = R.bwd(inp["g"], inp["x"], inp["norm"], inp["gamma_e"], inverse, t_dev=t)
    rt = ratio("d", tag, "t", R.band_ratio(t, t64, t64.abs(), R.K_T))
    rdx = ratio("d", tag, "dx", R.band_ratio(dx, dx64, mag, R.K_DX(C)))
    rcs = check_colsums("d", tag, pt, pdx, t, dx, P)
    assert rt <= 1.0 and rdx <= 1.0 and rcs <= 1.0, (rt, rdx, rcs)


# ---------------------------------------------------------------------------------------------
# e. one-sweep backward, recomputing the norm
# ---------------------------------------------------------------------------------------------
def _recompute_ratios(inp, n64, nq, amb, t, dx, C, inverse):
    """worst t and dx ratios: against rne_bf16(n64) everywhere, at ambiguous elements against the better of the two
    neighbouring bf16 norms"""
    t64, dx64, mag = R.bwd(inp["g"], inp["x"], nq, inp["gamma_e"], inverse, t_dev=t)
    r_t = R.band_ratios(t, t64, t64.abs(), R.K_T)
    r_dx = R.band_ratios(dx, dx64, mag, R.K_DX(C))
    if bool(amb.any()):
        idx = amb.nonzero(as_tuple=True)
        g, x = inp["g"].double()[idx], inp["x"].double()[idx]
        best_t = best_dx = None
        for n_alt in R.bf16_neighbours(n64[idx]):
            ta = R.t_of(g, x, n_alt, inverse)
            dxa, maga = R.with_other_norm(dx64[idx], mag[idx], g, nq[idx], n_alt, inverse)
            rt_a = R.band_ratios(t.double()[idx], ta, ta.abs(), R.K_T)
            rdx_a = R.band_ratios(dx.double()[idx], dxa, maga, R.K_DX(C))
            both = torch.maximum(rt_a, rdx_a)                    # (t and dx of one element come from the same norm)
            if best_t is None:
                best, best_t, best_dx = both, rt_a, rdx_a
            else:
                take = both < best
                best_t, best_dx = torch.where(take, rt_a, best_t), torch.where(take, rdx_a, best_dx)
        r_t[idx], r_dx[idx] = best_t, best_dx
    return float(r_t.max()), float(r_dx.max())


@pytest.mark.parametrize("case", SWEEP_CASES + R.BIG_CASES, ids=R.case_id)
def test_e_sweep_recomputing(env, case):
    C, inverse, P = case
    inp = banded(case)
    tag = R.case_id(case)
    n64, nq, _ = fwd_ref(case)
    amb = R.ambiguous(n64, C)
    share = float(amb.double().mean())
    print(f"AMBIGUOUS e {tag} {100 * share:.3f} %")
    assert share <= 0.01, share
    t, dx, _, _ = launch_sweep(env, case, inp, cs=False, recompute=True)       # gdn_bwd_bf16_kernel<C / 32, false, true>
    t2, dx2, pt, pdx = launch_sweep(env, case, inp, cs=True, recompute=True)   # gdn_bwd_bf16_kernel<C / 32, true, true>
    assert torch.equal(bits(t2), bits(t)) and torch.equal(bits(dx2), bits(dx)), "the column sums changed t or dx"
    rt, rdx = _recompute_ratios(inp, n64, nq, amb, t, dx, C, inverse)
    ratio("e", tag, "t", rt)
    ratio("e", tag, "dx", rdx)
    rcs = check_colsums("e", tag, pt, pdx, t, dx, P)
    assert rt <= 1.0 and rdx <= 1.0 and rcs <= 1.0, (rt, rdx, rcs)


@pytest.mark.parametrize("case", [c for c in SWEEP_CASES if c[2] in EXACT_SIZES], ids=R.case_id)
def test_e_sweep_recomputing_exact_pool(env, case):
    """with the exact forward inputs the recomputed pool is exact in fp32: nothing is ambiguous, the norm the sweep rounds
    is rne_bf16(n64) at every element -- so t is bit for bit the reading sweep's on that norm and dx is banded from it"""
    C, inverse, P = case
    f = R.exact_fwd_inputs(*case)
    inp = dict(f, g=banded(case)["g"])
    n64, nq, _ = R.fwd(f["x"], f["beta_e"], f["gamma_e"], inverse)
    for cs in (False, True):
        t, dx, _, _ = launch_sweep(env, case, inp, cs=cs, recompute=True)
        tr_, dxr, _, _ = launch_sweep(env, case, inp, cs=cs, norm=nq.float())
        assert torch.equal(bits(t), bits(tr_)), int((bits(t) != bits(tr_)).sum())
        t64, dx64, mag = R.bwd(inp["g"], inp["x"], nq, f["gamma_e"], inverse, t_dev=t)
        tag = f"exact-pool-{R.case_id(case)}-cs{int(cs)}"
        rt = ratio("e", tag, "t", R.band_ratio(t, t64, t64.abs(), R.K_T))
        rdx = ratio("e", tag, "dx", R.band_ratio(dx, dx64, mag, R.K_DX(C)))
        assert rt <= 1.0 and rdx <= 1.0, (rt, rdx)


# ---------------------------------------------------------------------------------------------
# f. exact backward
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _premise(env):
    """v_rsq_f32 and v_sqrt_f32 at 1 and 4 as fp32, read off a one-pixel launch of the two-launch route's second kernel
    writing fp32: with t = 0, gamma_e = 0 and g = 1 its output is fma(2 x, 0, g f(norm)) = f(norm)"""
    C = 64
    norm = torch.tensor([1.0, 4.0] * (C // 2)).reshape(1, C)
    inp = dict(g=torch.ones(1, C), x=torch.ones(1, C), gamma_e=torch.zeros(C, C), norm=norm)
    out = {}
    for inverse in (0, 1):
        f = launch_igemm_bwd(env, (C, inverse, 1), inp, torch.zeros(1, C, dtype=BF), out_f32=True)
        want = norm.sqrt() if inverse else 1.0 / norm.sqrt()
        out["sqrt" if inverse else "rsq"] = bool(torch.equal(bits(f), bits(want)))
        print("PREMISE", "v_sqrt_f32" if inverse else "v_rsq_f32", "at 1 and 4:", f[0, :2].tolist())
    return out


def test_f_rsq_and_sqrt_are_exact_at_1_and_4(env):
    """the premise of the exact backward cases"""
    p = _premise(env)
    assert all(p.values()), p


def _exact_bwd_reference(case):
    C, inverse, P = case
    inp = R.exact_bwd_inputs(*case)
    t64, dx64, _ = R.bwd(inp["g"], inp["x"], inp["norm"], inp["gamma_e"], inverse)
    assert R.is_bf16(t64)
    return inp, t64, R.rne_bf16(dx64)


def _same_bf16(got, ref, what):
    assert not bool(torch.isnan(got.float()).any()), f"{what}: an element kept its NaN"
    bad = R.bf16_bits(got) != R.bf16_bits(ref)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values differ, first in row {int(bad.any(1).nonzero()[0])}"


@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] in EXACT_SIZES], ids=R.case_id)
def test_f_exact_backward_two_launch(env, case):
    assert all(_premise(env).values()), _premise(env)
    inp, t64, dxq = _exact_bwd_reference(case)
    t = launch_dnorm(env, case, inp)
    _same_bf16(t, t64, "t")
    _same_bf16(launch_igemm_bwd(env, case, inp, t), dxq, "dx")


@pytest.mark.parametrize("cs", [False, True], ids=["plain", "colsums"])
@pytest.mark.parametrize("case", [c for c in SWEEP_CASES if c[2] in EXACT_SIZES], ids=R.case_id)
def test_f_exact_backward_sweep(env, case, cs):
    C, inverse, P = case
    assert all(_premise(env).values()), _premise(env)
    inp, t64, dxq = _exact_bwd_reference(case)
    t, dx, pt, pdx = launch_sweep(env, case, inp, cs=cs)
    _same_bf16(t, t64, "t")
    _same_bf16(dx, dxq, "dx")
    if cs:
        # sums of at most 357 multiples of 1/16 below 2^7: exact in fp32 in any order
        for part, src, what in ((pt, t64, "colsum_t_partial"), (pdx, dxq, "colsum_dx_partial")):
            ref, _ = R.tile_colsums(src, R.sweep_grid(P))
            assert not bool(torch.isnan(part).any()), f"{what}: a row kept its NaN"
            assert G.same_bits(part, ref), f"{what}: {int((G.canon_bits(part) != G.canon_bits(ref)).sum())} values differ"


# ---------------------------------------------------------------------------------------------
# g. a transposed panel fails
# ---------------------------------------------------------------------------------------------
def test_g_a_transposed_panel_misses_the_bands(env):
    case = (64, 0, 129)
    C, inverse, P = case
    inp = banded(case)
    n64, nq, y64 = fwd_ref(case)
    swapped = dict(inp, gamma_e=inp["gamma_e"].t().contiguous())
    _, norm = launch_fwd(env, case, swapped, 64)
    assert R.band_ratio(norm, n64, n64, R.K_FWD(C)) > 1.0
    t, dx, _, _ = launch_sweep(env, case, swapped, cs=False)
    t64, dx64, mag = R.bwd(inp["g"], inp["x"], inp["norm"], inp["gamma_e"], inverse, t_dev=t)
    assert R.band_ratio(t, t64, t64.abs(), R.K_T) <= 1.0          # (t does not read the panel)
    assert R.band_ratio(dx, dx64, mag, R.K_DX(C)) > 1.0


# ---------------------------------------------------------------------------------------------
# h. through the module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("C", R.WIDTHS)
def test_h_module_reaches_these_kernels(env, C, inverse):
    """layers.GDN(C, inverse)(x, bf16=True) forward and backward at B, H, W = 1, 17, 21 (P = 357).  d beta and d gamma:
    sums of P fp32 terms (t; the exact products t * rne_bf16(x^2), wgrad_bf16_kernel's SQB operand being sq8's
    round-to-nearest-even square) and one multiply in the re-parametrisation's backward: (P + 2) u of the magnitudes"""
    F_, FB, L, dev = env
    from neural_image_compression_amd.layers import GDN
    B, H, W = 1, 17, 21
    P = B * H * W
    case = (C, inverse, P)
    src = banded(case)
    m = GDN(C, inverse=bool(inverse)).to(dev)
    bb, gb, ped = m.beta_reparam.bound_value, m.gamma_reparam.bound_value, m.beta_reparam.pedestal_value
    with torch.no_grad():   # parameters whose re-parametrisation gives about the banded beta_eff, gamma_eff, above the bounds
        m.beta.copy_((src["beta_e"].double().clamp_min(1e-3) + ped).sqrt().float())
        m.gamma.copy_((src["gamma_e"].double() + ped).sqrt().float())
        assert float(m.beta.min()) > bb and float(m.gamma.min()) > gb
    beta_e, gamma_e = FB._gamma_eff(m.beta.detach(), bb, ped).cpu(), FB._gamma_eff(m.gamma.detach(), gb, ped).cpu()
    inp = dict(src, beta_e=beta_e, gamma_e=gamma_e)

    def nchw(a, grad=False):   # [P][C] -> NCHW-logical, channels_last, bf16
        t = bf(a, dev).reshape(B, H, W, C).permute(0, 3, 1, 2)
        assert t.is_contiguous(memory_format=torch.channels_last)
        return t.requires_grad_(grad)

    def pc(t):
        return t.detach().permute(0, 2, 3, 1).reshape(P, C).cpu()

    tx = nchw(inp["x"], True)
    names = set()
    F_.KERNEL_TRACE = names
    try:
        ty = m(tx, bf16=True)
        ty.backward(nchw(inp["g"]))
        torch.cuda.synchronize()
    finally:
        F_.KERNEL_TRACE = None
    print("TRACE h", C, inverse, sorted(names))
    sweep = C in SWEEP_WIDTHS
    assert any(n.startswith(f"igemm_bf16_kernel<64, {C // 64}, true, false") for n in names), names
    assert (f"gdn_bwd_bf16_kernel<{C // 32}>" in names) == sweep, names
    assert any(n.startswith("wgrad_bf16_kernel<") and "true" in n for n in names), names
    if not sweep:
        assert any(n.startswith(f"igemm_bf16_kernel<64, {C // 64}, false, false") for n in names), names
    # the C-ABI launches of a, e (c at 192) on the same operands
    y, norm = launch_fwd(env, case, inp, want_norm=not sweep)
    assert torch.equal(bits(pc(ty)), bits(y)), int((bits(pc(ty)) != bits(y)).sum())
    if sweep:
        t, dx, _, _ = launch_sweep(env, case, inp, cs=True, recompute=True)
    else:
        t = launch_dnorm(env, case, inp, norm=norm.float())
        dx = launch_igemm_bwd(env, case, inp, t, norm=norm.float())
    assert tx.grad.dtype == BF and torch.equal(bits(pc(tx.grad)), bits(dx)), int((bits(pc(tx.grad)) != bits(dx)).sum())
    tag = f"C{C}-{'igdn' if inverse else 'gdn'}-P{P}"
    t_ = t.double()
    sq = R.rne_bf16(inp["x"].double() ** 2)
    # (reparam_bwd is linear in its gradient argument: the bound passes through it as the sum of magnitudes does)
    rb_ = R.band_ratio(m.beta.grad.cpu(), R.reparam_bwd(m.beta.detach().cpu(), t_.sum(0), bb),
                       R.reparam_bwd(m.beta.detach().cpu(), t_.abs().sum(0), bb), P + 2, half_ulp=False)
    rg_ = R.band_ratio(m.gamma.grad.cpu(), R.reparam_bwd(m.gamma.detach().cpu(), t_.t() @ sq, gb),
                       R.reparam_bwd(m.gamma.detach().cpu(), t_.abs().t() @ sq, gb), P + 2, half_ulp=False)
    ratio("h", tag, "dbeta", rb_)
    ratio("h", tag, "dgamma", rg_)
    assert rb_ <= 1.0 and rg_ <= 1.0, (rb_, rg_)


# ---------------------------------------------------------------------------------------------
# i. refusals
# ---------------------------------------------------------------------------------------------
def test_i_refusals_launch_nothing(env):
    F_, FB, L, dev = env
    lib = L.load()
    C, P = 64, 129
    inp = banded((C, 0, P))
    g, x, n = bf(inp["g"], dev), bf(inp["x"], dev), bf(inp["norm"], dev)
    beta_e = inp["beta_e"].to(dev)
    gamma_e = inp["gamma_e"].to(dev).contiguous()
    gp = FB._pack_bf16(gamma_e, 1, C, C, 0, C, 1, kperm=True)
    gTp = FB._pack_bf16(gamma_e, 1, C, C, 0, 1, C, kperm=True)
    rows = lib.lic_gdn_bwd_bf16_partial_rows(P)
    assert lib.lic_gdn_bwd_bf16_partial_rows(0) == 0 and rows == 2 and lib.lic_gdn_bwd_bf16_partial_rows(R.BIG) == 2048
    outs = [Guarded(P, 192, dev), Guarded(P, 192, dev), Guarded(rows, 192, dev, torch.float32),
            Guarded(rows, 192, dev, torch.float32)]                    # wide enough for C = 192
    o_dx, o_t, o_pt, o_pdx = (o.t for o in outs)
    s = F_._stream()

    def read(g=g, x=x, n=n, gp=gp, dx=o_dx, t=o_t, pt=o_pt, pdx=o_pdx, P=P, C=C):
        return lib.lic_gdn_bwd_bf16(_ptr(g), _ptr(x), _ptr(n), _ptr(gp), _ptr(dx), _ptr(t), _ptr(pt), _ptr(pdx), P, C, 0, s)

    def recompute(g=g, x=x, gp=gp, gTp=gTp, beta_e=beta_e, dx=o_dx, t=o_t, pt=o_pt, pdx=o_pdx, P=P, C=C):
        return lib.lic_gdn_bwd_bf16_recompute(_ptr(g), _ptr(x), _ptr(gp), _ptr(gTp), _ptr(beta_e), _ptr(dx), _ptr(t), _ptr(pt),
                                              _ptr(pdx), P, C, 0, s)

    def off2(t):   # a device copy that starts 2 bytes (bf16) / 4 bytes (fp32) after a 16-byte boundary
        buf = torch.empty(t.numel() + 1, device=dev, dtype=t.dtype)
        v = buf[1:]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 16 == t.element_size()
        return v

    assert lib.lic_gdn_bwd_bf16_supported(192) == 0 and all(lib.lic_gdn_bwd_bf16_supported(c) == 1 for c in SWEEP_WIDTHS)
    for Cbad in (192, 96, 32):
        assert read(C=Cbad) == ERR_UNSUPPORTED and recompute(C=Cbad) == ERR_UNSUPPORTED, Cbad
    for fn in (read, recompute):
        assert fn(P=0) == ERR_INVALID and fn(P=-1) == ERR_INVALID
        assert fn(pt=None) == ERR_INVALID and fn(pdx=None) == ERR_INVALID       # both partial buffers or neither
    for k_, v in (("g", g), ("x", x), ("n", n), ("gp", gp), ("dx", o_dx), ("t", o_t)):
        assert read(**{k_: off2(v)}) == ERR_INVALID, k_
        assert read(**{k_: None}) == ERR_INVALID, k_
    for k_, v in (("g", g), ("x", x), ("gp", gp), ("gTp", gTp), ("beta_e", beta_e), ("dx", o_dx), ("t", o_t)):
        assert recompute(**{k_: off2(v)}) == ERR_INVALID, k_
        assert recompute(**{k_: None}) == ERR_INVALID, k_
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused call wrote to an output"
