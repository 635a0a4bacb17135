"""lic_gdn_fwd / lic_gdn_bwd (csrc/lic_gdn.hip: gdn_kernel<TN, 0>, gdn_bwd_reg_kernel<TN>, C in {64, 128, 192}) through
the C ABI against tests/gdn_ref64.py, the float64 statement of the operation:

  a. banded: random inputs over four decades of pixel magnitudes, every element of norm, y, t at the project's
     1e-6 + 1e-4 |ref| and every element of dx at 1e-4 of the float64 sum of the magnitudes of its own terms;
  b. exact: small-integer inputs for which fp32 forms every value without rounding in any order (proved on the CPU by
     tests/test_gdn_ref64.py): norm, t, dx and every row of both per-workgroup column-sum buffers bit for bit;
  c. the equalities include/lic.h and the kernel header state: t is lic_gdn_dnorm's, the pooled sums are the generic
     lic_igemm route's (prologue 1 forward, prologue 2 / 3 backward);
  d. optional operands (norm == NULL, res, either partial buffer) change nothing else, bit for bit;
  e. refusals launch nothing;
  f. layers.GDN with a residual at C = 64 and 192 reaches these kernels and agrees with the float64 reference.

Every output sits inside a larger allocation whose row in front and row behind hold a NaN pattern; every test checks
that those rows are unchanged.  Outputs are pre-filled with the same pattern, so an element the kernel does not write
fails its comparison.  Every figure is printed before it is asserted.
Run on the MI355X box:  python -m pytest tests/test_gpu_gdn_fp32.py -m gpu -q -s"""
import ctypes
import functools

import pytest
import torch

import gdn_ref64 as G
from guarded import Guarded

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
SMALL = [c for c in G.CASES if c[2] in (65, 357)]                 # two tiles with one pixel in the second; ragged, six tiles
SOME = SMALL + [c for c in G.CASES if c[2] == G.BIG and c[0] == 192]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, F_, L, torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# inputs and references are computed once per case and left unchanged; of the four largest cases (a quarter of a gigabyte
# of float64 each) only the latest is kept
_small_inputs = functools.lru_cache(maxsize=None)(G.banded_inputs)
_big_inputs = functools.lru_cache(maxsize=1)(G.banded_inputs)


def _banded(case):
    return (_big_inputs if case[2] == G.BIG else _small_inputs)(*case)


def _reference(case):
    C, inverse, P = case
    i = _banded(case)
    y, norm = G.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
    return dict(y=y, norm=norm, bwd=G.bwd(i["g"], i["x"], i["norm"], i["gamma_e"], inverse))


_small_reference = functools.lru_cache(maxsize=None)(_reference)
_big_reference = functools.lru_cache(maxsize=1)(_reference)


def _banded_ref(case):
    """float64 forward and backward of the banded inputs of `case` (the backward from the generated norm)"""
    return (_big_reference if case[2] == G.BIG else _small_reference)(case)


def launch_fwd(env, case, inp, res=None, want_norm=True):
    """lic_gdn_fwd on the operands packed as functional._gdn_operands packs them -> (y, norm) on the CPU"""
    nic, F_, L, dev = env
    C, inverse, P = case
    x, beta_e, gamma_e = inp["x"].to(dev), inp["beta_e"].to(dev), inp["gamma_e"].to(dev).contiguous()
    gT = F_._pack(gamma_e, 1, C, C, 0, 1, C)
    tres = None if res is None else res.to(dev)
    y, norm = Guarded(P, C, dev), Guarded(P, C, dev)
    L.check(L.load().lic_gdn_fwd(_ptr(x), _ptr(gT), _ptr(beta_e), _ptr(tres), _ptr(y.t), _ptr(norm.t) if want_norm else None,
                                 P, C, inverse, F_._stream()), "lic_gdn_fwd")
    torch.cuda.synchronize()
    y.check("y")
    norm.check("norm")
    if not want_norm:
        assert norm.untouched()
    return y.cpu(), norm.cpu()


def launch_bwd(env, case, inp, norm=None, partials="both"):
    """lic_gdn_bwd on the operands packed as functional._gdn_backward packs them -> (t, dx, cs_t, cs_dx) on the CPU"""
    nic, F_, L, dev = env
    C, inverse, P = case
    lib = L.load()
    g, x = inp["g"].to(dev), inp["x"].to(dev)
    n = (inp["norm"] if norm is None else norm).to(dev)
    gp = F_._pack_dense(inp["gamma_e"].to(dev).contiguous())
    rows = lib.lic_gdn_bwd_partial_rows(P)
    assert rows == (P + G.BLOCK - 1) // G.BLOCK
    t, dx = Guarded(P, C, dev), Guarded(P, C, dev)
    pt, pdx = Guarded(rows, C, dev), Guarded(rows, C, dev)
    L.check(lib.lic_gdn_bwd(_ptr(g), _ptr(x), _ptr(n), _ptr(gp), _ptr(dx.t), _ptr(t.t),
                            _ptr(pt.t) if partials in ("both", "t") else None,
                            _ptr(pdx.t) if partials in ("both", "dx") else None, P, C, inverse, F_._stream()), "lic_gdn_bwd")
    torch.cuda.synchronize()
    for o, what in ((t, "t"), (dx, "dx"), (pt, "colsum_t_partial"), (pdx, "colsum_dx_partial")):
        o.check(what)
    if partials not in ("both", "t"):
        assert pt.untouched()
    if partials not in ("both", "dx"):
        assert pdx.untouched()
    return t.cpu(), dx.cpu(), pt.cpu(), pdx.cpu()


def check_band(got, ref, what, tag):
    r = G.band_ratio(got, ref, *G.BAND)
    print(f"RATIO {tag} {what} {r:.4f}")
    return r


def check_partials(pt, pdx, t, dx, tag):
    """the per-workgroup column sums against the float64 block sums of the device's own t and dx: a sum of 64 fp32 terms,
    however it is associated, is within 63 u of the sum of their magnitudes (first order) -- held to 64 u"""
    worst = 0.0
    for part, src, what in ((pt, t, "cs_t"), (pdx, dx, "cs_dx")):
        ref, mag = G.block_colsums(src), G.block_colsums(src.double().abs())
        assert part.shape == ref.shape
        assert not bool(torch.isnan(part).any()), f"{what}: a row kept its NaN"
        err = (part.double() - ref).abs()
        bound = 64 * 2.0 ** -24 * mag
        r = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
        print(f"RATIO {tag} {what} {r:.4f}")
        worst = max(worst, r)
    return worst


# ---------------------------------------------------------------------------------------------
# a. banded, random inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_forward_banded(env, case):
    inp, ref = _banded(case), _banded_ref(case)
    tag = "fwd " + G.case_id(case)
    y, norm = launch_fwd(env, case, inp)
    rs = [check_band(norm, ref["norm"], "norm", tag), check_band(y, ref["y"], "y", tag)]
    assert max(rs) <= 1.0, rs
    # with the residual: the banded y plus res as one fp32 add (a band on the sum would be measured against a reference
    # that the two terms may cancel in)
    y_res, norm_res = launch_fwd(env, case, inp, res=inp["res"])
    assert torch.equal(bits(y_res), bits(y + inp["res"])) and torch.equal(bits(norm_res), bits(norm))


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_backward_banded(env, case):
    inp, ref = _banded(case), _banded_ref(case)
    tag = "bwd " + G.case_id(case)
    t64, dx64, mag = ref["bwd"]
    t, dx, pt, pdx = launch_bwd(env, case, inp)
    rt = check_band(t, t64, "t", tag)
    rdx = G.mag_ratio(dx, dx64, mag)
    print(f"RATIO {tag} dx {rdx:.4f}")
    rp = check_partials(pt, pdx, t, dx, tag)
    assert rt <= 1.0 and rdx <= 1.0 and rp <= 1.0, (rt, rdx, rp)


@pytest.mark.parametrize("case", G.OWN_NORM_CASES, ids=G.case_id)
def test_backward_banded_from_the_forward_kernels_norm(env, case):
    """the pair as a layer runs it: the backward reads the fp32 pool the forward kernel wrote (down to beta_eff = 1e-6 at
    the all-zero pixels); the reference backward starts from those same fp32 values"""
    C, inverse, P = case
    inp = _banded(case)
    tag = "bwd(own norm) " + G.case_id(case)
    _, norm = launch_fwd(env, case, inp)
    t64, dx64, mag = G.bwd(inp["g"], inp["x"], norm, inp["gamma_e"], inverse)
    t, dx, pt, pdx = launch_bwd(env, case, inp, norm=norm)
    rt = check_band(t, t64, "t", tag)
    rdx = G.mag_ratio(dx, dx64, mag)
    print(f"RATIO {tag} dx {rdx:.4f}")
    rp = check_partials(pt, pdx, t, dx, tag)
    assert rt <= 1.0 and rdx <= 1.0 and rp <= 1.0, (rt, rdx, rp)


def test_a_transposed_panel_fails_the_band(env):
    """the bands tell gamma_e from its transpose: the forward fed the backward's panel (and the reverse) misses them"""
    nic, F_, L, dev = env
    case = (64, 0, 65)
    C, inverse, P = case
    inp, ref = _banded(case), _banded_ref(case)
    swapped = dict(inp, gamma_e=inp["gamma_e"].t().contiguous())
    _, norm = launch_fwd(env, case, swapped)
    assert G.band_ratio(norm, ref["norm"], *G.BAND) > 1.0
    _, dx, _, _ = launch_bwd(env, case, swapped)
    assert G.mag_ratio(dx, ref["bwd"][1], ref["bwd"][2]) > 1.0


# ---------------------------------------------------------------------------------------------
# b. exact, order-independent inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_forward_exact(env, case):
    C, inverse, P = case
    inp = G.exact_fwd_inputs(*case)
    y64, n64 = G.fwd(inp["x"], inp["beta_e"], inp["gamma_e"], inverse)
    y, norm = launch_fwd(env, case, inp)
    assert G.same_bits(norm, n64), int((G.canon_bits(norm) != G.canon_bits(n64)).sum())
    assert check_band(y, y64, "y", "fwd-exact " + G.case_id(case)) <= 1.0


@functools.lru_cache(maxsize=1)
def _premise(env):
    """v_rsq_f32 and v_sqrt_f32 at 1 and 4, read off a one-pixel launch with g = x = 1 and gamma_e = 0: dx = f(norm),
    t = -1/2 norm^-3/2 (inverse: 1/2 norm^-1/2).  -> {what: bool}"""
    C = 64
    norm = torch.tensor([1.0, 4.0] * (C // 2)).reshape(1, C)
    inp = dict(g=torch.ones(1, C), x=torch.ones(1, C), gamma_e=torch.zeros(C, C), norm=norm)
    out = {}
    for inverse in (0, 1):
        t, dx, _, _ = launch_bwd(env, (C, inverse, 1), inp)
        want_dx = norm.sqrt() if inverse else 1.0 / norm.sqrt()
        want_t = 0.5 / norm.sqrt() if inverse else -0.5 * norm ** -1.5
        out["sqrt" if inverse else "rsq"] = bool(torch.equal(bits(dx), bits(want_dx)))
        out["t igdn" if inverse else "t gdn"] = bool(torch.equal(bits(t), bits(want_t)))
        print("PREMISE", "igdn" if inverse else "gdn", "dx", dx[0, :2].tolist(), "t", t[0, :2].tolist())
    return out


def test_rsq_and_sqrt_are_exact_at_1_and_4(env):
    """the premise of the exact backward case"""
    p = _premise(env)
    print("PREMISE", p)
    assert all(p.values()), p


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_backward_exact(env, case):
    C, inverse, P = case
    assert all(_premise(env).values()), _premise(env)
    inp = G.exact_bwd_inputs(*case)
    ref = G.exact_reference("bwd", inp, inverse)
    t, dx, pt, pdx = launch_bwd(env, case, inp)
    for got, name in ((t, "t"), (dx, "dx"), (pt, "cs_t"), (pdx, "cs_dx")):
        assert not bool(torch.isnan(got).any()), f"{name}: an element kept its NaN"
        assert got.shape == ref[name].shape
        bad = G.canon_bits(got) != G.canon_bits(ref[name])
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} values differ, first in row {int(bad.any(1).nonzero()[0])}"


# ---------------------------------------------------------------------------------------------
# c. the equalities the headers state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOME, ids=G.case_id)
def test_t_is_lic_gdn_dnorm(env, case):
    nic, F_, L, dev = env
    C, inverse, P = case
    inp = _banded(case)
    t, _, _, _ = launch_bwd(env, case, inp)
    g, x, n = inp["g"].to(dev), inp["x"].to(dev), inp["norm"].to(dev)
    out = Guarded(P, C, dev)
    L.check(L.load().lic_gdn_dnorm(_ptr(g), _ptr(x), _ptr(n), _ptr(out.t), P * C, inverse, F_._stream()), "lic_gdn_dnorm")
    torch.cuda.synchronize()
    out.check("lic_gdn_dnorm")
    assert torch.equal(bits(t), bits(out.t)), int((bits(t) != bits(out.t)).sum())


@pytest.mark.parametrize("case", SOME, ids=G.case_id)
def test_norm_is_the_generic_routes(env, case):
    """lic_igemm with prologue 1 and the GDN / IGDN epilogue, as the `else` branch of _GDNFn.forward calls it"""
    nic, F_, L, dev = env
    C, inverse, P = case
    inp = _banded(case)
    y, norm = launch_fwd(env, case, inp)
    x, beta_e = inp["x"].to(dev), inp["beta_e"].to(dev)
    gT = F_._pack(inp["gamma_e"].to(dev).contiguous(), 1, C, C, 0, 1, C)
    out, out2 = Guarded(P, C, dev), Guarded(P, C, dev)
    F_._igemm(x, gT, out.t, B=1, Hi=1, Wi=P, Cin=C, Ho=1, Wo=P, Cout=C, kh=1, kw=1, stride=1, pad=0, transposed=False,
              bias=beta_e, prologue=1, epilogue=L.EPI_IGDN if inverse else L.EPI_GDN, out2=out2.t, aux=x, res=None)
    torch.cuda.synchronize()
    out.check("generic y")
    out2.check("generic norm")
    assert torch.equal(bits(norm), bits(out2.t)), int((bits(norm) != bits(out2.t)).sum())
    assert torch.equal(bits(y), bits(out.t)), int((bits(y) != bits(out.t)).sum())


def _generic_bwd(env, case, inp):
    nic, F_, L, dev = env
    C, inverse, P = case
    g, x, n = inp["g"].to(dev), inp["x"].to(dev), inp["norm"].to(dev)
    gp = F_._pack_dense(inp["gamma_e"].to(dev).contiguous())
    dx, t = Guarded(P, C, dev), Guarded(P, C, dev)
    F_._igemm(g, gp, dx.t, B=1, Hi=1, Wi=P, Cin=C, Ho=1, Wo=P, Cout=C, kh=1, kw=1, stride=1, pad=0, transposed=False,
              prologue=3 if inverse else 2, epilogue=L.EPI_IGDN_BWD if inverse else L.EPI_GDN_BWD, aux=g, aux2=x, aux3=n,
              out2=t.t)
    torch.cuda.synchronize()
    dx.check("generic dx")
    t.check("generic t")
    return t.cpu(), dx.cpu()


@pytest.mark.parametrize("case", SOME, ids=G.case_id)
def test_backward_sum_is_the_generic_routes(env, case):
    """lic_igemm with prologue 2 / 3 and the GDN_BWD / IGDN_BWD epilogue, as _gdn_backward calls it for other widths.
    With every x a power of two 2 x s is exact, so dx = fl(g f + 2 x s) whether the epilogue fuses the multiply into the
    add or not: dx is then equal bit for bit exactly when the pooled sums s are.  With general x the two epilogues may
    round differently (reported, not asserted: the stated property is the order of the sums); t is equal either way."""
    C, inverse, P = case
    inp = dict(_banded(case))
    t, dx, _, _ = launch_bwd(env, case, inp, partials=None)
    t2, dx2 = _generic_bwd(env, case, inp)
    assert torch.equal(bits(t), bits(t2))
    print("EQUAL bwd", G.case_id(case), "dx bitwise the generic route's on general x:", bool(torch.equal(bits(dx), bits(dx2))),
          "differing share", float((bits(dx) != bits(dx2)).double().mean()))
    gen = torch.Generator().manual_seed(C + P)
    sign = torch.randint(2, (P, C), generator=gen) * 2.0 - 1.0
    inp["x"] = sign * 2.0 ** torch.randint(-3, 4, (P, C), generator=gen).float()
    t, dx, _, _ = launch_bwd(env, case, inp, partials=None)
    t2, dx2 = _generic_bwd(env, case, inp)
    assert torch.equal(bits(t), bits(t2))
    assert torch.equal(bits(dx), bits(dx2)), int((bits(dx) != bits(dx2)).sum())


# ---------------------------------------------------------------------------------------------
# d. optional operands
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=G.case_id)
def test_forward_optional_operands(env, case):
    inp = _banded(case)
    y, norm = launch_fwd(env, case, inp)
    y_nonorm, _ = launch_fwd(env, case, inp, want_norm=False)
    assert torch.equal(bits(y_nonorm), bits(y))
    y_res, norm_res = launch_fwd(env, case, inp, res=inp["res"])
    assert torch.equal(bits(y_res), bits(y + inp["res"]))          # one fp32 add
    assert torch.equal(bits(norm_res), bits(norm))
    y_both, _ = launch_fwd(env, case, inp, res=inp["res"], want_norm=False)
    assert torch.equal(bits(y_both), bits(y_res))


@pytest.mark.parametrize("case", SMALL, ids=G.case_id)
def test_backward_optional_operands(env, case):
    inp = _banded(case)
    t, dx, pt, pdx = launch_bwd(env, case, inp, partials="both")
    for mode in (None, "t", "dx"):
        t2, dx2, pt2, pdx2 = launch_bwd(env, case, inp, partials=mode)     # (asserts that an absent buffer stays untouched)
        assert torch.equal(bits(t2), bits(t)) and torch.equal(bits(dx2), bits(dx)), mode
        if mode == "t":
            assert torch.equal(bits(pt2), bits(pt))
        if mode == "dx":
            assert torch.equal(bits(pdx2), bits(pdx))


# ---------------------------------------------------------------------------------------------
# e. refusals
# ---------------------------------------------------------------------------------------------
def _off4(t):
    """a device copy of `t` that starts 4 bytes after a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=torch.float32)
    v = buf[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def test_refusals(env):
    nic, F_, L, dev = env
    lib = L.load()
    C, P = 64, 65
    inp = _banded((C, 0, P))
    x, g, n, res = (inp[k].to(dev) for k in ("x", "g", "norm", "res"))
    beta_e = inp["beta_e"].to(dev)
    gamma_e = inp["gamma_e"].to(dev).contiguous()
    gT, gp = F_._pack(gamma_e, 1, C, C, 0, 1, C), F_._pack_dense(gamma_e)
    rows = lib.lic_gdn_bwd_partial_rows(P)
    assert lib.lic_gdn_bwd_partial_rows(0) == 0 and lib.lic_gdn_bwd_partial_rows(64) == 1 and rows == 2
    outs = [Guarded(P, 256, dev) for _ in range(2)] + [Guarded(rows, 256, dev) for _ in range(2)]   # wide enough for C = 256
    o0, o1, p0, p1 = (o.t for o in outs)
    s = F_._stream()

    def fwd(x=x, gT=gT, beta_e=beta_e, res=res, y=o0, norm=o1, P=P, C=C):
        return lib.lic_gdn_fwd(_ptr(x), _ptr(gT), _ptr(beta_e), _ptr(res), _ptr(y), _ptr(norm), P, C, 0, s)

    def bwd(g=g, x=x, n=n, gp=gp, dx=o0, t=o1, pt=p0, pdx=p1, P=P, C=C):
        return lib.lic_gdn_bwd(_ptr(g), _ptr(x), _ptr(n), _ptr(gp), _ptr(dx), _ptr(t), _ptr(pt), _ptr(pdx), P, C, 0, s)

    for Cbad in (96, 256):
        assert lib.lic_gdn_supported(Cbad) == 0
        assert fwd(C=Cbad) == ERR_UNSUPPORTED and bwd(C=Cbad) == ERR_UNSUPPORTED, Cbad
    assert all(lib.lic_gdn_supported(c) == 1 for c in G.WIDTHS)
    assert fwd(P=0) == ERR_INVALID and bwd(P=0) == ERR_INVALID
    for k in ("x", "gT", "beta_e", "y"):
        assert fwd(**{k: None}) == ERR_INVALID, k
    for k in ("g", "x", "n", "gp", "dx", "t"):
        assert bwd(**{k: None}) == ERR_INVALID, k
    for k, v in (("x", x), ("gT", gT), ("beta_e", beta_e), ("res", res), ("y", o0), ("norm", o1)):
        assert fwd(**{k: _off4(v)}) == ERR_INVALID, k
    for k, v in (("g", g), ("x", x), ("n", n), ("gp", gp), ("dx", o0), ("t", o1)):
        assert bwd(**{k: _off4(v)}) == ERR_INVALID, k
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused call wrote to an output"


# ---------------------------------------------------------------------------------------------
# f. through the module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C", [64, 192])
def test_module_with_residual(env, C, inverse):
    """layers.GDN(C, inverse)(x, residual=) forward and backward (B, H, W = 2, 9, 7: P = 126) against the float64
    reference, the re-parametrisation of beta and gamma included (torch.autograd of the float64 forward gives d beta)"""
    nic, F_, L, dev = env
    from neural_image_compression_amd.layers import GDN
    B, H, W = 2, 9, 7
    P = B * H * W
    inp = G.banded_inputs(C, int(inverse), P)
    m = GDN(C, inverse=inverse).to(dev)
    bb, gb, ped = m.beta_reparam.bound_value, m.gamma_reparam.bound_value, m.beta_reparam.pedestal_value
    with torch.no_grad():   # parameters whose re-parametrisation gives (about) the generated beta_eff, gamma_eff
        # (beta_eff >= 1e-3: away from the lower bound, where the bound's one-sided gradient rule would apply)
        m.beta.copy_((inp["beta_e"].double().clamp_min(1e-3) + ped).sqrt().float())
        m.gamma.copy_((inp["gamma_e"].double() + ped).sqrt().float())
        assert float(m.beta.min()) > bb and float(m.gamma.min()) > gb

    def nchw(a, grad=False):   # [P][C] -> NCHW-logical, channels_last
        t = a.reshape(B, H, W, C).to(dev).permute(0, 3, 1, 2)
        assert t.is_contiguous(memory_format=torch.channels_last)
        return t.requires_grad_(grad)

    def pc(t):
        return t.detach().permute(0, 2, 3, 1).reshape(P, C).cpu()

    tx, tres = nchw(inp["x"], True), nchw(inp["res"], True)
    F_.KERNEL_TRACE = set()
    try:
        ty = m(tx, residual=tres)
        ty.backward(nchw(inp["g"]))
        torch.cuda.synchronize()
        names = F_.KERNEL_TRACE
    finally:
        F_.KERNEL_TRACE = None
    assert f"gdn_kernel<{C // 64}, {int(inverse)}>" in names and f"gdn_bwd_kernel<{C // 64}, {int(inverse)}>" in names, names
    # float64: the same parameters through max(p, bound)^2 - pedestal
    beta_p = m.beta.detach().cpu().double().requires_grad_(True)
    gamma_p = m.gamma.detach().cpu().double()
    beta_e = torch.clamp(beta_p, min=bb) ** 2 - ped
    gamma_e = torch.clamp(gamma_p, min=gb) ** 2 - ped
    y64, n64 = G.fwd(inp["x"], beta_e, gamma_e, inverse, inp["res"])
    tag = f"module C{C}-{'igdn' if inverse else 'gdn'}"
    ry = check_band(pc(ty), y64.detach(), "y", tag)
    # (the kernel's backward reads its own fp32 pool: within (C + 3) u of n64, far inside the bands)
    t64, dx64, mag = G.bwd(inp["g"], inp["x"], n64.detach(), gamma_e, inverse)
    rdx = G.mag_ratio(pc(tx.grad), dx64, mag)
    print(f"RATIO {tag} dx {rdx:.4f}")
    dbeta64, = torch.autograd.grad(beta_e, beta_p, t64.sum(0))
    e = float((m.beta.grad.cpu().double() - dbeta64).abs().max() / dbeta64.abs().max())
    print(f"RATIO {tag} dbeta {e / 1e-4:.4f}")
    assert ry <= 1.0 and rdx <= 1.0 and e <= 1e-4, (ry, rdx, e)
    assert torch.equal(bits(pc(tres.grad)), bits(inp["g"])), "d residual is not the upstream gradient"
