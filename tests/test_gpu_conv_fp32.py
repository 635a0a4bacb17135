"""lic_igemm, lic_wgrad, lic_pack_weight (csrc/lic_gemm.hip) and lic_im2col / lic_col2im (csrc/lic_elementwise.hip)
through the C ABI against tests/conv_ref64.py, the float64 statements of the operations:

  a. exact: small-integer inputs for which fp32 forms every partial sum without rounding in any order (S < 2^24, shown
     on the CPU by tests/test_conv_ref64.py): forward, the mirrored data-gradient launch, the weight gradient, the column
     kernels and the RGB route end to end, bit for bit -- under every forced tile and every forced split;
  b. banded: seeded normal inputs, EVERY element of y, dx, dw, db within A S of float64, S the sum of the magnitudes of
     that element's own terms (A per kernel family, measured; conv_ref64's docstring);
  c. the equalities the sources state: a second launch gives the same bits; a batch equals its single-image launches;
     functional.conv2d / conv_transpose2d under the same forced plan equal the direct launches; LEAKY with res leaves
     `out` as it is without;
  d. refusals launch nothing.

Every output, out2, split-K workspace and lic_wgrad workspace lives in a tests/guarded.py buffer: pre-filled with a NaN
pattern, canaries in front and behind and, for pitched outputs, in the columns outside the output; operands sit in the
same pattern, so a read outside them poisons the result.  Every figure is printed before it is asserted.
Run on the MI355X box:  python -m pytest tests/test_gpu_conv_fp32.py -m gpu -q -s"""
import copy
import ctypes
import functools

import pytest
import torch

import conv_ref64 as R
from guarded import CANARY, Guarded

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
WORST = {"igemm": 0.0, "split": 0.0, "wgrad": 0.0, "rgb": 0.0}       # worst err / S per family, printed by the last test


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()  # must be the in-tree HIP extension; raises if missing
    return F_, L, lib, torch.device("cuda:0")


def sync_clean(lib):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on the GPU from this process
        pytest.exit(f"the GPU reported {e}", returncode=3)
    assert lib.lic_last_hip_error() == 0, "a HIP error is pending"


def note(family, r, tag):
    print(f"RATIO {family} {tag} err/S = {r:.3e} = 2^{torch.log2(torch.tensor(max(r, 1e-300))).item():.2f}")
    WORST[family] = max(WORST[family], r)


# ---------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _cpu_case(name, exact):
    """inputs and float64 references of an lic_igemm case: computed once, left unchanged"""
    c = R.ICASE[name]
    inp = R.igemm_inputs(c, exact)
    return inp, R.igemm_reference(c, inp), (R.igemm_reference(c, inp, "dgrad") if c.dgrad else None)


class IgemmOperands:
    """the device operands of a layer case, packed as functional.py packs them"""

    def __init__(self, env, c, inp):
        F_, L, lib, dev = env
        self.c = c
        npix_in, npix_out = c.B * c.H * c.W, c.B * c.Ho * c.Wo
        self.x = Guarded.holding(inp["x"].reshape(npix_in, c.cin), dev, ld=c.cin + c.in_extra, shift=c.in_off)
        self.w = inp["w"].to(dev).contiguous()
        taps = c.k * c.k
        for dgrad in (False, True):
            assert R.pack_strides(c.kind, dgrad, c.cin, c.cout, taps) == tuple(F_._conv_weight_layout(self.w, c.kind == "convT", dgrad))
        self.wp = F_._pack(self.w, *R.pack_strides(c.kind, False, c.cin, c.cout, taps))
        self.wp_d = F_._pack(self.w, *R.pack_strides(c.kind, True, c.cin, c.cout, taps)) if c.dgrad else None
        self.b = None if inp["b"] is None else inp["b"].to(dev)
        self.dy = Guarded.holding(inp["dy"].reshape(npix_out, c.cout), dev) if c.dgrad else None
        self.res = Guarded.holding(inp["res"].reshape(npix_out, c.cout), dev) if c.epi == "leaky_res" else None
        self.aux = Guarded.holding(inp["aux"].reshape(npix_out, c.cout), dev, ld=c.cout + c.aux_extra) if c.epi == "mulmask" else None


def igemm_desc(env, c, ops, which, tile, split, out, out2=None, ws=None, ws_bytes=None):
    F_, L, lib, dev = env
    addr = {"in": (ops.x if which == "fwd" else ops.dy).ptr(), "w": (ops.wp if which == "fwd" else ops.wp_d).data_ptr(),
            "out": out.ptr(), "bias": None if ops.b is None else ops.b.data_ptr(), "out2": None if out2 is None else out2.ptr(),
            "res": None if ops.res is None else ops.res.ptr(), "aux": None if ops.aux is None else ops.aux.ptr(),
            "workspace": None if ws is None else ws.ptr(), "workspace_bytes": ws_bytes or 0}
    return R.fill_igemm_desc(L.IgemmDesc(), c, which, tile, split, addr)


def run_igemm(env, c, ops, which, tile, split):
    """one guarded launch -> (out, out2 or None, K slices) on the CPU; every canary checked"""
    F_, L, lib, dev = env
    g = c.geom(which)
    npix = g["B"] * g["Ho"] * g["Wo"]
    fwd = which == "fwd"
    out = Guarded(npix, g["Cout"], dev, ld=c.out_ld if fwd else None, col0=c.out_col0 if fwd else 0)
    out2 = Guarded(npix, g["Cout"], dev) if (fwd and c.epi == "leaky_res") else None
    ws, nbytes = None, 0
    if split not in (0, 1):
        probe = igemm_desc(env, c, ops, which, tile, split, out, out2)
        probe.workspace, probe.workspace_bytes = out.ptr(), 0     # (the query plans a copy with a workspace of its own)
        nbytes = lib.lic_igemm_workspace_bytes(ctypes.byref(probe))
        assert nbytes > 0 and nbytes % (4 * npix * g["Cout"]) == 0, (c, split, nbytes)
        ws = Guarded.flat(nbytes // 4, dev)
    d = igemm_desc(env, c, ops, which, tile, split, out, out2, ws, nbytes)
    tag = f"{c} {which} tile {tile} split {split}"
    assert lib.lic_igemm(ctypes.byref(d), F_._stream()) == OK, tag
    sync_clean(lib)
    out.check(tag + " out")
    if out2 is not None:
        out2.check(tag + " out2")
    if ws is not None:
        ws.check(tag + " workspace")
        assert ws.unwritten() == 0, f"{tag}: a slab element was not written"
    for o in (ops.x, ops.dy, ops.res, ops.aux):
        if o is not None:
            o.check(tag + " (an operand)")
    slices = nbytes // (4 * npix * g["Cout"]) if nbytes else 1
    return out.cpu().reshape(g["B"], g["Ho"], g["Wo"], g["Cout"]), (None if out2 is None else out2.cpu().reshape(g["B"], g["Ho"], g["Wo"], g["Cout"])), slices


class WgradOperands:
    def __init__(self, env, c, inp):
        F_, L, lib, dev = env
        g = c.g
        self.P = Guarded.holding(inp["P"].reshape(-1, g["Cp"]), dev, ld=g["Cp"] + c.p_extra, shift=c.p_off)
        self.G = Guarded.holding(inp["G"].reshape(-1, g["Cg"]), dev, ld=g["Cg"] + c.g_extra)


def run_wgrad(env, c, ops, split, stages=(0,), short=0):
    """guarded lic_wgrad (or lic_wgrad_stage for each of `stages`) -> (flat destination as int32 patterns, rc)"""
    F_, L, lib, dev = env
    _, _, _, span = c.dst_strides()
    dst = Guarded.flat(span, dev)
    d = R.fill_wgrad_desc(L.WgradDesc(), c, split, {"p": ops.P.ptr(), "g": ops.G.ptr(), "dst": dst.ptr()})
    nbytes = lib.lic_wgrad_workspace_bytes(ctypes.byref(d))
    tm, tn, sk = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.lic_wgrad_plan(ctypes.byref(d), ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sk)) == OK
    assert nbytes == 4 * sk.value * c.taps * c.Cm * c.Cn > 0
    ws = Guarded.flat(nbytes // 4, dev)
    tag = f"{c} split {split} stages {stages}"
    rc = OK
    for st in stages:
        if stages == (0,):
            rc = lib.lic_wgrad(ctypes.byref(d), ctypes.c_void_p(ws.ptr()), nbytes - short, F_._stream())
        else:
            rc = lib.lic_wgrad_stage(ctypes.byref(d), ctypes.c_void_p(ws.ptr()), nbytes - short, st, F_._stream())
        if rc != OK:
            break
    sync_clean(lib)
    dst.check(tag + " dst")
    ws.check(tag + " workspace")
    ops.P.check(tag + " P")
    ops.G.check(tag + " G")
    if rc == OK:
        assert ws.unwritten() == 0, f"{tag}: a slab element was not written"
    return dst, ws, rc


def wgrad_result(c, dst):
    """(R [taps,Cm,Cn] as the kernel scattered it, number of gap elements that no longer hold the pattern)"""
    flat = dst.cpu().reshape(-1)
    _, idx = R.scatter_dst(c, torch.zeros((c.taps, c.Cm, c.Cn)), 0.0)
    gaps = torch.ones(flat.numel(), dtype=torch.bool)
    gaps[idx] = False
    touched = int((flat.view(torch.int32)[gaps] != CANARY).sum())
    return flat[idx].reshape(c.taps, c.Cm, c.Cn), touched


# ---------------------------------------------------------------------------------------------
# a. exact cases, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.IGEMM_CASES])
def test_igemm_exact(env, name):
    """forward and mirrored launch under every forced tile and split of the case: each equals float64, hence all agree"""
    c = R.ICASE[name]
    inp, ref, dref = _cpu_case(name, True)
    ops = IgemmOperands(env, c, inp)
    bad = []
    for which, tile, split in c.launches():
        out, out2, _ = run_igemm(env, c, ops, which, tile, split)
        want = ref if which == "fwd" else dref
        if not R.same_bits(out, want["out"]):
            bad.append((which, tile, split, "out", int((out.double() != want["out"]).sum())))
        if out2 is not None and not R.same_bits(out2, want["out2"]):
            bad.append((which, tile, split, "out2", int((out2.double() != want["out2"]).sum())))
    print(f"EXACT {name}: {len(c.launches())} launches, {len(bad)} differ")
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in R.WGRAD_CASES])
def test_wgrad_exact(env, name):
    c = R.WCASE[name]
    inp = R.wgrad_inputs(c, True)
    ref = R.wgrad_reference(c, inp)["R"]
    ops = WgradOperands(env, c, inp)
    bad = []
    for split in c.splits:
        dst, _, rc = run_wgrad(env, c, ops, split)
        assert rc == OK
        got, touched = wgrad_result(c, dst)
        if touched or not R.same_bits(got, ref):
            bad.append((split, touched, int((got.double() != ref).sum())))
    print(f"EXACT {name}: splits {c.splits}, {len(bad)} differ")
    assert not bad, bad


@pytest.mark.parametrize("name", ["convT5-22f", "conv5-11r", "sqrow-23r", "conv5-33"])
def test_wgrad_stage_1_then_2_is_stage_0(env, name):
    c = R.WCASE[name]
    ops = WgradOperands(env, c, R.wgrad_inputs(c, False))
    split = c.splits[-1]
    whole, ws0, rc0 = run_wgrad(env, c, ops, split)
    staged, ws1, rc1 = run_wgrad(env, c, ops, split, stages=(1, 2))
    assert rc0 == rc1 == OK
    assert torch.equal(whole.buf, staged.buf) and torch.equal(ws0.buf, ws1.buf)
    only1, _, rc = run_wgrad(env, c, ops, split, stages=(1,))
    assert rc == OK and only1.untouched(), "stage 1 wrote the destination"


def _run_im2col(env, q, x, Kpad=None):
    F_, L, lib, dev = env
    Kpad = q["Kpad"] if Kpad is None else Kpad
    xg = Guarded.holding(x.reshape(-1, q["C"]), dev)
    col = Guarded(q["B"] * q["Ho"] * q["Wo"], max(Kpad, 1), dev)
    rc = lib.lic_im2col(ctypes.c_void_p(xg.ptr()), ctypes.c_void_p(col.ptr()), q["B"], q["H"], q["W"], q["C"], q["Ho"], q["Wo"],
                        q["k"], q["k"], q["s"], q["p"], Kpad, F_._stream())
    sync_clean(lib)
    col.check("im2col col")
    xg.check("im2col x")
    return col, rc


def _run_col2im(env, q, colv, bias, Kpad=None):
    """the transposed twin: columns on the Ho x Wo grid scattered to H x W"""
    F_, L, lib, dev = env
    Kpad = q["Kpad"] if Kpad is None else Kpad
    cg = colv if isinstance(colv, Guarded) else Guarded.holding(colv, dev)
    b = None if bias is None else bias.to(dev)
    out = Guarded(q["B"] * q["H"] * q["W"], q["C"], dev)
    rc = lib.lic_col2im(ctypes.c_void_p(cg.ptr()), None if b is None else ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(out.ptr()),
                        q["B"], q["Ho"], q["Wo"], q["C"], q["H"], q["W"], q["k"], q["k"], q["s"], q["p"], Kpad, F_._stream())
    sync_clean(lib)
    out.check("col2im out")
    cg.check("col2im col")
    return out, rc


def _col2im_args(q):
    return (q["B"], q["Ho"], q["Wo"], q["C"], q["H"], q["W"], q["k"], q["k"], q["s"], q["p"])


@pytest.mark.parametrize("c", R.COL_CASES, ids=lambda c: c[0])
def test_im2col_and_col2im_alone(env, c):
    """im2col is a copy: bit for bit on any input, zero columns included.  col2im: exact on integers with and without
    bias, and every element within A S on normal inputs."""
    q = R.col_geom(c)
    for exact in (True, False):
        inp = R.col_inputs(c, exact)
        col, rc = _run_im2col(env, q, inp["x"])
        assert rc == OK and torch.equal(col.cpu().double(), R.im2col(inp["x"], q["Ho"], q["Wo"], q["k"], q["k"], q["s"], q["p"], q["Kpad"]))
        for bias in (None, inp["b"]):
            out, rc = _run_col2im(env, q, inp["col"], bias)
            ref, S = R.col2im(inp["col"], bias, *_col2im_args(q))
            assert rc == OK
            got = out.cpu().reshape(ref.shape)
            if exact:
                assert R.same_bits(got, ref), int((got.double() != ref).sum())
            else:
                r = R.err_over_S(got, ref, S)
                note("rgb", r, f"col2im {c[0]} bias={bias is not None}")
                assert r <= R.A_RGB


def _dense_igemm(env, a, Wm, bias, npix, K, N):
    """lic_igemm as the RGB layers use it: a 1x1 launch over a [npix][K] matrix `a` (a Guarded), Wm [K][N] on the device"""
    F_, L, lib, dev = env
    out = Guarded(npix, N, dev)
    b = None if bias is None else bias.to(dev)
    d = F_._igemm_desc(a.t, F_._pack_dense(Wm.to(dev).contiguous()), out.t, 1, 1, npix, K, 1, npix, N, 1, 1, 1, 0, False, b, 0,
                       L.EPI_NONE, 0.0, 0, None, None, None, None, None, None)
    assert lib.lic_igemm(ctypes.byref(d), F_._stream()) == OK
    sync_clean(lib)
    out.check("dense igemm out")
    return out


@pytest.mark.parametrize("c", R.COL_CASES, ids=lambda c: c[0])
def test_rgb_route_end_to_end(env, c):
    """im2col -> lic_igemm(1x1, K = Kpad) is the convolution; lic_igemm -> col2im is the transposed convolution: exact on
    integers, banded on normal inputs"""
    q = R.col_geom(c)
    B, H, W, Cc, k, s, p, Ho, Wo, Kpad = (q[n] for n in ("B", "H", "W", "C", "k", "s", "p", "Ho", "Wo", "Kpad"))
    N, taps = 64, k * k
    for exact in (True, False):
        inp = R.col_inputs(c, exact)
        g_ = torch.Generator().manual_seed(17 + exact)
        if exact:
            w = torch.randint(-2, 3, (N, Cc, k, k), generator=g_).float()
            z = torch.randint(-3, 4, (B, Ho, Wo, N), generator=g_).float()
            bias_n = torch.randint(-4, 5, (N,), generator=g_).float()
        else:
            w = torch.randn((N, Cc, k, k), generator=g_) / (Cc * taps) ** 0.5
            z = torch.randn((B, Ho, Wo, N), generator=g_)
            bias_n = torch.randn(N, generator=g_)
        # the stem: conv [N,C,k,k] of x; Wm[(tap, c)][n] = w[n][c][tap], zero rows up to Kpad
        Wm = torch.zeros((Kpad, N))
        Wm[:taps * Cc] = w.permute(2, 3, 1, 0).reshape(taps * Cc, N)
        col, rc = _run_im2col(env, q, inp["x"])
        assert rc == OK
        y = _dense_igemm(env, col, Wm, bias_n, B * Ho * Wo, Kpad, N)
        geo = dict(B=B, Hi=H, Wi=W, Cin=Cc, Ho=Ho, Wo=Wo, Cout=N, kh=k, kw=k, stride=s, pad=p, transposed=0)
        ref, S = R.igemm(inp["x"], R.logical_weight(w, "conv", False), geo, bias_n)
        got = y.cpu().reshape(ref.shape)
        if exact:
            assert R.exact_ok(S) and R.same_bits(got, ref), int((got.double() != ref).sum())
        else:
            r = R.err_over_S(got, ref, S)
            note("rgb", r, f"stem {c[0]}")
            assert r <= R.A_RGB
        # the head: convT [N,C,k,k] of z; Wh[n][(tap, c)] = w[n][c][tap]
        Wh = torch.zeros((N, Kpad))
        Wh[:, :taps * Cc] = w.permute(0, 2, 3, 1).reshape(N, taps * Cc)
        zg = Guarded.holding(z.reshape(-1, N), env[3])
        cols = _dense_igemm(env, zg, Wh, None, B * Ho * Wo, N, Kpad)
        out, rc = _run_col2im(env, q, cols, inp["b"])
        geo_t = dict(B=B, Hi=Ho, Wi=Wo, Cin=N, Ho=H, Wo=W, Cout=Cc, kh=k, kw=k, stride=s, pad=p, transposed=1)
        ref, S = R.igemm(z, R.logical_weight(w, "convT", False), geo_t, inp["b"])
        got = out.cpu().reshape(ref.shape)
        if exact:
            assert rc == OK and R.exact_ok(S) and R.same_bits(got, ref), int((got.double() != ref).sum())
        else:
            r = R.err_over_S(got, ref, S)
            note("rgb", r, f"head {c[0]}")
            assert rc == OK and r <= R.A_RGB


@pytest.mark.parametrize("c", [c for c in R.COL_CASES if c[4] == 3], ids=lambda c: c[0])
def test_rgb_route_with_fused_leaky(env, c):
    """functional.image_conv2d with the LeakyReLU fused into the dense launch (the first block of the 3x3 model): exact on
    integers (the slope is a power of two), banded on normal inputs (the LeakyReLU is 1-Lipschitz)"""
    F_, L, lib, dev = env
    q = R.col_geom(c)
    B, H, W, Cc, k, s, p, Ho, Wo = (q[n] for n in ("B", "H", "W", "C", "k", "s", "p", "Ho", "Wo"))
    N = 64
    for exact in (True, False):
        inp = R.col_inputs(c, exact)
        g_ = torch.Generator().manual_seed(23 + exact)
        if exact:
            w = torch.randint(-2, 3, (N, Cc, k, k), generator=g_).float()
            bias_n = torch.randint(-4, 5, (N,), generator=g_).float()
        else:
            w = torch.randn((N, Cc, k, k), generator=g_) / (Cc * k * k) ** 0.5
            bias_n = torch.randn(N, generator=g_)
        x = inp["x"].reshape(B, H, W, Cc).to(dev).permute(0, 3, 1, 2)
        y = F_.image_conv2d(x, w.to(dev), bias_n.to(dev), s, p, True, R.SLOPE)
        sync_clean(lib)
        geo = dict(B=B, Hi=H, Wi=W, Cin=Cc, Ho=Ho, Wo=Wo, Cout=N, kh=k, kw=k, stride=s, pad=p, transposed=0)
        ref, S = R.igemm(inp["x"], R.logical_weight(w, "conv", False), geo, bias_n)
        ref = torch.where(ref > 0, ref, ref * R.SLOPE)
        got = y.detach().permute(0, 2, 3, 1).cpu().reshape(ref.shape)
        assert bool((ref < 0).any()) and bool((ref > 0).any())
        if exact:
            assert R.exact_ok(S) and R.same_bits(got, ref), int((got.double() != ref).sum())
        else:
            r = R.err_over_S(got, ref, S)
            note("rgb", r, f"stem+leaky {c[0]}")
            assert r <= R.A_RGB


# ---------------------------------------------------------------------------------------------
# b. banded cases: every element within A S
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.IGEMM_CASES])
def test_igemm_banded(env, name):
    c = R.ICASE[name]
    inp, ref, dref = _cpu_case(name, False)
    ops = IgemmOperands(env, c, inp)
    worst = {"igemm": 0.0, "split": 0.0}
    for which, tile, split in c.launches():
        out, out2, slices = run_igemm(env, c, ops, which, tile, split)
        want = ref if which == "fwd" else dref
        fam = "split" if slices > 1 else "igemm"
        r = R.err_over_S(out, want["out"], want["S"])
        worst[fam] = max(worst[fam], r)
        if out2 is not None:   # out + res as one fp32 add of the device's own out (a band on the sum would be measured against
            assert torch.equal(out2.view(torch.int32), (out + inp["res"]).view(torch.int32))   # terms that may cancel)
    for fam, r in worst.items():
        if r:
            note(fam, r, name)
    assert worst["igemm"] <= R.A_IGEMM and worst["split"] <= R.A_SPLIT, worst


@pytest.mark.parametrize("name", [c.name for c in R.WGRAD_CASES])
def test_wgrad_banded(env, name):
    c = R.WCASE[name]
    inp = R.wgrad_inputs(c, False)
    ref = R.wgrad_reference(c, inp)
    ops = WgradOperands(env, c, inp)
    worst = 0.0
    for split in c.splits:
        dst, _, rc = run_wgrad(env, c, ops, split)
        got, touched = wgrad_result(c, dst)
        assert rc == OK and touched == 0, (split, touched)
        worst = max(worst, R.err_over_S(got, ref["R"], ref["S"]))
    note("wgrad", worst, name)
    assert worst <= R.A_WGRAD


@pytest.mark.parametrize("name", ["c5s2-64-192", "t5s2-128", "k18-30", "pgroup-16-64"])
def test_bias_gradient_banded(env, name):
    """db = lic_colsum of the output gradient, as functional._bias_grad launches it"""
    F_, L, lib, dev = env
    c = R.ICASE[name]
    inp, _, _ = _cpu_case(name, False)
    P = c.B * c.Ho * c.Wo
    dy = Guarded.holding(inp["dy"].reshape(P, c.cout), dev)
    nbytes = lib.lic_colsum_workspace_bytes(P, c.cout)
    ws, out = Guarded.flat(max(nbytes // 4, 1), dev), Guarded.flat(c.cout, dev)
    assert lib.lic_colsum(ctypes.c_void_p(dy.ptr()), c.cout, P, c.cout, 1.0, ctypes.c_void_p(out.ptr()), ctypes.c_void_p(ws.ptr()),
                          nbytes, F_._stream()) == OK
    sync_clean(lib)
    for o in (dy, ws, out):
        o.check("colsum")
    ref, S = R.colsum(inp["dy"])
    r = R.err_over_S(out.cpu().reshape(-1), ref, S)
    note("wgrad", r, f"db {name}")
    assert r <= R.A_WGRAD


# ---------------------------------------------------------------------------------------------
# c. equalities the sources state
# ---------------------------------------------------------------------------------------------
REPEAT = [("split-48-64", (64, 1), 4), ("split-48-30", (0, 0), 7), ("split-128-192", (128, 3), 6), ("auto-ws", (0, 0), "ws"),
          ("t5s2-128", (128, 2), 0)]


@pytest.mark.parametrize("name,tile,split", REPEAT)
def test_a_second_igemm_launch_gives_the_same_bits(env, name, tile, split):
    c = R.ICASE[name]
    ops = IgemmOperands(env, c, _cpu_case(name, False)[0])
    a, _, _ = run_igemm(env, c, ops, "fwd", tile, split)
    b, _, _ = run_igemm(env, c, ops, "fwd", tile, split)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ["convT5-23f", "conv5-13r", "sqcol-33", "dense-auto"])
def test_a_second_wgrad_launch_gives_the_same_bits(env, name):
    c = R.WCASE[name]
    ops = WgradOperands(env, c, R.wgrad_inputs(c, False))
    for split in c.splits:
        a, wa, _ = run_wgrad(env, c, ops, split)
        b, wb, _ = run_wgrad(env, c, ops, split)
        assert torch.equal(a.buf, b.buf) and torch.equal(wa.buf, wb.buf)


BATCH = [("split-48-64", (64, 1), 4), ("split-48-64", (128, 1), 7), ("t5s2-128", (128, 2), 0), ("c5s2-64-192", (64, 3), 0),
         ("split-convT", (64, 2), 8), ("k18-30", (0, 0), 0), ("m5-64-128", (128, 1), 0)]


@pytest.mark.parametrize("name,tile,split", BATCH)
def test_a_batch_equals_its_single_image_launches(env, name, tile, split):
    """igemm_geo_split: the K split is "a function of per-image geometry only", and the tile does not change the order of a
    sum -- so under one forced tile and split every image's bits are those of its own launch"""
    c = R.ICASE[name]
    inp = _cpu_case(name, False)[0]
    whole, _, s_all = run_igemm(env, c, IgemmOperands(env, c, inp), "fwd", tile, split)
    assert c.B >= 2
    for b in range(c.B):
        one = copy.copy(c)
        one.B = 1
        sub = dict(inp)
        for key in ("x", "dy", "res", "aux"):
            sub[key] = inp[key][b:b + 1]
        got, _, s_one = run_igemm(env, one, IgemmOperands(env, one, sub), "fwd", tile, split)
        assert s_one == s_all
        assert torch.equal(got.view(torch.int32), whole[b:b + 1].contiguous().view(torch.int32)), f"image {b}"


# (split 1 = never split: functional.py hands small layers a workspace, with which the automatic plan would split)
FUNCTIONAL = [("c5s2-64-192", (128, 3), 1, (1, 3)), ("t5s2-128", (64, 2), 1, (2, 2)), ("split-48-64", (64, 1), 4, (1, 1)),
              ("m5-64-128", (64, 2), 1, (1, 1)), ("split-convT", (128, 1), 8, (1, 3))]


@pytest.mark.parametrize("name,tile,split,wtile", FUNCTIONAL)
def test_functional_layers_equal_the_direct_launches(env, name, tile, split, wtile):
    """functional.conv2d / conv_transpose2d with the same forced plan: y, dx and dw bit for bit what the guarded C-ABI
    launches of this file give -- what the tests above hold is what training runs"""
    F_, L, lib, dev = env
    c = R.ICASE[name]
    inp = _cpu_case(name, False)[0]
    ops = IgemmOperands(env, c, inp)
    y_direct, _, _ = run_igemm(env, c, ops, "fwd", tile, split)
    x = inp["x"].to(dev).permute(0, 3, 1, 2).requires_grad_(True)          # NCHW-logical, NHWC in memory
    w = inp["w"].to(dev).contiguous().requires_grad_(True)
    b = None if inp["b"] is None else inp["b"].to(dev)
    leaky = c.epi == "leaky"
    F_.FORCE_IGEMM, F_.FORCE_WGRAD = (tile[0], tile[1], split), (wtile[0], wtile[1], 2)
    try:
        if c.kind == "conv":
            y = F_.conv2d(x, w, b, c.s, c.p, leaky, R.SLOPE, c.tap_mask)
        else:
            y = F_.conv_transpose2d(x, w, b, c.s, c.p, c.op, leaky, R.SLOPE)
        yh = y.detach().permute(0, 2, 3, 1).contiguous().cpu()
        assert torch.equal(yh.view(torch.int32), y_direct.view(torch.int32)), "y"
        dtile = tile if tile in c.tile_list("dgrad") else (0, 0)
        if not leaky:
            F_.FORCE_IGEMM = (dtile[0], dtile[1], 1)
            y.backward(inp["dy"].to(dev).permute(0, 3, 1, 2))
            torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM = F_.FORCE_WGRAD = None
    if leaky:
        return
    wc = R.layer_wcase("as-layer", c.kind, c.k, c.s, c.p, c.op, c.B, c.H, c.W, c.cin, c.cout, tile=wtile, splits=(2,))
    wops = WgradOperands(env, wc, dict(P=inp["dy"] if c.kind == "conv" else inp["x"], G=inp["x"] if c.kind == "conv" else inp["dy"]))
    dst, _, rc = run_wgrad(env, wc, wops, 2)
    assert rc == OK and torch.equal(dst.cpu().reshape(-1).view(torch.int32), w.grad.detach().cpu().reshape(-1).view(torch.int32)), "dw"
    if c.dgrad:
        dx_direct, _, _ = run_igemm(env, c, ops, "dgrad", dtile, 1)
        dxh = x.grad.detach().permute(0, 2, 3, 1).contiguous().cpu()
        assert torch.equal(dxh.view(torch.int32), dx_direct.view(torch.int32)), "dx"


@pytest.mark.parametrize("name", ["leaky-res", "leaky-res-scalar"])
def test_leaky_with_res_leaves_out_as_without(env, name):
    c = R.ICASE[name]
    inp = _cpu_case(name, False)[0]
    plain = copy.copy(c)
    plain.epi = "leaky"
    for tile in c.tile_list():
        out_r, out2, _ = run_igemm(env, c, IgemmOperands(env, c, inp), "fwd", tile, 0)
        out_p, none, _ = run_igemm(env, plain, IgemmOperands(env, plain, inp), "fwd", tile, 0)
        assert none is None and torch.equal(out_r.view(torch.int32), out_p.view(torch.int32))
        assert torch.equal(out2.view(torch.int32), (out_r + inp["res"]).view(torch.int32))


# ---------------------------------------------------------------------------------------------
# d. refusals launch nothing
# ---------------------------------------------------------------------------------------------
def _refused(env, c, ops, tile, split, want, tweak=None, ws_short=0, which="fwd"):
    F_, L, lib, dev = env
    g = c.geom(which)
    npix = g["B"] * g["Ho"] * g["Wo"]
    out = Guarded(npix, g["Cout"], dev, ld=c.out_ld, col0=c.out_col0)
    out2 = Guarded(npix, g["Cout"], dev)
    ws = Guarded.flat(64 * npix * g["Cout"], dev)
    d = igemm_desc(env, c, ops, which, tile, split, out, out2 if c.epi == "leaky_res" else None, ws, 4 * 64 * npix * g["Cout"])
    if ws_short:
        need = lib.lic_igemm_workspace_bytes(ctypes.byref(d))
        assert need > 0
        d.workspace_bytes = need - ws_short
    if tweak:
        tweak(d)
    bm = ctypes.c_int32(0)
    rc = lib.lic_igemm(ctypes.byref(d), F_._stream())
    sync_clean(lib)
    assert rc == want, (rc, want)
    assert out.untouched() and out2.untouched() and ws.untouched(), "a refused launch wrote"
    if want != ERR_WORKSPACE:
        assert lib.lic_igemm_plan(ctypes.byref(d), ctypes.byref(bm), None, None) == want
    return d


def test_igemm_refusals(env):
    F_, L, lib, dev = env
    c = R.ICASE["split-48-64"]
    ops = IgemmOperands(env, c, _cpu_case(c.name, True)[0])
    _refused(env, c, ops, (64, 1), 4, ERR_WORKSPACE, ws_short=1)                       # a workspace one byte short
    _refused(env, c, ops, (0, 0), 27, ERR_WORKSPACE, ws_short=1)
    _refused(env, c, ops, (64, 2), 0, ERR_UNSUPPORTED)                                 # Npad 64 is no multiple of 128
    _refused(env, c, ops, (64, 3), 0, ERR_UNSUPPORTED)
    _refused(env, c, ops, (32, 1), 0, ERR_UNSUPPORTED)
    _refused(env, c, ops, (64, 0), 0, ERR_UNSUPPORTED)                                 # one of the two alone
    u = R.ICASE["unaligned-32-64"]
    _refused(env, u, IgemmOperands(env, u, _cpu_case(u.name, True)[0]), (64, 1), 0, ERR_UNSUPPORTED)   # forced tile, unaligned operand
    k = R.ICASE["k18-30"]
    _refused(env, k, IgemmOperands(env, k, _cpu_case(k.name, True)[0]), (64, 1), 0, ERR_UNSUPPORTED)   # ... Cin % 4 != 0

    def taps(kh, kw):
        def f(d):
            d.kh, d.kw = kh, kw
        return f
    _refused(env, c, ops, (0, 0), 0, ERR_UNSUPPORTED, taps(1, 29))                     # the tap list has 28 slots
    _refused(env, c, ops, (0, 0), 0, ERR_UNSUPPORTED, taps(5, 6))
    _refused(env, c, ops, (0, 0), 0, ERR_UNSUPPORTED, taps(4, 8))                      # 32 taps: what tap_mask could still name
    d = _refused(env, c, ops, (0, 0), 0, ERR_UNSUPPORTED, taps(1, 29))
    d.kh, d.kw = 4, 7                                                                  # 28 taps plan (nothing is launched here)
    assert lib.lic_igemm_plan(ctypes.byref(d), None, None, None) == OK

    def stride3(d):
        d.stride = 3
    _refused(env, c, ops, (0, 0), 0, ERR_UNSUPPORTED, stride3)
    r = R.ICASE["leaky-res"]

    def no_out2(d):
        d.out2 = None
    _refused(env, r, IgemmOperands(env, r, _cpu_case(r.name, True)[0]), (0, 0), 0, ERR_INVALID, no_out2)


def test_wgrad_refusals(env):
    F_, L, lib, dev = env
    c = R.WCASE["convT5-22f"]                     # 128 x 128 channels
    ops = WgradOperands(env, c, R.wgrad_inputs(c, True))
    for split in (1, 3):
        dst, ws, rc = run_wgrad(env, c, ops, split, short=1)                           # a workspace one byte short
        assert rc == ERR_WORKSPACE and dst.untouched() and ws.untouched()
    for tile in ((3, 3), (1, 2), (4, 1), (2, 4), (0, 2), (3, 1)):                      # (3,3) needs multiples of 192; the rest are not listed
        bad = copy.copy(c)
        bad.tile = tile
        _, _, _, span = bad.dst_strides()
        dst, ws = Guarded.flat(span, dev), Guarded.flat(1 << 20, dev)
        d = R.fill_wgrad_desc(L.WgradDesc(), bad, 2, {"p": ops.P.ptr(), "g": ops.G.ptr(), "dst": dst.ptr()})
        rc = lib.lic_wgrad(ctypes.byref(d), ctypes.c_void_p(ws.ptr()), 4 << 20, F_._stream())
        sync_clean(lib)
        assert rc == ERR_UNSUPPORTED and dst.untouched() and ws.untouched(), tile
        assert lib.lic_wgrad_plan(ctypes.byref(d), None, None, None) == ERR_UNSUPPORTED
    odd = R.WCASE["conv3-odd"]                    # a forced tile on channel counts that are no multiple of 4
    bad = copy.copy(odd)
    bad.tile = (1, 1)
    oops = WgradOperands(env, odd, R.wgrad_inputs(odd, True))
    dst, ws = Guarded.flat(bad.dst_strides()[3], dev), Guarded.flat(1 << 20, dev)
    d = R.fill_wgrad_desc(L.WgradDesc(), bad, 2, {"p": oops.P.ptr(), "g": oops.G.ptr(), "dst": dst.ptr()})
    assert lib.lic_wgrad(ctypes.byref(d), ctypes.c_void_p(ws.ptr()), 4 << 20, F_._stream()) == ERR_UNSUPPORTED
    sync_clean(lib)
    assert dst.untouched() and ws.untouched()
    d.force_tm = d.force_tn = 0
    assert lib.lic_wgrad_stage(ctypes.byref(d), ctypes.c_void_p(ws.ptr()), 4 << 20, 3, F_._stream()) == ERR_INVALID   # no such stage
    sync_clean(lib)
    assert dst.untouched() and ws.untouched()


@pytest.mark.parametrize("c", R.COL_CASES[:2], ids=lambda c: c[0])
def test_column_kernel_refusals(env, c):
    q = R.col_geom(c)
    inp = R.col_inputs(c, True)
    short = q["k"] * q["k"] * q["C"] - 1
    col, rc = _run_im2col(env, q, inp["x"], Kpad=short)
    assert rc == ERR_INVALID and col.untouched()
    out, rc = _run_col2im(env, q, inp["col"], inp["b"], Kpad=short)
    assert rc == ERR_INVALID and out.untouched()


def test_zz_report_the_worst_ratios(env):
    """the figures conv_ref64's bands come from: the worst err / S of each family over the banded cases above, and the
    smallest power of two at least 4 x it (printed; the bands themselves are asserted where they are measured)"""
    import math
    for fam, A in (("igemm", R.A_IGEMM), ("split", R.A_SPLIT), ("wgrad", R.A_WGRAD), ("rgb", R.A_RGB)):
        r = WORST[fam]
        if r > 0:
            need = 2.0 ** math.ceil(math.log2(4 * r))
            print(f"WORST {fam}: err/S {r:.3e} = 2^{math.log2(r):.2f}; 4 x -> A = 2^{int(math.log2(need))}; in use 2^{int(math.log2(A))}")
            assert A <= R.A_CEILING
