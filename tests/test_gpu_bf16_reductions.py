"""The bf16 backward contraction and reduction side through the C ABI, against tests/bf16_reduce_ref.py:
lic_wgrad_bf16 / lic_wgrad_bf16_partial (all 12 rows of the wgrad_bf16_kernel table, every ring tail, short last splits,
channel tails, gathered operands, strided destinations), lic_reduce_batch on hand-made slabs and partials, the bf16
column sums and the two elementwise kernels behind them.

Integer data ({-3..3}: exact in bf16, every sum an integer below 2^24 -- asserted by tests/test_bf16_reduce_ref.py) is
compared with `==`: no tolerance, so a kernel that loses, duplicates or misplaces one term fails.  Real-valued data is
compared bit for bit where the association order is documented (lic_reduce_batch) and under the derived summation
bound where it is not (the MFMA contraction).  Destinations and workspaces lie between sentinel-filled guard bands.
Which cases exist and what they cover is decided, and asserted on the CPU, in the two files named above.

Run on the MI355X box:  python -m pytest tests/test_gpu_bf16_reductions.py -m gpu -q -s"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bf16_reduce_ref as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = -777.25          # no integer sum times 1, 1/2 or -2 is this
SENT_BF = -768.0       # the same for bf16 buffers (exact in bf16)
GUARD = 256
_STOP = []              # the first launch that failed: nothing is launched after it


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd.functional import _stream
    lib = L.load()  # must be the in-tree HIP extension; raises if missing
    return SimpleNamespace(L=L, lib=lib, dev=torch.device("cuda:0"), stream=_stream, hip0=lib.lic_last_hip_error())


@pytest.fixture(autouse=True)
def _no_launch_after_a_failed_one():
    if _STOP:
        pytest.fail(f"not run: an earlier case failed to launch ({_STOP[0]})")


def ok(env, rc, what):
    if rc != 0:
        _STOP.append(f"{what}: status {rc}, hipError {env.lib.lic_last_hip_error()}")
        pytest.fail(_STOP[0])


def finish(env, what):
    """the one synchronisation of a case; lic_last_hip_error keeps the last failure, so it must not have moved"""
    try:
        torch.cuda.synchronize()
    except Exception as e:
        _STOP.append(f"{what}: {e}")
        raise
    if env.lib.lic_last_hip_error() != env.hip0:
        _STOP.append(f"{what}: hipError {env.lib.lic_last_hip_error()}")
        pytest.fail(_STOP[0])


def ptr(t):
    return C.c_void_p(t.data_ptr())


def guarded(env, n, fill=SENT):
    """(buffer, payload view): n floats of `fill` between two guard bands of the sentinel"""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=env.dev)
    v = buf[GUARD:GUARD + n]
    if fill != SENT:
        v.fill_(fill)
    return buf, v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def bands_intact(buf, what):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all(), f"{what}: guard band written"
    return h[GUARD:-GUARD]


def place_bf16(env, a, ld, offset=0):
    """rows of `a` [rows][C] at pitch ld in a bf16 device buffer, the base 16 bytes into its allocation when `offset`;
    the pad columns hold 3: a kernel that reads them gets wrong sums"""
    rows, Cc = a.shape
    host = np.full((rows, ld), 3.0, np.float32)
    host[:, :Cc] = a
    buf = torch.zeros(rows * ld + 8, dtype=BF, device=env.dev)
    v = buf[8 * offset:8 * offset + rows * ld]
    v.copy_(torch.from_numpy(host).reshape(-1).to(BF))
    assert v.data_ptr() % 16 == 0
    return v


# ---------------------------------------------------------------------------------------------
# lic_wgrad_bf16 / lic_wgrad_bf16_partial
# ---------------------------------------------------------------------------------------------
def _square_bf16(g):
    return ref.bf16_round((g * g).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _wgrad_expected(case):
    P, G = ref.wgrad_inputs(case)
    f = ref.wgrad_fields(case)
    want = ref.wgrad_ref(P, G, f, square=_square_bf16)
    weight = ref.wgrad_ref(P, G, f, square=_square_bf16, absolute=True) if case.data == "real" else None
    return P, G, want, weight


def _wgrad_desc(env, case, p, g, dst):
    d = ref.fill_desc(env.L.WgradDesc(), ref.wgrad_fields(case))
    d.p, d.g, d.dst = p.data_ptr(), g.data_ptr(), dst.data_ptr()
    return d


@pytest.mark.parametrize("case", ref.WGRAD_CASES, ids=[c.name for c in ref.WGRAD_CASES])
def test_wgrad_bf16_against_the_contraction(env, case):
    """dst of lic_wgrad_bf16 and of lic_wgrad_bf16_partial + lic_reduce_batch: equal to each other, equal to the integer
    contraction (integer data) or within (Ps + splitk + 2) 2^-24 |scale| sum |row| |col| of the float64 one (real
    data: any-order fp32 summation of exactly representable products); nothing else of dst or around it written"""
    lib = env.lib
    f = ref.wgrad_fields(case)
    P, G, want, weight = _wgrad_expected(case)
    TM, TN, splitk, cps, nloc = ref.plan_ref(f)
    Ps, ntaps = case.B * case.Hs * case.Ws, case.kh * case.kw
    Cm, Cn = want.shape[1:]
    sm, sn, stap, n_dst = ref.wgrad_layout(case)
    tp = place_bf16(env, P.reshape(Ps, case.Cp), f.p_ld, case.offset)
    tg = place_bf16(env, G.reshape(-1, case.Cg), f.g_ld, case.offset)
    outs = []
    for entry in ("lic_wgrad_bf16", "lic_wgrad_bf16_partial"):
        dbuf, dst = guarded(env, n_dst)
        d = _wgrad_desc(env, case, tp, tg, dst)
        nbytes = lib.lic_wgrad_bf16_workspace_bytes(C.byref(d))
        assert nbytes == splitk * ntaps * Cm * Cn * 4, (nbytes, splitk)
        wbuf, ws = guarded(env, nbytes // 4)
        if entry == "lic_wgrad_bf16":
            ok(env, lib.lic_wgrad_bf16(C.byref(d), ptr(ws), nbytes, env.stream()), f"{entry} {case.name}")
        else:
            job = env.L.ReduceJob()
            ok(env, lib.lic_wgrad_bf16_partial(C.byref(d), ptr(ws), nbytes, C.byref(job), env.stream()),
               f"{entry} {case.name}")
            assert (job.kind, job.splitk, job.ntaps, job.Cm, job.Cn) == (ref.SLABS, splitk, ntaps, Cm, Cn)
            ok(env, lib.lic_reduce_batch(C.byref(job), 1, env.stream()), f"lic_reduce_batch {case.name}")
        outs.append((dbuf, wbuf))
    finish(env, case.name)
    off = ref.scatter_offsets(ntaps, Cm, Cn, sm, sn, stap).reshape(-1)
    got = []
    for (dbuf, wbuf), entry in zip(outs, ("direct", "partial")):
        h = bands_intact(dbuf, f"{entry} dst")
        slabs = bands_intact(wbuf, f"{entry} workspace")
        assert not (slabs == SENT).any(), "a slab element was left unwritten"
        rest = np.ones(n_dst, bool)
        rest[off] = False
        assert (h[rest] == SENT).all(), f"{entry}: dst written outside the scatter pattern"
        got.append(h[off].reshape(want.shape))
    assert np.array_equal(bits(got[0]), bits(got[1])), "lic_wgrad_bf16 and partial + lic_reduce_batch differ"
    err = np.abs(got[0].astype(np.float64) - want)
    if case.data == "int":
        bad = np.argwhere(err != 0)
        print(case.name, f"<{TM},{TN}> splits {nloc}: {len(bad)} of {err.size} elements differ")
        assert len(bad) == 0, (f"first (tap, m, n) = {bad[0].tolist()}: got {got[0][tuple(bad[0])]}, "
                               f"want {want[tuple(bad[0])]}; {len(bad)} elements differ")
    else:
        bound = (Ps + splitk + 2) * 2.0 ** -24 * weight
        live = weight > 0
        print(case.name, f"<{TM},{TN}> splits {nloc}: worst error", float((err[live] / bound[live]).max()) if live.any() else 0.0,
              "of the summation bound")
        assert (err <= bound).all(), float((err - bound).max())


def test_wgrad_bf16_refusals(env):
    """what the ABI refuses, it refuses before any launch: the status, and dst keeps its sentinel"""
    lib, L = env.lib, env.L
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    Ps = 40
    tp = torch.ones(Ps * 256 + 64, dtype=BF, device=env.dev)
    tg = torch.ones(Ps * 256 + 64, dtype=BF, device=env.dev)
    dbuf, dst = guarded(env, 256 * 256)
    wbuf, ws = guarded(env, 256 * 256)

    def desc(Cp=64, Cg=64, p_ld=None, g_ld=None, g_is_row=0, sq_p=0, sq_g=0, p_off=0):
        d = L.WgradDesc()
        d.p, d.g, d.dst = tp.data_ptr() + p_off, tg.data_ptr(), dst.data_ptr()
        d.p_ld, d.g_ld = (Cp if p_ld is None else p_ld), (Cg if g_ld is None else g_ld)
        d.dst_sm, d.dst_sn, d.dst_stap = (Cp if g_is_row else Cg), 1, 0
        d.B, d.Hs, d.Ws, d.Cp, d.Hl, d.Wl, d.Cg = 1, 1, Ps, Cp, 1, Ps, Cg
        d.kh = d.kw = d.stride = 1
        d.pad, d.g_is_row, d.sq_p, d.sq_g, d.scale = 0, g_is_row, sq_p, sq_g, 1.0
        return d

    full = 256 * 256 * 4
    refused = [("Cp % 8", desc(Cp=60, p_ld=64), full, UNSUPPORTED),
               ("Cg % 8", desc(Cg=100, g_ld=104), full, UNSUPPORTED),
               ("p_ld % 8", desc(p_ld=68), full, UNSUPPORTED),
               ("g_ld % 8", desc(g_ld=100), full, UNSUPPORTED),
               ("squared row operand", desc(g_is_row=1, sq_g=1), full, UNSUPPORTED),
               ("squared plain operand", desc(sq_p=1), full, UNSUPPORTED),
               ("squared column, unequal tiles", desc(Cp=64, Cg=128, sq_g=1), full, UNSUPPORTED),
               ("workspace one byte short", desc(), 64 * 64 * 4 - 1, WORKSPACE),
               ("misaligned operand", desc(p_off=8), full, INVALID),
               ("empty grid", desc(Cp=0), full, INVALID)]
    for what, d, nbytes, status in refused:
        assert lib.lic_wgrad_bf16(C.byref(d), ptr(ws), nbytes, env.stream()) == status, what
        job = L.ReduceJob()
        assert lib.lic_wgrad_bf16_partial(C.byref(d), ptr(ws), nbytes, C.byref(job), env.stream()) == status, what
    d = desc()
    assert lib.lic_wgrad_bf16(C.byref(d), None, full, env.stream()) == INVALID
    assert lib.lic_wgrad_bf16_partial(C.byref(d), ptr(ws), full, None, env.stream()) == INVALID
    assert lib.lic_wgrad_bf16_workspace_bytes(C.byref(desc())) == 64 * 64 * 4          # ... and the accepted twin is one
    finish(env, "refusals")
    assert (dbuf.cpu().numpy() == SENT).all() and (wbuf.cpu().numpy() == SENT).all(), "a refused call launched"


# ---------------------------------------------------------------------------------------------
# lic_reduce_batch on hand-made slabs and partials
# ---------------------------------------------------------------------------------------------
def _reduce_job(env, j, src, dst, param):
    q = ref.fill_desc(env.L.ReduceJob(), j)
    q.src, q.dst, q.param = src.data_ptr(), dst.data_ptr(), (None if param is None else param.data_ptr())
    return q


def _stage_reduce(env, j):
    src, param = ref.reduce_inputs(j)
    t_src = torch.from_numpy(src).to(env.dev)
    dbuf, dst = guarded(env, j.extent)
    t_par = None if param is None else torch.from_numpy(param).to(env.dev)
    return SimpleNamespace(j=j, src=src, param=param, t_src=t_src, dbuf=dbuf, t_par=t_par,
                           job=_reduce_job(env, j, t_src, dst, t_par))


def _check_reduce(s):
    j = s.j
    h = bands_intact(s.dbuf, j.name)
    off, want = ref.reduce_ref(j, s.src, s.param)
    rest = np.ones(j.extent, bool)
    rest[off] = False
    assert (h[rest] == SENT).all(), f"{j.name}: written outside the destination pattern (Mvalid / Nvalid / strides)"
    bad = np.flatnonzero(bits(h[off]) != bits(want))
    assert bad.size == 0, f"{j.name}: {bad.size} of {off.size} differ, first at {off[bad[0]]}: {h[off][bad[0]]!r} vs {want[bad[0]]!r}"
    if j.data == "int" and j.epilogue == ref.EPI_NONE:
        total = s.src.astype(np.float64).sum(0) * j.scale
        if j.kind == ref.SLABS:
            total = total.reshape(j.ntaps, j.Cm, j.Cn)[:, :j.Mvalid or j.Cm, :j.Nvalid or j.Cn].reshape(-1)
        assert np.array_equal(h[off].astype(np.float64), total), f"{j.name}: not the integer sum"


@pytest.mark.parametrize("j", ref.REDUCE_CASES, ids=[j.name for j in ref.REDUCE_CASES])
def test_reduce_batch_one_job(env, j):
    """bit for bit reduce_slabs_ref / reduce_columns_ref (the documented association order), the integer sum on
    integer data; dropped rows and columns, gaps and the guard bands keep their sentinel"""
    s = _stage_reduce(env, j)
    ok(env, env.lib.lic_reduce_batch(C.byref(s.job), 1, env.stream()), f"lic_reduce_batch {j.name}")
    finish(env, j.name)
    _check_reduce(s)


def test_reduce_batch_33_jobs_two_launches(env):
    """one call with one job more than a launch's table holds, kinds mixed, depths from 1 to 600: the depth sort
    permutes them and block0 dispatch has to find each job's blocks"""
    staged = [_stage_reduce(env, j) for j in ref.batch33()]
    arr = (env.L.ReduceJob * len(staged))(*[s.job for s in staged])
    ok(env, env.lib.lic_reduce_batch(arr, len(staged), env.stream()), "lic_reduce_batch, 33 jobs")
    finish(env, "33 jobs")
    for s in staged:
        _check_reduce(s)
    assert env.lib.lic_reduce_batch(arr, 0, env.stream()) == 0 and env.lib.lic_reduce_batch(None, 1, env.stream()) == -1


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Cc,pad", ref.COLSUM_CASES, ids=[f"{P}x{Cc}+{pad}" for P, Cc, pad in ref.COLSUM_CASES])
def test_colsum_bf16_of_integers(env, P, Cc, pad):
    """lic_colsum_bf16, lic_colsum2_bf16 and their _partial forms + lic_reduce_batch: scale * the integer column sums,
    `==`; the pair variant on two different matrices"""
    lib, L = env.lib, env.L
    a, b = ref.colsum_inputs(P, Cc, pad), ref.colsum_inputs(P, Cc, pad, seed=1)
    ld = Cc + pad
    ta, tb = place_bf16(env, a[:, :Cc], ld), place_bf16(env, b[:, :Cc], ld, offset=1)
    nchunk = min(256, -(-P // 256))
    nbytes = lib.lic_colsum_bf16_workspace_bytes(P, Cc)
    assert nbytes == nchunk * Cc * 4
    scale = ref.SCALES[(P + Cc) % 3]
    want = [scale * m[:, :Cc].astype(np.float64).sum(0) for m in (a, b)]
    outs = []

    def bufs(k):
        o = [guarded(env, Cc) for _ in range(k)]
        w = guarded(env, k * nbytes // 4)
        outs.append((o, w, k))
        return [v for _, v in o], w[1]

    (o,), w = bufs(1)
    ok(env, lib.lic_colsum_bf16(ptr(ta), ld, P, Cc, scale, ptr(o), ptr(w), nbytes, env.stream()), "lic_colsum_bf16")
    (o,), w = bufs(1)
    job = L.ReduceJob()
    ok(env, lib.lic_colsum_bf16_partial(ptr(ta), ld, P, Cc, scale, ptr(o), ptr(w), nbytes, C.byref(job), env.stream()),
       "lic_colsum_bf16_partial")
    ok(env, lib.lic_reduce_batch(C.byref(job), 1, env.stream()), "lic_reduce_batch")
    (oa, ob), w = bufs(2)
    ok(env, lib.lic_colsum2_bf16(ptr(ta), ptr(tb), ld, P, Cc, scale, ptr(oa), ptr(ob), ptr(w), 2 * nbytes, env.stream()),
       "lic_colsum2_bf16")
    (oa, ob), w = bufs(2)
    jobs = (L.ReduceJob * 2)()
    ok(env, lib.lic_colsum2_bf16_partial(ptr(ta), ptr(tb), ld, P, Cc, scale, ptr(oa), ptr(ob), ptr(w), 2 * nbytes, jobs,
                                         env.stream()), "lic_colsum2_bf16_partial")
    ok(env, lib.lic_reduce_batch(jobs, 2, env.stream()), "lic_reduce_batch")
    assert lib.lic_colsum_bf16(ptr(ta), ld, P, Cc, scale, ptr(o), ptr(w), nbytes - 1, env.stream()) == -4
    finish(env, f"colsum {P}x{Cc}")
    for (o, w, k), entry in zip(outs, ("colsum", "colsum_partial", "colsum2", "colsum2_partial")):
        part = bands_intact(w[0], f"{entry} workspace")
        assert not (part == SENT).any(), f"{entry}: a partial sum was left unwritten"
        for i in range(k):
            got = bands_intact(o[i][0], f"{entry} out")
            assert np.array_equal(got.astype(np.float64), want[i]), \
                f"{entry} matrix {i}: {np.count_nonzero(got != want[i])} of {Cc} columns differ"


def _leaky_ref(y, dy, slope):
    """dx = y > 0 ? dy : bf16(fp32(dy) * slope): fp32 product, one round-to-nearest-even, wherever `y > 0` is false"""
    low = (dy.float() * torch.tensor(slope, dtype=torch.float32)).to(BF)
    return torch.where(y.float() > 0, dy, low)


def _leaky_inputs(n, seed, integers):
    """y with +0, -0 and the bf16 subnormals of either sign among normal deviates"""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(n, generator=gen).to(BF)
    special = torch.tensor([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -127, -2.0 ** -127, 1.0, -1.0]).to(BF)
    assert float(special[2]) > 0 and float(special[3]) < 0
    y[:8] = special
    if n >= 2048:
        y[n - 8:] = special.flip(0)
    if integers:
        dy = torch.randint(-3, 4, (n,), generator=gen).float().to(BF)
    else:
        dy = torch.randn(n, generator=gen).to(BF)
    return y, dy


@pytest.mark.parametrize("n", ref.ELEMENTWISE_N)
def test_leaky_bwd_bf16_exact(env, n):
    y, dy = _leaky_inputs(n, n % 1000, False)
    ty, tdy = y.to(env.dev), dy.to(env.dev)
    buf = torch.full((n + 16,), SENT_BF, dtype=BF, device=env.dev)
    ok(env, env.lib.lic_leaky_bwd_bf16(ptr(ty), ptr(tdy), ptr(buf[8:]), n, 0.01, env.stream()), "lic_leaky_bwd_bf16")
    finish(env, f"leaky {n}")
    h = buf.cpu()
    assert (h[:8].float() == SENT_BF).all() and (h[-8:].float() == SENT_BF).all(), "written outside dx"
    assert torch.equal(h[8:-8].view(torch.int16), _leaky_ref(y, dy, 0.01).view(torch.int16))


@pytest.mark.parametrize("n", ref.ELEMENTWISE_N)
@pytest.mark.parametrize("inverse", [0, 1])
def test_gdn_dnorm_bf16_vs_float64(env, n, inverse):
    """t = 0.5 g x / sqrt(norm) (inverse) or -0.5 g x norm^-1.5 in float64, at one bf16 rounding (bf16_close of
    tests/test_gpu_bf16.py: 2^-8 relative plus its scale floor)"""
    from test_gpu_bf16 import bf16_close
    gen = torch.Generator().manual_seed(n % 1000 + inverse)
    g, x = torch.randn(n, generator=gen).to(BF), torch.randn(n, generator=gen).to(BF)
    norm = (torch.rand(n, generator=gen) * 4 + 0.05).to(BF)
    g64, x64, n64 = g.double(), x.double(), norm.double()
    want = 0.5 * g64 * x64 / n64.sqrt() if inverse else -0.5 * g64 * x64 * n64 ** -1.5
    buf = torch.full((n + 16,), SENT_BF, dtype=BF, device=env.dev)
    tg, tx, tn = g.to(env.dev), x.to(env.dev), norm.to(env.dev)
    ok(env, env.lib.lic_gdn_dnorm_bf16(ptr(tg), ptr(tx), ptr(tn), ptr(buf[8:]), n, inverse, env.stream()),
       "lic_gdn_dnorm_bf16")
    finish(env, f"dnorm {n}")
    h = buf.cpu().float()
    assert (h[:8] == SENT_BF).all() and (h[-8:] == SENT_BF).all(), "written outside t"
    bf16_close(h[8:-8].numpy(), want.numpy(), f"dnorm n={n} inverse={inverse}")


LEAKY_COLSUM = [(P, Cc) for P, Cc, _ in ref.COLSUM_CASES if P <= 8191 or Cc < 640]


@pytest.mark.parametrize("P,Cc", LEAKY_COLSUM, ids=[f"{P}x{Cc}" for P, Cc in LEAKY_COLSUM])
def test_leaky_bwd_colsum_bf16(env, P, Cc):
    """dx as lic_leaky_bwd_bf16's statement, and its column sums: exact for integer dy and slope 1/2 (multiples of 1/2
    below 2^23), within (P + 2) 2^-24 sum |dx| of the float64 sums for real dy and slope 0.01; both ways of finishing"""
    lib, L = env.lib, env.L
    nbytes = lib.lic_colsum_bf16_workspace_bytes(P, Cc)
    runs = []
    for integers, slope in ((True, 0.5), (False, 0.01)):
        y, dy = _leaky_inputs(P * Cc, (P + Cc) % 1000, integers)
        ty, tdy = y.to(env.dev), dy.to(env.dev)
        for partial in (False, True):
            dx = torch.full((P * Cc + 16,), SENT_BF, dtype=BF, device=env.dev)
            obuf, out = guarded(env, Cc)
            wbuf, w = guarded(env, nbytes // 4)
            job = L.ReduceJob()
            ok(env, lib.lic_leaky_bwd_colsum_bf16(ptr(ty), ptr(tdy), ptr(dx[8:]), P, Cc, slope, ptr(out), ptr(w), nbytes,
                                                  C.byref(job) if partial else None, env.stream()),
               "lic_leaky_bwd_colsum_bf16")
            if partial:
                ok(env, lib.lic_reduce_batch(C.byref(job), 1, env.stream()), "lic_reduce_batch")
            runs.append((integers, slope, y, dy, dx, obuf, wbuf, partial, ty, tdy))
    finish(env, f"leaky colsum {P}x{Cc}")
    first = {}
    for integers, slope, y, dy, dx, obuf, wbuf, partial, _, _ in runs:
        want = _leaky_ref(y, dy, slope)
        h = dx.cpu()
        assert (h[:8].float() == SENT_BF).all() and (h[-8:].float() == SENT_BF).all(), "written outside dx"
        assert torch.equal(h[8:-8].view(torch.int16), want.view(torch.int16)), "dx"
        bands_intact(wbuf, "workspace")
        got = bands_intact(obuf, "out").astype(np.float64)
        w64 = want.double().reshape(P, Cc)
        sums, weight = w64.sum(0).numpy(), w64.abs().sum(0).numpy()
        if integers:
            assert np.array_equal(got, sums), f"{np.count_nonzero(got != sums)} of {Cc} column sums differ"
        else:
            assert (np.abs(got - sums) <= (P + 2) * 2.0 ** -24 * weight).all()
        assert np.array_equal(first.setdefault(integers, got), got), "finishing at once and through lic_reduce_batch differ"
