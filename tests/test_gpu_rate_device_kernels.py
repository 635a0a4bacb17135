"""lic_gain_rows_fwd / lic_gain_rows_bwd and lic_rd_loss_fwd_lam / lic_rd_loss_bwd_lam (qualities and lambdas
read from device memory) against the statements of tests/rate_device_ref.py and against the scalar loss entries, every
output between canaries (guarded.py).

Gain rows, (Q, M) in {(2, 5), (3, 16), (4, 192)}, B in {1, 3, 65}, k in {1, 4}; the qualities of a case are cut into
batches of B that together hold 0, every integer up to Q-1, fractions, a repeated value, -0.5, Q+1 and NaN:
  * the rows lie within 2^-23 + 2^-24 (1 + 3 max|T|) relative of float64 -- expf's documented 1 ulp, and the three
    roundings of the exponent (each at most 2^-24 max|T| absolute, an absolute error of the exponent being a relative
    error of the value); the worst share of the band is printed;
  * out-of-range and NaN qualities give the bytes of their clamped values; equal qualities give equal bytes; zero tables
    give 1.0 everywhere; at an integer q = i < Q-1 the rows do not depend on T[i+1];
  * the table gradient is the float32 statement bit for bit (shared levels, untouched levels -> exact zeros, a NULL
    d_rows -> a zero slice), the same bits on a second run, and within (2B + 2) 2^-24 sum|terms| of float64.
Loss, B in {1, 3, 65}, images of 3x64x64 and 3x5x7 (nx = 105: single floats), lambdas that differ and include a 0:
  * slots 1..8 and 16.. are lic_rd_loss_fwd's bits, out[0] = fl32(out[3] + out[9]), out[9] within 1 ulp of float64;
  * equal lambdas: the three gradients are lic_rd_loss_bwd's bytes; different ones: image b's dx_hat is the scalar
    launch with lambda_b; the 16-byte path and the single-float path (pointers moved by 4 bytes) agree.

Run on the MI355X box:  python -m pytest tests/test_gpu_rate_device_kernels.py -m gpu -q"""
import numpy as np
import pytest
import torch

import rate_device_ref as RD
from guarded import Guarded

pytestmark = pytest.mark.gpu

QM = [(2, 5), (3, 16), (4, 192)]
BATCHES = [1, 3, 65]
TMAX = 0.7


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    L.load()  # must be the in-tree HIP extension; raises if missing
    return L, F_, torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _tables(k, Q, M, seed):
    return np.random.RandomState(seed).uniform(-TMAX, TMAX, (k, Q, M)).astype(np.float32)


def _quality_batches(B, Q, seed):
    """arrays of B qualities that together hold the special values; fractions fill what is left"""
    r = np.random.RandomState(seed)
    special = [0.0] + [float(j) for j in range(1, Q)] + [0.25, Q - 1.5, 0.625, 0.625, -0.5, Q + 1.0, np.nan]
    n = -(-len(special) // B) * B
    vals = np.array(special + list(r.uniform(0, Q - 1, n - len(special))), np.float32)
    return [vals[j:j + B] for j in range(0, n, B)]


def _rows_fwd(env, q, T):
    """-> (rows [k][B][M], i [B], l [B]) as numpy, after the canary checks"""
    L, F_, dev = env
    k, Q, M = T.shape
    B = len(q)
    dq, dT = torch.from_numpy(np.ascontiguousarray(q)).to(dev), torch.from_numpy(T).to(dev)
    rows, lvl = Guarded(k * B, M, dev), Guarded.flat(2 * B, dev)
    L.check(L.load().lic_gain_rows_fwd(F_._ptr(dq), F_._ptr(dT), rows.ptr(), lvl.ptr(), k, Q, M, B, F_._stream()),
            "lic_gain_rows_fwd")
    torch.cuda.synchronize()
    assert rows.unwritten() == 0 and lvl.unwritten() == 0
    rows.check("rows")
    lvl.check("lvl")
    lv = lvl.cpu().numpy().reshape(-1)
    return rows.cpu().numpy().reshape(k, B, M), lv[:B].view(np.int32).copy(), lv[B:].copy(), (rows, lvl)


def _rows_bwd(env, held, d_rows, k, Q, M, B):
    L, F_, dev = env
    rows, lvl = held
    dg = [None if g is None else torch.from_numpy(np.ascontiguousarray(g)).to(dev) for g in d_rows] + [None] * (4 - k)
    dt = Guarded(k * Q, M, dev)
    L.check(L.load().lic_gain_rows_bwd(lvl.ptr(), rows.ptr(), *[F_._ptr(g) for g in dg], dt.ptr(), k, Q, M, B,
                                       F_._stream()), "lic_gain_rows_bwd")
    torch.cuda.synchronize()
    assert dt.unwritten() == 0
    dt.check("d_tables")
    return dt.cpu().numpy().reshape(k, Q, M)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Q,M", QM)
def test_gain_rows_forward(env, Q, M, B, k):
    T = _tables(k, Q, M, 100 + Q)
    band = 2.0 ** -23 + 2.0 ** -24 * (1 + 3 * float(np.abs(T).max()))
    share = 0.0
    for q in _quality_batches(B, Q, 7):
        rows, i, l, _ = _rows_fwd(env, q, T)
        wi, wl = RD.levels(q, Q)
        assert np.array_equal(i, wi) and np.array_equal(_bits(l), _bits(wl)), (q, i, l)
        want = RD.rows64(q, T)
        share = max(share, float((np.abs(rows - want) / want).max()) / band)
        # the clamp is the contract: -0.5, Q+1 and NaN are 0, Q-1 and 0
        qc = np.where(np.isnan(q), 0, np.clip(q, 0, Q - 1)).astype(np.float32)
        if not np.array_equal(_bits(qc), _bits(q)):
            clamped, *_ = _rows_fwd(env, qc, T)
            assert np.array_equal(_bits(rows), _bits(clamped)), q
        for a in range(B):
            for b in range(a + 1, B):
                if qc[a] == qc[b]:
                    assert np.array_equal(_bits(rows[:, a]), _bits(rows[:, b])), (a, b)
    print(f"Q={Q} M={M} B={B} k={k}: worst share of the float64 band {share:.3f}")
    assert share <= 1.0, share


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Q,M", QM)
def test_zero_tables_and_integer_qualities(env, Q, M, B):
    q = _quality_batches(B, Q, 8)[0]
    ones, *_ = _rows_fwd(env, q, np.zeros((4, Q, M), np.float32))
    assert np.array_equal(_bits(ones), _bits(np.ones_like(ones)))
    T = _tables(2, Q, M, 200 + Q)
    for lev in range(Q - 1):                                    # q = lev exactly: weight 0 on T[lev + 1]
        qi = np.full(B, lev, np.float32)
        base, *_ = _rows_fwd(env, qi, T)
        other = T.copy()
        other[:, lev + 1] = _tables(2, 1, M, 300 + lev)[:, 0]
        moved, *_ = _rows_fwd(env, qi, other)
        assert np.array_equal(_bits(base), _bits(moved)), lev
        assert np.allclose(base, np.exp(T[:, lev].astype(np.float64))[:, None, :], rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Q,M", QM)
def test_gain_rows_backward(env, Q, M, B, k):
    T = _tables(k, Q, M, 400 + Q)
    r = np.random.RandomState(401)
    # the special values; then qualities below 1: levels 0 and 1 shared by all images, the levels above untouched
    for q in _quality_batches(B, Q, 9)[:2] + [r.uniform(0, 1, B).astype(np.float32)]:
        rows, i, l, held = _rows_fwd(env, q, T)
        d_rows = [r.standard_normal((B, M)).astype(np.float32) for _ in range(k)]
        if k == 4:
            d_rows[2] = None                                    # no gradient for that table
        got = _rows_bwd(env, held, d_rows, k, Q, M, B)
        want32, _ = RD.table_grad(i, l, rows, d_rows, Q, np.float32)
        assert np.array_equal(_bits(got), _bits(want32)), q
        assert np.array_equal(_bits(_rows_bwd(env, held, d_rows, k, Q, M, B)), _bits(got))    # the same bits again
        want64, mag = RD.table_grad(i, l, rows, d_rows, Q, np.float64)
        assert (np.abs(got - want64) <= (2 * B + 2) * 2.0 ** -24 * mag).all()
        untouched = [j for j in range(Q) if j not in set(i) | set(i + 1)]
        assert not got[:, untouched].any() and not np.signbit(got[:, untouched]).any()
        if k == 4:
            assert not got[2].any()
    assert Q == 2 or untouched, "the last batch leaves a level untouched"


# ---------------------------------------------------------------------------------------------------------------------
# the loss with one lambda per image
# ---------------------------------------------------------------------------------------------------------------------
SIZES = {"3x64x64": (3 * 64 * 64, 64 * 64, 200, 24), "3x5x7": (105, 35, 11, 3)}     # nx, pixels, ny, nz
LAMBDAS = np.array([0.013, 0.0, 0.05, 0.002], np.float32)
_CACHE = {}


def _loss_inputs(env, B, size):
    """operands on the device, shared by the loss tests of one shape (never written)"""
    key = (B, size)
    if key not in _CACHE:
        _, _, dev = env
        nx, _, ny, nz = SIZES[size]
        r = np.random.RandomState(B + nx)
        up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
        x = r.rand(B, nx)
        _CACHE[key] = dict(ly=up(-r.gamma(2.0, 1.0, (B, ny))), lz=up(-r.gamma(2.0, 1.0, (B, nz))), x=up(x),
                           xh=up(np.clip(x + 0.05 * r.standard_normal((B, nx)), 0, 1)),
                           lam=LAMBDAS[r.randint(0, 4, B)] if B > 3 else LAMBDAS[:B].copy(),
                           gl=up(np.array([0.75])))
    return _CACHE[key]


def _loss_fwd(env, t, B, size, lam):
    """lam: a float (lic_rd_loss_fwd) or a float32 array [B] (lic_rd_loss_fwd_lam) -> out [16 + 2B] as numpy"""
    L, F_, dev = env
    nx, pixels, ny, nz = SIZES[size]
    lib = L.load()
    nbytes = lib.lic_rd_loss_workspace_bytes(B)
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    out = Guarded.flat(16 + 2 * B, dev)
    if isinstance(lam, float):
        fn, arg, keep = lib.lic_rd_loss_fwd, lam, None
    else:
        keep = torch.from_numpy(lam).to(dev)
        fn, arg = lib.lic_rd_loss_fwd_lam, F_._ptr(keep)
    L.check(fn(F_._ptr(t["ly"]), ny, F_._ptr(t["lz"]), nz, F_._ptr(t["xh"]), F_._ptr(t["x"]), nx, B, pixels, arg, out.ptr(),
               F_._ptr(ws), nbytes, F_._stream()), "rd_loss forward")
    torch.cuda.synchronize()
    assert out.unwritten() == 0
    out.check("out")
    return out.cpu().numpy().reshape(-1)


def _loss_bwd(env, t, B, size, lam, shift=0):
    """-> (dlogp_y, dlogp_z, dx_hat) as numpy; `shift`: x_hat, x and dx_hat moved that many floats off their alignment"""
    L, F_, dev = env
    nx, pixels, ny, nz = SIZES[size]
    lib = L.load()
    xh = Guarded.holding(t["xh"].reshape(1, -1), dev, shift=shift)
    x = Guarded.holding(t["x"].reshape(1, -1), dev, shift=shift)
    dy, dz, dx = Guarded.flat(B * ny, dev), Guarded.flat(B * nz, dev), Guarded(1, B * nx, dev, shift=shift)
    if isinstance(lam, float):
        fn, arg, keep = lib.lic_rd_loss_bwd, lam, None
    else:
        keep = torch.from_numpy(lam).to(dev)
        fn, arg = lib.lic_rd_loss_bwd_lam, F_._ptr(keep)
    L.check(fn(xh.ptr(), x.ptr(), ny, nz, nx, B, pixels, arg, F_._ptr(t["gl"]), dy.ptr(), dz.ptr(), dx.ptr(), F_._stream()),
            "rd_loss backward")
    torch.cuda.synchronize()
    for name, g in (("dlogp_y", dy), ("dlogp_z", dz), ("dx_hat", dx)):
        assert g.unwritten() == 0, name
        g.check(name)
    return dy.cpu().numpy().reshape(-1), dz.cpu().numpy().reshape(-1), dx.cpu().numpy().reshape(B, nx)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("B", BATCHES)
def test_per_image_loss_forward(env, B, size):
    t = _loss_inputs(env, B, size)
    lam = t["lam"]
    assert B == 1 or (len(set(lam.tolist())) > 1 and 0.0 in lam)
    scalar = _loss_fwd(env, t, B, size, 0.01)
    got = _loss_fwd(env, t, B, size, lam)
    assert np.array_equal(_bits(got[1:9]), _bits(scalar[1:9])) and np.array_equal(_bits(got[16:]), _bits(scalar[16:]))
    assert not got[10:16].any()
    assert _bits(got[0]) == _bits(RD.loss_slot0(got[3], got[9]))
    want = RD.distortion_term64(lam, got[16:16 + B])
    print(f"B={B} {size}: out[9] = {got[9]!r}, float64 {want!r}, apart {abs(float(got[9]) - want) / np.spacing(np.float32(want)):.3f} ulp")
    assert abs(float(got[9]) - want) <= np.spacing(np.float32(want))
    if B == 1 and lam[0] != 0:
        assert got[9] > 0


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("B", BATCHES)
def test_per_image_loss_backward(env, B, size):
    t = _loss_inputs(env, B, size)
    nx = SIZES[size][0]
    # all lambdas equal: the scalar entry's bytes, all three gradients
    same = _loss_bwd(env, t, B, size, np.full(B, LAMBDAS[0], np.float32))
    scalar = {float(v): _loss_bwd(env, t, B, size, float(v)) for v in sorted(set(t["lam"].tolist()) | {float(LAMBDAS[0])})}
    for a, b in zip(same, scalar[float(LAMBDAS[0])]):
        assert np.array_equal(_bits(a), _bits(b))
    # different lambdas: image b is the scalar launch with lambda_b
    dy, dz, dx = _loss_bwd(env, t, B, size, t["lam"])
    assert np.array_equal(_bits(dy), _bits(same[0])) and np.array_equal(_bits(dz), _bits(same[1]))
    for b, v in enumerate(t["lam"].tolist()):
        assert np.array_equal(_bits(dx[b]), _bits(scalar[v][2][b])), (b, v)
        if v == 0:
            assert not dx[b].any()
    # and the statement of kx: dx = (x_hat - x) * fl32(gl * kx_b)
    xh, x = t["xh"].cpu().numpy(), t["x"].cpu().numpy()
    for b, v in enumerate(t["lam"].tolist()):
        k = np.float32(np.float32(0.75) * RD.kx32(v, nx, B))
        assert np.array_equal(_bits(dx[b]), _bits((xh[b] - x[b]).astype(np.float32) * k)), b
    # single floats (every pointer 4 bytes off) against 16-byte pieces
    moved = _loss_bwd(env, t, B, size, t["lam"], shift=1)
    for a, b in zip(moved, (dy, dz, dx)):
        assert np.array_equal(_bits(a), _bits(b))
