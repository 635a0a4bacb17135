"""The numpy statements of the device-quality entries (tests/rate_device_ref.py) against what they restate, and the
per-image draw of the Trainer.  Host only."""
import random

import numpy as np

import gain_ref as G
import rate_device_ref as RD


def _tables(k, Q, M, seed):
    return np.random.RandomState(seed).uniform(-0.7, 0.7, (k, Q, M)).astype(np.float32)


def _qualities(Q):
    """0, every integer up to Q-1, fractions, a repeated value"""
    return np.array([0.0] + [float(j) for j in range(1, Q)] + [0.25, Q - 1.5, Q - 1 - 1e-3, 0.25], np.float32)


def test_rows_statement_is_gain_refs_interpolation():
    for Q, M in ((2, 5), (3, 16), (4, 192)):
        T = _tables(2, Q, M, Q)
        q = _qualities(Q)
        rows = RD.rows64(q, T)
        assert rows.shape == (2, len(q), M)
        for t in range(2):
            for b, qb in enumerate(q):
                want = G.interpolate(T[t], float(qb))
                assert np.allclose(rows[t, b], want, rtol=1e-15, atol=0), (Q, t, b)


def test_clamp_and_nan_of_the_levels():
    i, l = RD.levels(np.array([-0.5, 4.0, np.nan, 2.0, 1.75], np.float32), 3)
    assert i.tolist() == [0, 1, 0, 1, 1] and l.tolist() == [0.0, 1.0, 0.0, 1.0, 0.75]


def test_table_gradient_is_the_central_difference_of_the_rows():
    Q, M, k = 3, 4, 2
    T = _tables(k, Q, M, 11).astype(np.float64)
    q = np.array([0.0, 0.5, 0.5, 2.0, 1.25], np.float32)          # a shared level, an exact integer, the top
    g = np.random.RandomState(12).standard_normal((k, len(q), M))
    i, l = RD.levels(q, Q)
    got, _ = RD.table_grad(i, l, RD.rows64(q, T), list(g), Q, np.float64)
    h = 1e-6
    for idx in np.ndindex(k, Q, M):
        up, dn = T.copy(), T.copy()
        up[idx] += h
        dn[idx] -= h
        num = ((RD.rows64(q, up) - RD.rows64(q, dn)) * g).sum() / (2 * h)
        assert abs(got[idx] - num) <= 1e-8 * max(1.0, abs(num)), (idx, got[idx], num)
    # no gradient for a table: its slice is zeros, the others are unchanged
    part, _ = RD.table_grad(i, l, RD.rows64(q, T), [g[0], None], Q, np.float64)
    assert np.array_equal(part[0], got[0]) and not part[1].any()


def test_float32_gradient_statement_follows_the_float64_one():
    Q, M, k, B = 4, 7, 1, 9
    T = _tables(k, Q, M, 13)
    q = np.random.RandomState(14).uniform(0, 1.5, B).astype(np.float32)   # level 3 untouched
    g = np.random.RandomState(15).standard_normal((k, B, M)).astype(np.float32)
    i, l = RD.levels(q, Q)
    rows = RD.rows64(q, T).astype(np.float32)
    g32, _ = RD.table_grad(i, l, rows, list(g), Q, np.float32)
    g64, mag = RD.table_grad(i, l, rows, list(g), Q, np.float64)
    assert g32.dtype == np.float32 and not g32[0, 3].any()
    assert (np.abs(g32 - g64) <= (2 * B + 2) * 2.0 ** -24 * mag).all()


def test_loss_statements():
    lams = np.array([0.01, 0.0, 0.05], np.float32)
    mse = np.array([1e-3, 2e-3, 5e-4], np.float32)
    want = (0.01 * 65025 * 1e-3 + 0.05 * 65025 * 5e-4) / 3
    assert abs(RD.distortion_term64(lams, mse) - want) <= 1e-6 * want
    assert RD.loss_slot0(0.5, 0.25) == np.float32(0.75)
    # lic_rd_loss_bwd's host expression, written out in C order
    lam, nx, B = np.float32(0.013), 3 * 64 * 64, 3
    assert RD.kx32(lam, nx, B) == np.float32(np.float32(np.float32(lam * np.float32(65025)) * np.float32(2))
                                            / np.float32(np.float32(nx) * np.float32(B)))
    assert RD.kx32(0.0, nx, B) == 0.0


def test_per_image_draw_is_pinned_and_resumes():
    from neural_image_compression_amd.trainer import draw_rate_points
    points = [(0.0, 0.002), (1.0, 0.005), (2.0, 0.02), (3.0, 0.05)]
    rng = random.Random(5)
    drawn = [draw_rate_points(rng, points, 3) for _ in range(2)]
    assert [[points.index(p) for p in batch] for batch in drawn] == [[2, 2, 0], [3, 1, 0]]
    state = rng.getstate()
    nxt = [draw_rate_points(rng, points, 3) for _ in range(2)]
    assert [[points.index(p) for p in batch] for batch in nxt] == [[1, 0, 2], [3, 1, 3]]
    again = random.Random(99)
    again.setstate(state)
    assert [draw_rate_points(again, points, 3) for _ in range(2)] == nxt
    # one choice per image, in image order: the same stream as B single draws
    one = random.Random(5)
    assert [one.choice(points) for _ in range(3)] == drawn[0]
