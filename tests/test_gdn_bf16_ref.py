"""CPU checks of tests/gdn_bf16_ref.py, the float64 statement of the bf16-storage GDN / IGDN at the kernels' rounding
points that tests/test_gpu_gdn_bf16.py holds the bf16 kernels to: where every rounding is the identity it IS
gdn_ref64; its exactness claims hold; few elements are ambiguous; and its bands catch each of the errors they exist for."""
import pytest
import torch

import gdn_bf16_ref as R
import gdn_ref64 as G

SENS = (64, 0, 129)      # the case of the sensitivity tests: two sweep tiles, one pixel in the second


def test_rne_bf16_is_torchs_conversion_and_rounds_from_float64_directly():
    g_ = torch.Generator().manual_seed(1)
    a = torch.randn(4096, generator=g_) * 10.0 ** (torch.rand(4096, generator=g_) * 8 - 4)
    assert torch.equal(R.rne_bf16(a), a.to(torch.bfloat16).double())           # fp32 in: one rounding either way
    # ties go to the even significand (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6) ...
    assert R.rne_bf16(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])).tolist() == [1.0, 1 + 2.0 ** -6, -1.0]
    # ... and a float64 value just above a tie rounds up, where a detour through fp32 would land on the tie first
    assert R.rne_bf16(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)).tolist() == [1 + 2.0 ** -7]
    assert R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, 0.0, -3.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0, 2.0 ** -6]
    assert R.round_half_up(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1.3])).tolist() == \
        [1 + 2.0 ** -7, 1 + 2.0 ** -6, float(R.rne_bf16(torch.tensor([1.3]))[0])]


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("C", R.WIDTHS)
def test_it_is_gdn_ref64_where_every_rounding_is_the_identity(C, inverse):
    P = 129
    i = R.exact_fwd_inputs(C, inverse, P)         # x, x^2, gamma_e bf16-exact: the pool's operands are not rounded
    assert all(R.is_bf16(i[k]) for k in ("x", "gamma_e", "beta_e")) and R.is_bf16(i["x"] ** 2)
    n64, nq, y64 = R.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
    y_ref, n_ref = G.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
    assert torch.equal(n64, n_ref) and torch.equal(y64, y_ref)
    exact = nq == n64                              # ... and y is taken from the unrounded norm everywhere
    assert 0.0 < float(exact.double().mean()) < 1.0
    b = R.exact_bwd_inputs(C, inverse, P)          # norm in {1, 4}, t bf16-exact: nothing is rounded in front of the pool
    t64, dx64, mag = R.bwd(b["g"], b["x"], b["norm"], b["gamma_e"], inverse)
    t_ref, dx_ref, mag_ref = G.bwd(b["g"], b["x"], b["norm"], b["gamma_e"], inverse)
    assert torch.equal(t64, t_ref) and torch.equal(dx64, dx_ref) and torch.equal(mag, mag_ref)
    # the device's own t, where given, is what the pool contracts
    _, dx_dev, _ = R.bwd(b["g"], b["x"], b["norm"], b["gamma_e"], inverse, t_dev=2.0 * t64)
    u = b["g"].double() * (b["norm"].double().sqrt() if inverse else b["norm"].double().rsqrt())
    assert torch.equal(dx_dev - u, 2.0 * (dx64 - u))


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("C", R.WIDTHS)
def test_exactness_claims(C, inverse):
    """every value of the exact inputs is bf16-exact; the exact forward's pool is exact in fp32 and meets bf16 ties; the
    exact backward's t is bf16-exact and its dx exact in fp32.  GDN's exact dx (multiples of 1/16 up to about 100) is
    rounded by the bf16 store in 0.9 % (C = 64) to 8.6 % (C = 192) of elements from P = 31 up -- 1 % to 8 % in round
    figures -- with ties to the even and to the odd neighbour both among them: what pins round-to-nearest-even.  IGDN's
    exact dx (multiples of 1/2 below 128) is bf16-exact almost everywhere: it pins the values, not the rounding."""
    for P in (129, 357):
        f = R.exact_fwd_inputs(C, inverse, P)
        b = R.exact_bwd_inputs(C, inverse, P)
        assert all(R.is_bf16(v) for v in f.values()) and all(R.is_bf16(v) for v in b.values())
        n64, nq, _ = R.fwd(f["x"], f["beta_e"], f["gamma_e"], inverse)
        assert torch.equal(n64.float().double(), n64)
        # (exact in fp32, the pool needs no `ambiguous` mask: the store rounds n64 itself, ties among it)
        assert int(((n64 - nq).abs() == 0.5 * R.ulp_bf16(n64)).sum()) > 0
        t64, dx64, _ = R.bwd(b["g"], b["x"], b["norm"], b["gamma_e"], inverse)
        assert R.is_bf16(t64) and torch.equal(dx64.float().double(), dx64)
        rounded = R.rne_bf16(dx64) != dx64
        share = float(rounded.double().mean())
        print(f"C{C} inv{inverse} P{P}: dx rounds at the bf16 store in {100 * share:.2f} % of elements")
        tie = (dx64 - R.rne_bf16(dx64)).abs() == 0.5 * R.ulp_bf16(dx64)
        differs = R.round_half_up(dx64) != R.rne_bf16(dx64)
        assert bool(tie[differs].all())
        if inverse:
            assert share < 1e-3, share
        else:
            assert 0.009 <= share <= 0.086, share
            assert int(differs.sum()) > 0 and int((tie & rounded & ~differs).sum()) > 0


def test_ambiguous_share_is_at_most_one_percent():
    """the cap of test_gpu_gdn_bf16.py's recomputing-sweep cases, from the reference alone: per case and over all cases"""
    count = total = 0
    for C, inverse, P in R.CASES:
        i = R.banded_inputs(C, inverse, P)
        n64, _, _ = R.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
        amb = R.ambiguous(n64, C)
        share = float(amb.double().mean())
        count, total = count + int(amb.sum()), total + amb.numel()
        print(f"{R.case_id((C, inverse, P))}: {100 * share:.3f} % ambiguous")
        assert share <= 0.01, (C, inverse, P, share)
        # an unambiguous element rounds the same from anywhere inside the norm band
        lo, hi = n64 * (1 - R.K_FWD(C) * R.U), n64 * (1 + R.K_FWD(C) * R.U)
        same = (R.rne_bf16(lo) == R.rne_bf16(n64)) & (R.rne_bf16(hi) == R.rne_bf16(n64))
        assert bool(same[~amb].all())
    assert count / total <= 0.01, count / total


def test_neighbours_and_tile_colsums():
    n = torch.tensor([1.0, 1.003, 1.99, 2.0, 0.3], dtype=torch.float64)
    lo, hi = R.bf16_neighbours(n)
    assert R.is_bf16(lo) and R.is_bf16(hi) and bool((lo <= n).all()) and bool((n < hi).all())
    assert bool(((hi - lo) == R.ulp_bf16(n)).all())
    a = torch.arange(300 * 2, dtype=torch.float64).reshape(300, 2)
    rows, cnt = R.tile_colsums(a, 2)                 # tiles 0 and 2 -> row 0, tile 1 -> row 1
    assert torch.equal(rows[0], a[:128].sum(0) + a[256:].sum(0)) and torch.equal(rows[1], a[128:256].sum(0))
    assert cnt.tolist() == [128 + 44, 128]
    assert R.sweep_grid(1) == 1 and R.sweep_grid(129) == 2 and R.sweep_grid(R.BIG) == 2048
    assert R.colsum_ratio(rows.float(), a, 2) <= 1.0
    assert R.colsum_ratio(rows.flip(0).float(), a, 2) > 1.0
    one = torch.full((1, 2), 0.375, dtype=torch.float64)
    assert R.colsum_ratio(one, one, 1) == 0.0 and R.colsum_ratio(one * (1 + 2.0 ** -20), one, 1) == float("inf")


# ---------------------------------------------------------------------------------------------
# sensitivity: a perfect device (the reference rounded once) passes; each deliberate error misses the band
# ---------------------------------------------------------------------------------------------
def _perfect():
    C, inverse, P = SENS
    i = R.banded_inputs(C, inverse, P)
    n64, nq, y64 = R.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
    return i, n64, nq, y64


def _fwd_ratios(nq, yq, n64, y64, C):
    return R.band_ratio(nq, n64, n64, R.K_FWD(C)), R.band_ratio(yq, y64, y64.abs(), R.K_FWD(C))


def test_a_perfect_device_is_inside_every_band():
    C, inverse, P = SENS
    i, n64, nq, y64 = _perfect()
    rn, ry = _fwd_ratios(nq, R.rne_bf16(y64), n64, y64, C)
    assert rn <= 1.0 and ry <= 1.0, (rn, ry)
    t64, dx64, mag = R.bwd(i["g"], i["x"], i["norm"], i["gamma_e"], inverse)
    assert R.band_ratio(R.rne_bf16(t64), t64, t64.abs(), R.K_T) <= 1.0
    assert R.band_ratio(R.rne_bf16(dx64), dx64, mag, R.K_DX(C)) <= 1.0
    # the all-zero pixels: y, t exactly 0 and required to be
    z = G.zero_pixels(P)
    assert not bool(y64[z].any()) and not bool(t64[z].any())
    bad = R.rne_bf16(y64).clone()
    bad[z[0], 5] = 1e-30
    assert R.band_ratio(bad, y64, y64.abs(), R.K_FWD(C)) == float("inf")
    nan = R.rne_bf16(y64).clone()
    nan[7, 7] = float("nan")
    assert R.band_ratio(nan, y64, y64.abs(), R.K_FWD(C)) == float("inf")


def test_one_bf16_ulp_on_one_element_misses_the_band():
    C, inverse, P = SENS
    i, n64, nq, y64 = _perfect()
    for p, c in ((0, 0), (P - 1, C - 1), (128, 17), (31, 40)):       # the ragged last wave's pixel among them
        for sign in (1.0, -1.0):
            y = R.rne_bf16(y64).clone()
            y[p, c] += sign * R.ulp_bf16(y[p, c])
            if float(y64[p, c]) != 0.0:
                assert R.band_ratio(y, y64, y64.abs(), R.K_FWD(C)) > 1.0, (p, c, sign)
            n = nq.clone()
            n[p, c] += sign * R.ulp_bf16(n[p, c])
            assert R.band_ratio(n, n64, n64, R.K_FWD(C)) > 1.0, (p, c, sign)
    t64, dx64, mag = R.bwd(i["g"], i["x"], i["norm"], i["gamma_e"], inverse)
    # (pixel P - 1, alone in the last wave, has x = 0: t is 0 there and dx = g f)
    for a64, m, k, p in ((t64, t64.abs(), R.K_T, P - 2), (dx64, mag, R.K_DX(C), P - 1)):
        a = R.rne_bf16(a64).clone()
        a[p, 9] += R.ulp_bf16(a[p, 9])
        assert float(a64[p, 9]) != 0.0 and R.band_ratio(a, a64, m, k) > 1.0


@pytest.mark.parametrize("C", R.WIDTHS)
def test_a_dropped_chunk_and_a_transposed_gamma_miss_the_band(C):
    inverse, P = 0, 129
    i = R.banded_inputs(C, inverse, P)
    n64, nq, y64 = R.fwd(i["x"], i["beta_e"], i["gamma_e"], inverse)
    for chunk in range(C // 16):                 # a pool without the x channels 16 chunk .. 16 chunk + 15
        gam = i["gamma_e"].clone()
        gam[:, 16 * chunk:16 * chunk + 16] = 0.0
        nd, ndq, yd = R.fwd(i["x"], i["beta_e"], gam, inverse)
        rn, ry = _fwd_ratios(ndq, R.rne_bf16(yd), n64, y64, C)
        assert rn > 1.0 and ry > 1.0, (chunk, rn, ry)
    nt, ntq, yt = R.fwd(i["x"], i["beta_e"], i["gamma_e"].t().contiguous(), inverse)
    rn, ry = _fwd_ratios(ntq, R.rne_bf16(yt), n64, y64, C)
    assert rn > 1.0 and ry > 1.0, (rn, ry)
    t64, dx64, mag = R.bwd(i["g"], i["x"], i["norm"], i["gamma_e"], inverse)
    _, dxt, _ = R.bwd(i["g"], i["x"], i["norm"], i["gamma_e"].t().contiguous(), inverse)
    assert R.band_ratio(R.rne_bf16(dxt), dx64, mag, R.K_DX(C)) > 1.0
    # one 16-channel group of the output exchanged with its neighbour (swap_dword_pairs / unswap gone wrong)
    ys = R.rne_bf16(y64).clone()
    ys[:, 16:32], ys[:, 32:48] = R.rne_bf16(y64)[:, 32:48], R.rne_bf16(y64)[:, 16:32]
    assert R.band_ratio(ys, y64, y64.abs(), R.K_FWD(C)) > 1.0


def test_y_from_the_rounded_norm_misses_the_band():
    C, inverse, P = SENS
    i, n64, nq, y64 = _perfect()
    x = i["x"].double()
    for inv in (0, 1):
        n64, nq, y64 = R.fwd(i["x"], i["beta_e"], i["gamma_e"], inv)
        wrong = R.rne_bf16(x * (nq.sqrt() if inv else nq.rsqrt()))
        differs = wrong != R.rne_bf16(y64)
        share = float(differs.double().mean())
        print(f"y from the bf16 norm differs from y from the fp32 norm in {100 * share:.1f} % of elements")
        assert share > 0.05
        assert R.band_ratio(wrong, y64, y64.abs(), R.K_FWD(C)) > 1.0
        # ... and at most of the elements where it differs, not at one lucky one
        err = (wrong - y64).abs() / (0.5 * R.ulp_bf16(y64) + R.K_FWD(C) * R.U * y64.abs())
        assert float((err[differs] > 1.0).double().mean()) > 0.9


@pytest.mark.parametrize("C", R.WIDTHS)
def test_round_half_up_is_told_from_nearest_even_by_the_exact_case(C):
    """At a tie both neighbours lie exactly half a bf16 ulp from the exact value, so NO band around the exact value can
    tell them apart (asserted: the ratio stays below 1).  That is why the exact backward case compares bit for bit with
    rne_bf16(exact dx): against that comparison round-half-up fails, at ties only."""
    inverse, P = 0, 129
    b = R.exact_bwd_inputs(C, inverse, P)
    _, dx64, mag = R.bwd(b["g"], b["x"], b["norm"], b["gamma_e"], inverse)
    up, even = R.round_half_up(dx64), R.rne_bf16(dx64)
    wrong = up != even
    assert int(wrong.sum()) > 0
    assert bool(((dx64 - even).abs()[wrong] == 0.5 * R.ulp_bf16(dx64)[wrong]).all())
    assert R.band_ratio(up, dx64, mag, R.K_DX(C)) <= 1.0
    assert not torch.equal(R.bf16_bits(up), R.bf16_bits(even))
    assert R.band_ratio(up, even, torch.zeros_like(mag), 0, half_ulp=False) == float("inf")
    assert R.band_ratio(even, even, torch.zeros_like(mag), 0, half_ulp=False) == 0.0


def test_reparam_bwd_is_the_oracles():
    from oracle import oracle as O
    g_ = torch.Generator().manual_seed(3)
    p = torch.rand(257, generator=g_) * 2e-3
    d = torch.randn(257, generator=g_)
    for minimum in (1e-6, 0.0):
        bound = float(O.gdn_bounds(minimum))
        p[:3] = torch.tensor([bound, bound * 0.5, 0.0])
        ref = torch.from_numpy(O.gdn_reparam_bwd(p.numpy(), d.numpy(), minimum)).double()
        got = R.reparam_bwd(p, d, bound)
        assert bool(((got - ref).abs() <= 2 * R.U * got.abs()).all())
        assert torch.equal(got == 0, ref == 0)


def test_case_table():
    assert len(R.CASES) == len(set(R.CASES)) == 3 * 2 * 7
    assert R.SIZES == (1, 31, 33, 127, 128, 129, 357) and R.BIG == 128 * 2048 + 77
    assert R.BIG_CASES == [(64, 0, R.BIG), (128, 1, R.BIG)]
    for C, inverse, P in R.CASES:
        i = R.banded_inputs(C, inverse, P)
        assert all(R.is_bf16(i[k]) for k in ("x", "g", "norm")) and not R.is_bf16(i["gamma_e"])
        assert i["x"].dtype == torch.float32
