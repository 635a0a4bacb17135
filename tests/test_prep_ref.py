"""tests/prep_ref.py against itself, and lic_prep_plan (a host function: no GPU) on the case table of
tests/test_gpu_prep_layouts.py: block bookkeeping, the (tiled, v4) values recorded for the conv-weight rows, and the
condition that the table reaches every branch of the packers.  CPU only."""
import os

import numpy as np
import pytest

import prep_ref as R


# ---------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (9, 20, 33), (25, 40, 40), (4, 64, 64), (1, 75, 24), (1, 100, 100), (3, 31, 65)]


@pytest.mark.parametrize("kind", [R.PACK_F32, R.PACK_BF16, R.PACK_BF16_KPERM])
@pytest.mark.parametrize("taps,K,N", SHAPES)
def test_forward_map_is_injective_and_in_range(kind, taps, K, N):
    idx = R.dest(kind, taps, K, N)
    assert idx.shape == (taps, K, N)
    flat = idx.reshape(-1)
    assert flat.min() >= 0 and flat.max() < R.packed_elems(kind, taps, K, N)
    assert np.unique(flat).size == flat.size


def test_packed_sizes_are_the_headers():
    # [tap][ceil(K/16)][npad/32][2][64][4], npad = 32 if N <= 32 else ceil64(N); [tap][ceil(K/32)][ceil64(N)/32][2][64][8]
    assert R.packed_elems(R.PACK_F32, 25, 192, 192) == 25 * 12 * 6 * 2 * 64 * 4
    assert R.packed_elems(R.PACK_F32, 1, 80, 75) == 5 * 4 * 2 * 64 * 4
    assert R.packed_elems(R.PACK_F32, 9, 17, 24) == 9 * 2 * 1 * 2 * 64 * 4
    assert R.packed_elems(R.PACK_F32, 9, 17, 33) == 9 * 2 * 2 * 2 * 64 * 4
    assert R.packed_elems(R.PACK_BF16, 25, 192, 192) == 25 * 6 * 6 * 2 * 64 * 8
    assert R.packed_elems(R.PACK_BF16_KPERM, 1, 80, 75) == 3 * 4 * 2 * 64 * 8
    assert R.packed_elems(R.PACK_BF16, 1, 1, 1) == 2 * 2 * 64 * 8


@pytest.mark.parametrize("kind", [R.PACK_F32, R.PACK_BF16, R.PACK_BF16_KPERM])
@pytest.mark.parametrize("taps,K,N", SHAPES)
def test_unpack_returns_the_source_and_padding_is_plus_zero(kind, taps, K, N):
    rng = np.random.default_rng(taps * 1000 + K * 10 + N)
    v = rng.standard_normal((taps, K, N)).astype(np.float32)
    v[0, 0, 0] = -0.0
    packed = R.pack(kind, v)
    want = R.f32_bits(v) if kind == R.PACK_F32 else R.bf16_bits(v)
    assert np.array_equal(R.unpack(kind, packed, taps, K, N), want)
    rest = np.ones(packed.size, bool)
    rest[R.dest(kind, taps, K, N).reshape(-1)] = False
    assert not packed[rest].any()
    assert packed[R.dest(kind, taps, K, N)[0, 0, 0]] == (0x80000000 if kind == R.PACK_F32 else 0x8000)


def test_fp32_layout_spot_values():
    """the header's sentence, by hand: (k, n) of a chunk at lane (n%32) + 32*((k%16)/8), load q = (k%8)/4, float k%4"""
    idx = R.dest_f32(2, 40, 70)         # cpt 3, npad 128 -> 4 tiles of 512 floats per chunk
    assert idx[0, 0, 0] == 0
    assert idx[0, 5, 3] == 1 * 256 + 3 * 4 + 1                    # q 1, lane 3, float 1
    assert idx[0, 9, 33] == 512 + 0 * 256 + (1 + 32) * 4 + 1      # tile 1, lane 32 + 1, q 0
    assert idx[0, 17, 0] == 4 * 512 + 1                           # chunk 1
    assert idx[1, 39, 69] == ((1 * 3 + 2) * 4 + 2) * 512 + 1 * 256 + 5 * 4 + 3


def test_bf16_layout_spot_values_and_kperm_is_a_permutation_within_groups():
    idx = R.dest_bf16(1, 64, 40)        # cpt 2, npad 64 -> 2 tiles; a k-step of a tile is 512 elements
    assert idx[0, 0, 0] == 0 and idx[0, 7, 0] == 7
    assert idx[0, 8, 0] == 32 * 8                                 # h = 1: lane 32
    assert idx[0, 16, 1] == 512 + 8                               # k-step 1, lane 1
    assert idx[0, 45, 39] == ((1 * 2 + 1) * 2 + 0) * 512 + (7 + 32) * 8 + 5
    for taps, K, N in SHAPES:
        Kp = -(-K // 16) * 16           # whole groups, so that both orders fill the same slots
        a, b = R.dest_bf16(taps, Kp, N), R.dest_bf16(taps, Kp, N, kperm=True)
        ga = np.sort(a.reshape(taps, Kp // 16, 16, N), axis=2)
        gb = np.sort(b.reshape(taps, Kp // 16, 16, N), axis=2)
        assert np.array_equal(ga, gb), "kperm must permute slots inside each group of 16 k of a column"
        assert Kp < 8 or not np.array_equal(a, b)
    # slot (h, e) holds k = 8*(e/4) + 4*h + e%4, stated the header's way round
    b = R.dest_bf16(1, 16, 1, kperm=True)[0, :, 0]
    for h in range(2):
        for e in range(8):
            assert b[8 * (e // 4) + 4 * h + e % 4] == (32 * h) * 8 + e


def test_stem_operand():
    w = np.arange(1, 7 * 75 + 1, dtype=np.float32).reshape(7, 3, 5, 5)
    m = R.stem_logical(w)
    assert m.shape == (1, 80, 7)
    for k in range(80):
        r, jj = divmod(k, 16)
        if jj == 15:
            assert not m[0, k].any()
        else:
            s, c = divmod(jj, 3)
            assert np.array_equal(m[0, k], w[:, c, r, s])
    assert np.count_nonzero(m) == 7 * 75
    c = R.Case("s", R.PACK_BF16_STEM, "w", N=7)
    packed = R.expected(c, w.reshape(-1))
    assert packed.size == 3 * 64 * 32 == c.dst_bytes() // 2     # K = 80 padded to 96
    assert np.count_nonzero(packed) == 7 * 75
    assert np.array_equal(R.unpack(R.PACK_BF16, packed, 1, 80, 7), R.bf16_bits(m))


def test_bf16_rounding_ties_go_to_even_both_ways():
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)
    # lower neighbour even: the tie goes down; odd: up; one ulp of fp32 either side of the tie decides by itself
    assert R.bf16_bits(f([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000])).tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]
    assert R.bf16_bits(f([0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF])).tolist() == [0x3F81, 0x3F80, 0x3F82, 0x3F81]
    assert R.bf16_bits(f([0x3FFF8000, 0x7EFF8000])).tolist() == [0x4000, 0x7F00]      # the carry runs into the exponent
    assert R.bf16_bits(np.array([0.0, -0.0, 1.0], np.float32)).tolist() == [0, 0x8000, 0x3F80]


def test_job_semantics():
    src = np.arange(100, 100 + 6 * 75, dtype=np.float32)
    # the stem form: k = 3*tap + colour of a [N][3][25] weight
    c = R.Case("stem", R.PACK_F32, "w", K=75, N=6, kdiv=3, s_kq=1, s_kr=25, s_nq=75)
    v = R.gather(c, src)
    w = src.reshape(6, 3, 25)
    for k in (0, 1, 2, 3, 40, 74):
        assert np.array_equal(v[0, k], w[:, k % 3, k // 3])
    # the head form: n = 3*tap + colour
    c = R.Case("head", R.PACK_F32, "w", K=6, N=75, s_kq=75, ndiv=3, s_nq=1, s_nr=25)
    v = R.gather(c, src)
    for n in (0, 1, 2, 3, 40, 74):
        assert np.array_equal(v[0, :, n], w[:, n % 3, n // 3])
    # an element offset, and taps
    c = R.Case("conv", R.PACK_F32, "w", off=3, taps=5, K=3, N=4, s_tap=1, s_kq=5, s_nq=15)
    assert R.gather(c, src)[2, 1, 3] == src[3 + 2 + 5 + 45]
    # value = src * mask keeps the sign of a masked negative
    m = R.masked(np.array([-2.0, 3.0, -4.0], np.float32), np.array([0.0, 0.0, 1.0], np.float32))
    assert R.f32_bits(m).tolist() == [0x80000000, 0, 0xC0800000]


def test_reparam_candidates():
    v = np.array([0.5, 0.1, -3.0, 0.3, 1.0 + 2.0 ** -23, 0.7], np.float32)
    fused, unfused = R.reparam_candidates(v, 0.3, 0.1)
    b = np.float32(0.3)
    assert fused[1] == fused[2] == fused[3] and unfused[1] == unfused[3]        # at or below the bound: the bound's value
    assert fused[0] == np.float32(0.25 - np.float64(np.float32(0.1)))
    x = np.float64(np.float32(1.0 + 2.0 ** -23))
    assert unfused[4] == np.float32(np.float64(np.float32(x * x)) - np.float64(np.float32(0.1)))
    assert abs(float(fused[3]) - (float(b) ** 2 - float(np.float32(0.1)))) <= 2.0 ** -24 * 0.1
    many = np.random.default_rng(0).standard_normal(20000).astype(np.float32)
    f, u = R.reparam_candidates(many, 0.3, 0.1)
    assert (f != u).any(), "the two forms must differ somewhere, or the test of them says nothing"
    assert np.abs(f.astype(np.float64) - u).max() <= 2.0 ** -23 * np.abs(many).max() ** 2
    f, u = R.reparam_candidates(np.array([2.0 ** -18, 0.0], np.float32), 2.0 ** -18, 2.0 ** -36)
    assert not f.any() and not u.any()                                          # on the bound: exactly zero


# ---------------------------------------------------------------------------------------------
# the planner and the case table
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    cases, sources = R.build_table()
    at, _ = R.source_layout(sources)
    dat, _ = R.dest_layout(cases)
    SRC, DST = 0x7F0000000000, 0x7E0000000000      # never dereferenced: the planner reads only their alignment
    arr = (_lib.PrepJob * len(cases))()
    for j, c, d in zip(arr, cases, dat):
        R.fill_job(j, c, SRC, at, DST + d)
    total = lib.lic_prep_plan(arr, len(cases))
    return _lib, lib, cases, arr, total


def test_table_plans_and_block0_is_the_running_sum(planned):
    _lib, lib, cases, arr, total = planned
    assert total > 0 and len(cases) >= 100
    run = 0
    for j, c in zip(arr, cases):
        assert j.block0 == run, c.name
        assert j.nblocks >= 1
        run += j.nblocks
        if c.kind in (R.MAP, R.MASK_INPLACE):
            assert j.total == c.N and j.nblocks == -(-c.N // R.MAP_BLOCK), c.name
        else:
            K = 80 if c.kind == R.PACK_BF16_STEM else c.K
            bk = 32 if c.half else 16
            npad = R.npad_bf16(c.N) if c.half else R.npad_f32(c.N)
            assert (j.cpt, j.npad) == (-(-K // bk), npad), c.name
            assert j.total * (2 if c.half else 4) == c.dst_bytes(), c.name
            assert j.nblocks == (j.cpt * npad // 8 if j.tiled else -(-j.total // R.MAP_BLOCK)), c.name
    assert run == total
    sizes = {j.nblocks for j in arr}
    assert 1 in sizes and max(sizes) >= 100 and len(sizes) >= 12, "mixed block counts for the block-to-job search"


def test_planner_gives_the_recorded_paths(planned):
    _lib, lib, cases, arr, total = planned
    seen = 0
    for j, c in zip(arr, cases):
        if c.expect is not None:
            assert (j.tiled, j.v4) == c.expect, (c.name, j.tiled, j.v4)
            seen += 1
    assert seen >= 2 * (2 * len(R.CONV_ROWS) + 1) + 2 * 4
    by = {c.name: j for j, c in zip(arr, cases)}
    assert by["conv24x32x3x3.f32.fwd"].npad == 32 and by["conv33x20x3x3.f32.fwd"].npad == 64
    assert by["conv8x8x4x7.f32.fwd"].taps == 28 and by["conv8x8x5x6.f32.fwd"].taps == 30


def _v4_blockers(j, c):
    """which of the four conditions of the 16-byte branch a tiled job misses"""
    bk = 32 if c.half else 16
    pitch = j.s_nq if j.tiled == 1 else j.s_kq
    return {name for name, bad in (("shape", c.K % bk != 0 or c.N % 8 != 0), ("align", j.src % 16 != 0),
                                   ("pitch", pitch % 4 != 0)) if bad}


def test_table_reaches_every_branch(planned):
    """a condition on the table: a case list that stops covering a branch of the packers fails here"""
    _lib, lib, cases, arr, total = planned
    for kind in (R.PACK_F32, R.PACK_BF16):
        paths = {(j.tiled, j.v4) for j, c in zip(arr, cases) if c.kind == kind}
        assert paths == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)}, (kind, paths)     # (v4 exists only when tiled)
        tiled = [(j, c) for j, c in zip(arr, cases) if c.kind == kind and j.tiled]
        for t in (1, 2):
            assert any(j.v4 and j.tiled == t and j.npad > c.N for j, c in tiled), "whole-block zero fill (v4, npad > N)"
            # the scalar branch's guards: ragged K, ragged N, and blocks wholly past N
            sc = [(j, c) for j, c in tiled if not j.v4 and j.tiled == t]
            bk = 32 if kind == R.PACK_BF16 else 16
            assert any(c.K % bk and c.K > bk for j, c in sc) and any(c.N % 8 for j, c in sc)
            assert any(j.npad - c.N >= 8 for j, c in sc)
        assert any(not j.v4 and _v4_blockers(j, c) == {"align"} for j, c in tiled), "v4 lost only to a source 4 bytes off"
        assert any(not j.v4 and _v4_blockers(j, c) == {"pitch"} for j, c in tiled), "v4 lost only to the pitch"
        for j, c in tiled:
            assert bool(j.v4) == (not _v4_blockers(j, c)), c.name
        assert any(c.taps == 28 for j, c in tiled)
        assert any(c.N in range(33, 64) for j, c in tiled)
    kinds = {c.kind for c in cases}
    assert kinds == set(range(6))
    assert any(c.kdiv for c in cases) and any(c.ndiv for c in cases)
    assert any(c.mask and c.transform and (c.kdiv or c.ndiv) for c in cases)
    assert any(c.s_tap not in (0, 1) for c in cases)
    assert {c.N for c in cases if c.kind == R.MASK_INPLACE} >= set(R.EDGE_N)
    assert {c.N for c in cases if c.kind == R.MAP} >= set(R.EDGE_N)
    for kind in (R.PACK_F32, R.PACK_BF16, R.PACK_BF16_KPERM):
        for C_ in R.GAMMA_C:
            got = {(c.s_kq, c.s_nq) for c in cases if c.kind == kind and c.transform and c.K == c.N == C_}
            assert got == {(1, C_), (C_, 1)}
    # a masked pack job in the same launch as the MASK_INPLACE job of its tensor, before and after it
    i = next(k for k, c in enumerate(cases) if c.name == "ctx.mask_inplace")
    same = [k for k, c in enumerate(cases) if c.src == cases[i].src and c.mask == cases[i].mask and k != i]
    assert min(same) < i < max(same)


def test_planner_rejects_what_it_cannot_run(planned):
    _lib, lib, cases, arr, total = planned
    one = (_lib.PrepJob * 1)()
    assert lib.lic_prep_plan(None, 1) == -1 and lib.lic_prep_plan(one, 0) == -1
    R.fill_job(one[0], cases[0], 0x1000, {cases[0].src: 0}, 0x2000)
    assert lib.lic_prep_plan(one, 1) == arr[0].nblocks
    one[0].dst = 0x2004                                   # packed destinations are written 16 bytes at a time
    assert lib.lic_prep_plan(one, 1) == -1
    one[0].dst, one[0].src = 0x2000, None
    assert lib.lic_prep_plan(one, 1) == -1
    one[0].src, one[0].kind = 0x1000, 9
    assert lib.lic_prep_plan(one, 1) < 0
