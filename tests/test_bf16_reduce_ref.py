"""tests/bf16_reduce_ref.py against torch on the CPU and against the library's host planner, and the coverage
conditions on the case lists of tests/test_gpu_bf16_reductions.py: what the GPU file is said to cover (every row of
the wgrad_bf16_kernel table, unsplit launches of 1 .. 7 chunks, short last splits of every length mod 3, integer
data that stays exact) is asserted here, so the GPU test cannot quietly cover less.  CPU only: the planning entry
points never dereference operand pointers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_reduce_ref as ref

_STANDIN = C.create_string_buffer(256)
ALIGNED = (C.addressof(_STANDIN) + 15) & ~15


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _desc(L, case):
    d = ref.fill_desc(L.WgradDesc(), ref.wgrad_fields(case))
    d.p = d.g = d.dst = ALIGNED
    return d


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ---- the reference against torch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,pad,H,W", [(5, 2, 2, 8, 12), (5, 2, 2, 7, 11), (3, 1, 1, 6, 5), (1, 2, 0, 6, 4),
                                              (1, 1, 0, 3, 5)])
@pytest.mark.parametrize("g_is_row", [0, 1])
def test_wgrad_ref_is_the_weight_gradient_of_conv2d(k, stride, pad, H, W, g_is_row):
    """conv2d: P = the output gradient (small grid), G = the input (large grid).  g_is_row = 0 gives dw as
    [Cout][Cin][kh][kw] through (sm, sn, stap) = (Cin k^2, k^2, 1), g_is_row = 1 its transpose."""
    gen = torch.Generator().manual_seed(k * 100 + H)
    B, Cin, Cout = 2, 5, 7
    x = torch.randn(B, Cin, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, k, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (dw,) = torch.autograd.grad(y, w, dy)
    d = ref.SimpleNamespace(B=B, Hs=y.shape[2], Ws=y.shape[3], Cp=Cout, Hl=H, Wl=W, Cg=Cin, kh=k, kw=k, stride=stride,
                            pad=pad, g_is_row=g_is_row, sq_g=0, scale=-0.5)
    R = ref.wgrad_ref(_nhwc(dy), _nhwc(x), d)
    want = -0.5 * dw.numpy().reshape(Cout, Cin, k * k)
    want = want.transpose(2, 1, 0) if g_is_row else want.transpose(2, 0, 1)
    np.testing.assert_allclose(R, want, rtol=1e-12, atol=1e-12)
    # ... and the scatter: offsets of the [Cout][Cin][kh][kw] weight
    Cm, Cn = (Cin, Cout) if g_is_row else (Cout, Cin)
    sm, sn = (k * k, Cin * k * k) if g_is_row else (Cin * k * k, k * k)
    dst = np.zeros(Cout * Cin * k * k)
    dst[ref.scatter_offsets(k * k, Cm, Cn, sm, sn, 1).reshape(-1)] = R.reshape(-1)
    np.testing.assert_allclose(dst.reshape(Cout, Cin, k, k), -0.5 * dw.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k,stride,pad,op,H,W", [(5, 2, 2, 1, 4, 6), (5, 2, 2, 0, 4, 6), (3, 1, 1, 0, 5, 4)])
def test_wgrad_ref_is_the_weight_gradient_of_conv_transpose2d(k, stride, pad, op, H, W):
    """conv_transpose2d: the roles swap -- P = the input (small grid), G = the output gradient (large grid, 2 H or
    2 H - 1 rows); dw is [Cin][Cout][kh][kw]"""
    gen = torch.Generator().manual_seed(k * 10 + op)
    B, Cin, Cout = 2, 6, 4
    x = torch.randn(B, Cin, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Cin, Cout, k, k, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, stride=stride, padding=pad, output_padding=op)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (dw,) = torch.autograd.grad(y, w, dy)
    d = ref.SimpleNamespace(B=B, Hs=H, Ws=W, Cp=Cin, Hl=y.shape[2], Wl=y.shape[3], Cg=Cout, kh=k, kw=k, stride=stride,
                            pad=pad, g_is_row=0, sq_g=0, scale=1.0)
    R = ref.wgrad_ref(_nhwc(x), _nhwc(dy), d)
    np.testing.assert_allclose(R, dw.numpy().reshape(Cin, Cout, k * k).transpose(2, 0, 1), rtol=1e-12, atol=1e-12)


def test_wgrad_ref_squared_column_operand():
    gen = torch.Generator().manual_seed(3)
    t = torch.randn(2, 3, 5, 8, generator=gen, dtype=torch.float64)
    x = torch.randn(2, 3, 5, 8, generator=gen, dtype=torch.float64)
    d = ref.SimpleNamespace(B=2, Hs=3, Ws=5, Cp=8, Hl=3, Wl=5, Cg=8, kh=1, kw=1, stride=1, pad=0, g_is_row=0, sq_g=1,
                            scale=2.0)
    want = 2.0 * torch.einsum("bhwm,bhwn->mn", t, x * x).numpy()
    np.testing.assert_allclose(ref.wgrad_ref(t.numpy(), x.numpy(), d)[0], want, rtol=1e-12, atol=1e-12)
    wabs = 2.0 * torch.einsum("bhwm,bhwn->mn", t.abs(), x * x).numpy()
    np.testing.assert_allclose(ref.wgrad_ref(t.numpy(), x.numpy(), d, absolute=True)[0], wabs, rtol=1e-12, atol=1e-12)


def test_bf16_round_is_torch_bfloat16():
    a = torch.randn(100_000, generator=torch.Generator().manual_seed(1)) * 37.0
    a[:4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])      # ties: to even, both ways
    assert np.array_equal(ref.bf16_round(a.numpy()), a.to(torch.bfloat16).float().numpy())


# ---- the planner restatement against the library -------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(lib):
    """{case name: (plan_ref detail, library workspace bytes, library kernel name)}"""
    L, h = lib, lib.load()
    buf = C.create_string_buffer(96)
    out = {}
    for c in ref.WGRAD_CASES:
        d = _desc(L, c)
        assert h.lic_wgrad_bf16_kernel_name(C.byref(d), buf, 96) == 0, c.name
        out[c.name] = (ref.plan_ref(ref.wgrad_fields(c), detail=True), h.lic_wgrad_bf16_workspace_bytes(C.byref(d)),
                       buf.value.decode())
    return out


def test_plan_ref_is_the_library_planner(plans):
    assert len({c.name for c in ref.WGRAD_CASES}) == len(ref.WGRAD_CASES)
    for c in ref.WGRAD_CASES:
        pl, ws, name = plans[c.name]
        Cm, Cn = (c.Cg, c.Cp) if c.g_is_row else (c.Cp, c.Cg)
        assert ws == pl.splitk * c.kh * c.kw * Cm * Cn * 4, (c.name, ws, vars(pl))
        assert name == ref.kernel_name_ref(ref.wgrad_fields(c)), (c.name, name)
        assert sum(pl.nloc) == pl.nchunks and min(pl.nloc) >= 1, (c.name, pl.nloc)


def test_the_planner_ignores_the_force_fields(lib):
    """lic_wgrad_bf16 plans from the shape alone (include/lic.h): force_tm / force_tn / force_split change nothing"""
    L, h = lib, lib.load()
    buf = C.create_string_buffer(96)
    for c in ref.WGRAD_CASES[::7]:
        d = _desc(L, c)
        ws = h.lic_wgrad_bf16_workspace_bytes(C.byref(d))
        assert h.lic_wgrad_bf16_kernel_name(C.byref(d), buf, 96) == 0
        name = buf.value
        d.force_tm, d.force_tn, d.force_split = 1, 3, 5
        assert h.lic_wgrad_bf16_workspace_bytes(C.byref(d)) == ws
        assert h.lic_wgrad_bf16_kernel_name(C.byref(d), buf, 96) == 0 and buf.value == name


# ---- coverage conditions on the case list -------------------------------------------------------------------------
def test_cases_reach_every_row_of_the_kernel_table(plans):
    rows = {"wgrad_bf16_kernel<1, 1, false>", "wgrad_bf16_kernel<1, 2, false>", "wgrad_bf16_kernel<1, 3, false>",
            "wgrad_bf16_kernel<2, 1, false>", "wgrad_bf16_kernel<2, 2, false>", "wgrad_bf16_kernel<2, 3, false>",
            "wgrad_bf16_kernel<3, 1, false>", "wgrad_bf16_kernel<3, 2, false>", "wgrad_bf16_kernel<3, 3, false>",
            "wgrad_bf16_kernel<1, 1, true>", "wgrad_bf16_kernel<2, 2, true>", "wgrad_bf16_kernel<3, 3, true>"}
    assert set(ref.TABLE_ROWS) == rows
    for data in ("int", "real"):
        got = {plans[c.name][2] for c in ref.WGRAD_CASES if c.data == data}
        assert got == rows, (data, sorted(rows ^ got))


def test_cases_cover_every_ring_tail_and_last_split(plans):
    ints = [c for c in ref.WGRAD_CASES if c.data == "int"]
    unsplit = {plans[c.name][0].nloc[0] for c in ints if plans[c.name][0].splitk == 1}
    assert set(range(1, 8)) <= unsplit, sorted(unsplit)
    split = [plans[c.name][0] for c in ints if plans[c.name][0].splitk > 1]
    short = [pl for pl in split if pl.nloc[-1] < pl.cps]
    assert {pl.nloc[-1] % 3 for pl in short} == {0, 1, 2}, sorted(pl.nloc for pl in short)
    assert {pl.cps % 3 for pl in split} == {0, 1, 2}
    assert any(pl.splitk >= 3 for pl in split)
    # the issue's reading of the planner, now the restatement's (and through test_plan_ref_*, the library's)
    by_name = {c.name: plans[c.name][0] for c in ints}
    assert by_name["split-1x2x260-k5s1-64x64-weight-int"].nloc == [9, 8]
    assert by_name["split-1x2x545-k5s1-64x64-weight-int"].nloc == [12, 12, 11]
    # one launch whose split count comes from the machine's rounds, not from the 16-chunk clip
    eff = [pl for pl in split if pl.picked < pl.max_sk]
    assert eff and any(pl.base == 100 for pl in eff), [(pl.picked, pl.max_sk) for pl in split]
    assert any(c.kh == 1 and plans[c.name][0].splitk > 1 for c in ints)      # a split 1x1 product as well
    # ragged last chunk and a full one
    Ps = {c.B * c.Hs * c.Ws % 32 for c in ints}
    assert 0 in Ps and 1 in Ps and 31 in Ps


def test_cases_cover_tails_gather_and_layout():
    cs = ref.WGRAD_CASES
    pairs = {(c.Cp, c.Cg) for c in cs}
    assert {(8, 192), (72, 136), (200, 64), (320, 72), (136, 200)} <= pairs
    assert {(c.Cp, c.sq_g) for c in cs if c.sq_g} >= {(64, 1), (128, 1), (192, 1), (72, 1), (136, 1)}
    assert all(c.Cp == c.Cg and not c.g_is_row for c in cs if c.sq_g)
    gathered = [c for c in cs if not (c.kh == 1 and c.stride == 1 and c.Hl == c.Hs)]
    assert {(c.kh, c.stride, c.pad) for c in gathered} >= {(5, 2, 2), (3, 1, 1), (1, 2, 0)}
    assert any(c.kh == 5 and c.Hl == 2 * c.Hs for c in gathered) and any(c.kh == 5 and c.Hl == 2 * c.Hs - 1 for c in gathered)
    borders = [c for c in gathered if c.name.startswith("gather")]
    for geo in {(c.kh, c.stride, c.Hl - 2 * c.Hs) for c in borders}:     # each geometry in either role
        assert {c.g_is_row for c in borders if (c.kh, c.stride, c.Hl - 2 * c.Hs) == geo} == {0, 1}, geo
    assert len({(c.kh, c.stride, c.Hl - 2 * c.Hs) for c in borders}) >= 4
    assert {(c.B, c.Hs, c.Ws) for c in gathered} >= {(5, 1, 1), (1, 7, 1), (3, 5, 7)}
    assert {c.layout for c in cs} == {"weight", "transpose", "gaps"}
    assert any(c.p_pad == 8 and c.g_pad == 16 and c.offset for c in cs) and any(not c.p_pad and not c.offset for c in cs)
    assert {c.scale for c in cs} == set(ref.SCALES)
    for c in cs:       # layouts scatter without collisions, inside dst
        sm, sn, stap, n = ref.wgrad_layout(c)
        Cm, Cn = (c.Cg, c.Cp) if c.g_is_row else (c.Cp, c.Cg)
        off = ref.scatter_offsets(c.kh * c.kw, Cm, Cn, sm, sn, stap).reshape(-1)
        assert off.min() == 0 and off.max() < n and len(np.unique(off)) == off.size, c.name


def test_integer_cases_stay_exact():
    """every partial sum of an integer case is an integer (or, scaled, a multiple of 1/2) below 2^24"""
    for c in ref.WGRAD_CASES:
        if c.data == "int":
            assert ref.integer_bound(c) < ref.INT_LIMIT, c.name
            P, G = ref.wgrad_inputs(c)
            assert np.abs(P).max() <= 3 and np.abs(G).max() <= 3 and np.array_equal(P, np.rint(P))
    for P, Cc, pad in ref.COLSUM_CASES:
        assert P * 3 * 2 < ref.INT_LIMIT
    for j in ref.REDUCE_CASES:
        if j.data == "int":
            assert j.splitk * 3 * 2 < ref.INT_LIMIT


def test_colsum_and_reduce_cases_cover_what_they_claim():
    assert {P for P, _, _ in ref.COLSUM_CASES} == set(ref.COLSUM_P) == {1, 31, 32, 33, 255, 256, 257, 8191, 65536, 65537, 70001}
    assert {Cc for _, Cc, _ in ref.COLSUM_CASES} == {8, 64, 72, 640}
    assert {pad for _, _, pad in ref.COLSUM_CASES} == {0, 8} and (70001, 640, 8) in ref.COLSUM_CASES
    slabs = [j for j in ref.REDUCE_CASES if j.kind == ref.SLABS]
    cols = [j for j in ref.REDUCE_CASES if j.kind == ref.COLUMNS]
    for data in ("int", "real"):
        assert {j.splitk for j in slabs if j.data == data} >= {1, 7, 8, 9, 15, 31, 32, 33, 40, 47, 71}
        assert {j.splitk for j in cols if j.data == data} >= {1, 15, 16, 17, 113, 128, 129, 300}
    assert any(j.Cn % 16 for j in cols) and all((j.ntaps * j.Cm * j.Cn) % 256 for j in slabs if j.name.startswith("slabs"))
    assert any(j.ntaps * j.Cm * j.Cn > 256 for j in slabs)
    assert any(0 < j.Mvalid < j.Cm and 0 < j.Nvalid < j.Cn for j in slabs)
    assert any(j.mdiv for j in slabs) and any(j.ndiv for j in slabs)
    assert {j.kind for j in ref.REDUCE_CASES if j.epilogue == ref.EPI_REPARAM} == {ref.SLABS, ref.COLUMNS}
    batch = ref.batch33()
    depth = [j.splitk * (2 if j.kind == ref.COLUMNS else 1) for j in batch[:ref.MAX_JOBS]]
    assert len(batch) == ref.MAX_JOBS + 1 and {j.kind for j in batch} == {ref.SLABS, ref.COLUMNS}
    assert depth != sorted(depth, reverse=True) and max(depth) >= 100 * min(depth)
    for j in ref.REDUCE_CASES:       # destinations do not collide and stay inside the extent
        src, param = ref.reduce_inputs(j)
        off, _ = ref.reduce_ref(j, src, param)
        assert off.min() >= 0 and off.max() < j.extent and len(np.unique(off)) == off.size, j.name


# ---- restatement properties ---------------------------------------------------------------------------------------
def test_rgb_maps_are_the_weight_layouts():
    """the stem map sends row tap * 3 + c, column co to dw[co][c][tap]; the head map column tap * 3 + c, row ci to
    dw[ci][c][tap] ([.][3][5][5] weights)"""
    by = {j.name: j for j in ref.REDUCE_CASES}
    j = by["stem-map"]
    src = np.zeros((1, 80, 64), np.float32)
    src[0, 7 * 3 + 2, 11] = 5.0
    off, v = ref.reduce_slabs_ref(SimpleNamespaceWith(j, splitk=1), src)
    dw = np.zeros(64 * 75, np.float32)
    dw[off] = v
    assert dw.reshape(64, 3, 25)[11, 2, 7] == 5.0 and np.count_nonzero(dw) == 1 and off.size == 75 * 64
    j = by["head-map"]
    src = np.zeros((1, 64, 80), np.float32)
    src[0, 13, 24 * 3 + 1] = 5.0
    off, v = ref.reduce_slabs_ref(SimpleNamespaceWith(j, splitk=1), src)
    dw = np.zeros(64 * 75, np.float32)
    dw[off] = v
    assert dw.reshape(64, 3, 25)[13, 1, 24] == 5.0 and np.count_nonzero(dw) == 1 and off.size == 75 * 64


def SimpleNamespaceWith(j, **kw):
    d = dict(vars(j))
    d.update(kw)
    return ref.SimpleNamespace(**d)


def test_reductions_of_integers_are_the_plain_sum():
    for j in ref.REDUCE_CASES:
        if j.data != "int" or j.epilogue != ref.EPI_NONE:
            continue
        src, _ = ref.reduce_inputs(j)
        off, v = ref.reduce_ref(j, src)
        total = src.astype(np.float64).sum(0) * j.scale
        if j.kind == ref.SLABS:
            Mv, Nv = j.Mvalid or j.Cm, j.Nvalid or j.Cn
            total = total.reshape(j.ntaps, j.Cm, j.Cn)[:, :Mv, :Nv].reshape(-1)
        assert np.array_equal(v.astype(np.float64), total), j.name


def test_reductions_of_reals_are_within_the_summation_bound():
    """a sanity check of the restatement, not of the kernel: |ref - sum| <= splitk 2^-24 sum |.| (|scale| inside)"""
    for j in ref.REDUCE_CASES:
        if j.data != "real" or j.epilogue != ref.EPI_NONE:
            continue
        src, _ = ref.reduce_inputs(j)
        off, v = ref.reduce_ref(j, src)
        s64 = src.astype(np.float64)
        total, weight = s64.sum(0) * j.scale, np.abs(s64).sum(0) * abs(j.scale)
        if j.kind == ref.SLABS:
            Mv, Nv = j.Mvalid or j.Cm, j.Nvalid or j.Cn
            total, weight = (a.reshape(j.ntaps, j.Cm, j.Cn)[:, :Mv, :Nv].reshape(-1) for a in (total, weight))
        assert (np.abs(v - total) <= j.splitk * 2.0 ** -24 * weight).all(), j.name


def test_the_slab_order_is_a_statement():
    """on real data the documented order and a plain left-to-right fp32 sum give different bits somewhere: a kernel
    held to reduce_slabs_ref bit for bit is held to the order"""
    j = next(j for j in ref.REDUCE_CASES if j.name == "slabs47-real")
    src, _ = ref.reduce_inputs(j)
    _, v = ref.reduce_slabs_ref(ref.SimpleNamespace(**{**vars(j), "scale": 1.0}), src)
    naive = np.zeros(src.shape[1], np.float32)
    for z in range(j.splitk):
        naive = naive + src[z]
    assert not np.array_equal(naive, v)


def test_reparam_rule():
    """g = v * 2 * max(p, bound), kept when p >= bound or g < 0 -- below, on and above the bound, both signs"""
    j = ref.SimpleNamespace(kind=ref.COLUMNS, splitk=1, Cn=6, scale=1.0, epilogue=ref.EPI_REPARAM, bound=0.25)
    parts = np.array([[1.0, 1.0, 1.0, -1.0, -1.0, -1.0]], np.float32)
    param = np.array([0.125, 0.25, 0.75, 0.125, 0.25, 0.75], np.float32)
    _, v = ref.reduce_columns_ref(j, parts, param)
    assert v.tolist() == [0.0, 0.5, 1.5, -0.5, -0.5, -1.5]
    j = ref.SimpleNamespace(kind=ref.SLABS, splitk=1, ntaps=1, Cm=2, Cn=3, Mvalid=0, Nvalid=0, mdiv=0, ndiv=0, sm=3, smr=0,
                            sn=1, snr=0, stap=0, scale=1.0, epilogue=ref.EPI_REPARAM, bound=0.25)
    off, v = ref.reduce_slabs_ref(j, parts, param)
    assert off.tolist() == list(range(6)) and v.tolist() == [0.0, 0.5, 1.5, -0.5, -0.5, -1.5]
