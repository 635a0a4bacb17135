"""tests/conv_image_bf16_ref.py (the float64 statement, case tables, mutants, exact cases and bands of
test_gpu_image_bf16.py) against the CPU oracle and itself.  CPU only.

  * the reference equals oracle.conv2d_fwd / conv2d_bwd / convT2d_fwd / convT2d_bwd at 1e-12 relative.  The oracle
    returns fp32, so the pin uses integer-valued operands: every sum is exact in fp32 and in float64 and the two must
    agree to the last bit (1e-12 then holds with room; on random operands an fp32 result could not meet it);
  * the operand rounding is rne_bf16 of the image / the image gradient / the weights, and it matters: the reference on
    unrounded operands misses the band;
  * A meets its two non-measured conditions for every case, forward and data gradient;
  * the coverage properties the case tables claim, computed from the kernels' tile constants;
  * the six mutants miss their bands by more than 8x; the unmutated reference holds them;
  * the exact cases are exact (integer sums below 2^24; bf16-exact stem outputs) and the stem's tells round-to-nearest-even
    from truncation, from round-half-up and from no rounding of the image."""
import numpy as np
import pytest
import torch

import conv_image_bf16_ref as R
from oracle import oracle as O


def rel(a, b):
    a, b = R.f64(a), R.f64(b)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def _ints(key, cin, cout, B, H, W, tr):
    r = R._rng(key)
    x = r.randint(-3, 4, size=(B, cin, H, W)).astype(np.float32)
    w = r.randint(-2, 3, size=(cin, cout, 5, 5) if tr else (cout, cin, 5, 5)).astype(np.float32)
    b = r.randint(-4, 5, size=(cout,)).astype(np.float32)
    return x, w, b, r


# ---------------------------------------------------------------------------------------------
# against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cin,cout,B,H,W", [("stem", 3, 8, 2, 7, 6), ("stem", 3, 4, 1, 1, 1), ("halo", 8, 6, 2, 5, 9)])
def test_strided_vs_oracle(fam, cin, cout, B, H, W):
    x, w, b, r = _ints(f"o-{fam}-{H}-{W}", cin, cout, B, H, W, False)
    ref = R.layer_ref(fam, x, w, b)          # (integers are bf16-exact: the rounding is the identity here)
    assert tuple(ref.y.shape[2:]) == R.out_hw(fam, H, W)
    assert rel(ref.y, O.conv2d_fwd(x, w, b, 2, 2)) <= 1e-12
    g = r.randint(-3, 4, size=tuple(ref.y.shape)).astype(np.float32)
    gr = R.conv_grads(x, w, b, g, 5, 2, 2)
    dx, dw, db = O.conv2d_bwd(x, w, g, 2, 2)
    assert rel(gr.dx, dx) <= 1e-12 and rel(gr.dw, dw) <= 1e-12 and rel(gr.db, db) <= 1e-12
    assert ref.n == 25 * cin and gr.n_dx == 9 * cout


@pytest.mark.parametrize("fam,cin,cout,B,H,W", [("head", 8, 3, 2, 5, 7), ("head", 4, 3, 3, 1, 1), ("halot", 6, 8, 1, 4, 3)])
def test_transposed_vs_oracle(fam, cin, cout, B, H, W):
    x, w, b, r = _ints(f"o-{fam}-{H}-{W}", cin, cout, B, H, W, True)
    ref = R.layer_ref(fam, x, w, b)
    assert tuple(ref.y.shape[2:]) == (2 * H, 2 * W) == R.out_hw(fam, H, W)
    assert rel(ref.y, O.convT2d_fwd(x, w, b, 2, 2, 1)) <= 1e-12
    g = r.randint(-3, 4, size=tuple(ref.y.shape)).astype(np.float32)
    gr = R.conv_grads(x, w, b, g, 5, 2, 2, True, 1)
    dx, dw, db = O.convT2d_bwd(x, w, g, 2, 2, 1)
    assert rel(gr.dx, dx) <= 1e-12 and rel(gr.dw, dw) <= 1e-12 and rel(gr.db, db) <= 1e-12
    assert ref.n == 9 * cin and gr.n_dx == 25 * cout
    # the head's data gradient IS the stem's convolution of the image gradient with the same [C][3][5][5] tensor
    # (what lic_stem_conv_bf16 computes)
    if fam == "head":
        assert torch.equal(gr.dx, R.conv_ref(g, w, None, 5, 2, 2).y)


def test_operand_rounding_is_stated_and_matters():
    case = ("stem", 64, (3, 21, 19))
    i = R.inputs(case)
    ref = R.forward_ref(case)
    by_hand = R.conv_ref(R.rne_bf16(i["x"]), R.rne_bf16(i["w"]), i["b"], 5, 2, 2)
    assert torch.equal(ref.y, by_hand.y) and torch.equal(ref.S, by_hand.S)
    for what, xq, wq in (("image not rounded", i["x"], R.rne_bf16(i["w"])), ("weight not rounded", R.rne_bf16(i["x"]), i["w"]),
                         ("image truncated", R.trunc_bf16(i["x"]), R.rne_bf16(i["w"]))):
        wrong = R.rne_bf16(R.conv_ref(xq, wq, i["b"], 5, 2, 2).y)
        assert R.half_ulp_ratio(wrong, ref.y, ref.S) > 8.0, what
    assert R.half_ulp_ratio(R.rne_bf16(ref.y), ref.y, ref.S) <= 1.0
    # the head's image gradient
    case = ("head", 64, (2, 5, 33))
    i, gr = R.inputs(case), R.grads_ref(case)
    by_hand = R.conv_ref(R.rne_bf16(i["g"]), R.rne_bf16(i["w"]), None, 5, 2, 2)
    assert torch.equal(gr.dx, by_hand.y) and torch.allclose(gr.S_dx, by_hand.S, rtol=1e-14, atol=0)
    wrong = R.rne_bf16(R.conv_ref(R.trunc_bf16(i["g"]), R.rne_bf16(i["w"]), None, 5, 2, 2).y)
    assert R.half_ulp_ratio(wrong, gr.dx, gr.S_dx) > 8.0


# ---------------------------------------------------------------------------------------------
# the band constants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_A_meets_its_conditions(case):
    fam, C, _ = case
    n, n_dx = R.products(case), R.products(case, dgrad=True)
    assert n == {"stem": 75, "head": 9 * C, "halo": 25 * C, "halot": 9 * C}[fam]
    assert R.check_A(R.A[fam], n), (case, n)
    if fam != "stem":        # (the stem has no data gradient)
        dfam = {"head": "stem", "halo": "halot", "halot": "halo"}[fam]     # the kernel the data gradient runs
        assert n_dx == {"head": 75, "halo": 9 * 128, "halot": 25 * 128}[fam]
        assert R.check_A(R.A[dfam], n_dx), (case, n_dx)
    if fam in ("stem", "head"):
        assert R.A32 <= n * 2.0 ** -23 and R.A32 <= (75 if fam == "head" else n) * 2.0 ** -23
    for f, m in R.A_MEASURED.items():
        a = R.A32 if f == "rgb32" else R.A[f]
        assert 4.0 * m <= a, (f, m, a)       # the rule the constant is chosen by


def test_products_are_the_references_own_count():
    for case in (("stem", 64, (1, 5, 6)), ("head", 64, (2, 5, 33)), ("halo", 64, (2, 17, 65)), ("halot", 64, (1, 9, 33))):
        assert R.forward_ref(case).n == R.products(case), case
        if case[0] != "stem":
            assert R.grads_ref(case).n_dx == R.products(case, dgrad=True), case


# ---------------------------------------------------------------------------------------------
# coverage of the case tables
# ---------------------------------------------------------------------------------------------
def test_case_tables_cover_what_they_claim():
    # head: 4 x 32 feature tiles
    assert any(Wi % R.HD_TW == 1 for _, _, Wi in R.HEAD_SHAPES) and any(Hi % R.HD_TH == 1 for _, Hi, _ in R.HEAD_SHAPES)
    assert any((Hi, Wi) == (R.HD_TH, R.HD_TW) for _, Hi, Wi in R.HEAD_SHAPES)              # exactly one tile per image
    assert any(Wi > 2 * R.HD_TW for _, _, Wi in R.HEAD_SHAPES)                             # three x tiles
    assert any(Wi % R.HD_TW == R.HD_TW - 1 for _, _, Wi in R.HEAD_SHAPES)                  # one short of a tile
    assert max(R.head_tiles(*s) for s in R.HEAD_SHAPES) <= 12
    # halo kernels: 8 x 32 tiles of the output (strided) / of the input (transposed)
    assert any(R.halo_tiles(1, H, W) == 1 and R.out_hw("halo", H, W) == (R.HALO_TH, R.HALO_TW) for _, H, W in R.HALO_SHAPES)
    assert any(R.out_hw("halo", H, W) == (R.HALO_TH + 1, R.HALO_TW + 1) for _, H, W in R.HALO_SHAPES)
    assert any(H % 2 and W % 2 for _, H, W in R.HALO_SHAPES) and any(not H % 2 and not W % 2 for _, H, W in R.HALO_SHAPES)
    assert any(R.halot_tiles(1, H, W) == 1 and (H, W) == (R.HALOT_TH, R.HALOT_TW) for _, H, W in R.HALOT_SHAPES)
    assert any((H, W) == (R.HALOT_TH + 1, R.HALOT_TW + 1) for _, H, W in R.HALOT_SHAPES)
    # the strided layer's data gradient reaches the transposed kernel for even inputs only: one aligned and two ragged shapes
    even = [s for s in R.HALO_SHAPES + R.HALO_DGRAD_SHAPES if not s[1] % 2 and not s[2] % 2]
    q = [(H // 2, W // 2) for _, H, W in even]           # the phase grid the transposed kernel tiles
    assert (R.HALOT_TH, R.HALOT_TW) in q and (R.HALOT_TH + 1, R.HALOT_TW + 1) in q
    assert any(h % R.HALOT_TH and w % R.HALOT_TW and h > 2 * R.HALOT_TH and w > R.HALOT_TW for h, w in q)
    assert all(R.check_A(R.A["halot"], R.products(c, dgrad=True)) for c in R.HALO_DGRAD_CASES)
    assert (2, 1, 1) in R.HALO_SHAPES and (2, 1, 1) in R.HALOT_SHAPES                       # a tile that is almost all padding
    # stem: 128 pixels per tile (256 at C = 192), 15 consecutive floats per filter row
    assert R.stem_tile(64) == R.stem_tile(128) == 128 and R.stem_tile(192) == 256
    assert R.stem_out(21, 19) == (11, 10) and R.stem_tile_spans_images(64, 3, 21, 19) and R.stem_tile_spans_images(192, 3, 21, 19)
    assert R.stem_tiles(64, 3, 21, 19) == 3                                                # more than one block
    assert R.stem_fast_lanes(300, 1) == 0 and R.stem_fast_lanes(1, 1) == 0                 # no lane takes the fast path
    assert R.stem_fast_lanes(7, 300) > 280 and R.stem_seam_inside_row(64, 1, 7, 300)       # fast path, seams inside a row
    assert any(W % 2 for _, _, W in R.STEM_SHAPES) and any(not W % 2 for _, _, W in R.STEM_SHAPES)
    assert any(H % 2 for _, H, _ in R.STEM_SHAPES) and any(not H % 2 for _, H, _ in R.STEM_SHAPES)
    # group e: tiles per image
    assert R.stem_tiles(64, 1, *R.E_STEM_HW) == 32 and R.stem_tiles(192, 1, *R.E_STEM_HW) == 16
    assert R.head_tiles(1, *R.E_HEAD_HW) == 8 and R.halo_tiles(1, *R.E_HALO_HW) == 4 and R.halot_tiles(1, *R.E_HALOT_HW) == 4
    assert [R.max_workgroups_per_cu("stem", C) for C in R.WIDTHS] == [8, 8, 4]
    assert len(R.ALL_CASES) == 3 * (7 + 6 + 5 + 5) and len({R.case_id(c) for c in R.ALL_CASES}) == len(R.ALL_CASES)


# ---------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------
def _f32(y):
    return y.to(torch.float32)


def _worst(fam, cases, mutate, bf16_out):
    """the worst band ratio of a mutant over `cases`; the unmutated reference, rounded like the device output, holds the band"""
    worst = 0.0
    for case in cases:
        i, ref = R.inputs(case), R.forward_ref(case)
        m = mutate(case, i, ref)
        if bf16_out:
            assert R.half_ulp_ratio(R.rne_bf16(ref.y), ref.y, ref.S, R.A[fam]) <= 1.0
            worst = max(worst, R.half_ulp_ratio(R.rne_bf16(m), ref.y, ref.S, R.A[fam]))
        else:
            assert R.band_ratio(_f32(ref.y), ref.y, ref.S, R.A[fam]) <= 1.0
            worst = max(worst, R.band_ratio(_f32(m), ref.y, ref.S, R.A[fam]))
    return worst


STEM64 = [c for c in R.STEM_CASES if c[1] == 64]
HEAD64 = [c for c in R.HEAD_CASES if c[1] == 64]
HALO64 = [c for c in R.HALO_CASES if c[1] == 64 and c[2] != (1, 37, 45)]
HALOT64 = [c for c in R.HALOT_CASES if c[1] == 64 and c[2] != (2, 19, 37)]


def test_mutant_1_clamp_to_edge():
    assert _worst("stem", STEM64, lambda c, i, ref: R.mutant_clamp_edge("stem", i["x"], i["w"], i["b"]), True) > 8.0
    assert _worst("halo", HALO64, lambda c, i, ref: R.mutant_clamp_edge("halo", i["x"], i["w"], i["b"]), False) > 8.0


def test_mutant_2_one_tap_dropped_at_one_channel():
    assert _worst("stem", STEM64, lambda c, i, ref: R.mutant_drop_tap("stem", i["x"], i["w"], i["b"]), True) > 8.0
    assert _worst("head", HEAD64, lambda c, i, ref: R.mutant_drop_tap("head", i["x"], i["w"], i["b"]), False) > 8.0
    assert _worst("halo", HALO64, lambda c, i, ref: R.mutant_drop_tap("halo", i["x"], i["w"], i["b"]), False) > 8.0
    assert _worst("halot", HALOT64, lambda c, i, ref: R.mutant_drop_tap("halot", i["x"], i["w"], i["b"]), False) > 8.0
    # at the widest layer too (25 x 192 products: the condition A n <= 1 / 8 at work)
    assert _worst("halo", [("halo", 192, (2, 16, 64))],
                  lambda c, i, ref: R.mutant_drop_tap("halo", i["x"], i["w"], i["b"]), False) > 8.0


def test_mutant_3_stem_sixteenth_slot_live():
    assert _worst("stem", STEM64, lambda c, i, ref: R.mutant_stem_slot15(i["x"], i["w"], i["b"]), True) > 8.0
    # the slot holds nothing at W = 1 (column 2 ox + 3 lies outside the row): there the mutant is the reference
    i = R.inputs(("stem", 64, (1, 300, 1)))
    assert torch.equal(R.mutant_stem_slot15(i["x"], i["w"], i["b"]), R.forward_ref(("stem", 64, (1, 300, 1))).y)


def test_mutant_4_head_phase_of_odd_columns():
    assert _worst("head", HEAD64, lambda c, i, ref: R.mutant_head_phase(ref.y), False) > 8.0


def test_mutant_5_head_second_x_tile_off_by_one_column():
    wide = [c for c in HEAD64 if c[2][2] > R.HD_TW + 1]
    assert wide and _worst("head", wide, lambda c, i, ref: R.mutant_head_halo_column(ref.y), False) > 8.0
    one = ("head", 64, (2, 4, 32))       # a single x tile: nothing to shift
    assert torch.equal(R.mutant_head_halo_column(R.forward_ref(one).y), R.forward_ref(one).y)


def test_mutant_6_transposed_phases_swapped():
    assert _worst("halot", HALOT64, lambda c, i, ref: R.mutant_swap_phases(ref.y), False) > 8.0
    assert _worst("head", HEAD64, lambda c, i, ref: R.mutant_swap_phases(ref.y), False) > 8.0


def test_column_route_band_is_wider_by_its_half_ulps_only():
    case = ("head", 64, (2, 5, 33))
    i, ref = R.inputs(case), R.forward_ref(case)
    hu = R.column_route_half_ulps(i["x"], i["w"])
    assert tuple(hu.shape) == tuple(ref.y.shape) and float(hu.min()) > 0
    # an interior element gathers 9 / 6 / 6 / 4 column terms, each |col| <= S: the term is at most 9 half ulps of S
    assert bool((hu <= 9 * 0.5 * 2.0 ** -7 * ref.S).all())
    # the route as stated -- columns rounded to bf16, then summed -- holds its band; a dropped tap does not
    wq = R.rne_bf16(i["w"])
    y = R.f64(i["b"])[None, :, None, None].expand_as(ref.y).clone()
    for ky in range(5):
        for kx in range(5):
            col = R.rne_bf16(torch.einsum("bchw,cd->bdhw", R.f64(i["x"]), wq[:, :, ky, kx]))
            one = torch.zeros((3, 1, 5, 5), dtype=torch.float64)
            one[:, 0, ky, kx] = 1.0
            y += torch.nn.functional.conv_transpose2d(col, one, None, stride=2, padding=2, output_padding=1, groups=3)
    assert R.column_route_ratio(_f32(y), ref.y, ref.S, hu) <= 1.0
    assert R.band_ratio(_f32(y), ref.y, ref.S) > 8.0         # (the direct kernel's band does tell the two routes apart)
    assert R.column_route_ratio(_f32(R.mutant_drop_tap("head", i["x"], i["w"], i["b"])), ref.y, ref.S, hu) > 8.0


# ---------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.WIDTHS)
def test_exact_stem_separates_the_roundings(C):
    x, w = R.exact_stem(C, 2, 9, 14)
    y = R.exact_stem_out(x, w)
    assert R.is_bf16(y), "the exact stem's outputs must be bf16-exact"
    # every term is a bf16 value times a power of two and there are at most two of them: exact in fp32 in any order
    assert torch.equal(y.to(torch.float32).double(), y)
    single = slice(0, C - R.TWO_TAP)
    xq = R.rne_bf16(x)
    assert set(np.unique(x.abs().numpy())) == {np.float32(v) for v in R.TIE_VALUES}
    # ties of both parities: 1 + 2^-8 -> 1 (even, down), 1 + 3 2^-8 -> 1 + 2^-6 (even, up)
    assert float(R.rne_bf16(torch.tensor([R.TIE_EVEN_DOWN]))) == 1.0 and float(R.rne_bf16(torch.tensor([R.TIE_EVEN_UP]))) == 1.0 + 2.0 ** -6
    assert bool(((x.double().abs() == R.TIE_EVEN_DOWN) & (xq.abs() == 1.0)).any())
    assert bool(((x.double().abs() == R.TIE_EVEN_UP) & (xq.abs() == 1.0 + 2.0 ** -6)).any())
    t, h, n = (R.exact_stem_out(x, w, R.trunc_bf16), R.exact_stem_out(x, w, R.round_half_up), R.exact_stem_out(x, w, None))
    assert not torch.equal(y, t) and not torch.equal(y, h) and not torch.equal(t, h)
    assert not torch.equal(y[:, single], t[:, single]) and not torch.equal(y[:, single], h[:, single])
    # no rounding of the image shows only where two taps meet: behind ONE power-of-two tap the store's rounding gives
    # the same value, which is why the last TWO_TAP channels are there
    assert torch.equal(y[:, single], n[:, single]) and not torch.equal(y[:, C - R.TWO_TAP:], n[:, C - R.TWO_TAP:])
    # every tap position and colour is used by some single-tap channel at C >= 128
    if C >= 128:
        assert int((w[single] != 0).any(0).sum()) == 75


@pytest.mark.parametrize("fam,C,B,H,W", [("head", 64, 2, 5, 33), ("head", 192, 1, 3, 65), ("halo", 192, 2, 17, 65),
                                          ("halot", 192, 1, 9, 33), ("halo", 64, 2, 1, 1)])
def test_exact_int_cases_are_exact(fam, C, B, H, W):
    x, w, b = R.exact_int(fam, C, B, H, W)
    ref = R.layer_ref(fam, x, w, b)
    assert R.is_bf16(x) and R.is_bf16(w)
    assert float(ref.S.max()) < 2 ** 24 and torch.equal(ref.y, ref.y.round())      # integers below 2^24: any order is exact
    assert torch.equal(ref.y.to(torch.float32).double(), ref.y)
    if H * W > 1:
        assert not R.is_bf16(ref.y), "some outputs must need the store's rounding to fit bf16"
