"""tests/resblock_ref.py held to direct nested loops, its case table to the widths and tiles it must reach, its bands to
their conditions, and its mutants to the bands they must miss.  CPU only.

Run:  python -m pytest tests/test_resblock_ref.py -q -s"""
import numpy as np
import pytest
import torch

import conv_bf16_ref as CB
import resblock_ref as R

TINY = (2, 4, 3)        # (B, h, w) of the nested-loop cases; channels cut to 3 -> 2


def loops_conv(x, w, b, k, s, p, transposed, op):
    """the convolution as nested loops over every index, in float64 numpy"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Cin, H, W = x.shape
    if transposed:
        Cout = w.shape[1]
        Ho, Wo = (H - 1) * s - 2 * p + k + op, (W - 1) * s - 2 * p + k + op
    else:
        Cout = w.shape[0]
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = np.zeros((B, Cout, Ho, Wo))
    for n in range(B):
        for co in range(Cout):
            for ci in range(Cin):
                for r in range(k):
                    for t in range(k):
                        if transposed:
                            for ih in range(H):
                                for iw in range(W):
                                    oh, ow = ih * s - p + r, iw * s - p + t
                                    if 0 <= oh < Ho and 0 <= ow < Wo:
                                        y[n, co, oh, ow] += x[n, ci, ih, iw] * w[ci, co, r, t]
                        else:
                            for oh in range(Ho):
                                for ow in range(Wo):
                                    ih, iw = oh * s - p + r, ow * s - p + t
                                    if 0 <= ih < H and 0 <= iw < W:
                                        y[n, co, oh, ow] += x[n, ci, ih, iw] * w[co, ci, r, t]
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return y


@pytest.mark.parametrize("role", [l.role for l in R.LAYERS3(64)])
def test_reference_conv_is_the_nested_loop_conv(role):
    lay = R.layer(role, 64)
    r = R._rng("loops-" + role)
    B, h, w = TINY
    cin, cout = 3, 2
    x = r.standard_normal((B, cin, h, w))
    wt = r.standard_normal((cin, cout, lay.k, lay.k) if lay.transposed else (cout, cin, lay.k, lay.k))
    b = r.standard_normal(cout)
    ref = R.conv_ref(x, wt, b, lay.k, lay.s, lay.p, lay.transposed, lay.op)
    want = loops_conv(x, wt, b, lay.k, lay.s, lay.p, lay.transposed, lay.op)
    assert tuple(ref.y.shape) == want.shape == (B, cout) + tuple(R.out_size(lay, h, w))
    assert float(np.abs(ref.y.numpy() - want).max()) <= 1e-13
    wantS = loops_conv(np.abs(x), np.abs(wt), np.abs(b), lay.k, lay.s, lay.p, lay.transposed, lay.op)
    assert float(np.abs(ref.S.numpy() - wantS).max()) <= 1e-13


def test_column_matrices_are_the_nested_loop_gather_and_scatter():
    r = R._rng("cols")
    for (k, s, p, op) in ((3, 2, 1, 1), (1, 2, 0, 1)):
        for (B, H, W) in ((2, 6, 4), (1, 5, 3)):
            C, Kp = 3, R.kpad8(k, 3)
            x = r.random_sample((B, C, H, W)).astype(np.float32)
            Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            col = R.im2col_ref(torch.as_tensor(x), k, s, p, Kp)
            xq = R.rne_bf16(x).numpy()
            want = np.zeros((B, Ho, Wo, Kp))
            for n in range(B):
                for oh in range(Ho):
                    for ow in range(Wo):
                        for rr in range(k):
                            for t in range(k):
                                ih, iw = oh * s - p + rr, ow * s - p + t
                                if 0 <= ih < H and 0 <= iw < W:
                                    want[n, oh, ow, (rr * k + t) * C:(rr * k + t + 1) * C] = xq[n, :, ih, iw]
            assert np.array_equal(col.numpy(), want.reshape(-1, Kp)) and not col[:, k * k * C:].any()
            # col2im: the scatter of a column matrix of Ho x Wo feature pixels back onto H' x W'
            Hc, Wc = Ho, Wo
            Hq, Wq = (Hc - 1) * s - 2 * p + k + op, (Wc - 1) * s - 2 * p + k + op
            cm = r.standard_normal((B * Hc * Wc, Kp))
            bias = r.standard_normal(C)
            out, S = R.col2im_ref(torch.as_tensor(cm), torch.as_tensor(bias), B, Hc, Wc, C, k, s, p, op)
            w_ = np.zeros((B, C, Hq, Wq)) + bias[None, :, None, None]
            c4 = cm.reshape(B, Hc, Wc, Kp)
            for n in range(B):
                for ih in range(Hc):
                    for iw in range(Wc):
                        for rr in range(k):
                            for t in range(k):
                                oh, ow = ih * s - p + rr, iw * s - p + t
                                if 0 <= oh < Hq and 0 <= ow < Wq:
                                    w_[n, :, oh, ow] += c4[n, ih, iw, (rr * k + t) * C:(rr * k + t + 1) * C]
            assert float(np.abs(out.numpy() - w_).max()) <= 1e-13 and bool((S >= out.abs() - 1e-13).all())


def test_dropped_roles_are_identical_to_layers_that_run_already():
    ran = set(R.ROWS)
    for M in R.WIDTHS:
        for role, (table, other) in R.DROPPED.items():
            mine = R.layer(role, M)
            theirs = CB.layer(other, M, 1) if table == "latent" else R.layer(other, M)
            assert mine[1:] == theirs[1:], (role, other, mine, theirs)
            if table == "latent":      # dropped exactly where the latent file runs it; run here otherwise
                there = any(r == other and m == M for (r, m, _) in CB.ROWS)
                assert R.dropped(role, M) == there and ((role, M) in ran) == (not there), (role, M)
            else:
                assert R.dropped(role, M) and (role, M) not in ran
                assert (other, M) in ran or R.dropped(other, M)
    assert ("rbs1", 64) in ran and ("rbs1", 128) in ran and ("rb1", 128) in ran and ("rbs1", 192) not in ran
    assert set(R.IGEMM_ROLES) | set(R.RGB_ROLES) | {"rb2", "hd_up1"} == {l.role for l in R.LAYERS3(192)}


def test_case_table_meets_its_widths_tiles_and_conditions():
    rows192 = {r for (r, M) in R.ROWS if M == 192}
    assert rows192 == {r for r in R.IGEMM_ROLES if not R.dropped(r, 192)}
    for (r, M) in R.ROWS:
        if M != 192:
            a, b = R.layer(r, M), R.layer(r, 192)
            assert (R.npad(a.cout), R.n_tile(a.cout)) != (R.npad(b.cout), R.n_tile(b.cout)), (r, M)
    for M in (64, 128):
        for r in R.IGEMM_ROLES:
            a, b = R.layer(r, M), R.layer(r, 192)
            assert ((r, M) in R.ROWS) == (not R.dropped(r, M) and
                                          (R.npad(a.cout), R.n_tile(a.cout)) != (R.npad(b.cout), R.n_tile(b.cout)))
    assert {R.npad(R.layer(r, M).cout) for (r, M) in R.ROWS} == set(R.REQUIRED_NPAD)
    assert {R.n_tile(R.layer(r, M).cout) for (r, M) in R.ROWS} == set(R.REQUIRED_TN)
    assert (R.npad(288), R.n_tile(288)) == (320, 1)
    # grids: odd sides, a 1x1, one with a second 64-row tile at the strided layers' output
    assert any(h % 2 and w % 2 for (_, h, w) in R.GRIDS) and (2, 1, 1) in R.GRIDS
    assert any(B * ((h + 1) // 2) * ((w + 1) // 2) > 64 for (B, h, w) in R.GRIDS)
    assert any(h % 2 and w % 2 for (_, h, w) in R.RGB_SIZES) and any(h % 2 == 0 for (_, h, w) in R.RGB_SIZES)
    # the transposed cases' four output phases have different sizes where an input side is odd -- they never do with
    # output_padding 1 (2 h x 2 w); the phases differ in their TAP counts instead: 1, 2, 2 and 4
    assert R.column_terms() == 4
    # the band conditions, forward and data gradient, every case
    for case in R.CASES + R.STEM_CASES + R.HEAD_CASES:
        lay = R.inputs(case)["lay"]
        for n in (R.products(lay), R.products(lay, dgrad=True)):
            assert R.check_A(R.band_A(n), n), (R.case_id(case), n)
    assert R.products(R.layer("skip_rgb", 64)) == 3 and R.band_A(3) == 4 * 2.0 ** -23 < R.A_BAND
    assert R.products(R.layer("stem3", 64)) == 27 and R.band_A(27) == R.A_BAND
    assert R.products(R.layer("head3", 64)) == 4 * 64 and R.products(R.layer("head3", 64), dgrad=True) == 27
    assert R.products(R.layer("up", 192)) == 4 * 192 and R.products(R.layer("up", 192), dgrad=True) == 9 * 192
    assert R.products(R.layer("skip", 192)) == 192 and R.products(R.layer("skip", 192), dgrad=True) == 192
    assert R.kpad8(3, 3) == 32 and R.kpad8(1, 3) == 8
    # a measurement, once recorded, keeps 4 x itself under the constant in use
    for fam, v in R.A_MEASURED.items():
        assert v is None or 4 * v <= R.A_BAND, (fam, v)


def test_head_column_route_band_has_at_most_four_half_ulps():
    case = ("head3", 64, 0, (2, 9, 7))
    i = R.inputs(case)
    hu = R.column_route_half_ulps(i["x"], i["w"], 3, 2, 1, 1)
    ref = R.forward_ref(case)
    assert hu.shape == ref.y.shape
    # at most 4 terms: the bound is at most 4 half ulps of the largest column value
    xq, wq, _ = R.rounded_operands(case)
    biggest = max(float(torch.einsum("bchw,cd->bdhw", xq, wq[:, :, r, t]).abs().max()) for r in range(3) for t in range(3))
    assert float(hu.max()) <= 4 * 0.5 * float(R.ulp_bf16(torch.tensor([biggest], dtype=torch.float64))) + 1e-300
    # even-even output elements gather one term, odd-odd four
    assert float((hu[..., 1::2, 1::2] / hu[..., 0::2, 0::2].clamp_min(1e-300)).median()) > 2.0


def test_inputs_give_every_band_room():
    """the bands are narrow against the values they hold (a band as wide as the value would hold nothing) and a leaky case
    has both signs"""
    for case in R.CASES + R.STEM_CASES + R.HEAD_CASES:
        i, ref = R.inputs(case), R.forward_ref(case)
        A = R.band_A(ref.n)
        rel = float((A * ref.S).median() / ref.y.abs().median())
        assert rel <= 2.0 ** -14, (R.case_id(case), rel)
        if i["lay"].leaky and ref.y.numel() >= 64:
            neg = float((ref.y <= 0).double().mean())
            assert 0.35 <= neg <= 0.65, (R.case_id(case), neg)


def test_share_of_elements_where_the_neighbouring_bf16_value_is_accepted():
    """Every bf16 output tests/test_gpu_resblocks.py holds at half a bf16 ulp + A S for want of an fp32 twin (the stem's
    outputs, the fused conv_out, the blocks' stored conv outputs: resblock_ref.no_twin_outputs): the share of its
    elements whose float64 value lies within A S of a bf16 rounding boundary -- where the band accepts the neighbouring
    bf16 value as well -- is printed and is at most 1 %, on the reference alone.  Every other bf16 output of that module is
    held bit for bit to the rounding of the device's own fp32 launch, which excludes nothing."""
    worst, count = (0.0, ""), 0
    for tag, y64, S, A in R.no_twin_outputs():
        share = R.near_boundary_share(y64, S, A)
        print(f"SHARE {tag} within A S of a bf16 rounding boundary {share:.5f} of {y64.numel()}")
        assert share <= 0.01, (tag, share)
        assert bool((y64 < 0).any()) and bool((y64 > 0).any()), tag
        worst, count = max(worst, (share, tag)), count + 1
    print(f"SHARE worst {worst[0]:.5f} ({worst[1]}) over {count} outputs (allowed 0.01)")
    assert count == len(R.STEM_CASES) + len(R.WIDTHS) * 2 * len(R.FUSED_GRIDS) + \
        sum({"rbs_rgb": 3, "rbs": 2, "rb": 0, "rbu": 2}[k] for k in R.BLOCK_KINDS) * len(R.BLOCK_WIDTHS)


def _miss(tag, n):
    print(f"MUTANT {tag}: {n} elements out of band")
    return n


def test_mutants_miss_their_bands():
    # 1. a dropped tap: every role with taps to drop
    for role in ("up", "enc_last", "hd_c", "hd_up2", "skip"):
        case = (role, 64, 0, (2, 9, 7))
        ref = R.forward_ref(case)
        lay = R.inputs(case)["lay"]
        y = R.mutant_drop_tap(case, r=0 if lay.k == 1 else None)
        if R.inputs(case)["lay"].leaky:
            y, want = R.leaky_ref(y), R.leaky_ref(ref.y)
        else:
            want = ref.y
        assert _miss(f"1 dropped tap {role}", R.out_of_band(y, want, ref.S, R.band_A(ref.n), lay.out != "f32")) > 0
    for role in ("stem3", "skip_rgb"):
        case = (role, 64, 0, (2, 18, 14))
        ref = R.forward_ref(case)
        y = R.mutant_drop_tap(case, r=0, t=0)
        assert _miss(f"1 dropped tap {role}", R.out_of_band(y, ref.y, ref.S, R.band_A(ref.n), True)) > 0
    case = ("head3", 64, 0, (2, 9, 7))
    i, ref = R.inputs(case), R.forward_ref(case)
    hu = R.column_route_half_ulps(i["x"], i["w"], 3, 2, 1, 1)
    y = R.mutant_drop_tap(case)
    assert _miss("1 dropped tap head3 (column-route band)", int(((y - ref.y).abs() > R.A_BAND * ref.S + hu).sum())) > 0
    # 2. output_padding ignored
    for role in ("up", "hd_up2"):
        case = (role, 64, 0, (3, 5, 6))
        ref = R.forward_ref(case)
        y, want = R.mutant_no_output_padding(case), ref.y
        if R.inputs(case)["lay"].leaky:
            y, want = R.leaky_ref(y), R.leaky_ref(want)
        assert _miss(f"2 output_padding ignored {role}", R.out_of_band(y, want, ref.S, R.A_BAND, True)) > 0
    y = R.mutant_no_output_padding(case := ("head3", 64, 0, (3, 5, 6)))
    i, ref = R.inputs(case), R.forward_ref(case)
    hu = R.column_route_half_ulps(i["x"], i["w"], 3, 2, 1, 1)
    assert _miss("2 output_padding ignored head3", int(((y - ref.y).abs() > R.A_BAND * ref.S + hu).sum())) > 0
    # 3. the stride-2 skip sampled at offset 1
    for case in (("skip", 64, 0, (2, 9, 7)), ("skip_rgb", 64, 0, (2, 18, 14))):
        ref = R.forward_ref(case)
        assert _miss(f"3 skip at offset 1 {case[0]}", R.out_of_band(R.mutant_skip_offset(case), ref.y, ref.S, R.band_A(ref.n), True)) > 0
    # 3 / 4 / 5 on the blocks: against the block's last band (the skip add: half a bf16 ulp of the result)
    for kind, grid in (("rbs", (2, 9, 7)), ("rbs_rgb", (2, 18, 14)), ("rb", (2, 9, 7)), ("rbu", (2, 5, 6))):
        P, x = R.block_params(kind, 64), R.block_input(kind, 64, grid)
        good = R.block_forward(kind, x, P)["out"]
        for mutant in ("no_skip", "leaky_positive") + (("skip_offset",) if kind.startswith("rbs") else ()):
            bad = R.block_forward(kind, x, P, mutant)["out"]
            n = int(((bad - good).abs() > 0.5 * R.ulp_bf16(good)).sum())
            assert _miss(f"{ {'no_skip': 4, 'leaky_positive': 5, 'skip_offset': 3}[mutant]} {mutant} block {kind}", n) > 0
    # 5. LeakyReLU on the positive side, one layer
    case = ("up_l", 64, 0, (2, 9, 7))
    ref = R.forward_ref(case)
    assert _miss("5 leaky on the positive side up_l",
                 R.out_of_band(R.mutant_leaky_positive(ref.y), R.leaky_ref(ref.y), ref.S, R.A_BAND, True)) > 0
    # 6. the transposed weight not flipped
    for case in (("up", 64, 0, (2, 9, 7)), ("hd_up2", 64, 0, (2, 9, 7))):
        ref = R.forward_ref(case)
        y, want = R.mutant_not_flipped(case), ref.y
        if R.inputs(case)["lay"].leaky:
            y, want = R.leaky_ref(y), R.leaky_ref(want)
        assert _miss(f"6 weight not flipped {case[0]}", R.out_of_band(y, want, ref.S, R.A_BAND, True)) > 0
    # 7. the padding columns of the stem's matrix live
    for role in ("stem3", "skip_rgb"):
        case = (role, 64, 0, (2, 18, 14))
        i, ref = R.inputs(case), R.forward_ref(case)
        lay = i["lay"]
        col_m, y = R.mutant_live_padding_columns(case)
        col = R.im2col_ref(i["x"], lay.k, lay.s, lay.p, R.kpad8(lay.k, 3))
        assert _miss(f"7 live padding columns {role}: matrix", int((col_m != col).sum())) > 0
        assert _miss(f"7 live padding columns {role}: output", R.out_of_band(y, ref.y, ref.S, R.band_A(ref.n), True)) > 0
        # (and the reference's own matrix product is the reference convolution)
        m = R.stem_matrix_weight(i["w"], col.shape[1])
        y0 = (col @ m).reshape(ref.y.shape[0], i["Ho"], i["Wo"], lay.cout).permute(0, 3, 1, 2) + R.f64(i["b"])[None, :, None, None]
        assert float((y0 - ref.y).abs().max()) <= 1e-12
    # 8. a weight-gradient row sent to tap Cin + c
    for role in ("stem3",):
        case = (role, 64, 0, (2, 18, 14))
        i = R.inputs(case)
        gr = R.grads_ref(case)
        xq, _, gq = R.rounded_operands(case)
        weight = R.wgrad_weight(xq, gq, i["lay"])
        P = gq.shape[0] * gq.shape[2] * gq.shape[3]
        bad = R.mutant_wgrad_rows(gr.dw)
        n = int(((bad - gr.dw).abs() > (P + 3) * 2.0 ** -24 * weight).sum())
        assert _miss(f"8 weight-gradient rows {role}", n) > 0
        assert R.wgrad_ratio(gr.dw, gr.dw, weight, P, 1) == 0.0 and R.wgrad_ratio(bad, gr.dw, weight, P, 1) > 1.0
    # skip_rgb has one tap: the two index maps coincide there, and the mutant must say so rather than pass by accident
    gr1 = R.grads_ref(("skip_rgb", 64, 0, (2, 18, 14)))
    assert torch.equal(R.mutant_wgrad_rows(gr1.dw), gr1.dw)


def test_rounding_point_statements():
    """the element-wise statements against torch's own bf16 arithmetic on the CPU"""
    r = R._rng("elementwise")
    a = torch.as_tensor(r.standard_normal(4096).astype(np.float32)).to(torch.bfloat16)
    b = torch.as_tensor((r.standard_normal(4096) * 3).astype(np.float32)).to(torch.bfloat16)
    assert torch.equal(R.add_bf16_ref(a.float(), b.float()), (a + b).double())
    assert torch.equal(R.torch_leaky_bf16_ref(a.float()), torch.nn.functional.leaky_relu(a, 0.01).double())
    ar = a.clone().requires_grad_(True)
    torch.nn.functional.leaky_relu(ar, 0.01).backward(b)
    assert torch.equal(R.torch_leaky_bf16_bwd_ref(a.float(), b.float()), ar.grad.double())


def test_fp32_block_statement_is_autograd_consistent():
    """block_forward_fp32 is differentiable plain torch: its gradient exists for every parameter it names"""
    for kind, grid in (("rbs", (1, 5, 4)), ("rb", (1, 3, 3)), ("rbu", (1, 3, 2)), ("rbs_rgb", (1, 6, 5))):
        P = {k: v.double().requires_grad_(True) for k, v in R.block_params(kind, 64).items()}
        x = R.block_input(kind, 64, grid).double().requires_grad_(True)
        out = R.block_forward_fp32(kind, x, P)
        gs = torch.autograd.grad(out.square().sum(), [x] + list(P.values()))
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in gs), kind
