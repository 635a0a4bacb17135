"""The checkerboard context without a GPU: the mask, the two-pass schedule `codec.two_pass` against the brute-force
schedule of checker_ref.py, the merged schedule, the LICBITS7 container and the codec's refusals."""
import struct
import types

import numpy as np
import pytest
import torch

import checker_ref as CR
import test_bitstream_golden as BG

SHAPES = [(1, 1), (1, 5), (4, 1), (3, 5), (4, 8), (5, 4)]
HEAD = dict(family=1, M=32, K=3, z_lo=-32, z_S=65, y_W=24, B=2, H=70, W=100, top=0, left=0)
CRCS = [0x12345678, 0x9ABCDEF0]


@pytest.fixture(scope="module")
def codec():
    from neural_image_compression_amd import codec as CD
    return CD


def _stub_model(tap_mask):
    masked = types.SimpleNamespace(kernel_size=(5, 5), padding=(2, 2), _tap_mask=tap_mask)
    return types.SimpleNamespace(context_model=types.SimpleNamespace(masked=masked), M=32, K=3)


def test_mask_has_twelve_live_taps_and_tap_mask_agrees():
    from neural_image_compression_amd.entropy import ContextModel, MaskedConv2d
    mc = MaskedConv2d("checkerboard", in_channels=3, out_channels=6, kernel_size=5, stride=1, padding=2)
    m = mc.mask.numpy()
    assert m.shape == (6, 3, 5, 5) and (m == CR.mask(5)[None, None]).all()
    assert int(m[0, 0].sum()) == 12 == len(CR.live_taps(5)) == bin(mc._tap_mask).count("1")
    assert mc._tap_mask == CR.tap_mask(5)
    for r in range(5):
        for s in range(5):
            assert ((mc._tap_mask >> (r * 5 + s)) & 1) == int(m[0, 0, r, s]) == int(((r - 2) + (s - 2)) % 2 == 1)
    m3 = MaskedConv2d("checkerboard", in_channels=1, out_channels=1, kernel_size=3, stride=1, padding=1)
    assert (m3.mask.numpy()[0, 0] == CR.mask(3)).all() and m3._tap_mask == CR.tap_mask(3) == 0b010101010
    assert ContextModel(4, mask_type="checkerboard").masked._tap_mask == CR.tap_mask(5)
    # the raster masks are what they were
    a = MaskedConv2d("A", in_channels=1, out_channels=1, kernel_size=5, stride=1, padding=2)
    assert a._tap_mask == (1 << 12) - 1 and int(a.mask.sum()) == 12 and ContextModel(4).masked._tap_mask == (1 << 12) - 1
    with pytest.raises(AssertionError):
        MaskedConv2d("C", in_channels=1, out_channels=1, kernel_size=5)


def test_models_take_the_context_option():
    import neural_image_compression_amd as nic
    for cls in (nic.JointAutoregressiveHierarchical, nic.HierarchicalMixtureResidual):
        raster, checker = cls(8, 1), cls(8, 1, context="checkerboard")
        assert raster.context == cls(8, 1, context="raster").context == "raster"
        assert raster.context_model.masked._tap_mask == (1 << 12) - 1
        assert checker.context_model.masked._tap_mask == CR.tap_mask(5)
        assert list(raster.state_dict()) == list(checker.state_dict())
        with pytest.raises(ValueError, match="context"):
            cls(8, 1, context="diagonal")


@pytest.mark.parametrize("h,w", SHAPES)
def test_two_pass_is_the_brute_force_schedule(codec, h, w):
    steps = codec.two_pass(h, w)
    want = CR.brute_force_schedule(h, w)
    assert [list(zip(ii.tolist(), jj.tolist())) for ii, jj in steps] == want
    assert len(steps) == (1 if h * w == 1 else 2)
    seen = np.zeros((h, w), np.int64)
    step = np.zeros((h, w), np.int64)
    for t, (ii, jj) in enumerate(steps):
        assert ii.dtype == jj.dtype == np.int64
        np.add.at(seen, (ii, jj), 1)
        step[ii, jj] = t
    assert (seen == 1).all()                                         # every pixel exactly once
    anc = CR.is_anchor(h, w)
    assert (step == 0)[anc].all() and (step == 1)[~anc].all()
    for i in range(h):
        for j in range(w):
            for r, s in CR.live_taps(5):
                a, b = i + r - 2, j + s - 2
                if not (0 <= a < h and 0 <= b < w):
                    continue
                if step[i, j] == 1:
                    assert step[a, b] == 0                           # a step-1 pixel reads decoded anchors only
                else:
                    assert not anc[a, b]                             # a step-0 pixel's taps lie on what anchor() zeroes
    cc = object.__new__(codec.ContextCodec)
    cc.pad, cc.schedule = 2, "checkerboard"
    assert all((a == c).all() and (b == d).all() for (a, b), (c, d) in zip(cc._wavefront(h, w), steps))
    with pytest.raises(codec.CodecError, match="slice_rows"):
        cc._wavefront(h, w, 2)


def test_merged_schedule_has_two_steps_and_restricts_to_two_pass(codec):
    shapes = [(4, 8), (1, 1), (3, 5)]
    sched = codec.merged_wavefront(shapes, 2, [None] * 3, "checkerboard")
    assert sched.T == 2 and sched.seg.shape == (2, 3, 2) and sched.step_off.tolist() == [0, 16 + 1 + 8, 32 + 1 + 15]
    for b, (h, w) in enumerate(shapes):
        steps = codec.two_pass(h, w)
        for t in range(2):
            first, n = sched.seg[t, b]
            rows = sched.rows[:, sched.step_off[t] + first:sched.step_off[t] + first + n]
            assert (rows[0] == b).all()
            if t >= len(steps):
                assert n == 0
                continue
            ii, jj = steps[t]
            assert rows[1].tolist() == (ii * w + jj).tolist()
            assert rows[2].tolist() == ((ii + 2) * (w + 4) + jj + 2).tolist()
    # the raster schedule is untouched by the new argument's default
    a, b = codec.merged_wavefront(shapes, 2, [None] * 3), codec.merged_wavefront(shapes, 2, [None] * 3, "raster")
    assert a.T == b.T == 8 + 3 * 3 and (a.rows == b.rows).all()
    with pytest.raises(codec.CodecError, match="slice_rows"):
        codec.merged_wavefront(shapes, 2, [None, 2, None], "checkerboard")
    with pytest.raises(codec.CodecError, match="schedule"):
        codec.merged_wavefront(shapes, 2, [None] * 3, "diagonal")


def test_encode_plan_follows_two_pass(codec):
    plan = codec.ragged_encode_plan([(4, 8), (3, 5)], 4, 2, None, 3, "checkerboard")
    assert plan.images.tolist() == [[0, 32, 0, 2], [32, 15, 2, 2]]
    assert plan.step_len.tolist() == [64, 64, 32, 28]
    want = [np.concatenate([ii * w + jj for ii, jj in codec.two_pass(h, w)]) for h, w in ((4, 8), (3, 5))]
    assert plan.order.tolist() == np.concatenate(want).tolist()
    with pytest.raises(codec.CodecError, match="slice_rows"):
        codec.ragged_encode_plan([(4, 8)], 4, 2, 2, 3, "checkerboard")


# ---- LICBITS7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 8])
def test_licbits7_round_trip_is_licbits5_under_its_own_magic(codec, G):
    zs, zes = BG._subs(2 * G)
    ys, es = [s + b"xy" for s in zs], list(reversed(zes))
    blob = codec.pack_bitstream_checker(HEAD, zs, zes, ys, es, CRCS, G)
    assert blob[:8] == b"LICBITS7" == codec.BITSTREAM_MAGIC_CHECKER
    head, zs2, zes2, ys2, es2, crcs, groups = codec.unpack_bitstream_checker(blob)
    assert (head, zs2, zes2, ys2, es2, crcs, groups) == (HEAD, zs, zes, ys, es, CRCS, G)
    five = codec.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, G)
    assert blob[8:-4] == five[8:-4] and struct.unpack_from("<2I", blob, 56) == (64 * G, 0)
    assert codec._format_of_magic(blob[:8]) == codec._FORMAT_CHECKER


def test_licbits7_refuses_damage(codec):
    zs, zes = BG._subs(4)
    blob = codec.pack_bitstream_checker(HEAD, zs, zes, zs, zes, CRCS, 2)
    five = codec.pack_bitstream_zrans(HEAD, zs, zes, zs, zes, CRCS, 2)
    u = codec.unpack_bitstream_checker
    for at in list(range(0, 96)) + [len(blob) // 2, len(blob) - 5, len(blob) - 1]:
        with pytest.raises(codec.CodecError):
            u(BG._flip(blob, at, 0x10))                               # any flipped byte: magic, length or CRC-32
    with pytest.raises(codec.CodecError, match="CRC-32"):
        u(BG._flip(blob, len(blob) // 2, 0x01))
    for cut in (blob[:-1], blob[:63], blob[:70], blob[:20], b"", blob + b"\0"):
        with pytest.raises(codec.CodecError, match="truncated"):
            u(cut)
    with pytest.raises(codec.CodecError, match=r"damaged \(slice_rows = 3"):
        u(BG._patched(blob, 60, 3))
    with pytest.raises(codec.CodecError, match="not a LICBITS7"):
        u(five)
    with pytest.raises(codec.CodecError, match="not a LICBITS5"):
        codec.unpack_bitstream_zrans(blob)
    for lanes in (0, 96, 576):
        with pytest.raises(codec.CodecError, match="interleaves"):
            u(BG._patched(blob, 56, lanes))
    with pytest.raises(codec.CodecError, match="slice_rows"):
        codec._pack(codec._FORMAT_CHECKER, dict(HEAD, slice_rows=4), (zs, zes), zs, zes, CRCS, 2)


# ---- the codec's view of a mask ----------------------------------------------------------------------
def test_codec_layer_classifies_its_mask(codec):
    assert codec.CodecLayer(_stub_model((1 << 12) - 1), "context_model", "entropy_parameters").kind == "raster"
    assert codec.CodecLayer(_stub_model(CR.tap_mask(5)), "context_model", "entropy_parameters").kind == "checkerboard"
    for bad in ((1 << 25) - 1, (1 << 13) - 1, CR.tap_mask(5) | 1):
        with pytest.raises(codec.CodecError, match="raster.*checkerboard"):
            codec.CodecLayer(_stub_model(bad), "context_model", "entropy_parameters")


def test_checkerboard_codec_refusals_at_construction(codec):
    stub = lambda: _stub_model(CR.tap_mask(5))
    for enc in ("host", "device"):
        for G in (1, 8):
            for zc in ("range", "rans"):
                cc = codec.ContextCodec(stub(), coder="rans", encoder=enc, groups=G, z_coder=zc, y_W=2)
                assert cc.schedule == "checkerboard" and len(cc._wavefront(32, 48)) == 2
    with pytest.raises(codec.CodecError, match="coder='range'.*needs coder='rans'"):
        codec.ContextCodec(stub())
    with pytest.raises(codec.CodecError, match="coder='range'"):
        codec.ContextCodec(stub(), coder="range")
    with pytest.raises(codec.CodecError, match="slice_rows=4"):
        codec.ContextCodec(stub(), coder="rans", slice_rows=4)
    assert codec.ContextCodec(BG._stub_model(), coder="rans").schedule == "raster"


def test_schedule_mismatches_are_refused_on_the_host(codec):
    """a blob of the other schedule, and strings of the other schedule, are refused before anything is launched: the
    stub models have no parameters, so any launch would fail with another error"""
    zs, zes = BG._subs(2)
    seven = codec.pack_bitstream_checker(HEAD, zs, zes, zs, zes, CRCS, 1)
    five = codec.pack_bitstream_zrans(HEAD, zs, zes, zs, zes, CRCS, 1)
    two = codec.pack_bitstream_rans(HEAD, b"z", zs, zes, CRCS)
    raster = codec.ContextCodec(BG._stub_model(), coder="rans")
    checker = codec.ContextCodec(_stub_model(CR.tap_mask(5)), coder="rans", z_coder="rans")
    for cc, blobs in ((raster, [seven]), (checker, [five, two])):
        for blob in blobs:
            with pytest.raises(codec.CodecError, match="schedule mismatch"):
                cc.decompress_image(blob)
            with pytest.raises(codec.CodecError, match="blob 0: schedule mismatch"):
                cc.decompress_images([blob])
    shape, z_shape = (2, 32, 5, 7), (2, 32, 2, 2)
    with pytest.raises(codec.CodecError, match="schedule mismatch"):
        raster.decompress({"schedule": "checkerboard", "coder": "rans"}, shape, z_shape)
    with pytest.raises(codec.CodecError, match="schedule mismatch"):
        checker.decompress({"coder": "rans"}, shape, z_shape)
    with pytest.raises(codec.CodecError, match="item 0: schedule mismatch"):
        checker.decompress_many([({"coder": "rans"}, shape, z_shape)])
    with pytest.raises(codec.CodecError, match="z_coder='range'"):
        codec.ContextCodec(_stub_model(CR.tap_mask(5)), coder="rans").compress_image(torch.zeros(1, 3, 8, 8))
