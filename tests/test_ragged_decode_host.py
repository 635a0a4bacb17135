"""The host half of ContextCodec.decompress_images: `merged_wavefront` against the plain-loop restatement of
ragged_steps_ref.py and against `wavefront` image by image, and the refusals of decompress_images that need no GPU.
CPU only."""
import itertools
import struct

import numpy as np
import pytest

import ragged_steps_ref as RS

SHAPES = [(2, 3), (4, 4), (1, 7), (5, 2)]
PAD = 2
R_MIXES = [(None, None, None, None), (1, 2, 3, None), (3, None, 1, 2), (2, 1, None, 3), (None, 3, 2, 1)]


@pytest.fixture(scope="module")
def codec():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec
    return codec


@pytest.mark.parametrize("Rs", R_MIXES)
def test_merged_wavefront_is_the_restatement(codec, Rs):
    s = codec.merged_wavefront(SHAPES, PAD, Rs)
    T, seg, rows = RS.merged(SHAPES, PAD, Rs)
    assert s.T == T and s.seg.dtype == np.int32 and s.seg.shape == (T, len(SHAPES), 2)
    assert s.seg.tolist() == [[list(p) for p in step] for step in seg]
    assert s.rows.dtype == np.int64 and s.rows.shape == (3, len(rows))
    assert s.rows.T.tolist() == [list(r) for r in rows]
    assert s.step_off.tolist() == [0] + list(itertools.accumulate(sum(n for _, n in step) for step in seg))


@pytest.mark.parametrize("Rs", R_MIXES)
def test_every_image_keeps_its_own_wavefront(codec, Rs):
    s = codec.merged_wavefront(SHAPES, PAD, Rs)
    per = [codec.wavefront(h, w, PAD, R) for (h, w), R in zip(SHAPES, Rs)]
    assert s.T == max(len(steps) for steps in per)
    assert int(s.step_off[-1]) == s.rows.shape[1] == sum(h * w for h, w in SHAPES)
    for t in range(s.T):
        batch = s.rows[:, s.step_off[t]:s.step_off[t + 1]]
        at = 0
        for b, (h, w) in enumerate(SHAPES):
            first, n = s.seg[t, b]
            assert first == at, "segments are contiguous, a finished image's included"
            if t >= len(per[b]):
                assert n == 0
                continue
            ii, jj = per[b][t]
            assert n == len(ii) > 0
            mine = batch[:, first:first + n]
            assert (mine[0] == b).all()
            assert np.array_equal(mine[1], ii * w + jj)
            assert np.array_equal(mine[2], (ii + PAD) * (w + 2 * PAD) + jj + PAD)
            at += n
        assert at == batch.shape[1]
    for b in range(len(SHAPES)):
        # the step lengths `compress` codes image b with, per latent channel
        assert s.seg[:len(per[b]), b, 1].tolist() == [len(ii) for ii, _ in per[b]]
        assert (s.seg[len(per[b]):, b, 1] == 0).all()


@pytest.mark.parametrize("h,w,R", [(4, 4, None), (5, 2, 2), (1, 7, 1), (6, 9, 4), (3, 2, None)])
def test_one_image_alone_gives_the_index_arrays_of_the_single_decoder(codec, h, w, R):
    """`_step_indices` is what ContextCodec._step_front_end uploads for one image: raster indices and indices into
    the framed plane.  (3, 2): narrower than the mask, so some step numbers hold no pixel"""
    steps = codec.wavefront(h, w, PAD, R)
    idx = codec._step_indices(steps, w, PAD)
    assert idx.shape == (2, h * w) and sorted(idx[0].tolist()) == list(range(h * w))
    s = codec.merged_wavefront([(h, w)], PAD, [R])
    assert s.T == len(steps)
    assert np.array_equal(s.rows[1:], idx) and s.rows[1:].dtype == idx.dtype
    assert (s.rows[0] == 0).all() and (s.seg[:, 0, 0] == 0).all()
    assert s.seg[:, 0, 1].tolist() == [len(ii) for ii, _ in steps]


def test_every_call_returns_arrays_of_its_own(codec):
    a = codec.merged_wavefront(SHAPES, PAD, [None] * 4)
    a.rows[:] = -1
    a.seg[:] = -1
    b = codec.merged_wavefront(SHAPES, PAD, [None] * 4)
    assert (b.rows >= 0).all() and (b.seg >= 0).all()


def test_merged_wavefront_of_nothing_and_of_mismatched_lists(codec):
    s = codec.merged_wavefront([], PAD, [])
    assert s.T == 0 and s.seg.shape == (0, 0, 2) and s.rows.shape == (3, 0) and s.step_off.tolist() == [0]
    with pytest.raises(codec.CodecError):
        codec.merged_wavefront(SHAPES, PAD, [None])
    with pytest.raises(codec.CodecError):
        codec.merged_wavefront([(2, 2)], PAD, [0])


# ---- decompress_images: what it refuses before the GPU is touched -------------------------------------------
HEAD = dict(family=1, M=16, K=1, z_lo=-32, z_S=65, y_W=24, B=1, H=70, W=100, top=0, left=0)
STATES = struct.pack("<64I", *([1 << 16] * 64))


@pytest.fixture(scope="module")
def cc(codec):
    import neural_image_compression_amd as nic
    return codec.ContextCodec(nic.JointAutoregressiveHierarchical(16, 1), coder="rans")      # on the CPU: no GPU needed


def _rans(codec, **head):
    return codec.pack_bitstream_rans(dict(HEAD, **head), b"z", [STATES], [b""], [0])


def _grouped(codec, G, **head):
    return codec.pack_bitstream_grouped(dict(HEAD, **head), b"z", [STATES] * G, [b""] * G, [0], G)


def test_an_empty_list_is_an_empty_list(cc):
    assert cc.decompress_images([]) == [] and cc.decompress_images(()) == []


def test_a_range_coded_blob_in_the_list_is_refused_by_its_index(codec, cc):
    b1 = codec.pack_bitstream(HEAD, b"z", [b"y"], [0])
    with pytest.raises(codec.CodecError, match=r"^blob 2: .*LICBITS1"):
        cc.decompress_images([_rans(codec), _grouped(codec, 1), b1, _rans(codec)])
    with pytest.raises(codec.CodecError, match=r"^blob 0: .*LICBITS1"):
        cc.decompress_images([b1])


def test_windows_that_differ_are_refused(codec, cc):
    with pytest.raises(codec.CodecError, match=r"^blob 1: y_W = 32, blob 0 has y_W = 24"):
        cc.decompress_images([_rans(codec), _rans(codec, y_W=32)])


def test_group_counts_that_differ_are_refused(codec, cc):
    with pytest.raises(codec.CodecError, match=r"^blob 2: G = 2 .*blob 0 has G = 1"):
        cc.decompress_images([_rans(codec), _grouped(codec, 1), _grouped(codec, 2)])
    sliced = codec.pack_bitstream_sliced(HEAD, b"z", [STATES] * 4, [b""] * 4, [0], 4, 8)
    with pytest.raises(codec.CodecError, match=r"^blob 1: G = 1 .*blob 0 has G = 4"):
        cc.decompress_images([sliced, _rans(codec)])


def test_the_window_is_judged_before_the_groups_and_licbits1_before_both(codec, cc):
    b1 = codec.pack_bitstream(HEAD, b"z", [b"y"], [0])
    with pytest.raises(codec.CodecError, match=r"^blob 1: y_W = 32"):
        cc.decompress_images([_rans(codec), _grouped(codec, 2, y_W=32)])
    with pytest.raises(codec.CodecError, match=r"^blob 2: .*LICBITS1"):
        cc.decompress_images([_rans(codec), _grouped(codec, 2, y_W=32), b1])


def test_what_one_blob_is_refused_for_names_the_blob(codec, cc):
    good = _rans(codec)
    at = len(good) - 10                                                           # a state byte: the trailing CRC fails
    damaged = good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:]
    with pytest.raises(codec.CodecError) as single:
        cc.decompress_image(damaged)
    assert "CRC-32" in str(single.value)
    with pytest.raises(codec.CodecError) as many:
        cc.decompress_images([good, damaged, good])
    assert str(many.value) == "blob 1: " + str(single.value)
    # the model check and the window limit are decompress_image's too, with the index in front
    for bad in (_rans(codec, M=32), _rans(codec, K=3), _rans(codec, family=2), _rans(codec, y_W=65), good[:-1], b""):
        with pytest.raises(codec.CodecError) as single:
            cc.decompress_image(bad)
        with pytest.raises(codec.CodecError) as many:
            cc.decompress_images([good, good, bad])
        assert str(many.value) == "blob 2: " + str(single.value)
    # the first bad blob speaks, before any rule of the call as a whole
    with pytest.raises(codec.CodecError, match=r"^blob 1: .*CRC-32"):
        cc.decompress_images([good, damaged, codec.pack_bitstream(HEAD, b"z", [b"y"], [0]), b""])
