"""Codec slices without a GPU: the schedule `codec.wavefront` against the slice rule restated in ctx_slices_ref.py
(every pixel once, every live tap strictly earlier, nothing the rule kills needed or read, the step count, R >= h is
the schedule the codec always had), the LICBITS4 container, and the constructor's refusals."""
import struct
import zlib

import numpy as np
import pytest

import ctx_slices_ref as SR
import test_bitstream_golden as BG

SHAPES = [(1, 1), (1, 5), (4, 4), (5, 7), (8, 12)]
CASES = [(h, w, R) for h, w in SHAPES for R in (1, 2, 3, h, h + 1)]


@pytest.fixture(scope="module")
def codec():
    from neural_image_compression_amd import codec as CD
    return CD


def _codec_without_model(codec):
    cc = object.__new__(codec.ContextCodec)
    cc.pad = SR.PAD
    return cc


@pytest.mark.parametrize("h,w,R", CASES)
def test_schedule_follows_the_slice_rule(codec, h, w, R):
    steps = codec.wavefront(h, w, SR.PAD, R)
    assert SR.same_schedule(steps, SR.schedule(h, w, R))
    assert SR.same_schedule(steps, _codec_without_model(codec)._wavefront(h, w, R))
    assert len(steps) == SR.n_steps(h, w, R)
    step = -np.ones((h, w), np.int64)
    for t, (ii, jj) in enumerate(steps):
        assert ii.dtype == jj.dtype == np.int64 and (np.diff(ii) > 0).all()
        assert (step[ii, jj] == -1).all()                       # every pixel in exactly one step
        step[ii, jj] = t
    assert (step >= 0).all()
    killed_and_later = 0
    for i in range(h):
        for j in range(w):
            for dr, ds in SR.TAPS:
                a, b = i + dr, j + ds
                if SR.tap_live(i, j, dr, ds, h, w, R):
                    assert step[a, b] < step[i, j]              # a live tap is decoded before it is read
                elif 0 <= a < h and 0 <= b < w:
                    # a tap the rule kills lies in another slice: it may be decoded later than the pixel, so reading
                    # it would be wrong, and with more than one slice some really are
                    assert a // R != i // R and dr < 0
                    killed_and_later += step[a, b] >= step[i, j]
    if (h, w, R) == (8, 12, 2):
        assert killed_and_later > 0


@pytest.mark.parametrize("h,w,R", CASES)
def test_killed_taps_are_not_read(h, w, R):
    """the gather's restatement on a plane without a zero in it: a window entry is zero exactly where the rule kills
    the tap, and the value of the tap's pixel elsewhere"""
    M = 3
    y = (1.0 + np.arange(2 * h * w * M, dtype=np.float32)).reshape(2, h, w, M)
    win, _ = SR.gather(y, R, list(range(h * w)))
    win = win.reshape(2, h, w, len(SR.TAPS), M)
    for i in range(h):
        for j in range(w):
            for t, (dr, ds) in enumerate(SR.TAPS):
                killed = not (0 <= i + dr < h and 0 <= j + ds < w) or (dr < 0 and (i % R) + dr < 0)
                if killed:
                    assert (win[:, i, j, t] == 0).all()
                else:
                    assert np.array_equal(win[:, i, j, t], y[:, i + dr, j + ds])


@pytest.mark.parametrize("h,w", SHAPES + [(32, 48), (7, 3), (3, 1)])
def test_one_slice_is_the_schedule_the_codec_always_had(codec, h, w):
    old = SR.unsliced_schedule(h, w)
    cc = _codec_without_model(codec)
    assert SR.same_schedule(cc._wavefront(h, w), old)
    for R in (h, h + 1, 10 * h):
        assert SR.same_schedule(codec.wavefront(h, w, SR.PAD, R), old)
        assert SR.same_schedule(cc._wavefront(h, w, R), old)


def test_step_counts_of_the_kodak_size_latent(codec):
    assert [len(codec.wavefront(32, 48, 2, R)) for R in (None, 16, 8, 4)] == [141, 93, 69, 57]


@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "4"])
def test_bad_slice_heights_are_refused(codec, bad):
    with pytest.raises(codec.CodecError, match="slice_rows"):
        codec.wavefront(4, 4, 2, bad)
    with pytest.raises(codec.CodecError, match="slice_rows"):
        codec.ContextCodec(BG._stub_model(), coder="rans", slice_rows=bad)


def test_slices_need_the_rans_coder(codec):
    with pytest.raises(codec.CodecError, match="needs coder='rans'"):
        codec.ContextCodec(BG._stub_model(), slice_rows=4)
    with pytest.raises(codec.CodecError, match="needs coder='rans'"):
        codec.ContextCodec(BG._stub_model(), coder="range", slice_rows=4)
    for enc in ("host", "device"):
        for G in (1, 4):
            assert codec.ContextCodec(BG._stub_model(), coder="rans", encoder=enc, groups=G, slice_rows=4).slice_rows == 4
    assert codec.ContextCodec(BG._stub_model(), coder="rans").slice_rows is None


# ---- LICBITS4 -------------------------------------------------------------------------------------
HEAD2 = dict(family=1, M=32, K=3, z_lo=-32, z_S=65, y_W=24, B=2, H=70, W=100, top=0, left=0)    # 8 latent rows
CRC2 = [0x12345678, 0x9ABCDEF0]


@pytest.mark.parametrize("G,R", [(1, 1), (1, 3), (4, 3), (4, 8), (8, 4000000000)])
def test_licbits4_packs_and_unpacks(codec, G, R):
    """R = 3 leaves the 8 latent rows of a 70 x 100 image a ragged last slice; the container is LICBITS3's with the
    magic changed and one word behind `lanes`"""
    ys, es = BG._subs(2 * G)
    blob = codec.pack_bitstream_sliced(HEAD2, b"zzzzz", ys, es, CRC2, G, R)
    assert blob[:8] == b"LICBITS4" == codec.BITSTREAM_MAGIC_SLICED
    head, z, ys2, es2, crcs, groups, rows = codec.unpack_bitstream_sliced(blob)
    assert (z, ys2, es2, crcs, groups, rows) == (b"zzzzz", ys, es, CRC2, G, R)
    assert head == dict(HEAD2, slice_rows=R)
    g3 = codec.pack_bitstream_grouped(HEAD2, b"zzzzz", ys, es, CRC2, G)
    body = b"LICBITS4" + g3[8:60] + struct.pack("<I", R) + g3[60:-4]
    assert blob == body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)
    assert struct.unpack_from("<I", blob, 56)[0] == 64 * G


def test_licbits4_refuses_damage(codec):
    ys, es = BG._subs(4)
    blob = codec.pack_bitstream_sliced(HEAD2, b"zzzzz", ys, es, CRC2, 2, 3)
    u = codec.unpack_bitstream_sliced
    for at in list(range(0, 96)) + [len(blob) // 2, len(blob) - 5, len(blob) - 1]:
        with pytest.raises(codec.CodecError):
            u(BG._flip(blob, at, 0x10))                               # any flipped byte: magic, length or CRC-32
    for cut in (blob[:-1], blob[:63], blob[:70], blob[:20], b"", blob + b"\0"):
        with pytest.raises(codec.CodecError, match="truncated"):
            u(cut)
    with pytest.raises(codec.CodecError, match="slice_rows = 0"):
        u(BG._patched(blob, 60, 0))
    assert u(BG._patched(blob, 60, 5))[6] == 5
    for lanes in (0, 96, 576):
        with pytest.raises(codec.CodecError, match="interleaves"):
            u(BG._patched(blob, 56, lanes))
    with pytest.raises(codec.CodecError, match="shorter than its 64 states"):
        u(codec.pack_bitstream_sliced(HEAD2, b"z", [bytes(255)] + ys[1:], es, CRC2, 2, 3))
    for bad in (0, -3, None, 2.0, 1 << 32):
        with pytest.raises(codec.CodecError, match="slice_rows"):
            codec.pack_bitstream_sliced(HEAD2, b"zzzzz", ys, es, CRC2, 2, bad)
    with pytest.raises(codec.CodecError):
        codec.pack_bitstream_sliced(HEAD2, b"zzzzz", ys[:3], es[:3], CRC2, 2, 3)
    # every reader refuses every other format's magic
    g3 = codec.pack_bitstream_grouped(HEAD2, b"zzzzz", ys, es, CRC2, 2)
    with pytest.raises(codec.CodecError, match="not a LICBITS4"):
        u(g3)
    for reader in (codec.unpack_bitstream, codec.unpack_bitstream_rans, codec.unpack_bitstream_grouped):
        with pytest.raises(codec.CodecError, match="bad magic"):
            reader(blob)


def test_the_older_containers_parse_to_the_same_fields(codec):
    """the pinned LICBITS1/2/3 bytes still read back to their inputs, none gains a slice_rows field, and the format
    table maps four magics"""
    import json
    with open(BG.FIXTURE) as f:
        golden = json.load(f)["containers"]
    for name, case in BG.CASES.items():
        blob = bytes.fromhex(golden[name])
        assert BG.pack(case) == blob
        got = BG.unpack(case[0], blob)
        assert got == BG._unpacked(case) and "slice_rows" not in got[0]
    assert codec._FORMAT_OF_MAGIC == {b"LICBITS1": ("range", False), b"LICBITS2": ("rans", False),
                                      b"LICBITS3": ("rans", True), b"LICBITS4": ("rans", "sliced")}


def test_decompress_image_reads_licbits4_from_its_header_alone(codec):
    """a codec built without slice arguments takes the container as far as the checks that need a model: a stub model
    is no family, a real one of another shape is named"""
    states = struct.pack("<64I", *([1 << 16] * 64))
    one = dict(HEAD2, B=1)
    blob = codec.pack_bitstream_sliced(one, b"z", [states] * 2, [b""] * 2, [0], 2, 4)
    with pytest.raises(codec.CodecError, match="no bitstream family id"):
        codec.ContextCodec(BG._stub_model()).decompress_image(blob)
    with pytest.raises(codec.CodecError, match="y_W = 100"):
        codec.ContextCodec(BG._stub_model()).decompress_image(
            codec.pack_bitstream_sliced(dict(one, y_W=100), b"z", [states], [b""], [0], 1, 4))
    with pytest.raises(codec.CodecError, match="slice_rows = 0"):
        codec.ContextCodec(BG._stub_model()).decompress_image(BG._patched(blob, 60, 0))
    import neural_image_compression_amd as nic
    cc = codec.ContextCodec(nic.JointAutoregressiveHierarchical(16, 1))
    with pytest.raises(codec.CodecError, match="written by family 1 with M=32, K=3"):
        cc.decompress_image(blob)
    with pytest.raises(codec.CodecError, match="written by family 2"):
        cc.decompress_image(codec.pack_bitstream_sliced(dict(one, family=2, M=16, K=1), b"z", [states], [b""], [0], 1, 4))
