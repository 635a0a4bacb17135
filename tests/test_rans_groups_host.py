"""The "rANS-64 x G" y streams on the host: codec.rans_deal against the plain restatement of the dealing rule
(tests/rans_groups_ref.py), grouped coding against the restatement byte for byte, the LICBITS3 container, the
constructor rules of ContextCodec(groups=...) and the two device entries' argument checks.  CPU only."""
import struct
import types
import zlib

import numpy as np
import pytest

import rans_groups_ref as GR
import rans_ref as RR

GROUPS = (1, 2, 3, 4, 8)
# partial rounds in non-zero groups, an empty step, fewer rounds than G, one symbol, a step of exactly 8 rounds
STEP_LISTS = ([32, 96, 327, 1, 0, 576, 64], [1], [0, 0, 5], [64 * 8])


@pytest.fixture(scope="module")
def codec():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec as CD
    return CD


@pytest.fixture(scope="module")
def images():
    return GR.synthetic_images()


# ---- dealing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("steps", STEP_LISTS, ids=lambda s: "-".join(map(str, s)))
def test_deal_matches_the_restatement(codec, steps, G):
    got, want = codec.rans_deal(steps, G), GR.deal(steps, G)
    assert len(got) == len(want) == G
    n = sum(steps)
    for (pos, lens), (rpos, rlens) in zip(got, want):
        assert pos.dtype == np.int64 and lens.dtype == np.int64
        assert pos.tolist() == rpos and lens.tolist() == rlens
        assert (np.diff(pos) > 0).all()                                      # order is kept
        assert len(lens) == len(steps) and lens.sum() == len(pos)
    every = np.concatenate([pos for pos, _ in got])
    assert sorted(every.tolist()) == list(range(n))                          # a partition of the positions
    assert (np.sum([lens for _, lens in got], axis=0) == np.array(steps)).all()
    if G == 1:
        assert got[0][0].tolist() == list(range(n)) and got[0][1].tolist() == list(steps)
    assert codec.rans_group_sizes(steps, G).tolist() == [len(rpos) for rpos, _ in want]


def test_deal_by_hand(codec):
    """327 symbols are rounds 0..5, the last of 7 symbols: with G = 4 round 5 lands in group 1"""
    lens = [l.tolist() for _, l in codec.rans_deal([32, 96, 327, 1], 4)]
    assert lens == [[32, 64, 128, 1], [0, 32, 64 + 7, 0], [0, 0, 64, 0], [0, 0, 64, 0]]
    pos = codec.rans_deal([32, 96, 327, 1], 4)[1][0]
    assert pos[:3].tolist() == [32 + 64, 32 + 65, 32 + 66] and pos[-1] == 128 + 326
    for bad in (0, 9, 2.5, "2"):
        with pytest.raises(codec.CodecError):
            codec.rans_deal([64], bad)


# ---- coding -------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
def test_grouped_encoder_matches_the_restatement(codec, images, G):
    tabs, idx = images
    S = tabs.shape[-1] - 1
    for b in range(3):
        streams, escs = codec.rans_encode_grouped(tabs[b], idx[b], GR.STEPS, G)
        assert len(streams) == len(escs) == G
        ref = GR.encode(tabs[b], idx[b], GR.STEPS, G)
        assert streams == ref[0], f"image {b}: a sub-stream differs from the restatement's"
        assert escs == ref[1], f"image {b}: an escape list differs"
        assert all(len(s) >= 256 and len(s) % 2 == 0 for s in streams)
        # every edge symbol's escape is in exactly one list
        assert sum(map(len, escs)) == 4 * int(((idx[b] <= 0) | (idx[b] >= S - 1)).sum())
        assert (codec.rans_decode_grouped(streams, escs, tabs[b], GR.STEPS) == idx[b]).all()
        assert (GR.decode(streams, escs, tabs[b], GR.STEPS) == idx[b]).all()
        if G == 1:
            one = codec.rans_encode(tabs[b], idx[b], GR.STEPS)
            assert (streams[0], escs[0]) == one


def test_short_images_leave_sub_streams_empty(codec, images):
    """fewer rounds than G: the sub-streams without a symbol are their 256 bytes of initial states"""
    tabs, idx = images
    streams, escs = codec.rans_encode_grouped(tabs[0][:100], idx[0][:100], [100], 8)
    empty = struct.pack("<64I", *([1 << 16] * 64))
    assert streams[2:] == [empty] * 6 and escs[2:] == [b""] * 6 and len(streams[0]) > 256
    assert (codec.rans_decode_grouped(streams, escs, tabs[0][:100], [100]) == idx[0][:100]).all()


def test_a_cut_sub_stream_is_reported(codec, images):
    tabs, idx = images
    streams, escs = codec.rans_encode_grouped(tabs[0], idx[0], GR.STEPS, 4)
    assert len(streams[2]) > 258
    cut = streams[:2] + [streams[2][:-2]] + streams[3:]
    with pytest.raises(codec.CodecError):
        codec.rans_decode_grouped(cut, escs, tabs[0], GR.STEPS)
    with pytest.raises(RR.Corrupt):
        GR.decode(cut, escs, tabs[0], GR.STEPS)
    with pytest.raises(codec.CodecError):
        codec.rans_decode_grouped(streams, escs[:3], tabs[0], GR.STEPS)


# ---- container ----------------------------------------------------------------------------------
_HEAD = {"family": 1, "M": 32, "K": 3, "z_lo": -32, "z_S": 65, "y_W": 24, "B": 2, "H": 70, "W": 100, "top": 0,
         "left": 0}
_CRC = [0x12345678, 0x9ABCDEF0]


def _parts(G=2):
    ys = [bytes(range(256)) + b"ab", bytes(256), bytes(256) + b"wxyz", bytes(256)] * (G // 2)
    es = [struct.pack("<2I", 7, 100000), b"", b"", struct.pack("<I", 1 << 31)] * (G // 2)
    return ys, es


def _blob(codec, G=2):
    ys, es = _parts(G)
    return codec.pack_bitstream_grouped(_HEAD, b"zzzzz", ys, es, _CRC, G), ys, es


def _reseal(body):
    """a container with `body` damaged on purpose but a trailing CRC that fits: only the named check can refuse it"""
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)


@pytest.mark.parametrize("G", [2, 4, 8])
def test_licbits3_round_trip_and_layout(codec, G):
    blob, ys, es = _blob(codec, G)
    assert blob[:8] == b"LICBITS3"
    head, z, y2, e2, crc, groups = codec.unpack_bitstream_grouped(blob)
    assert head == _HEAD and z == b"zzzzz" and y2 == ys and e2 == es and crc == _CRC and groups == G
    # the LICBITS1 header, z length, lanes; B checksums; B * G rows of (bytes, escape count); z; streams + escapes
    assert struct.unpack_from("<II", blob, 52) == (5, 64 * G)
    assert struct.unpack_from("<II", blob, 60) == tuple(_CRC)
    rows = 68
    assert struct.unpack_from("<II", blob, rows) == (258, 2) and struct.unpack_from("<II", blob, rows + 8) == (256, 0)
    assert struct.unpack_from("<II", blob, rows + 24) == (256, 1)
    at = rows + 8 * 2 * G
    assert blob[at:at + 5] == b"zzzzz" and blob[at + 5:at + 5 + 258] == ys[0] and blob[at + 263:at + 271] == es[0]
    assert len(blob) == at + 5 + sum(map(len, ys)) + sum(map(len, es)) + 4
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == zlib.crc32(blob[:-4]) & 0xFFFFFFFF


def test_licbits3_with_one_group(codec):
    """lanes = 64 is legal in this container; compress_image still writes LICBITS2 for groups = 1"""
    blob = codec.pack_bitstream_grouped(_HEAD, b"z", [bytes(256), bytes(258)], [b"", b"abcd"], _CRC, 1)
    assert codec.unpack_bitstream_grouped(blob)[2:] == ([bytes(256), bytes(258)], [b"", b"abcd"], _CRC, 1)


def test_licbits3_damage_is_reported(codec):
    blob, ys, es = _blob(codec)
    flipped = bytearray(blob)
    flipped[100] ^= 0x40
    for bad in (bytes(flipped), blob[:-1], blob[:70], blob[:20], blob + b"\x00"):
        with pytest.raises(codec.CodecError):
            codec.unpack_bitstream_grouped(bad)
    for lanes in (96, 576, 0):
        body = bytearray(blob[:-4])
        struct.pack_into("<I", body, 56, lanes)
        with pytest.raises(codec.CodecError, match=str(lanes)):
            codec.unpack_bitstream_grouped(_reseal(body))
    # a valid CRC and a consistent total length, but a sub-stream of 255 bytes, and one of odd length
    for n in (255, 257):
        short = codec.pack_bitstream_grouped(_HEAD, b"zzzzz", [bytes(n)] + ys[1:], es, _CRC, 2)
        with pytest.raises(codec.CodecError, match="sub-stream"):
            codec.unpack_bitstream_grouped(short)
    # a table row that promises more bytes than there are
    body = bytearray(blob[:-4])
    struct.pack_into("<I", body, 68, 1 << 30)
    with pytest.raises(codec.CodecError, match="length"):
        codec.unpack_bitstream_grouped(_reseal(body))
    # an inconsistent header under a valid CRC
    body = bytearray(blob[:-4])
    struct.pack_into("<I", body, 8 + 4 * 9, 64)                             # top = 64
    with pytest.raises(codec.CodecError, match="inconsistent"):
        codec.unpack_bitstream_grouped(_reseal(body))
    # packing refuses lists of the wrong length and groups outside 1..8
    with pytest.raises(codec.CodecError):
        codec.pack_bitstream_grouped(_HEAD, b"z", ys[:3], es[:3], _CRC, 2)
    with pytest.raises(codec.CodecError):
        codec.pack_bitstream_grouped(_HEAD, b"z", ys * 9, es * 9, _CRC, 18)


def test_each_unpacker_refuses_the_other_two_magics(codec):
    b3, ys, es = _blob(codec)
    b2 = codec.pack_bitstream_rans(_HEAD, b"zzzzz", ys[:2], es[:2], _CRC)
    b1 = codec.pack_bitstream(_HEAD, b"zzzzz", [b"abc", b"defg"], _CRC)
    assert (b1[:8], b2[:8], b3[:8]) == (b"LICBITS1", b"LICBITS2", b"LICBITS3")
    unpackers = (codec.unpack_bitstream, codec.unpack_bitstream_rans, codec.unpack_bitstream_grouped)
    for i, unpack in enumerate(unpackers):
        for j, blob in enumerate((b1, b2, b3)):
            if i == j:
                unpack(blob)
            else:
                with pytest.raises(codec.CodecError, match="magic"):
                    unpack(blob)


# ---- ContextCodec(groups=...) ------------------------------------------------------------------
def _stub_model():
    """what ContextCodec's constructor reads: a causal 5x5 mask (type A: the 12 taps before the centre)"""
    masked = types.SimpleNamespace(kernel_size=(5, 5), padding=(2, 2), _tap_mask=(1 << 12) - 1)
    return types.SimpleNamespace(context_model=types.SimpleNamespace(masked=masked))


def test_groups_argument_rules(codec):
    m = _stub_model()
    assert codec.RANS_MAX_GROUPS == 8
    assert codec.ContextCodec(m).groups == 1
    for coder in ("range", "rans"):
        assert codec.ContextCodec(m, coder=coder, groups=1).groups == 1
    for G in (2, 8):
        for encoder in ("host", "device"):
            assert codec.ContextCodec(m, coder="rans", encoder=encoder, groups=G).groups == G
    for bad in (0, 9, 2.5, -1, None):
        with pytest.raises(codec.CodecError, match="groups"):
            codec.ContextCodec(m, coder="rans", groups=bad)
    with pytest.raises(codec.CodecError, match="rans"):
        codec.ContextCodec(m, coder="range", groups=2)
    with pytest.raises(codec.CodecError):
        codec.ContextCodec(m, groups=2)                                     # the default coder is "range"


# ---- the device entries' argument checks --------------------------------------------------------
def test_group_entries_check_their_arguments_without_a_gpu():
    import os
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    assert _lib.RANS_MAX_GROUPS == 8
    INVALID, UNSUPPORTED = -1, -2
    p = 4096                                                               # an aligned non-null address, never used
    dec = lambda G, B=1, ptr=p: L.lic_rans_decode_step_groups(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, G, 1, 32, 24,
                                                              ptr, ptr, 16, None)
    assert dec(2, ptr=None) == INVALID
    assert dec(0) == INVALID and dec(9) == INVALID and dec(-1) == INVALID
    assert dec(2, B=0) == INVALID
    assert dec(8, B=8192) == UNSUPPORTED                                    # B * G above 65535
    assert L.lic_rans_decode_step_groups(p, p, p, p, p, p, p, p, 1, 2, 1, 32, 65, p, p, 16, None) == UNSUPPORTED
    enc = lambda G, B=1, ptr=p, slot=128, cap=64: L.lic_rans_encode_groups(ptr, ptr, ptr, 1, B, G, 64, ptr, slot, ptr,
                                                                          cap, ptr, None)
    assert enc(2, ptr=None) == INVALID
    assert enc(0) == INVALID and enc(9) == INVALID and enc(-1) == INVALID
    assert enc(2, B=0) == INVALID
    assert enc(2, slot=130) == INVALID and enc(2, slot=0) == INVALID        # whole dwords, at least one
    assert enc(2, cap=0) == INVALID
    assert enc(8, B=8192) == UNSUPPORTED
    assert L.lic_rans_encode_groups(p, p, p + 4, 1, 1, 2, 64, p, 128, p, 64, p, None) == INVALID   # step_len: 8-byte aligned
    assert L.lic_rans_encode_groups(p, p, p, 1, 1, 2, 1 << 31, p, 128, p, 64, p, None) == UNSUPPORTED
