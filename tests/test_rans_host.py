"""The "rANS-64" y-stream coder on the host (include/lic_codec.h): the C++ encoder against the plain Python
restatement (tests/rans_ref.py) byte for byte, the C++ decoder as its inverse, the round rule at every step
length that takes another path, extreme frequencies, escapes, damaged streams, the LICBITS2 container, the
stream size, and the device entry's argument check.  CPU only."""
import struct
import zlib

import numpy as np
import pytest

import rans_ref as RR
from oracle import codec_ref as CR


@pytest.fixture(scope="module")
def codec():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec as CD
    return CD


def _tables(r, T, S):
    """random valid tables: positive frequencies summing to 65536"""
    f = r.gamma(0.3, 1.0, size=(T, S)) + 1e-9
    f = f / f.sum(1, keepdims=True)
    F = np.concatenate([np.zeros((T, 1)), np.cumsum(f, 1)], 1)
    F[:, -1] = 1.0
    return CR.quantize_cdf(F)


def _draw(r, t):
    """one symbol per table, drawn from it"""
    u = r.randint(0, 65536, size=t.shape[0])
    return np.array([np.searchsorted(t[i], u[i], side="right") - 1 for i in range(t.shape[0])], np.int32)


def _both_ways(codec, t, idx, steps):
    data, esc = codec.rans_encode(t, idx, steps)
    ref_data, ref_esc = RR.encode(t, idx, steps)
    assert data == ref_data, "C++ and Python encoders must emit identical bytes"
    assert esc == ref_esc
    assert (codec.rans_decode(data, esc, t, steps) == idx).all()
    assert (RR.decode(data, esc, t, steps) == idx).all()
    return data, esc


@pytest.mark.parametrize("steps", [[1], [63], [64], [65], [32, 96, 327, 1], []])
def test_encoder_matches_restatement_and_decoder_inverts_it(codec, steps):
    r = np.random.RandomState(11)
    S, n = 49, int(sum(steps))
    t = _tables(r, n, S) if n else np.zeros((0, S + 1), np.uint32)
    idx = _draw(r, t) if n else np.zeros(0, np.int32)
    data, esc = _both_ways(codec, t, idx, steps)
    assert len(data) >= 256 and len(data) % 2 == 0
    if n == 0:
        assert data == struct.pack("<64I", *([1 << 16] * 64)) and esc == b""
    # the same symbols under another split of the steps give another stream: the round rule is part of the format
    if steps == [65]:
        other, _ = codec.rans_encode(t, idx, [64, 1])
        assert other == RR.encode(t, idx, [64, 1])[0]
        assert (codec.rans_decode(other, esc, t, [64, 1]) == idx).all()


def test_extreme_frequencies(codec):
    """tables whose symbols have frequency 1 except one with 65536 - (S-1), coded at both kinds of symbol"""
    S, n = 49, 400
    r = np.random.RandomState(12)
    big = r.randint(0, S, size=n)
    t = np.zeros((n, S + 1), np.uint32)
    for i in range(n):
        f = np.ones(S, np.int64)
        f[big[i]] = 65536 - (S - 1)
        t[i, 1:] = np.cumsum(f)
    assert (t[:, -1] == 65536).all()
    idx = np.where(r.rand(n) < 0.5, big, r.randint(1, S - 1, size=n)).astype(np.int32)
    freq = t[np.arange(n), idx + 1] - t[np.arange(n), idx]
    assert (freq == 1).sum() > 50 and (freq == 65536 - (S - 1)).sum() > 50
    _both_ways(codec, t, idx, [100, 300])
    _both_ways(codec, t, np.clip(big, 1, S - 2).astype(np.int32), [n])      # almost free symbols: hardly any words


def test_escapes_at_both_edges(codec):
    r = np.random.RandomState(13)
    S, steps = 17, [70, 130, 1]
    n = sum(steps)
    t = _tables(r, n, S)
    idx = r.randint(1, S - 1, size=n).astype(np.int32)
    forced = [0, -1, -100000, S - 1, S, S - 1 + 100000]                       # excess 0, 1, 100000 at each edge
    at = r.choice(n, size=len(forced) * 3, replace=False)
    for j, i in enumerate(at):
        idx[i] = forced[j % len(forced)]
    data, esc = _both_ways(codec, t, idx, steps)
    assert len(esc) == 4 * len(at)
    want = [(-v if v <= 0 else v - (S - 1)) for v in idx if v <= 0 or v >= S - 1]
    assert list(struct.unpack("<%dI" % len(at), esc)) == want                    # symbol order, 32 bits each
    assert abs(codec.rans_ideal_bits(t, idx) - RR.ideal_bits(t, idx)) < 1e-6 * RR.ideal_bits(t, idx)


def test_damaged_streams_are_reported(codec):
    r = np.random.RandomState(14)
    S, steps = 33, [200, 77, 500]
    n = sum(steps)
    t = _tables(r, n, S)
    idx = _draw(r, t)
    idx[::50] = S + 5
    data, esc = codec.rans_encode(t, idx, steps)
    assert len(esc) >= 4
    lib = codec._codec()
    assert lib.lic_rans_decode(None, 0, None, 0, None, S, 0, None, 0, None) == -1

    def status(d, e):
        buf, eb = np.frombuffer(d, np.uint8), np.frombuffer(e, np.uint32)
        out, st = np.empty(n, np.int32), np.array(steps, np.int64)
        return lib.lic_rans_decode(codec._p(buf, codec.C.c_uint8), buf.size, codec._p(eb, codec.C.c_uint32), eb.size,
                                   codec._p(t, codec.C.c_uint32), S, n, codec._p(st, codec.C.c_int64), st.size,
                                   codec._p(out, codec.C.c_int32))
    CORRUPT = -3
    assert status(data, esc) == 0
    assert status(data[:-2], esc) == CORRUPT                                      # cut by one word
    assert status(data + b"\x00\x00", esc) == CORRUPT                             # one word appended
    assert status(data, esc[:-4]) == CORRUPT                                      # escape list one entry short
    assert status(data, esc + b"\x00\x00\x00\x00") == CORRUPT                     # and one too many
    assert status(data[:100], esc) == CORRUPT                                     # not even the states
    with pytest.raises(codec.CodecError):
        codec.rans_decode(data[:-2], esc, t, steps)
    for bad, e in ((data[:-2], esc), (data + b"\x00\x00", esc), (data, esc[:-4])):
        with pytest.raises(RR.Corrupt):
            RR.decode(bad, e, t, steps)


def test_stream_size_against_the_ideal(codec):
    """One fixed input of 60 000 symbols (S = 65) drawn from its own tables, in steps of 6144 symbols and two shorter
    ones with partial last rounds.  1794 of the drawn symbols are edge symbols, whose excess (0) costs 32 bits each in
    the escape list; ideal_bits counts those 32 bits, so the size compared is stream + escape list.
    Measured with tests/rans_ref.py (not the code under test): stream 276 000 bits + escapes 57 408 bits = 333 408
    bits against ideal_bits + 2048 = 333 713.1: the measured excess is -305.1 bits, i.e. none -- the 64 flushed states
    (2048 bits) carry part of the payload, which more than pays for the coding loss of this input.  Twice an excess
    of zero is zero: the host encoder's stream + escapes must not exceed ideal_bits + 2048."""
    measured_excess = 0.0                                     # max(0, -305.1), see above
    r = np.random.RandomState(15)
    S, n = 65, 60000
    steps = [6144] * 9 + [4000, 704]
    assert sum(steps) == n
    t = _tables(r, n, S)
    idx = _draw(r, t)
    ideal = RR.ideal_bits(t, idx)
    ref = RR.encode(t, idx, steps)
    ref_bits = 8 * (len(ref[0]) + len(ref[1]))
    print(f"restatement: {8 * len(ref[0])} + {8 * len(ref[1])} bits, ideal + 2048 = {ideal + 2048:.1f}, "
          f"excess {ref_bits - (ideal + 2048):.1f}")
    data, esc = codec.rans_encode(t, idx, steps)
    print(f"host encoder: {8 * len(data)} + {8 * len(esc)} bits")
    assert abs(codec.rans_ideal_bits(t, idx) - ideal) < 1e-6 * ideal
    assert 8 * (len(data) + len(esc)) - (ideal + 2048) <= 2 * measured_excess


# ---- container ----------------------------------------------------------------------------------
_HEAD = {"family": 1, "M": 32, "K": 3, "z_lo": -32, "z_S": 65, "y_W": 24, "B": 2, "H": 70, "W": 100, "top": 0,
         "left": 0}


def _blob(codec, lanes=64):
    ys = [bytes(range(256)) + b"ab", bytes(256)]
    es = [struct.pack("<2I", 7, 100000), b""]
    return codec.pack_bitstream_rans(_HEAD, b"zzzzz", ys, es, [0x12345678, 0x9ABCDEF0], lanes=lanes), ys, es


def test_licbits2_round_trip(codec):
    blob, ys, es = _blob(codec)
    assert blob[:8] == b"LICBITS2"
    head, z, y2, e2, crc = codec.unpack_bitstream_rans(blob)
    assert head == _HEAD and z == b"zzzzz" and y2 == ys and e2 == es and crc == [0x12345678, 0x9ABCDEF0]
    # layout: the LICBITS1 header, then lanes; 12-byte rows; each escape list behind its stream
    assert struct.unpack_from("<I", blob, 56)[0] == 64
    assert struct.unpack_from("<III", blob, 60) == (258, 0x12345678, 2)
    assert len(blob) == 60 + 2 * 12 + 5 + 258 + 8 + 256 + 4
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == zlib.crc32(blob[:-4]) & 0xFFFFFFFF


def test_licbits2_damage_is_reported(codec):
    blob, _, _ = _blob(codec)
    flipped = bytearray(blob)
    flipped[100] ^= 0x40
    for bad in (bytes(flipped), blob[:-1], blob[:70], blob[:20], blob + b"\x00"):
        with pytest.raises(codec.CodecError):
            codec.unpack_bitstream_rans(bad)
    wide, _, _ = _blob(codec, lanes=128)                       # a valid container of an interleaving not implemented
    with pytest.raises(codec.CodecError, match="128"):
        codec.unpack_bitstream_rans(wide)
    with pytest.raises(codec.CodecError):
        codec.unpack_bitstream(blob)                           # the old function does not take the new magic
    with pytest.raises(codec.CodecError):
        codec.unpack_bitstream_rans(codec.pack_bitstream(_HEAD, b"z", [b"a", b"b"], [1, 2]))


def test_licbits1_still_unpacks(codec):
    blob = codec.pack_bitstream(_HEAD, b"zzzzz", [b"abc", b"defg"], [1, 2])
    assert blob[:8] == b"LICBITS1"
    head, z, ys, crc = codec.unpack_bitstream(blob)
    assert head == _HEAD and z == b"zzzzz" and ys == [b"abc", b"defg"] and crc == [1, 2]


def test_unknown_coder_is_refused(codec):
    with pytest.raises(codec.CodecError):
        codec.ContextCodec(None, coder="huffman")


def test_decode_step_rejects_null_pointers_without_a_gpu():
    from neural_image_compression_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    assert L.lic_rans_decode_step(None, None, None, None, None, None, None, None, 1, 1, 32, 24, None, None, 16,
                                  None) == -1
