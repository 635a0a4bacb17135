"""LICBITS5, the container of a codec with z_coder="rans": round trips for G in {1, 3} with and without slices, the
trailing CRC-32 against every single-byte flip, the reader's refusals, a byte pin (tests/golden/bitstream_licbits5.json)
and the four older formats' pinned blobs read through the same reader as before.  Host only.

Regenerating the pin, only for a deliberate change of the format:  python tests/test_bitstream_zrans.py"""
import json
import os
import struct
import zlib

import pytest

from neural_image_compression_amd import bitstream as BS
from neural_image_compression_amd import codec as CD

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = os.path.join(HERE, "golden", "bitstream_licbits5.json")
HEAD = dict(family=1, M=8, K=1, z_lo=-1, z_S=4, y_W=32, B=2, H=100, W=75, top=0, left=0)
CRCS = [0xDEADBEEF, 12345]
HEAD_BYTES = 8 + 14 * 4


def _blocks(n, seed):
    """n sub-streams (256 bytes, 258, longer, ...) and escape lists (some empty)"""
    ys = [bytes((seed + i + k) % 256 for k in range(256 + 2 * ((i * 7) % 5))) for i in range(n)]
    es = [struct.pack("<%dI" % (i % 3), *[seed + i, 1 << 31][:i % 3]) for i in range(n)]
    return ys, es


def _case(G, R):
    zs, zes = _blocks(2 * G, 3)
    ys, es = _blocks(2 * G, 90)
    return zs, zes, ys, es


def _reseal(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)


@pytest.mark.parametrize("R", (0, 2))
@pytest.mark.parametrize("G", (1, 3))
def test_round_trip(G, R):
    zs, zes, ys, es = _case(G, R)
    blob = CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, G, R)
    assert blob[:8] == b"LICBITS5" == CD.BITSTREAM_MAGIC_ZRANS
    vals = struct.unpack_from("<3I", blob, HEAD_BYTES - 12)                       # z-section length, lanes, slice_rows
    z_section = 8 * 2 * G + sum(map(len, zs)) + sum(map(len, zes))
    assert vals == (z_section, 64 * G, R)
    assert len(blob) == HEAD_BYTES + 4 * 2 + 8 * 2 * G + z_section + sum(map(len, ys)) + sum(map(len, es)) + 4
    assert CD.unpack_bitstream_zrans(blob) == (HEAD if R == 0 else dict(HEAD, slice_rows=R), zs, zes, ys, es, CRCS, G,
                                               R or None)
    assert CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, G, None if R == 0 else R) == blob
    # the z section: block table, then every block's stream followed by its escape list
    at = HEAD_BYTES + 4 * 2 + 8 * 2 * G
    assert struct.unpack_from("<%dI" % (4 * G), blob, at) == tuple(v for s, e in zip(zs, zes) for v in (len(s), len(e) // 4))
    assert blob[at + 8 * 2 * G:at + z_section] == b"".join(p for s, e in zip(zs, zes) for p in (s, e))


def test_every_single_byte_flip_is_caught():
    zs, zes, ys, es = _case(1, 2)
    blob = CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, 1, 2)
    for at in range(len(blob)):
        with pytest.raises(CD.CodecError):
            CD.unpack_bitstream_zrans(blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:])


def test_refusals():
    G = 3
    zs, zes, ys, es = _case(G, 0)
    blob = CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, G)
    body = bytearray(blob[:-4])
    with pytest.raises(CD.CodecError, match="magic"):
        CD.unpack_bitstream_zrans(b"LICBITS4" + blob[8:])
    for cut in (blob[:20], blob[:-1], blob + b"\0", blob[:HEAD_BYTES + 10]):
        with pytest.raises(CD.CodecError, match="truncated"):
            CD.unpack_bitstream_zrans(cut)
    lanes = HEAD_BYTES - 8
    for bad in (0, 32, 96, 64 * 9):
        with pytest.raises(CD.CodecError, match="interleaves"):
            CD.unpack_bitstream_zrans(_reseal(body[:lanes] + struct.pack("<I", bad) + body[lanes + 4:]))
    ztab = HEAD_BYTES + 4 * 2 + 8 * 2 * G                                         # where the z section starts
    old = struct.unpack_from("<I", body, HEAD_BYTES - 12)[0]

    def with_section(rows, payload_bytes):
        """the blob with another z section: any block table, `payload_bytes` bytes behind it"""
        sec = b"".join(struct.pack("<2I", *r) for r in rows) + bytes(payload_bytes)
        out = bytearray(body[:ztab]) + sec + body[ztab + old:]
        struct.pack_into("<I", out, HEAD_BYTES - 12, len(sec))
        return _reseal(out)

    good = [(len(s), len(e) // 4) for s, e in zip(zs, zes)]
    total = sum(ln + 4 * ne for ln, ne in good)
    assert CD.unpack_bitstream_zrans(with_section(good, total))[6] == G           # the helper itself is sound
    with pytest.raises(CD.CodecError, match="z sub-stream shorter"):              # 252 bytes: fewer than 64 states
        CD.unpack_bitstream_zrans(with_section([(252, 1)] + good[1:], total - good[0][0] - 4 * good[0][1] + 256))
    with pytest.raises(CD.CodecError, match="odd length"):
        CD.unpack_bitstream_zrans(with_section([(257, 0)] + good[1:], total - good[0][0] - 4 * good[0][1] + 257))
    for off in (-4, 2, 4):                                                        # a section that does not add up
        with pytest.raises(CD.CodecError, match="add up"):
            CD.unpack_bitstream_zrans(with_section(good, total + off))
    with pytest.raises(CD.CodecError, match="z block table"):                     # shorter than its own table
        CD.unpack_bitstream_zrans(with_section(good[:2], 0))
    ytab = HEAD_BYTES + 4 * 2                                                     # LICBITS3's refusal for a y block
    y_short = bytearray(body)
    struct.pack_into("<I", y_short, ytab, 254)
    with pytest.raises(CD.CodecError):
        CD.unpack_bitstream_zrans(_reseal(y_short))
    # what the writer refuses
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream_zrans(HEAD, zs[:-1], zes[:-1], ys, es, CRCS, G)
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream_zrans(HEAD, zs, [e + b"\0" for e in zes], ys, es, CRCS, G)
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream_zrans(HEAD, b"one range stream", zes, ys, es, CRCS, G)
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, G, -1)


def _pinned_case():
    zs, zes, ys, es = _case(3, 2)
    return CD.pack_bitstream_zrans(HEAD, zs, zes, ys, es, CRCS, 3, 2)


def test_pinned_bytes():
    pin = json.load(open(PIN))
    assert _pinned_case().hex() == pin["licbits5_g3_r2_two_images"]
    zs, zes, ys, es = _case(3, 2)
    assert CD.unpack_bitstream_zrans(bytes.fromhex(pin["licbits5_g3_r2_two_images"])) == \
        (dict(HEAD, slice_rows=2), zs, zes, ys, es, CRCS, 3, 2)


def test_older_formats_read_as_before():
    """every pinned blob of LICBITS1 to 4 goes through `_unpack` by its magic and packs back to the same bytes"""
    import test_bitstream_golden as TG
    pinned = json.load(open(TG.FIXTURE))["containers"]
    seen = set()
    for name, case in TG.CASES.items():
        blob = bytes.fromhex(pinned[name])
        fmt = BS._FORMAT_OF_MAGIC[blob[:8]]
        seen.add(blob[:8])
        head, z, ys, es, crcs, G = BS._unpack(fmt, blob)
        assert TG.unpack(case[0], blob) == TG._unpacked(case)
        assert isinstance(z, bytes) and z == case[2] and head == case[1] and "slice_rows" not in head
        assert BS._pack(fmt, head, z, ys, es if fmt[0] == "rans" else None, crcs, G) == blob
    assert seen == {b"LICBITS1", b"LICBITS2", b"LICBITS3"}
    sliced = CD.pack_bitstream_sliced(HEAD, b"zz", *_blocks(2, 5), CRCS, 1, 3)
    assert sliced[:8] == b"LICBITS4" and CD.unpack_bitstream_sliced(sliced)[-1] == 3
    with pytest.raises(CD.CodecError, match="slice_rows"):                        # R = 0 stays a damaged LICBITS4 header
        CD.unpack_bitstream_sliced(_reseal(sliced[:HEAD_BYTES - 4] + struct.pack("<I", 0) + sliced[HEAD_BYTES:-4]))
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream_sliced(HEAD, b"zz", *_blocks(2, 5), CRCS, 1, 0)


if __name__ == "__main__":
    json.dump({"comment": "LICBITS5 as tests/test_bitstream_zrans.py::_pinned_case packs it",
               "licbits5_g3_r2_two_images": _pinned_case().hex()}, open(PIN, "w"), indent=1)
    print("wrote", PIN)
