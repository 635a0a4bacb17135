"""The self-describing container of ContextCodec.compress_image: host-only packing, no GPU."""
import struct
import zlib

import pytest

from neural_image_compression_amd import codec as CD

HEAD = dict(family=2, M=192, K=3, z_lo=-64, z_S=129, y_W=32, B=3, H=375, W=500, top=4, left=6)
Z = bytes(range(7))
YS = [bytes([1, 2, 3]), b"", bytes(range(50, 91))]
CRCS = [0xDEADBEEF, 0, 12345]


def _packed():
    return CD.pack_bitstream(HEAD, Z, YS, CRCS)


def test_pack_unpack_reproduces_every_field():
    data = _packed()
    assert data[:8] == b"LICBITS1"
    assert len(data) == 8 + 12 * 4 + 3 * 8 + len(Z) + sum(map(len, YS)) + 4
    assert struct.unpack_from("<I", data, len(data) - 4)[0] == zlib.crc32(data[:-4]) & 0xFFFFFFFF
    head, z, ys, crcs = CD.unpack_bitstream(data)
    assert head == HEAD and z == Z and ys == YS and crcs == CRCS
    neg = dict(HEAD, z_lo=-200, top=0, left=0, B=1)
    assert CD.unpack_bitstream(CD.pack_bitstream(neg, b"", [b"x"], [7]))[0] == neg


def _with_crc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def test_damage_is_refused():
    data = _packed()
    flipped_magic = bytes([data[0] ^ 0x20]) + data[1:]
    with pytest.raises(CD.CodecError, match="magic"):
        CD.unpack_bitstream(flipped_magic)
    with pytest.raises(CD.CodecError):
        CD.unpack_bitstream(data[:-1])
    with pytest.raises(CD.CodecError):
        CD.unpack_bitstream(data[:20])
    with pytest.raises(CD.CodecError):
        CD.unpack_bitstream(data + b"\0")
    at = 8 + 12 * 4 + 3 * 8 + 2                                   # a payload byte
    one_bit = data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    with pytest.raises(CD.CodecError, match="CRC"):
        CD.unpack_bitstream(one_bit)
    m_changed = data[:12] + struct.pack("<I", 128) + data[16:]    # M sits after magic and family
    with pytest.raises(CD.CodecError):
        CD.unpack_bitstream(m_changed)
    with pytest.raises(CD.CodecError):
        CD.pack_bitstream(HEAD, Z, YS[:2], CRCS)


def test_a_well_formed_stream_of_another_model_is_refused_before_the_gpu():
    """header M changed AND the CRC recomputed: only the model check can catch it; it runs before any GPU work, so
    this passes on a machine without one"""
    import neural_image_compression_amd as nic
    model = nic.JointAutoregressiveHierarchical(16, 1)
    codec = CD.ContextCodec(model)
    ok = dict(HEAD, family=1, M=16, K=1, B=1)
    for wrong in (dict(ok, M=32), dict(ok, K=3), dict(ok, family=2)):
        with pytest.raises(CD.CodecError, match="this model"):
            codec.decompress_image(CD.pack_bitstream(wrong, b"z", [b"y"], [0]))
    body = _packed()[:-4]
    with pytest.raises(CD.CodecError):
        codec.decompress_image(_with_crc(body[:30] + body[31:]))
