"""Byte pins for the three containers of ContextCodec.compress_image (LICBITS1/2/3): the bitstream is a published
format, so a change meant to leave it alone must write the same bytes, read them back to the same values, and refuse
the same damage with the same words.  tests/golden/bitstream_containers.json holds, per case below, the packed bytes
(hex) and, per damage case, the CodecError message, as the commit named in its "comment" produced them.

Regenerating the fixture: only for a DELIBERATE change of a container or of a message.  On the tree whose output is to
be pinned run

    python tests/test_bitstream_golden.py COMMIT        (host only; keeps the fixture's other keys)

then commit the file with the change and say in the commit what moved and why.  The module uses the six public
pack_ / unpack_ functions, CodecError and ContextCodec.decompress_image only, so it runs unchanged on older trees."""
import json
import os
import struct
import types
import zlib

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bitstream_containers.json")

# the inputs of test_bitstream_container.py
HEAD = dict(family=2, M=192, K=3, z_lo=-64, z_S=129, y_W=32, B=3, H=375, W=500, top=4, left=6)
Z = bytes(range(7))
YS = [bytes([1, 2, 3]), b"", bytes(range(50, 91))]
CRCS = [0xDEADBEEF, 0, 12345]
ESCS = [b"", struct.pack("<I", 7), struct.pack("<3I", 1, 1 << 31, 100000)]           # 0, 4 and 12 bytes
NEG = dict(HEAD, z_lo=-200, top=0, left=0, B=1)


def _subs(n):
    """n sub-streams: exactly 256 bytes, 258 bytes, one longer, then 256 again; the second escape list is empty"""
    ys = [bytes(range(256)), bytes(256) + b"ab", bytes(range(255, -1, -1)) + bytes(range(46))] + [bytes(256)] * n
    es = [struct.pack("<2I", 7, 100000), b"", struct.pack("<I", 1 << 31)] + [struct.pack("<I", i) for i in range(n)]
    return ys[:n], es[:n]


# name -> (format, head, z, y streams, escape lists or None, checksums, groups or None)
CASES = {
    "licbits1": (1, HEAD, Z, YS, None, CRCS, None),
    "licbits1_neg_z_lo_one_image": (1, NEG, b"", [b"x"], None, [7], None),
    "licbits2": (2, HEAD, Z, YS, ESCS, CRCS, None),
    "licbits2_neg_z_lo_one_image": (2, NEG, b"", [b"x"], [b""], [7], None),
    "licbits3_g1": (3, HEAD, Z) + _subs(3) + (CRCS, 1),
    "licbits3_g3_one_image": (3, NEG, Z) + _subs(3) + ([7], 3),
    "licbits3_g8_one_image": (3, NEG, b"") + _subs(8) + ([0xFFFFFFFF], 8),
    "licbits3_g3_three_images": (3, HEAD, Z) + _subs(9) + (CRCS, 3),
}


def _codec():
    from neural_image_compression_amd import codec
    return codec


def pack(case):
    fmt, head, z, ys, es, crcs, G = case
    c = _codec()
    if fmt == 1:
        return c.pack_bitstream(head, z, ys, crcs)
    if fmt == 2:
        return c.pack_bitstream_rans(head, z, ys, es, crcs)
    return c.pack_bitstream_grouped(head, z, ys, es, crcs, G)


def unpack(fmt, blob):
    c = _codec()
    return (c.unpack_bitstream, c.unpack_bitstream_rans, c.unpack_bitstream_grouped)[fmt - 1](blob)


def _unpacked(case):
    """what the format's reader returns for the case's inputs"""
    fmt, head, z, ys, es, crcs, G = case
    return {1: (head, z, ys, crcs), 2: (head, z, ys, es, crcs), 3: (head, z, ys, es, crcs, G)}[fmt]


def _reseal(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)


def _patched(blob, at, value, reseal=True):
    body = bytearray(blob[:-4])
    struct.pack_into("<I", body, at, value)
    return _reseal(body) if reseal else bytes(body) + blob[-4:]


def _flip(blob, at, bit):
    return blob[:at] + bytes([blob[at] ^ bit]) + blob[at + 1:]


def _stub_model():
    """what ContextCodec's constructor reads; it is no model family, so a container that passes every check of its
    own is refused at the family check, before any GPU work"""
    masked = types.SimpleNamespace(kernel_size=(5, 5), padding=(2, 2), _tap_mask=(1 << 12) - 1)
    return types.SimpleNamespace(context_model=types.SimpleNamespace(masked=masked))


def damage_cases():
    """name -> callable that must raise CodecError: every damage case of test_bitstream_container.py,
    test_rans_host.py, test_rans_groups_host.py and test_rans_windows_host.py"""
    c = _codec()
    d = {}
    b1, b2 = pack(CASES["licbits1"]), pack(CASES["licbits2"])
    head2 = dict(family=1, M=32, K=3, z_lo=-32, z_S=65, y_W=24, B=2, H=70, W=100, top=0, left=0)
    crc2 = [0x12345678, 0x9ABCDEF0]
    ys3 = [bytes(range(256)) + b"ab", bytes(256), bytes(256) + b"wxyz", bytes(256)]
    es3 = [struct.pack("<2I", 7, 100000), b"", b"", struct.pack("<I", 1 << 31)]
    r1 = c.pack_bitstream(head2, b"zzzzz", [b"abc", b"defg"], crc2)
    r2 = c.pack_bitstream_rans(head2, b"zzzzz", ys3[:2], es3[:2], crc2)
    r3 = c.pack_bitstream_grouped(head2, b"zzzzz", ys3, es3, crc2, 2)
    blobs = {1: (b1, r1), 2: (b2, r2), 3: (None, r3)}
    for fmt in (1, 2, 3):
        own, r = blobs[fmt]
        u = lambda blob, fmt=fmt: (lambda: unpack(fmt, blob))
        for name, bad in (("flipped_magic", _flip(r, 0, 0x20)), ("flipped_payload_bit", _flip(r, len(r) - 6, 0x40)),
                          ("one_byte_short", r[:-1]), ("cut_at_70", r[:70]), ("cut_at_20", r[:20]),
                          ("one_byte_long", r + b"\0"), ("M_changed_crc_stale", _patched(r, 12, 128, reseal=False)),
                          ("top_64_resealed", _patched(r, 8 + 4 * 9, 64)), ("B_zero_resealed", _patched(r, 8 + 4 * 6, 0)),
                          ("first_row_too_long_resealed", _patched(r, {1: 56, 2: 60, 3: 68}[fmt], 1 << 30))):
            d[f"licbits{fmt}_{name}"] = u(bad)
        for other in (1, 2, 3):
            if other != fmt:
                d[f"licbits{fmt}_reader_given_licbits{other}"] = u(blobs[other][1])
    d["licbits1_payload_bit"] = lambda: c.unpack_bitstream(_flip(b1, 8 + 12 * 4 + 3 * 8 + 2, 1))
    d["licbits1_pack_two_streams_for_three_images"] = lambda: c.pack_bitstream(HEAD, Z, YS[:2], CRCS)
    d["licbits2_pack_two_escape_lists_for_three_images"] = lambda: c.pack_bitstream_rans(HEAD, Z, YS, ESCS[:2], CRCS)
    d["licbits2_pack_escape_list_of_5_bytes"] = lambda: c.pack_bitstream_rans(HEAD, Z, YS, [b"", b"12345", b""], CRCS)
    d["licbits2_lanes_128"] = lambda: c.unpack_bitstream_rans(
        c.pack_bitstream_rans(head2, b"zzzzz", ys3[:2], es3[:2], crc2, lanes=128))
    for lanes in (96, 576, 0):
        d[f"licbits3_lanes_{lanes}"] = lambda lanes=lanes: c.unpack_bitstream_grouped(_patched(r3, 56, lanes))
    for n in (255, 257):
        d[f"licbits3_sub_stream_of_{n}_bytes"] = lambda n=n: c.unpack_bitstream_grouped(
            c.pack_bitstream_grouped(head2, b"zzzzz", [bytes(n)] + ys3[1:], es3, crc2, 2))
    d["licbits3_pack_three_streams_for_two_by_two"] = lambda: c.pack_bitstream_grouped(head2, b"z", ys3[:3], es3[:3],
                                                                                        crc2, 2)
    d["licbits3_pack_18_groups"] = lambda: c.pack_bitstream_grouped(head2, b"z", ys3 * 9, es3 * 9, crc2, 18)
    d["licbits3_pack_escape_list_of_5_bytes"] = lambda: c.pack_bitstream_grouped(head2, b"z", ys3, [b"12345"] * 4, crc2, 2)
    # decompress_image: what it refuses from the container alone
    cc = c.ContextCodec(_stub_model())
    one = dict(head2, B=1)
    states = struct.pack("<64I", *([1 << 16] * 64))
    d["image_licbits2_y_W_65"] = lambda: cc.decompress_image(
        c.pack_bitstream_rans(dict(one, y_W=65), b"z", [states], [b""], [0]))
    d["image_licbits3_y_W_100"] = lambda: cc.decompress_image(
        c.pack_bitstream_grouped(dict(one, y_W=100), b"z", [states] * 2, [b""] * 2, [0], 2))
    d["image_licbits1_y_W_100_no_family"] = lambda: cc.decompress_image(
        c.pack_bitstream(dict(one, y_W=100), b"z", [b"y"], [0]))
    d["image_licbits2_y_W_64_no_family"] = lambda: cc.decompress_image(
        c.pack_bitstream_rans(dict(one, y_W=64), b"z", [states], [b""], [0]))
    d["image_unknown_magic"] = lambda: cc.decompress_image(b"LICBITS9" + r1[8:])
    d["image_empty"] = lambda: cc.decompress_image(b"")
    d["image_licbits1_byte_30_removed_resealed"] = lambda: cc.decompress_image(_reseal(b1[:30] + b1[31:-4]))
    return d


def other_model_cases():
    """a well-formed LICBITS1 container of another model, per changed field -> callable (needs a real model)"""
    import neural_image_compression_amd as nic
    c = _codec()
    cc = c.ContextCodec(nic.JointAutoregressiveHierarchical(16, 1))
    ok = dict(HEAD, family=1, M=16, K=1, B=1)
    return {f"image_other_model_{k}": (lambda wrong=dict(ok, **{k: v}): cc.decompress_image(
        c.pack_bitstream(wrong, b"z", [b"y"], [0]))) for k, v in (("M", 32), ("K", 3), ("family", 2))}


def _message(fn):
    try:
        fn()
    except _codec().CodecError as e:
        return str(e)
    return None


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_writers_give_the_pinned_bytes_and_readers_return_the_inputs(golden, name):
    case = CASES[name]
    blob = bytes.fromhex(golden["containers"][name])
    assert pack(case) == blob
    assert unpack(case[0], blob) == _unpacked(case)
    assert blob[:8] == b"LICBITS%d" % case[0]
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == zlib.crc32(blob[:-4]) & 0xFFFFFFFF


def test_every_damage_case_is_refused_in_the_pinned_words(golden):
    cases = dict(damage_cases(), **other_model_cases())
    assert set(cases) == set(golden["messages"])
    got = {name: _message(fn) for name, fn in cases.items()}
    assert all(m is not None for m in got.values()), [n for n, m in got.items() if m is None]
    assert got == golden["messages"]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    doc = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            doc = json.load(f)
    doc["comment"] = ("containers, messages: what the pack_ / unpack_ functions of codec.py and decompress_image gave "
                      "at commit %s (python tests/test_bitstream_golden.py COMMIT)" % sys.argv[1])
    doc["containers"] = {name: pack(case).hex() for name, case in sorted(CASES.items())}
    doc["messages"] = {name: _message(fn) for name, fn in sorted(dict(damage_cases(), **other_model_cases()).items())}
    assert all(m is not None for m in doc["messages"].values()), doc["messages"]
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, len(doc["containers"]), "containers,", len(doc["messages"]), "messages")
