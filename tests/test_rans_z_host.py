"""The host side of z_coder="rans": lic_rans_encode_shared / lic_rans_decode_shared against the plain restatement of
the format on expanded tables (tests/rans_groups_ref.py), their refusals, table_of = NULL against lic_rans_encode /
lic_rans_decode, the layout `z_encode_plan` gives lic_rans_encode_ragged, the constructor rules and the argument checks
of the two device entries.  CPU only."""
import ctypes as C
import struct

import numpy as np
import pytest

import rans_groups_ref as GR
import rans_z_cases as ZC

CASES = [(3, 2, 130, 3), (5, 4, 257, 2), (192, 129, 1152, 8), (1, 3, 1, 1)]          # (M, S, n, G)


@pytest.fixture(scope="module")
def codec():
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import codec as CD
    return CD


def _case(M, S, n):
    return ZC.shared_tables(M, S, 7 * M + S), ZC.symbols(S, n, M + n)


@pytest.mark.parametrize("M,S,n,G", CASES)
def test_shared_coder_is_the_restatement_on_expanded_tables(codec, M, S, n, G):
    t, idx = _case(M, S, n)
    assert ((idx <= 0) | (idx >= S - 1)).any() and (np.abs(idx.astype(np.int64)) >= 100000).any()
    want_s, want_e = ZC.reference(t, idx, G)
    expanded = t[np.arange(n) % M]
    for g, (pos, steps_g) in enumerate(codec.rans_deal([n], G)):
        tof = (pos % M).astype(np.int32)
        s, e = codec.rans_encode_shared(t, idx[pos], steps_g, tof)
        assert s == want_s[g] and e == want_e[g]
        assert (codec.rans_decode_shared(s, e, t, steps_g, tof) == idx[pos]).all()
        # table_of = NULL is lic_rans_encode / lic_rans_decode: one table per symbol
        assert codec.rans_encode_shared(expanded[pos], idx[pos], steps_g) == (s, e) == \
            codec.rans_encode(expanded[pos], idx[pos], steps_g)
        assert (codec.rans_decode_shared(s, e, expanded[pos], steps_g) == idx[pos]).all()
    assert (GR.decode(want_s, want_e, expanded, [n]) == idx).all()


def _raw_decode(codec, s, e, t, tof, T, n):
    lib = codec._codec()
    buf = np.frombuffer(s, np.uint8)
    ebuf = np.frombuffer(e, np.dtype("<u4")).astype(np.uint32)
    steps, out = np.array([n], np.int64), np.empty(max(n, 1), np.int32)
    u8, u32, i32, i64 = (C.POINTER(c) for c in (C.c_uint8, C.c_uint32, C.c_int32, C.c_int64))
    return lib.lic_rans_decode_shared(buf.ctypes.data_as(u8), buf.size, ebuf.ctypes.data_as(u32), ebuf.size,
                                      t.ctypes.data_as(u32), None if tof is None else tof.ctypes.data_as(i32), T,
                                      t.shape[1] - 1, n, steps.ctypes.data_as(i64), 1, out.ctypes.data_as(i32))


def test_damage_is_refused(codec):
    M, S, n = 5, 9, 700
    t = ZC.shared_tables(M, S, 3)
    idx = ZC.symbols(S, n, 4)
    tof = (np.arange(n) % M).astype(np.int32)
    s, e = codec.rans_encode_shared(t, idx, [n], tof)
    assert len(s) > 256 + 2 and len(e) >= 8
    INVALID, CORRUPT = -1, -3
    assert _raw_decode(codec, s, e, t, tof, M, n) == 0
    assert _raw_decode(codec, s[:-2], e, t, tof, M, n) == CORRUPT                  # truncated by one word
    assert _raw_decode(codec, s, e[:-4], t, tof, M, n) == CORRUPT                  # truncated by one escape
    assert _raw_decode(codec, s + b"\0\0", e, t, tof, M, n) == CORRUPT             # a trailing word
    assert _raw_decode(codec, s, e + b"\0\0\0\0", t, tof, M, n) == CORRUPT         # a trailing escape
    assert _raw_decode(codec, s[:-1], e, t, tof, M, n) == CORRUPT                  # odd length
    assert _raw_decode(codec, s[:252], e, t, tof, M, n) == CORRUPT                 # shorter than its states
    # final states other than 2^16: one symbol fewer is decoded than was coded
    assert _raw_decode(codec, s, e, t, tof[:n - 1].copy(), M, n - 1) == CORRUPT
    for bad in (M, -1):                                                            # table_of outside [0, T)
        wrong = tof.copy()
        wrong[n - 3] = bad
        assert _raw_decode(codec, s, e, t, wrong, M, n) == INVALID
        with pytest.raises(codec.CodecError):
            codec.rans_encode_shared(t, idx, [n], wrong)
    assert _raw_decode(codec, s, e, t, tof, M - 1, n) == INVALID                   # T too small for the entries
    for col, val in ((0, 1), (S, 65535)):                                          # malformed tables
        broken = t.copy()
        broken[2, col] = val
        assert _raw_decode(codec, s, e, broken, tof, M, n) == INVALID
        with pytest.raises(codec.CodecError):
            codec.rans_encode_shared(broken, idx, [n], tof)
    flat = t.copy()
    flat[1, 4] = flat[1, 3]                                                        # a zero frequency
    with pytest.raises(codec.CodecError):
        codec.rans_encode_shared(flat, np.full(n, 3, np.int32), [n], tof)
    with pytest.raises(codec.CodecError):
        codec.rans_decode_shared(s, e[:-4], t, [n], tof)
    with pytest.raises(codec.CodecError):
        codec.rans_encode_shared(t, idx, [n], tof[:-1])


@pytest.mark.parametrize("G", (1, 3, 8))
def test_z_encode_plan_is_one_step_per_image(codec, G):
    M, pixels = 5, [1, 7, 40]
    images, blocks, step_len, rows, words_len, esc_len = codec.z_encode_plan(pixels, M, G)
    assert rows == sum(pixels) and step_len.tolist() == [P * M for P in pixels]
    assert images.tolist() == [[0, 1, 0, 1], [1, 7, 1, 1], [8, 40, 2, 1]]
    at_w = at_e = 0
    for b, P in enumerate(pixels):
        fullest = max(max(len(pos) for pos, _ in codec.rans_deal([P * M], G)), 1)
        for g in range(G):
            off, slot, e_off, cap = blocks[b * G + g]
            assert (off, e_off) == (at_w, at_e) and slot % 4 == 0 and slot >= 2 * fullest and cap == fullest
            at_w, at_e = at_w + slot, at_e + cap
    assert (words_len, esc_len) == (at_w, at_e)


def test_constructor_rules(codec):
    import neural_image_compression_amd as nic
    model = nic.JointAutoregressiveHierarchical(8, 1)
    assert codec.ContextCodec(model).z_coder == "range"
    assert codec.ContextCodec(model, coder="rans", z_coder="rans", groups=4, slice_rows=2).z_coder == "rans"
    with pytest.raises(codec.CodecError, match="z_coder"):
        codec.ContextCodec(model, z_coder="rans")                                  # needs coder="rans"
    with pytest.raises(codec.CodecError, match="z_coder"):
        codec.ContextCodec(model, coder="rans", z_coder="arithmetic")
    with pytest.raises(codec.CodecError, match="z_S"):
        codec.ContextCodec(model, z_S=1, coder="rans", z_coder="rans")
    assert codec.ContextCodec(model, z_lo=0, z_S=2, coder="rans", z_coder="rans").z_S == 2


def test_strings_that_cannot_be_are_refused_before_the_gpu(codec):
    import neural_image_compression_amd as nic
    cd = codec.ContextCodec(nic.JointAutoregressiveHierarchical(8, 1), coder="rans", z_coder="rans")
    shape, z_shape = (1, 8, 4, 4), (1, 8, 1, 1)
    y = [bytes(256)]
    with pytest.raises(codec.CodecError, match="z_coder"):
        cd.decompress({"coder": "rans", "z_coder": "huffman", "y": y, "y_esc": [b""], "z": [bytes(256)], "z_esc": [b""]},
                      shape, z_shape)
    with pytest.raises(codec.CodecError, match="z_coder"):
        cd.decompress({"z_coder": "rans", "y": y, "z": [bytes(256)], "z_esc": [b""]}, shape, z_shape)
    for z, z_esc in ((bytes(256), [b""]), ([bytes(256)], None), ([bytes(256)] * 2, [b""] * 2), ([bytes(255)], [b""])):
        with pytest.raises(codec.CodecError):
            cd.decompress({"coder": "rans", "z_coder": "rans", "y": y, "y_esc": [b""], "z": z, "z_esc": z_esc}, shape,
                          z_shape)


def test_device_entries_refuse_bad_arguments_without_a_launch():
    from neural_image_compression_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd, odd8 = C.c_void_p(p.value + 2), C.c_void_p(p.value + 4)
    pick = lambda **k: lib.lic_rans_z_pick(*[k.get(a, d) for a, d in (
        ("tables", p), ("M", 5), ("lo", -2), ("S", 4), ("z", p), ("n", 10), ("sf", p), ("exc", p), ("err", p),
        ("stream", None))])
    for bad in (dict(tables=None), dict(z=None), dict(sf=None), dict(exc=None), dict(err=None), dict(M=0), dict(S=1),
                dict(n=0), dict(n=11), dict(tables=odd), dict(z=odd), dict(err=odd)):
        assert pick(**bad) == -1, bad
    for bad in (dict(S=_lib.RANS_Z_MAX_S + 1), dict(M=_lib.RANS_Z_MAX_M + 1, n=_lib.RANS_Z_MAX_M + 1),
                dict(n=5 * (1 << 29))):
        assert pick(**bad) == -2, bad
    dec = lambda **k: lib.lic_rans_z_decode(*[k.get(a, d) for a, d in (
        ("streams", p), ("stream_off", p), ("stream_bytes", p), ("escapes", p), ("esc_off", p), ("state", p),
        ("tables", p), ("M", 5), ("lo", -2), ("S", 4), ("nimg", 2), ("G", 2), ("nsym", p), ("z_base", p), ("z", p),
        ("z_len", 16), ("path", 0), ("stream", None))])
    for name in ("streams", "stream_off", "stream_bytes", "escapes", "esc_off", "state", "tables", "nsym", "z_base", "z"):
        assert dec(**{name: None}) == -1, name
    for bad in (dict(M=0), dict(S=1), dict(nimg=0), dict(z_len=0), dict(G=0), dict(G=9), dict(path=3), dict(path=-1),
                dict(tables=odd), dict(z=odd), dict(state=odd), dict(stream_off=odd8), dict(nsym=odd8),
                dict(z_base=odd8), dict(M=1024, S=129, path=_lib.RANS_Z_RESIDENT)):
        assert dec(**bad) == -1, bad
    for bad in (dict(S=_lib.RANS_Z_MAX_S + 1), dict(M=_lib.RANS_Z_MAX_M + 1), dict(nimg=40000), dict(z_len=(1 << 40) + 1)):
        assert dec(**bad) == -2, bad
    # which path AUTO takes: the default codec's tables stay on chip, 1024 x 129 do not fit the budget
    path = lib.lic_rans_z_decode_path
    assert path(192, 129) == _lib.RANS_Z_RESIDENT and path(5, 4) == _lib.RANS_Z_RESIDENT
    assert path(1024, 129) == _lib.RANS_Z_GLOBAL
    assert 192 * 130 * 2 <= _lib.RANS_Z_LDS_BYTES < 1024 * 130 * 2
    assert path(0, 4) == -1 and path(4, 1) == -1 and path(4, _lib.RANS_Z_MAX_S + 1) == -2
