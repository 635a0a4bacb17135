"""lic_ctx_gather_layers_ragged and lic_rans_decode_step_layers_ragged refuse bad arguments before any launch, so their
status codes can be checked without a GPU (as test_abi_layers.py does for the equal-size entries).  The pointers below
are never dereferenced: every call here ends in a refusal.  The host half of codec.ScalableCodec's many-blob decoders
(`_open_blobs`) runs without a device too: containers with made-up streams are enough for what it refuses."""
import os

import pytest

P16 = 0x10000                       # a 16-byte aligned address that nothing reads
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_the_abi_version_stays_and_both_entries_are_declared(lib):
    header = open(os.path.join(os.path.dirname(lib.LIB_PATH), "..", "include", "lic.h")).read()
    assert "#define LIC_ABI_VERSION 4" in header and lib.load().lic_version() == 4
    for name in ("lic_ctx_gather_layers_ragged", "lic_rans_decode_step_layers_ragged"):
        assert f"int {name}(" in header and hasattr(lib.load(), name)


def _ctx_layers(lib, rows):
    t = (lib.CtxLayer * max(len(rows), 1))()
    for e, (win, comb, ld, c0, M) in zip(t, rows):
        e.win, e.comb, e.comb_ld, e.c0, e.M = win, comb, ld, c0, M
    return t


def _gather(lib, table, **kw):
    a = dict(y=P16, y_len=1 << 20, y_pix=32, images=P16, nimg=3, taps=P16, nt=12, row_image=P16, row_pix=P16, rows=40,
             psi=P16, psi_len=1 << 16, Cpsi=64, layers=_ctx_layers(lib, table), L=len(table), path=lib.CTX_AUTO,
             stream=None)
    a.update(kw)
    return lib.load().lic_ctx_gather_layers_ragged(*a.values())


def test_ctx_gather_layers_ragged_validates_before_it_launches(lib):
    two = [(P16, P16, 128, 0, 20), (P16 + 4096, P16 + 8192, 128, 20, 12)]
    for bad in (dict(y=None), dict(images=None), dict(taps=None), dict(row_image=None), dict(row_pix=None),
                dict(layers=None), dict(L=0), dict(L=5), dict(L=-1), dict(nimg=0), dict(rows=0), dict(rows=-2),
                dict(nt=0), dict(y_len=0), dict(y_len=-5), dict(psi_len=0), dict(path=3), dict(y_pix=31), dict(y_pix=0),
                dict(Cpsi=0), dict(y=P16 + 2), dict(psi=P16 + 1), dict(taps=P16 + 2), dict(images=P16 + 4),
                dict(row_image=P16 + 4), dict(row_pix=P16 + 12)):
        assert _gather(lib, two, **bad) == INVALID, bad
    for rows in ([(None, P16, 128, 0, 20), two[1]],                       # a layer without win
                 [two[0], (P16, None, 128, 20, 12)],                      # psi, and a layer without comb
                 [two[0], (P16, P16, 63, 20, 12)],                        # comb_ld < Cpsi
                 [(P16, P16, 128, 0, 0), two[1]],                         # M_l <= 0
                 [(P16, P16, 128, -1, 20), two[1]],                       # c0 < 0
                 [two[0], (P16, P16, 128, 20, 13)],                       # c0 + M_l > y_pix
                 [two[0], (P16, P16, 128, 19, 12)],                       # overlapping channel ranges
                 [two[1], two[0], (P16, P16, 128, 31, 1)],                # ... whatever the order
                 [(P16 + 2, P16, 128, 0, 20), two[1]],                    # a misaligned win
                 [two[0], (P16, P16 + 3, 128, 20, 12)]):                  # a misaligned comb
        assert _gather(lib, rows) == INVALID, rows
    # the 16-byte path forced where a layer cannot take it: c0 = 17, M_l = 13; a pitch, a comb_ld or a win that cannot
    odd = [(P16, P16, 128, 0, 17), (P16, P16, 128, 17, 13)]
    assert _gather(lib, odd, path=lib.CTX_VECTOR) == INVALID
    assert _gather(lib, [(P16, P16, 128, 0, 20), (P16, P16, 128, 20, 12)], path=lib.CTX_VECTOR, y_pix=33) == INVALID
    assert _gather(lib, [two[0], (P16, P16, 130, 20, 12)], path=lib.CTX_VECTOR) == INVALID
    assert _gather(lib, [two[0], (P16 + 4, P16, 128, 20, 12)], path=lib.CTX_VECTOR) == INVALID
    # the size limits of lic_ctx_gather_ragged, per layer where they name M
    for bad in (dict(y_len=(1 << 40) + 4), dict(psi_len=(1 << 40) + 4), dict(rows=(1 << 40) + 1)):
        assert _gather(lib, two, **bad) == UNSUPPORTED, bad
    big = [(P16, P16, 128, 0, 1 << 28)]
    assert _gather(lib, big, y_pix=1 << 28) == UNSUPPORTED                # nt * M_l + Cpsi


def _rans_layers(lib, rows):
    t = (lib.RansLayer * max(len(rows), 1))()
    for e, (tables, center, c0, M) in zip(t, rows):
        e.tables, e.center, e.c0, e.M = tables, center, c0, M
    return t


def _step(lib, rows, **kw):
    a = dict(streams=P16, stream_off=P16, stream_bytes=P16, escapes=P16, esc_off=P16, state=P16,
             layers=_rans_layers(lib, rows), L=len(rows), seg=P16, nimg=2, G=3, total_rows=5, W=24, dest=P16, ypad=P16,
             y_base=P16, pixels=P16, ypad_len=1 << 20, y_pix=32, stream=None)
    a.update(kw)
    return lib.load().lic_rans_decode_step_layers_ragged(*a.values())


def test_rans_decode_step_layers_ragged_validates_before_it_launches(lib):
    two = [(P16, P16, 0, 20), (P16, P16, 20, 12)]
    for bad in (dict(streams=None), dict(stream_off=None), dict(stream_bytes=None), dict(escapes=None), dict(esc_off=None),
                dict(state=None), dict(layers=None), dict(seg=None), dict(dest=None), dict(ypad=None), dict(y_base=None),
                dict(pixels=None), dict(L=0), dict(L=5), dict(nimg=0), dict(G=0), dict(G=9), dict(total_rows=0),
                dict(total_rows=-3), dict(W=0), dict(ypad_len=0), dict(y_pix=31), dict(y_pix=0), dict(streams=P16 + 2),
                dict(stream_off=P16 + 4), dict(stream_bytes=P16 + 4), dict(esc_off=P16 + 4), dict(dest=P16 + 4),
                dict(y_base=P16 + 4), dict(pixels=P16 + 12), dict(seg=P16 + 2), dict(ypad=P16 + 1), dict(state=P16 + 2),
                dict(escapes=P16 + 2)):
        assert _step(lib, two, **bad) == INVALID, bad
    for rows in ([(None, P16, 0, 20), two[1]], [two[0], (P16, None, 20, 12)],       # NULL tables / centres
                 [(P16 + 4, P16, 0, 20), two[1]], [two[0], (P16, P16 + 2, 20, 12)],  # tables 16 bytes, centres 4
                 [(P16, P16, 0, 0), two[1]], [(P16, P16, -1, 20), two[1]],           # M_l <= 0, c0 < 0
                 [two[0], (P16, P16, 20, 13)], [two[0], (P16, P16, 19, 12)],         # beyond y_pix, overlapping
                 [two[1], (P16, P16, 8, 4), (P16, P16, 11, 2), two[0]]):
        assert _step(lib, rows) == INVALID, rows
    assert _step(lib, two, W=65) == UNSUPPORTED
    assert _step(lib, two, nimg=4096, G=8) == UNSUPPORTED                            # L * nimg * G > 65535
    assert _step(lib, [(P16, P16, 3, 5)], nimg=65535 // 3 + 1) == UNSUPPORTED
    assert _step(lib, two, total_rows=(1 << 31) // 20) == UNSUPPORTED                # total_rows * M_l >= 2^31 - 64
    assert _step(lib, two, total_rows=1 << 31) == UNSUPPORTED
    assert _step(lib, two, ypad_len=(1 << 40) + 1) == UNSUPPORTED


# ---- the host half of ScalableCodec.decompress_images / decompress_base_images ------------------------------------------
@pytest.fixture(scope="module")
def codec_env():
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import codec
    model = nic.ScalableImageCoding(32, 20, 1).eval()
    return codec, model


def _blob(codec, cc, G=1, y_W=None, H=64, W=64):
    """a LICBITS6 container around made-up streams: every sub-stream its 64 states and a few words, no escapes"""
    from neural_image_compression_amd.bitstream import pack_bitstream_layered
    m = cc.model
    head = {"family": cc._family(), "M": m.M, "K": m.K, "z_lo": cc.z_lo, "z_S": cc.z_S, "y_W": cc.y_W if y_W is None else y_W,
            "B": 1, "H": H, "W": W, "top": 0, "left": 0, "M1": m.M1}
    stream = lambda l, g: bytes([l + 1, g + 1] * 128) + bytes(8)
    layers = [{"y": [stream(l, g) for g in range(G)], "y_esc": [b""] * G, "y_crc32": [7 + l]} for l in range(2)]
    return pack_bitstream_layered(head, [stream(2, g) for g in range(G)], [b""] * G, layers, G)


def test_the_host_half_of_the_many_blob_decoders(codec_env):
    codec, model = codec_env
    cc = codec.ScalableCodec(model)
    assert cc.decompress_images([]) == [] and cc.decompress_base_images([]) == []
    a, b = _blob(codec, cc), _blob(codec, cc, H=70, W=100)
    opened, dec = cc._open_blobs([a, b], False)
    assert dec is cc and [h["H"] for h, _ in opened] == [64, 70] and all(len(s["layers"]) == 2 for _, s in opened)
    # a G or a y_W that is not blob 0's is refused naming the blob, for both depths
    for other, what in ((_blob(codec, cc, G=4), "G = 4"), (_blob(codec, cc, y_W=24), "y_W = 24")):
        for base_only in (False, True):
            with pytest.raises(codec.CodecError, match=f"blob 1: {what}"):
                cc._open_blobs([a, other], base_only)
        for call in (cc.decompress_images, cc.decompress_base_images):
            with pytest.raises(codec.CodecError, match=f"blob 1: {what}"):
                call([a, other])
    # blobs written with another window than this codec's: read from the blobs, one decoder for all of them
    w24 = _blob(codec, cc, y_W=24)
    opened, dec = cc._open_blobs([w24, w24], False)
    assert dec is not cc and dec.y_W == 24 and dec.model is model
    # a base prefix: refused as truncated by the full decoder, taken by the base decoder beside a whole blob
    nb = cc.base_bytes_of(b)
    with pytest.raises(codec.CodecError, match="blob 1: .*truncated"):
        cc.decompress_images([a, b[:nb]])
    opened, dec = cc._open_blobs([a, b[:nb], b[:nb] + b"\x5a" * 33], True)
    assert dec is cc and all(len(s["layers"]) == 1 for _, s in opened) and opened[1][0] == opened[2][0]
    assert opened[1][1]["layers"][0]["y"] == opened[2][1]["layers"][0]["y"]
    # whatever the single-blob call refuses for a blob is refused under its name
    bad = bytearray(b)
    bad[nb - 40] ^= 0x10
    for call in (cc.decompress_images, cc.decompress_base_images):
        with pytest.raises(codec.CodecError, match="blob 2: .*CRC-32"):
            call([a, a, bytes(bad)])
    other = codec.ScalableCodec(type(model)(32, 12, 1).eval())
    with pytest.raises(codec.CodecError, match="blob 0: .*M1=20"):
        other.decompress_base_images([a[:cc.base_bytes_of(a)]])
