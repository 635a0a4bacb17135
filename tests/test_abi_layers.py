"""lic_ctx_gather_layers and lic_rans_decode_step_layers refuse bad arguments before any launch, so their status codes
can be checked without a GPU (as test_abi.py::test_argument_validation_without_gpu does for the older entries).  The
pointers below are never dereferenced: every call here ends in a refusal."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


P16 = 0x10000                       # a 16-byte aligned address that nothing reads
INVALID, UNSUPPORTED = -1, -2


def _ctx_layers(lib, rows):
    t = (lib.CtxLayer * max(len(rows), 1))()
    for e, (win, comb, ld, c0, M) in zip(t, rows):
        e.win, e.comb, e.comb_ld, e.c0, e.M = win, comb, ld, c0, M
    return t


def _gather(lib, rows, **kw):
    a = dict(y=P16, y_batch=16 * 32, y_row=4 * 32, y_pix=32, y_origin=0, B=1, h=4, w=4, taps=P16, nt=12, R=4, pix=P16,
             n=3, psi=P16, Cpsi=64, layers=_ctx_layers(lib, rows), L=len(rows), path=lib.CTX_AUTO, stream=None)
    a.update(kw)
    return lib.load().lic_ctx_gather_layers(*a.values())


def test_the_layer_tables_have_the_header_layout(lib):
    assert lib.MAX_LAYERS == 4
    assert C.sizeof(lib.CtxLayer) == 32 and lib.CtxLayer.c0.offset == 24 and lib.CtxLayer.M.offset == 28
    assert C.sizeof(lib.RansLayer) == 24 and lib.RansLayer.c0.offset == 16 and lib.RansLayer.M.offset == 20
    header = open(os.path.join(os.path.dirname(lib.LIB_PATH), "..", "include", "lic.h")).read()
    assert "#define LIC_MAX_LAYERS 4" in header and "#define LIC_ABI_VERSION 4" in header


def test_ctx_gather_layers_validates_before_it_launches(lib):
    two = [(P16, P16, 128, 0, 20), (P16 + 4096, P16 + 8192, 128, 20, 12)]
    for bad in (dict(y=None), dict(taps=None), dict(pix=None), dict(layers=None), dict(L=0), dict(L=5), dict(L=-1),
                dict(B=0), dict(h=0), dict(w=-1), dict(n=0), dict(nt=0), dict(R=0), dict(path=3), dict(y_pix=31),
                dict(y_batch=-1), dict(y_origin=-4), dict(Cpsi=0), dict(y=P16 + 2), dict(pix=P16 + 4), dict(psi=P16 + 1)):
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
    # the 16-byte path forced where a layer cannot take it: c0 = 17, M_l = 13
    odd = [(P16, P16, 128, 0, 17), (P16, P16, 128, 17, 13)]
    assert _gather(lib, odd, path=lib.CTX_VECTOR) == INVALID
    assert _gather(lib, two, path=lib.CTX_VECTOR, y_origin=2) == INVALID
    # the size limits of lic_ctx_gather
    assert _gather(lib, two, n=1 << 31) == UNSUPPORTED
    assert _gather(lib, two, B=1 << 20, n=(1 << 20) + 1) == UNSUPPORTED
    big = [(P16, P16, 128, 0, 1 << 28)]
    assert _gather(lib, big, y_pix=1 << 28, y_row=1 << 30, y_batch=1 << 32) == UNSUPPORTED


def _rans_layers(lib, rows):
    t = (lib.RansLayer * max(len(rows), 1))()
    for e, (tables, center, c0, M) in zip(t, rows):
        e.tables, e.center, e.c0, e.M = tables, center, c0, M
    return t


def _step(lib, rows, **kw):
    a = dict(streams=P16, stream_off=P16, stream_bytes=P16, escapes=P16, esc_off=P16, state=P16,
             layers=_rans_layers(lib, rows), L=len(rows), B=2, G=3, n=5, W=24, dest=P16, ypad=P16, pixels=100, y_pix=32,
             stream=None)
    a.update(kw)
    return lib.load().lic_rans_decode_step_layers(*a.values())


def test_rans_decode_step_layers_validates_before_it_launches(lib):
    two = [(P16, P16, 0, 20), (P16, P16, 20, 12)]
    for bad in (dict(streams=None), dict(stream_off=None), dict(stream_bytes=None), dict(escapes=None), dict(esc_off=None),
                dict(state=None), dict(layers=None), dict(dest=None), dict(ypad=None), dict(L=0), dict(L=5), dict(B=0),
                dict(G=0), dict(G=9), dict(n=0), dict(W=0), dict(pixels=0), dict(y_pix=31), dict(y_pix=0),
                dict(streams=P16 + 2), dict(stream_off=P16 + 4), dict(dest=P16 + 4), dict(ypad=P16 + 1), dict(state=P16 + 2)):
        assert _step(lib, two, **bad) == INVALID, bad
    for rows in ([(None, P16, 0, 20), two[1]], [two[0], (P16, None, 20, 12)],       # NULL tables / centres
                 [(P16 + 4, P16, 0, 20), two[1]], [two[0], (P16, P16 + 2, 20, 12)],  # tables 16 bytes, centres 4
                 [(P16, P16, 0, 0), two[1]], [(P16, P16, -1, 20), two[1]],           # M_l <= 0, c0 < 0
                 [two[0], (P16, P16, 20, 13)], [two[0], (P16, P16, 19, 12)],         # beyond y_pix, overlapping
                 [two[1], (P16, P16, 8, 4), (P16, P16, 11, 2), two[0]]):
        assert _step(lib, rows) == INVALID, rows
    assert _step(lib, two, W=65) == UNSUPPORTED
    assert _step(lib, two, B=4096, G=8) == UNSUPPORTED                               # L * B * G > 65535
    assert _step(lib, two, n=(1 << 31) // 20) == UNSUPPORTED                         # n * M_l >= 2^31 - 64
    assert _step(lib, [(P16, P16, 3, 5)], B=65535 // 3 + 1) == UNSUPPORTED
