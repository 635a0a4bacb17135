"""The device-quality entries of the C ABI (lic_gain_rows_fwd / _bwd, lic_rd_loss_fwd_lam / _bwd_lam): exported, bound, and
their argument validation returns LIC_ERR_INVALID before anything is launched.  CPU only."""
import ctypes
import os
import re
import subprocess

import pytest

NEW = ("lic_gain_rows_fwd", "lic_gain_rows_bwd", "lic_rd_loss_fwd_lam", "lic_rd_loss_bwd_lam")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_new_symbols_are_exported_and_bound(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (lic_[a-z0-9_]+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(lib.SIGNATURES)
    L = lib.load()
    assert L.lic_version() == 4                                   # additive: the ABI version stays
    assert lib.GAIN_ROWS_MAX_TABLES == 4
    for name in NEW:
        assert getattr(L, name).argtypes == lib.SIGNATURES[name][1]


def test_gain_rows_argument_validation(lib):
    L = lib.load()
    host = ctypes.create_string_buffer(256)        # a non-null, 16-byte-capable address; never dereferenced
    p = ctypes.addressof(host) + (-ctypes.addressof(host)) % 16
    ok = dict(k=1, Q=2, M=1, B=1)
    fwd = lambda q=p, t=p, r=p, lvl=p, **kw: L.lic_gain_rows_fwd(q, t, r, lvl, *[{**ok, **kw}[n] for n in "kQMB"], None)
    bwd = lambda lvl=p, r=p, d=(p, None, None, None), dt=p, **kw: \
        L.lic_gain_rows_bwd(lvl, r, *d, dt, *[{**ok, **kw}[n] for n in "kQMB"], None)
    for null in ("q", "t", "r", "lvl"):
        assert fwd(**{null: None}) == INVALID, null
    for bad in (dict(k=0), dict(k=5), dict(Q=1), dict(Q=0), dict(M=0), dict(B=0), dict(B=-3)):
        assert fwd(**bad) == INVALID, bad
        assert bwd(**bad) == INVALID, bad
    for null in ("lvl", "r", "dt"):
        assert bwd(**{null: None}) == INVALID, null
    assert bwd(d=(p, p, None, None)) == INVALID                    # a gradient behind the k-th table
    assert fwd(q=p + 2) == INVALID and bwd(dt=p + 1) == INVALID    # not float-aligned


def test_per_image_loss_argument_validation(lib):
    L = lib.load()
    host = ctypes.create_string_buffer(256)
    p = ctypes.addressof(host)
    nbytes = L.lic_rd_loss_workspace_bytes(2)

    def fwd(ly=p, lz=p, xh=p, x=p, lam=p, out=p, ws=p, ny=4, nz=4, nx=4, B=2, npix=4, wsb=nbytes):
        return L.lic_rd_loss_fwd_lam(ly, ny, lz, nz, xh, x, nx, B, npix, lam, out, ws, wsb, None)

    def bwd(xh=p, x=p, lam=p, gl=p, dy=p, dz=p, dx=p, ny=4, nz=4, nx=4, B=2, npix=4):
        return L.lic_rd_loss_bwd_lam(xh, x, ny, nz, nx, B, npix, lam, gl, dy, dz, dx, None)

    for null in ("ly", "lz", "xh", "x", "lam", "out", "ws"):
        assert fwd(**{null: None}) == INVALID, null
    for null in ("xh", "x", "lam", "gl", "dy", "dz", "dx"):
        assert bwd(**{null: None}) == INVALID, null
    for bad in ("ny", "nz", "nx", "B", "npix"):
        assert fwd(**{bad: 0}) == INVALID and fwd(**{bad: -1}) == INVALID, bad
        assert bwd(**{bad: 0}) == INVALID and bwd(**{bad: -1}) == INVALID, bad
    assert fwd(wsb=nbytes - 1) == -4                               # LIC_ERR_WORKSPACE, as lic_rd_loss_fwd
