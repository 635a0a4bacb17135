"""lic_msssim_bwd at the C ABI: exported, bound, and bad arguments come back as status codes without touching a
GPU (the version stays 4: the entry is an addition).  CPU only."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def L():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_workspace_sizes_are_host_functions(L):
    assert L.lic_version() == 4
    # the gradients of the pooled planes of scales 1..4: 128^2 + 64^2 + 32^2 + 16^2 floats per image-channel
    assert L.lic_msssim_bwd_workspace_bytes(2, 3, 256, 256) == 6 * (128 * 128 + 64 * 64 + 32 * 32 + 16 * 16) * 4
    # odd sides are padded by one before each pooling: 200x161 -> 100x81 -> 50x41 -> 25x21 -> 13x11
    assert L.lic_msssim_bwd_workspace_bytes(1, 1, 200, 161) == (100 * 81 + 50 * 41 + 25 * 21 + 13 * 11) * 4
    assert L.lic_msssim_bwd_workspace_bytes(1, 3, 160, 300) == 0      # side <= 160: unsupported, as the forward


def test_bad_arguments_return_status_codes(L):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before a launch
    fwd, bwd = L.lic_msssim_workspace_bytes(1, 3, 256, 256), L.lic_msssim_bwd_workspace_bytes(1, 3, 256, 256)
    assert fwd > 0 and bwd > 0

    def call(x=p, y=p, H=256, W=256, levels=p, fws=p, fbytes=fwd, gout=p, dx=p, ws=p, wbytes=bwd, B=1, C=3):
        return L.lic_msssim_bwd(x, y, B, C, H, W, C * H * W, H * W, W, 1, 1.0, levels, fws, fbytes, gout, dx, ws,
                                wbytes, None)

    for name in ("x", "y", "levels", "fws", "gout", "dx", "ws"):
        assert call(**{name: None}) == -1, name                      # LIC_ERR_INVALID
    assert call(H=160) == -2                                          # LIC_ERR_UNSUPPORTED
    assert call(B=0) == -2
    assert call(fbytes=fwd - 1) == -4                                 # LIC_ERR_WORKSPACE
    assert call(wbytes=bwd - 1) == -4
    assert call(B=30000, fbytes=1 << 60, wbytes=1 << 60) == -2        # more image-channels than a grid holds
