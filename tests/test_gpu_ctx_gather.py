"""lic_ctx_gather on an MI355X through the C ABI, `==` against ctx_slices_ref.gather.  Every input value is distinct
(latents positive, psi negative, the frame around a framed plane a third range), so a wrong index cannot hide; every
output sits between canary rows and, for the psi columns, between canary columns of a wider buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctx_slices_ref as SR

pytestmark = pytest.mark.gpu

B, P = 2, SR.PAD
CANARY = -12345.0
GUARD = 3                                          # canary rows in front of and behind every output
C0, CEXTRA = 8, 4                                  # the psi columns start at C0 of a buffer CEXTRA columns wider
SHAPES = [(4, 4), (5, 7)]
MS = [4, 6, 192]                                   # 6: no 16-byte pieces, the element path


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    dev = torch.device("cuda:0")
    taps = torch.tensor(SR.TAPS, dtype=torch.int32, device=dev)
    return _lib, F_, dev, taps


_INPUTS = {}


def _inputs(h, w, M):
    """(y [B,h,w,M], psi [B,h*w,2M]) with no value twice, and per R the reference for ALL pixels, computed once"""
    key = (h, w, M)
    if key not in _INPUTS:
        y = (1.0 + np.arange(B * h * w * M, dtype=np.float32)).reshape(B, h, w, M)
        psi = -(1.0 + np.arange(B * h * w * 2 * M, dtype=np.float32)).reshape(B, h * w, 2 * M)
        ref = {R: SR.gather(y, R, list(range(h * w)), psi=psi) for R in (1, 2, 3, h + 1)}
        _INPUTS[key] = (y, psi, ref)
    return _INPUTS[key]


def _expected(h, w, M, R, pix):
    """the rows of the all-pixel reference that `pix` selects; zeros for an index outside the plane"""
    _, _, ref = _inputs(h, w, M)
    win_all, psi_all = (a.reshape(B, h * w, -1) for a in ref[R])
    n = len(pix)
    win, rows = np.zeros((B, n, win_all.shape[2]), np.float32), np.zeros((B, n, psi_all.shape[2]), np.float32)
    for k, px in enumerate(pix):
        if 0 <= px < h * w:
            win[:, k], rows[:, k] = win_all[:, px], psi_all[:, px]
    return win.reshape(B * n, -1), rows.reshape(B * n, -1)


def _plane(env, y, addressing):
    """the latents on the device -> (tensor, y_batch, y_row, y_pix, y_origin).  "framed": inside a frame of P pixels
    that is NOT zero; "pitched": 4 unused floats behind every pixel's M"""
    _, _, dev, _ = env
    _, h, w, M = y.shape
    if addressing == "plain":
        return torch.from_numpy(y).to(dev), h * w * M, w * M, M, 0
    if addressing == "pitched":
        buf = np.full((B, h, w, M + 4), 7e6, np.float32)
        buf[..., :M] = y
        return torch.from_numpy(buf).to(dev), h * w * (M + 4), w * (M + 4), M + 4, 0
    buf = (5e6 + np.arange(B * (h + 2 * P) * (w + 2 * P) * M, dtype=np.float32)).reshape(B, h + 2 * P, w + 2 * P, M)
    buf[:, P:P + h, P:P + w] = y
    return torch.from_numpy(buf).to(dev), (h + 2 * P) * (w + 2 * P) * M, (w + 2 * P) * M, M, (P * (w + 2 * P) + P) * M


def _gather(env, h, w, M, R, pix, addressing="plain", with_psi=True, path=0, c0=C0, bad=None):
    """one call -> (status, win buffer [GUARD + B*n + GUARD, 12M], comb buffer [GUARD + B*n + GUARD, C0 + 2M + CEXTRA])
    as numpy, canaries included.  `bad`: arguments to replace, by name"""
    _lib, F_, dev, taps = env
    y, psi, _ = _inputs(h, w, M)
    n, nt = len(pix), len(SR.TAPS)
    yd, y_batch, y_row, y_pix, y_origin = _plane(env, y, addressing)
    rows = B * max(n, 1)
    win = torch.full((rows + 2 * GUARD, nt * M), CANARY, device=dev)
    ld = C0 + 2 * M + CEXTRA
    comb = torch.full((rows + 2 * GUARD, ld), CANARY, device=dev)
    d_pix = torch.tensor(list(pix) or [0], dtype=torch.int64, device=dev)
    d_psi = torch.from_numpy(psi).to(dev)
    a = dict(y=F_._ptr(yd), y_batch=y_batch, y_row=y_row, y_pix=y_pix, y_origin=y_origin, B=B, h=h, w=w, M=M,
             taps=F_._ptr(taps), nt=nt, R=R, pix=F_._ptr(d_pix), n=n, win=C.c_void_p(win[GUARD].data_ptr()),
             psi=F_._ptr(d_psi) if with_psi else None, Cpsi=2 * M if with_psi else 0,
             comb=C.c_void_p(comb[GUARD].data_ptr() + 4 * c0) if with_psi else None, comb_ld=ld if with_psi else 0,
             path=path, stream=F_._stream())
    a.update(bad or {})
    rc = _lib.load().lic_ctx_gather(*a.values())
    torch.cuda.synchronize()
    return rc, win.cpu().numpy(), comb.cpu().numpy()


def _check(got, h, w, M, R, pix, with_psi=True, c0=C0):
    rc, win, comb = got
    assert rc == 0
    n = len(pix)
    want_win, want_psi = _expected(h, w, M, R, pix)
    assert (win[:GUARD] == CANARY).all() and (win[GUARD + B * n:] == CANARY).all()
    assert np.array_equal(win[GUARD:GUARD + B * n], want_win)
    want = np.full_like(comb, CANARY)
    if with_psi:
        want[GUARD:GUARD + B * n, c0:c0 + 2 * M] = want_psi
    assert np.array_equal(comb, want)


def _lists(h, w, R):
    steps = SR.schedule(h, w, R)
    ii, jj = steps[len(steps) // 2]
    widest = max(steps, key=lambda s: len(s[0]))
    return {"one pixel": [h * w - 1], "one step": list(ii * w + jj), "widest step": list(widest[0] * w + widest[1]),
            "all": list(range(h * w)), "one index past the plane": [2, h * w + 5, 0], "a negative index": [1, -1, 3]}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_gather_matches_the_restatement(env, h, w, M):
    for R in (1, 2, 3, h + 1):
        for name, pix in _lists(h, w, R).items():
            for addressing in ("framed", "plain"):
                for with_psi in (True, False):
                    _check(_gather(env, h, w, M, R, pix, addressing, with_psi), h, w, M, R, pix, with_psi)


@pytest.mark.parametrize("M", MS)
def test_a_pixel_pitch_wider_than_M_and_a_slice_height_beyond_the_plane(env, M):
    h, w = 5, 7
    pix = list(range(h * w))
    _check(_gather(env, h, w, M, 2, pix, "pitched"), h, w, M, 2, pix)
    got = _gather(env, h, w, M, 1 << 30, pix, "framed")
    _check(got, h, w, M, h + 1, pix)                                      # any R >= h is one slice


@pytest.mark.parametrize("M", [4, 192])
def test_vector_and_element_paths_write_the_same_bytes(env, M):
    _lib = env[0]
    h, w, R = 5, 7, 2
    for pix in (list(range(h * w)), [2, h * w + 5, 0]):
        for addressing in ("framed", "plain"):
            vec = _gather(env, h, w, M, R, pix, addressing, path=_lib.CTX_VECTOR)
            one = _gather(env, h, w, M, R, pix, addressing, path=_lib.CTX_ELEMENT)
            auto = _gather(env, h, w, M, R, pix, addressing)
            _check(vec, h, w, M, R, pix)
            for a, b in ((vec, one), (vec, auto)):
                assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_bases_that_are_not_16_byte_aligned_take_the_element_path(env):
    """M = 4 with the psi columns starting at column 2: the automatic path still writes the right bytes.  The forced
    vector path is refused there, for a plane origin of 2 floats and for M = 6, and writes nothing"""
    _lib, F_, dev, _ = env
    h, w, M, R = 4, 4, 4, 2
    pix = list(range(h * w))
    _check(_gather(env, h, w, M, R, pix, c0=2), h, w, M, R, pix, c0=2)
    rc, win, comb = _gather(env, h, w, M, R, pix, c0=2, path=_lib.CTX_VECTOR)
    assert rc == -1 and (win == CANARY).all() and (comb == CANARY).all()
    for addressing in ("plain", "framed"):
        rc, win, comb = _gather(env, h, w, M, R, pix, addressing, path=_lib.CTX_VECTOR, bad=dict(y_origin=2))
        assert rc == -1 and (win == CANARY).all() and (comb == CANARY).all()
    rc, win, comb = _gather(env, h, w, 6, R, pix, path=_lib.CTX_VECTOR)
    assert rc == -1 and (win == CANARY).all() and (comb == CANARY).all()


def test_refusals_launch_nothing(env):
    h, w, M, R = 4, 4, 4, 2
    pix = [0, 5]
    for bad in (dict(y=None), dict(taps=None), dict(pix=None), dict(win=None), dict(comb=None), dict(n=0), dict(n=-2),
                dict(R=0), dict(R=-1), dict(nt=0), dict(B=0), dict(h=0), dict(w=-4), dict(M=0), dict(path=3),
                dict(y_pix=M - 1), dict(Cpsi=0), dict(comb_ld=2 * M - 1)):
        rc, win, comb = _gather(env, h, w, M, R, pix, bad=bad)
        assert rc == -1, bad
        assert (win == CANARY).all() and (comb == CANARY).all(), bad
    _check(_gather(env, h, w, M, R, pix), h, w, M, R, pix)
