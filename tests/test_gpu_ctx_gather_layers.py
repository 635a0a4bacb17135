"""lic_ctx_gather_layers on an MI355X through the C ABI: every layer's rows bit for bit what lic_ctx_gather writes when
it is called for that layer alone with y + c0, and what the numpy statement (ctx_layers_ref.py) says.  Every input
value is distinct, every output lives between canaries (guarded.py), psi columns inside a wider pitched buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctx_layers_ref as LR
import ctx_slices_ref as SR
from guarded import Guarded

pytestmark = pytest.mark.gpu

P = SR.PAD
NT = len(SR.TAPS)
CPSI = 8
# (layers [(c0, M_l)], y_pix): (17, 13) has a misaligned c0 and odd widths: the float path, per layer
SPLITS = [([(0, 20), (20, 12)], 32), ([(0, 12), (12, 20)], 32), ([(0, 17), (17, 13)], 32), ([(0, 1), (1, 7)], 8),
          ([(0, 8), (8, 4), (12, 4)], 16), ([(4, 8)], 16)]
PLANES = [(4, 4), (5, 7), (8, 12)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    dev = torch.device("cuda:0")
    return _lib, F_, dev, torch.tensor(SR.TAPS, dtype=torch.int32, device=dev)


def _inputs(B, h, w, y_pix):
    y = (1.0 + np.arange(B * h * w * y_pix, dtype=np.float32)).reshape(B, h, w, y_pix)
    psi = -(1.0 + np.arange(B * h * w * CPSI, dtype=np.float32)).reshape(B, h * w, CPSI)
    return y, psi


def _plane(dev, y, framed):
    """-> (device tensor, y_batch, y_row, y_origin); "framed": inside a frame of P pixels that is NOT zero"""
    B, h, w, y_pix = y.shape
    if not framed:
        return torch.from_numpy(y).to(dev), h * w * y_pix, w * y_pix, 0
    buf = (5e6 + np.arange(B * (h + 2 * P) * (w + 2 * P) * y_pix, dtype=np.float32)).reshape(B, h + 2 * P, w + 2 * P, y_pix)
    buf[:, P:P + h, P:P + w] = y
    return torch.from_numpy(buf).to(dev), (h + 2 * P) * (w + 2 * P) * y_pix, (w + 2 * P) * y_pix, (P * (w + 2 * P) + P) * y_pix


def _outputs(dev, layers, rows):
    """per layer a guarded win [rows][NT * M_l] and a guarded comb whose psi columns start behind 2 M_l others"""
    outs = []
    for _, M in layers:
        cctx = 2 * M
        ld = (cctx + CPSI + 4 + 3) // 4 * 4 if M % 2 == 0 else cctx + CPSI + 3
        outs.append((Guarded(rows, NT * M, dev), Guarded(rows, CPSI, dev, ld=ld, col0=cctx)))
    return outs


def _layers_call(env, yd, geo, y_pix, B, h, w, R, pix, psi, layers, path=0):
    _lib, F_, dev, taps = env
    n = len(pix)
    outs = _outputs(dev, layers, B * n)
    table = (_lib.CtxLayer * len(layers))()
    for t, (c0, M), (win, comb) in zip(table, layers, outs):
        t.win, t.comb, t.comb_ld, t.c0, t.M = win.ptr(), comb.ptr() if psi is not None else None, comb.ld, c0, M
    d_pix = torch.tensor(list(pix), dtype=torch.int64, device=dev)
    rc = _lib.load().lic_ctx_gather_layers(F_._ptr(yd), geo[0], geo[1], y_pix, geo[2], B, h, w, F_._ptr(taps), NT, R,
                                           F_._ptr(d_pix), n, F_._ptr(psi), CPSI if psi is not None else 0, table,
                                           len(layers), path, F_._stream())
    torch.cuda.synchronize()
    return rc, outs


def _one_layer_call(env, yd, geo, y_pix, B, h, w, R, pix, psi, layer, path=0):
    """lic_ctx_gather for this layer alone, the plane's pointer moved to channel c0"""
    _lib, F_, dev, taps = env
    n = len(pix)
    (win, comb), = _outputs(dev, [layer], B * n)
    c0, M = layer
    d_pix = torch.tensor(list(pix), dtype=torch.int64, device=dev)
    rc = _lib.load().lic_ctx_gather(C.c_void_p(yd.data_ptr() + 4 * c0), geo[0], geo[1], y_pix, geo[2], B, h, w, M,
                                    F_._ptr(taps), NT, R, F_._ptr(d_pix), n, C.c_void_p(win.ptr()), F_._ptr(psi),
                                    CPSI if psi is not None else 0, C.c_void_p(comb.ptr()) if psi is not None else None,
                                    comb.ld if psi is not None else 0, path, F_._stream())
    torch.cuda.synchronize()
    return rc, win, comb


def _select(all_rows, B, hw, pix):
    """(win, psi rows) of ALL pixels -> those of the list `pix`, zeros for an index outside [0, hw)"""
    out = []
    for a in all_rows:
        a = a.reshape(B, hw, -1)
        sel = np.zeros((B, len(pix), a.shape[2]), a.dtype)
        for k, px in enumerate(pix):
            if 0 <= px < hw:
                sel[:, k] = a[:, px]
        out.append(sel.reshape(B * len(pix), -1))
    return tuple(out)


def _lists(h, w, R):
    steps = SR.schedule(h, w, R)
    widest = max(steps, key=lambda s: len(s[0]))
    return [list(widest[0] * w + widest[1]), list(range(h * w)), [2, h * w + 5, 0], [1, -1, 3]]


@pytest.mark.parametrize("layers,y_pix", SPLITS)
@pytest.mark.parametrize("h,w", PLANES)
def test_layers_match_the_one_layer_gather_and_the_restatement(env, h, w, layers, y_pix):
    dev = env[2]
    for B in (1, 2):
        y, psi = _inputs(B, h, w, y_pix)
        d_psi = torch.from_numpy(psi).to(dev)
        # the restatement once per R for all pixels; a list selects its rows (zeros for an index outside the plane)
        ref = {R: LR.gather_layers(y, R, list(range(h * w)), layers, psi=psi) for R in (h, 2, 3)}
        for framed in (True, False):
            yd, *geo = _plane(dev, y, framed)
            for R in (h, 2, 3):                                            # h: no slices
                for pix in _lists(h, w, R):
                    want = [_select(a, B, h * w, pix) for a in ref[R]]
                    rc, outs = _layers_call(env, yd, geo, y_pix, B, h, w, R, pix, d_psi, layers)
                    assert rc == 0
                    for l, (layer, (win, comb), (want_win, want_psi)) in enumerate(zip(layers, outs, want)):
                        what = f"B={B} framed={framed} R={R} layer {l} pix={pix[:4]}"
                        win.check(what)
                        comb.check(what)
                        assert np.array_equal(win.cpu().numpy(), want_win), what
                        assert np.array_equal(comb.cpu().numpy(), want_psi), what
                        rc1, win1, comb1 = _one_layer_call(env, yd, geo, y_pix, B, h, w, R, pix, d_psi, layer)
                        assert rc1 == 0
                        assert win.buf.cpu().numpy().tobytes() == win1.buf.cpu().numpy().tobytes(), what
                        assert comb.buf.cpu().numpy().tobytes() == comb1.buf.cpu().numpy().tobytes(), what


def test_without_psi_no_comb_is_touched(env):
    dev = env[2]
    h, w, (layers, y_pix) = 5, 7, SPLITS[0]
    y, _ = _inputs(2, h, w, y_pix)
    yd, *geo = _plane(dev, y, True)
    pix = list(range(h * w))
    rc, outs = _layers_call(env, yd, geo, y_pix, 2, h, w, 2, pix, None, layers)
    assert rc == 0
    for (win, comb), (want_win, _) in zip(outs, LR.gather_layers(y, 2, pix, layers)):
        win.check()
        assert np.array_equal(win.cpu().numpy(), want_win) and comb.untouched()


def test_vector_and_element_paths_write_the_same_bytes(env):
    _lib, _, dev, _ = env
    h, w = 5, 7
    for layers, y_pix in (SPLITS[0], SPLITS[4]):
        y, psi = _inputs(2, h, w, y_pix)
        d_psi = torch.from_numpy(psi).to(dev)
        for framed in (True, False):
            yd, *geo = _plane(dev, y, framed)
            for pix in (list(range(h * w)), [2, h * w + 5, 0]):
                runs = [_layers_call(env, yd, geo, y_pix, 2, h, w, 2, pix, d_psi, layers, path)
                        for path in (_lib.CTX_VECTOR, _lib.CTX_ELEMENT, _lib.CTX_AUTO)]
                assert [r[0] for r in runs] == [0, 0, 0]
                for l in range(len(layers)):
                    for other in runs[1:]:
                        for k in (0, 1):
                            assert runs[0][1][l][k].buf.cpu().numpy().tobytes() == other[1][l][k].buf.cpu().numpy().tobytes()
    # a layer that cannot take 16-byte pieces: the forced vector path is refused and writes nothing
    layers, y_pix = SPLITS[2]
    y, psi = _inputs(1, h, w, y_pix)
    yd, *geo = _plane(dev, y, False)
    rc, outs = _layers_call(env, yd, geo, y_pix, 1, h, w, 2, [0, 1], torch.from_numpy(psi).to(dev), layers, _lib.CTX_VECTOR)
    assert rc == -1 and all(win.untouched() and comb.untouched() for win, comb in outs)
