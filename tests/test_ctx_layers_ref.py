"""The numpy statement of the layered gather (ctx_layers_ref.py) against the one-layer statement it extends
(ctx_slices_ref.py): with one layer over all channels it is that gather, and with several it is that gather on every
layer's channel slice.  Host only."""
import numpy as np
import pytest

import ctx_layers_ref as LR
import ctx_slices_ref as SR

B = 2
PLANES = [(4, 4), (5, 7)]


def _plane(h, w, y_pix):
    y = (1.0 + np.arange(B * h * w * y_pix, dtype=np.float32)).reshape(B, h, w, y_pix)
    psi = -(1.0 + np.arange(B * h * w * 6, dtype=np.float32)).reshape(B, h * w, 6)
    return y, psi


def _lists(h, w):
    return [list(range(h * w)), [h * w - 1], [2, h * w + 5, 0], [1, -1, 3]]


@pytest.mark.parametrize("h,w", PLANES)
def test_one_layer_over_all_channels_is_the_one_layer_gather(h, w):
    y, psi = _plane(h, w, 6)
    for R in (1, 2, 3, h + 1):
        for pix in _lists(h, w):
            for p in (psi, None):
                (win, rows), = LR.gather_layers(y, R, pix, [(0, 6)], psi=p)
                want_win, want_rows = SR.gather(y, R, pix, psi=p)
                assert np.array_equal(win, want_win)
                assert (rows is None and want_rows is None) or np.array_equal(rows, want_rows)


@pytest.mark.parametrize("split", [[(0, 20), (20, 12)], [(0, 17), (17, 13)], [(0, 1), (1, 7)], [(0, 8), (8, 4), (12, 4)],
                                   [(3, 5)]])
@pytest.mark.parametrize("h,w", PLANES)
def test_every_layer_is_the_one_layer_gather_on_its_channel_slice(h, w, split):
    y_pix = max(c0 + M for c0, M in split) + 2                       # two channels no layer owns
    y, psi = _plane(h, w, y_pix)
    for R in (2, h + 1):
        for pix in _lists(h, w):
            got = LR.gather_layers(y, R, pix, split, psi=psi)
            assert len(got) == len(split)
            for (c0, M), (win, rows) in zip(split, got):
                want_win, want_rows = SR.gather(np.ascontiguousarray(y[..., c0:c0 + M]), R, pix, psi=psi)
                assert win.shape == (B * len(pix), len(SR.TAPS) * M)
                assert np.array_equal(win, want_win) and np.array_equal(rows, want_rows)


def test_the_layers_do_not_see_each_other():
    """changing layer 1's channels leaves layer 0's rows as they are"""
    h, w = 4, 4
    y, psi = _plane(h, w, 8)
    pix = list(range(h * w))
    a = LR.gather_layers(y, 2, pix, [(0, 3), (3, 5)], psi=psi)
    y2 = y.copy()
    y2[..., 3:] += 1000.0
    b = LR.gather_layers(y2, 2, pix, [(0, 3), (3, 5)], psi=psi)
    assert np.array_equal(a[0][0], b[0][0]) and not np.array_equal(a[1][0], b[1][0])
