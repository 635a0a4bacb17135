"""lic_ctx_gather_layers_ragged on an MI355X through the C ABI: every layer's rows of three images of different sizes
and slice heights in one launch, `==` against lic_ctx_gather_ragged run per layer (M = M_l, every Y_ORIGIN raised by c0)
and against the numpy statements (ctx_layers_ref.py, whose tap rule is ctx_slices_ref's).  The planes lie framed in one
flat buffer with guard floats between them, every input value is distinct (latents positive, psi negative, frames and
guards a third and fourth range), and every output lives between canaries (guarded.py)."""
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
SHAPES = [(3, 5), (4, 4), (1, 7)]
RS = [2, 4, 1]
BAD_ROWS = [(1, 4 * 4 + 3), (7, 0), (-1, 0), (0, -1), (3, 2)]   # pixel past the plane, image past the table, negatives
# (layers [(c0, M_l)], y_pix): (17, 13) has a misaligned c0 and odd widths, y_pix 30 / 33 a pitch no 16-byte piece fits
SPLITS = [([(0, 20), (20, 12)], 32), ([(0, 17), (17, 13)], 30), ([(0, 17), (17, 13)], 33),
          ([(0, 8), (8, 4), (12, 4)], 16), ([(5, 12)], 20)]
GAPS = [0, 3]                                       # guard floats: plane bases that are, and are not, multiples of 4


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    dev = torch.device("cuda:0")
    return _lib, F_, dev, torch.tensor(SR.TAPS, dtype=torch.int32, device=dev)


_CASES = {}


def _case(split, gap):
    """the flat buffers of SPLITS[split] with `gap` guard floats in front of every plane, the descriptor table, the row
    lists and the restatement's rows per layer, computed once -> dict"""
    if (split, gap) in _CASES:
        return _CASES[split, gap]
    layers, y_pix = SPLITS[split]
    r = np.random.RandomState(5)
    desc, yparts, psiparts, y_at, psi_at, per_image = [], [], [], 0, 0, []
    for b, (h, w) in enumerate(SHAPES):
        y = (1.0 + 3000 * b + np.arange(h * w * y_pix, dtype=np.float32)).reshape(h, w, y_pix)
        psi = -(1.0 + 3000 * b + np.arange(h * w * CPSI, dtype=np.float32)).reshape(h * w, CPSI)
        frame = 5e6 + 3000 * b + np.arange((h + 2 * P) * (w + 2 * P) * y_pix, dtype=np.float32)
        frame = frame.reshape(h + 2 * P, w + 2 * P, y_pix)
        frame[P:P + h, P:P + w] = y
        yparts += [np.full(gap, 9e6, np.float32), frame.ravel()]
        psiparts += [np.full(gap, -9e6, np.float32), psi.ravel()]
        y_at, psi_at = y_at + gap, psi_at + gap
        desc.append([y_at, (w + 2 * P) * y_pix, (P * (w + 2 * P) + P) * y_pix, psi_at, h, w, RS[b], 0])
        y_at, psi_at = y_at + frame.size, psi_at + psi.size
        per_image.append(LR.gather_layers(y[None], RS[b], list(range(h * w)), layers, psi=psi[None]))
    yparts.append(np.full(gap + 4, 9e6, np.float32))
    psiparts.append(np.full(gap + 4, -9e6, np.float32))
    rows = [(b, px) for b, (h, w) in enumerate(SHAPES) for px in range(h * w)]
    rows = [rows[k] for k in r.permutation(len(rows))]                      # shuffled image order
    for k, bad in zip((2, 9, 17, 30, 41), BAD_ROWS):
        rows.insert(k, bad)
    want = []
    for l, (c0, M) in enumerate(layers):
        win, prow = np.zeros((len(rows), NT * M), np.float32), np.zeros((len(rows), CPSI), np.float32)
        for k, (b, px) in enumerate(rows):
            if 0 <= b < len(SHAPES) and 0 <= px < SHAPES[b][0] * SHAPES[b][1]:
                win[k], prow[k] = per_image[b][l][0][px], per_image[b][l][1][px]
        want.append((win, prow))
    _CASES[split, gap] = dict(layers=layers, y_pix=y_pix, y=np.concatenate(yparts), psi=np.concatenate(psiparts),
                              desc=np.array(desc, np.int64), rows=rows, want=want)
    return _CASES[split, gap]


def _outputs(dev, layers, rows):
    """per layer a guarded win [rows][NT * M_l] and a guarded comb whose psi columns start behind 2 M_l others"""
    outs = []
    for _, M in layers:
        cctx = 2 * M
        ld = (cctx + CPSI + 4 + 3) // 4 * 4 if M % 2 == 0 else cctx + CPSI + 3
        outs.append((Guarded(rows, NT * M, dev), Guarded(rows, CPSI, dev, ld=ld, col0=cctx)))
    return outs


def _device(env, case, desc=None):
    dev = env[2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = case["rows"]
    return (up(case["y"]), up(case["psi"]), up(case["desc"] if desc is None else desc),
            up(np.array([b for b, _ in rows], np.int64)), up(np.array([px for _, px in rows], np.int64)))


def _layers_ragged(env, case, path=0, with_psi=True, desc=None, y_len=None):
    """one call of the new entry -> (status, [(guarded win, guarded comb) per layer])"""
    _lib, F_, dev, taps = env
    layers, n = case["layers"], len(case["rows"])
    d_y, d_psi, d_desc, d_img, d_pix = _device(env, case, desc)
    outs = _outputs(dev, layers, n)
    table = (_lib.CtxLayer * len(layers))()
    for t, (c0, M), (win, comb) in zip(table, layers, outs):
        t.win, t.comb, t.comb_ld, t.c0, t.M = win.ptr(), comb.ptr() if with_psi else None, comb.ld, c0, M
    rc = _lib.load().lic_ctx_gather_layers_ragged(
        F_._ptr(d_y), d_y.numel() if y_len is None else y_len, case["y_pix"], F_._ptr(d_desc), len(SHAPES), F_._ptr(taps),
        NT, F_._ptr(d_img), F_._ptr(d_pix), n, F_._ptr(d_psi) if with_psi else None, d_psi.numel() if with_psi else 0,
        CPSI if with_psi else 0, table, len(layers), path, F_._stream())
    torch.cuda.synchronize()
    return rc, outs


def _one_layer_ragged(env, case, layer, path=0, desc=None):
    """lic_ctx_gather_ragged for this layer alone: M = M_l, every descriptor's Y_ORIGIN raised by c0"""
    _lib, F_, dev, taps = env
    c0, M = layer
    n = len(case["rows"])
    moved = (case["desc"] if desc is None else desc).copy()
    moved[:, 2] += c0
    d_y, d_psi, d_desc, d_img, d_pix = _device(env, case, moved)
    (win, comb), = _outputs(dev, [layer], n)
    rc = _lib.load().lic_ctx_gather_ragged(
        F_._ptr(d_y), d_y.numel(), case["y_pix"], F_._ptr(d_desc), len(SHAPES), M, F_._ptr(taps), NT, F_._ptr(d_img),
        F_._ptr(d_pix), n, C.c_void_p(win.ptr()), F_._ptr(d_psi), d_psi.numel(), CPSI, C.c_void_p(comb.ptr()), comb.ld,
        path, F_._stream())
    torch.cuda.synchronize()
    return rc, win, comb


def _check(case, outs, want, what, with_psi=True):
    for l, ((win, comb), (want_win, want_psi)) in enumerate(zip(outs, want)):
        win.check(f"{what} layer {l}")
        assert np.array_equal(win.cpu().numpy(), want_win), (what, l)
        if with_psi:
            comb.check(f"{what} layer {l}")
            assert np.array_equal(comb.cpu().numpy(), want_psi), (what, l)
        else:
            assert comb.untouched(), (what, l)


def _can_vector(case):
    return case["y_pix"] % 4 == 0 and all(c0 % 4 == 0 and M % 4 == 0 for c0, M in case["layers"])


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("split", range(len(SPLITS)))
def test_layers_of_three_images_match_the_ragged_gather_per_layer_and_the_restatement(env, split, gap):
    _lib = env[0]
    case = _case(split, gap)
    paths = [_lib.CTX_AUTO, _lib.CTX_ELEMENT] + ([_lib.CTX_VECTOR] if _can_vector(case) else [])
    runs = {}
    for path in paths:
        rc, outs = _layers_ragged(env, case, path)
        assert rc == 0
        _check(case, outs, case["want"], f"split {split} gap {gap} path {path}")
        runs[path] = outs
    # the five bad rows are rows of zeros in every layer
    for win, comb in runs[_lib.CTX_AUTO]:
        w_, c_ = win.cpu().numpy(), comb.cpu().numpy()
        for k, row in enumerate(case["rows"]):
            if row in BAD_ROWS:
                assert (w_[k] == 0).all() and (c_[k] == 0).all()
    # bit for bit the one-layer ragged entry, fences and pitch columns included; every path writes the same bytes
    for l, layer in enumerate(case["layers"]):
        rc, win1, comb1 = _one_layer_ragged(env, case, layer)
        assert rc == 0
        for path in paths:
            win, comb = runs[path][l]
            assert win.buf.cpu().numpy().tobytes() == win1.buf.cpu().numpy().tobytes(), (l, path)
            assert comb.buf.cpu().numpy().tobytes() == comb1.buf.cpu().numpy().tobytes(), (l, path)
    if not _can_vector(case):                                   # forced where a layer cannot hold it: refused, nothing written
        rc, outs = _layers_ragged(env, case, _lib.CTX_VECTOR)
        assert rc == -1 and all(win.untouched() and comb.untouched() for win, comb in outs)


def test_without_psi_no_comb_is_touched(env):
    for split in (0, 2):
        case = _case(split, 3)
        rc, outs = _layers_ragged(env, case, with_psi=False)
        assert rc == 0
        _check(case, outs, case["want"], f"split {split} without psi", with_psi=False)


def _without_image(case, b):
    mine = np.array([bb == b for bb, _ in case["rows"]])
    want = []
    for win, prow in case["want"]:
        win, prow = win.copy(), prow.copy()
        win[mine], prow[mine] = 0, 0
        want.append((win, prow))
    return want


def test_a_descriptor_that_cannot_be_right_gives_zero_rows_in_every_layer(env):
    """each damaged field of image 1's descriptor zeroes image 1's rows of every layer and leaves the others exact"""
    case = _case(0, 0)
    want = _without_image(case, 1)
    y_len, psi_len = case["y"].size, case["psi"].size
    for word, value in ((0, -4), (0, y_len), (0, 1 << 50), (1, -8), (1, y_len), (2, -4), (2, 1 << 41), (3, -8),
                        (3, psi_len - 8), (3, 1 << 62), (4, 0), (4, 1 << 20), (5, 0), (5, 1 << 33), (6, 0), (6, -3)):
        desc = case["desc"].copy()
        desc[1, word] = value
        rc, outs = _layers_ragged(env, case, desc=desc)
        assert rc == 0
        _check(case, outs, want, f"word {word} = {value}")


@pytest.mark.parametrize("split", [0, 4])
def test_the_last_float_is_measured_for_the_widest_layer(env, split):
    """y_len one float short of the last plane's last pixel's channel max(c0 + M_l): that image is refused in every
    layer, the narrower ones included; with that float inside, every row is exact.  The buffer itself stays whole."""
    case = _case(split, 3)
    widest = max(c0 + M for c0, M in case["layers"])
    d = case["desc"][2]
    last = int(d[0] + d[2] + (d[4] - 1) * d[1] + (d[5] - 1) * case["y_pix"] + widest)
    rc, outs = _layers_ragged(env, case, y_len=last)
    assert rc == 0
    _check(case, outs, case["want"], "the last float inside")
    rc, outs = _layers_ragged(env, case, y_len=last - 1)
    assert rc == 0
    _check(case, outs, _without_image(case, 2), "the last float outside")
