"""lic_ctx_gather_ragged on an MI355X through the C ABI: rows of three images of different sizes and slice heights
in one launch, `==` against lic_ctx_gather run on every image alone and against ctx_slices_ref.gather.  The planes lie
framed in one flat buffer with guard floats between them, every input value is distinct (latents positive, psi
negative, frames and guards a third and fourth range), and every output sits between canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctx_slices_ref as SR

pytestmark = pytest.mark.gpu

P = SR.PAD
SHAPES = [(3, 5), (4, 4), (1, 7)]
RS = [2, 4, 1]
CANARY = -12345.0
GUARD = 3                                          # canary rows in front of and behind every output
C0, CEXTRA = 8, 4                                  # the psi columns start at C0 of a buffer CEXTRA columns wider
NT = len(SR.TAPS)
BAD_ROWS = [(1, 4 * 4 + 3), (7, 0), (-1, 0), (0, -1), (3, 2)]   # pixel past the plane, image past the table, negatives


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    dev = torch.device("cuda:0")
    return _lib, F_, dev, torch.tensor(SR.TAPS, dtype=torch.int32, device=dev)


_CASES = {}


def _case(M, gap):
    """the flat buffers for M channels with `gap` guard floats in front of every plane, the descriptor table, the row
    lists and the restatement's rows, computed once -> dict"""
    if (M, gap) in _CASES:
        return _CASES[M, gap]
    r = np.random.RandomState(5)
    ys, psis, desc, yparts, psiparts, y_at, psi_at = [], [], [], [], [], 0, 0
    for b, (h, w) in enumerate(SHAPES):
        y = (1.0 + 1000 * b + np.arange(h * w * M, dtype=np.float32)).reshape(h, w, M)
        psi = -(1.0 + 1000 * b + np.arange(h * w * 2 * M, dtype=np.float32)).reshape(h * w, 2 * M)
        frame = 5e6 + 1000 * b + np.arange((h + 2 * P) * (w + 2 * P) * M, dtype=np.float32)
        frame = frame.reshape(h + 2 * P, w + 2 * P, M)
        frame[P:P + h, P:P + w] = y
        yparts += [np.full(gap, 9e6, np.float32), frame.ravel()]
        psiparts += [np.full(gap, -9e6, np.float32), psi.ravel()]
        y_at, psi_at = y_at + gap, psi_at + gap
        desc.append([y_at, (w + 2 * P) * M, (P * (w + 2 * P) + P) * M, psi_at, h, w, RS[b], 0])
        y_at, psi_at = y_at + frame.size, psi_at + psi.size
        ys.append(y)
        psis.append(psi)
    yparts.append(np.full(gap, 9e6, np.float32))
    psiparts.append(np.full(gap, -9e6, np.float32))
    rows = [(b, px) for b, (h, w) in enumerate(SHAPES) for px in range(h * w)]
    rows = [rows[k] for k in r.permutation(len(rows))]                      # shuffled image order
    for k, bad in zip((2, 9, 17, 30, 41), BAD_ROWS):
        rows.insert(k, bad)
    want_win = np.zeros((len(rows), NT * M), np.float32)
    want_psi = np.zeros((len(rows), 2 * M), np.float32)
    for k, (b, px) in enumerate(rows):
        if 0 <= b < len(SHAPES) and 0 <= px < SHAPES[b][0] * SHAPES[b][1]:
            win, prow = SR.gather(ys[b][None], RS[b], [px], psi=psis[b][None])
            want_win[k], want_psi[k] = win[0], prow[0]
    _CASES[M, gap] = dict(M=M, y=np.concatenate(yparts), psi=np.concatenate(psiparts), desc=np.array(desc, np.int64),
                          rows=rows, want_win=want_win, want_psi=want_psi)
    return _CASES[M, gap]


def _ragged(env, case, path=0, with_psi=True, c0=C0, bad=None, desc=None):
    """one call -> (status, win buffer, comb buffer) with their canary rows, as numpy.  `bad`: arguments to replace"""
    _lib, F_, dev, taps = env
    M, rows = case["M"], case["rows"]
    n = len(rows)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_y, d_psi, d_desc = up(case["y"]), up(case["psi"]), up(case["desc"] if desc is None else desc)
    d_img, d_pix = up(np.array([b for b, _ in rows], np.int64)), up(np.array([px for _, px in rows], np.int64))
    win = torch.full((n + 2 * GUARD, NT * M), CANARY, device=dev)
    ld = C0 + 2 * M + CEXTRA
    comb = torch.full((n + 2 * GUARD, ld), CANARY, device=dev)
    a = dict(y=F_._ptr(d_y), y_len=d_y.numel(), y_pix=M, images=F_._ptr(d_desc), nimg=len(SHAPES), M=M,
             taps=F_._ptr(taps), nt=NT, row_image=F_._ptr(d_img), row_pix=F_._ptr(d_pix), rows=n,
             win=C.c_void_p(win[GUARD].data_ptr()), psi=F_._ptr(d_psi) if with_psi else None,
             psi_len=d_psi.numel() if with_psi else 0, Cpsi=2 * M if with_psi else 0,
             comb=C.c_void_p(comb[GUARD].data_ptr() + 4 * c0) if with_psi else None, comb_ld=ld if with_psi else 0,
             path=path, stream=F_._stream())
    a.update(bad or {})
    rc = _lib.load().lic_ctx_gather_ragged(*a.values())
    torch.cuda.synchronize()
    return rc, win.cpu().numpy(), comb.cpu().numpy()


def _check(got, want_win, want_psi, with_psi=True, c0=C0):
    rc, win, comb = got
    assert rc == 0
    n, M2 = want_win.shape[0], want_psi.shape[1]
    assert (win[:GUARD] == CANARY).all() and (win[GUARD + n:] == CANARY).all()
    assert np.array_equal(win[GUARD:GUARD + n], want_win)
    want = np.full_like(comb, CANARY)
    if with_psi:
        want[GUARD:GUARD + n, c0:c0 + M2] = want_psi
    assert np.array_equal(comb, want)


def _single(env, case, b):
    """lic_ctx_gather on image b alone, for the pixels the ragged call lists for it -> (row numbers, win, psi rows)"""
    _lib, F_, dev, taps = env
    M, d = case["M"], case["desc"][b]
    h, w = SHAPES[b]
    ks = [k for k, (bb, px) in enumerate(case["rows"]) if bb == b and 0 <= px < h * w]
    pix = torch.tensor([case["rows"][k][1] for k in ks], dtype=torch.int64, device=dev)
    y = torch.from_numpy(case["y"][d[0]:d[0] + (h + 2 * P) * (w + 2 * P) * M].copy()).to(dev)
    psi = torch.from_numpy(case["psi"][d[3]:d[3] + h * w * 2 * M].copy()).to(dev)
    win = torch.empty((len(ks), NT * M), device=dev)
    comb = torch.empty((len(ks), 2 * M), device=dev)
    rc = _lib.load().lic_ctx_gather(F_._ptr(y), y.numel(), int(d[1]), M, int(d[2]), 1, h, w, M, F_._ptr(taps), NT, RS[b],
                                    F_._ptr(pix), len(ks), F_._ptr(win), F_._ptr(psi), 2 * M, F_._ptr(comb), 2 * M,
                                    _lib.CTX_AUTO, F_._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return ks, win.cpu().numpy(), comb.cpu().numpy()


@pytest.mark.parametrize("M,gap", [(4, 8), (3, 5), (4, 3), (8, 0)])
def test_rows_of_three_images_match_each_image_alone_and_the_restatement(env, M, gap):
    """M = 4 with guards of 8 floats: the 16-byte kernel; M = 3: single floats; M = 4 with guards of 3 floats: the
    16-byte kernel meets bases that are no multiple of 4 and moves those rows float by float"""
    case = _case(M, gap)
    for with_psi in (True, False):
        got = _ragged(env, case, with_psi=with_psi)
        _check(got, case["want_win"], case["want_psi"], with_psi)
    rc, win, comb = got = _ragged(env, case)
    for k, bad in enumerate(case["rows"]):
        if bad in BAD_ROWS:
            assert (win[GUARD + k] == 0).all() and (comb[GUARD + k, C0:C0 + 2 * M] == 0).all()
    for b in range(len(SHAPES)):
        ks, swin, spsi = _single(env, case, b)
        assert len(ks) == SHAPES[b][0] * SHAPES[b][1]
        assert np.array_equal(win[GUARD:][ks], swin) and np.array_equal(comb[GUARD:][ks, C0:C0 + 2 * M], spsi)


@pytest.mark.parametrize("gap", [8, 3])
def test_forced_paths_write_the_same_bytes(env, gap):
    _lib = env[0]
    case = _case(4, gap)
    vec, one, auto = (_ragged(env, case, path=p) for p in (_lib.CTX_VECTOR, _lib.CTX_ELEMENT, _lib.CTX_AUTO))
    _check(vec, case["want_win"], case["want_psi"])
    for other in (one, auto):
        assert other[0] == 0 and other[1].tobytes() == vec[1].tobytes() and other[2].tobytes() == vec[2].tobytes()


def test_a_descriptor_that_cannot_be_right_gives_zero_rows_and_reads_nothing(env):
    """each damaged field of image 1's descriptor zeroes image 1's rows and leaves the other images' rows exact"""
    case = _case(4, 8)
    mine = np.array([b == 1 for b, _ in case["rows"]])
    want_win, want_psi = case["want_win"].copy(), case["want_psi"].copy()
    want_win[mine], want_psi[mine] = 0, 0
    y_len, psi_len = case["y"].size, case["psi"].size
    for word, value in ((0, -4), (0, y_len), (0, 1 << 50), (1, -8), (1, y_len), (2, -4), (2, 1 << 41), (3, -8),
                        (3, psi_len - 8), (3, 1 << 62), (4, 0), (4, -1), (4, 1 << 20), (4, 1 << 40), (5, 0),
                        (5, 1 << 33), (6, 0), (6, -3)):
        desc = case["desc"].copy()
        desc[1, word] = value
        _check(_ragged(env, case, desc=desc), want_win, want_psi)
    desc = case["desc"].copy()
    desc[1, 6] = 1 << 40                                                         # any R >= h is one slice: image 1's own R
    _check(_ragged(env, case, desc=desc), case["want_win"], case["want_psi"])


def test_refusals_launch_nothing(env):
    _lib, F_, dev, _ = env
    case = _case(4, 8)
    odd = torch.zeros(64, device=dev)
    at = lambda nbytes: C.c_void_p(odd.data_ptr() + nbytes)
    for bad in (dict(y=None), dict(images=None), dict(taps=None), dict(row_image=None), dict(row_pix=None),
                dict(win=None), dict(comb=None), dict(rows=0), dict(rows=-2), dict(nimg=0), dict(M=0), dict(nt=0),
                dict(y_len=0), dict(y_len=-5), dict(psi_len=0), dict(y_pix=3), dict(path=3), dict(Cpsi=0),
                dict(comb_ld=7), dict(y=at(2)), dict(win=at(1)), dict(images=at(4)), dict(row_image=at(4)),
                dict(row_pix=at(12)), dict(taps=at(2))):
        rc, win, comb = _ragged(env, case, bad=bad)
        assert rc == -1, bad
        assert (win == CANARY).all() and (comb == CANARY).all(), bad
    for bad in (dict(y_len=(1 << 40) + 4), dict(psi_len=(1 << 40) + 4)):
        rc, win, comb = _ragged(env, case, bad=bad)
        assert rc == -2 and (win == CANARY).all() and (comb == CANARY).all(), bad
    # the forced 16-byte path where the entry sees it cannot hold: M = 3, psi columns that start at column 2
    rc, win, comb = _ragged(env, _case(3, 5), path=_lib.CTX_VECTOR)
    assert rc == -1 and (win == CANARY).all() and (comb == CANARY).all()
    rc, win, comb = _ragged(env, case, path=_lib.CTX_VECTOR, c0=2)
    assert rc == -1 and (win == CANARY).all() and (comb == CANARY).all()
    _check(_ragged(env, case, c0=2), case["want_win"], case["want_psi"], c0=2)     # the automatic path takes it
    _check(_ragged(env, case), case["want_win"], case["want_psi"])
