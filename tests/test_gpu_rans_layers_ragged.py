"""lic_rans_decode_step_layers_ragged on an MI355X: all layers of a step of three images that bring different numbers
of rows, or none, in one launch.  Eleven consecutive launches carry the state blocks.  After every step the state
blocks (all 67 words) and the decoded values are compared with lic_rans_decode_step_ragged run per layer into a plane
of that layer's own; after the last step with the symbols of the Python decoder of tests/rans_groups_ref.py, whose
coder wrote the streams over synthetic tables.  The planes lie in one flat buffer between guard floats, everything
pre-filled with a sentinel.  With equal images the entry is compared with lic_rans_decode_step_layers.

A table row has S + 1 = 2 W + 2 dwords, an even number, so an image's tables start at 0 or 2 mod 4 dwords: both occur
here (odd M_l behind an odd number of rows), and the test says so."""
import numpy as np
import pytest
import torch

import rans_groups_ref as GR

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
GAP = 5                                            # sentinel floats in front of every plane and behind the last
NIMG = 3
# rows per (image, step): image 0 grows to 11 rows (220 symbols with M_l = 20: more than 64 G for G = 1, 3), image 1 is
# idle in four steps, image 2 finishes after five
RAGGED = ((1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11), (3, 0, 5, 0, 7, 1, 0, 11, 2, 0, 4), (11, 10, 9, 8, 6, 0, 0, 0, 0, 0, 0))
EQUAL = (tuple(range(1, 12)),) * 3
STEPS = 11


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    return _lib, F_, torch.device("cuda:0")


_DATA = {}


def _layer_images(rows, M, W, escapes, seed, G):
    """one layer's three images: tables, symbols, centres and the Python coder's G sub-streams each, made once"""
    key = (rows, M, W, escapes, seed, G)
    if key in _DATA:
        return _DATA[key]
    from oracle import codec_ref as CR
    S = 2 * W + 1
    r = np.random.RandomState(seed)
    imgs = []
    for b, shape in enumerate((0.3, 0.05, 2.0)):
        steps = [n * M for n in rows[b]]
        nsym = sum(steps)
        f = r.gamma(shape, 1.0, size=(nsym, S)) + 1e-9
        F = np.concatenate([np.zeros((nsym, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
        F[:, -1] = 1.0
        t = CR.quantize_cdf(F).astype(np.uint32)
        u = r.randint(0, 65536, size=nsym)
        idx = np.array([np.searchsorted(t[k], u[k], side="right") - 1 for k in range(nsym)], np.int32)
        idx = idx.clip(1, max(S - 2, 1))
        if escapes:       # edge symbols by hand: first symbol, the last lane of a full round, the middle, the last symbols
            for k, v in ((0, -3), (min(63, nsym - 1), S + 100000), (nsym // 2, -100000), (nsym // 2 + 1, 0),
                         (nsym - 2, S - 1), (nsym - 1, S + 7)):
                idx[k] = v
        streams, escs = GR.encode(t, idx, steps, G)
        assert (GR.decode(streams, escs, t, steps) == idx).all()
        assert escapes or all(len(e) == 0 for e in escs)
        imgs.append(dict(steps=steps, tabs=t, idx=idx, center=r.randint(-10, 11, size=nsym).astype(np.int32),
                         streams=streams, escs=escs))
    _DATA[key] = imgs
    return imgs


def _case(rows, split, W, G):
    """per layer its three images; escapes in layer 0 only"""
    return [_layer_images(rows, M, W, l == 0, 40 + 7 * l, G) for l, (_, M) in enumerate(split)]


def _dests(rows):
    """per image: its plane's pixel count and the destination of every row, distinct over the whole call"""
    r = np.random.RandomState(3)
    out = []
    for b in range(NIMG):
        npx = sum(rows[b]) + 3
        out.append((npx, r.permutation(npx)[:sum(rows[b])].astype(np.int64)))
    return out


def _stage(env, streams, escs, shorten=None):
    """streams and escape lists -> (the six staging tensors of the decode entries, the seed state blocks)"""
    _lib, _, dev = env
    nb = len(streams)
    s_off = np.zeros(nb + 1, np.int64)
    for i in range(nb):
        s_off[i + 1] = s_off[i] + (len(streams[i]) + 3) // 4 * 4
    s_len = np.array([len(s) for s in streams], np.int64)
    if shorten is not None:
        s_len[shorten] -= 2
    buf = np.zeros(int(s_off[nb]) + 64, np.uint8)
    state = np.zeros((nb, _lib.RANS_STATE_WORDS), np.uint32)
    for i in range(nb):
        buf[s_off[i]:s_off[i] + len(streams[i])] = np.frombuffer(streams[i], np.uint8)
        state[i, :64] = np.frombuffer(streams[i][:256], "<u4")
    e_off = np.concatenate([[0], np.cumsum([len(e) // 4 for e in escs])]).astype(np.int64)
    e_all = np.frombuffer(b"".join(escs) + bytes(4), "<u4").astype(np.uint32)
    up = lambda a: torch.from_numpy(a).to(dev)
    return [up(buf), up(s_off), up(s_len), up(e_all.view(np.int32)), up(e_off), up(state.view(np.int32))], state


def _layout(rows, pitch, gap):
    dests, y_base, at = _dests(rows), [], 0
    for npx, _ in dests:
        y_base.append(at + gap)
        at += gap + npx * pitch
    return dests, y_base, at + gap


def _all_blocks(case):
    return [s for imgs in case for im in imgs for s in im["streams"]], [e for imgs in case for im in imgs for e in im["escs"]]


def _run(env, rows, split, y_pix, W, G, shorten=None, per_layer=True, gap=GAP):
    """the eleven launches of the new entry; with `per_layer`, lic_rans_decode_step_ragged per layer beside it, compared
    after every step -> (flat plane buffer, y_base, state blocks [L * 3 * G][67], table start offsets mod 4 seen)"""
    _lib, F_, dev = env
    lib, case, S1 = _lib.load(), _case(rows, split, W, G), 2 * W + 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    staged, _ = _stage(env, *_all_blocks(case), shorten)
    dests, y_base, size = _layout(rows, y_pix, gap)
    ypad = torch.full((size,), SENTINEL, device=dev)
    d_ybase, d_pixels = up(np.array(y_base, np.int64)), up(np.array([npx for npx, _ in dests], np.int64))
    own = []                                                             # per layer: its own staging, plane and bases
    for l, (imgs, (_, M)) in enumerate(zip(case, split)):
        short = None if shorten is None or shorten // (NIMG * G) != l else shorten % (NIMG * G)
        st, _ = _stage(env, [s for im in imgs for s in im["streams"]], [e for im in imgs for e in im["escs"]], short)
        _, base_l, size_l = _layout(rows, M, gap)
        own.append((st, torch.full((size_l,), SENTINEL, device=dev), base_l, up(np.array(base_l, np.int64))))
    row_at, starts = [0] * NIMG, set()
    for t in range(STEPS):
        n = [rows[b][t] for b in range(NIMG)]
        first = [sum(n[:b]) for b in range(NIMG)]
        dst = up(np.concatenate([dests[b][1][row_at[b]:row_at[b] + n[b]] for b in range(NIMG)]))
        seg = up(np.array([[first[b], n[b]] for b in range(NIMG)], np.int32))
        table, keep = (_lib.RansLayer * len(split))(), []
        for l, (imgs, (c0, M)) in enumerate(zip(case, split)):
            part = lambda key: np.concatenate([imgs[b][key][row_at[b] * M:(row_at[b] + n[b]) * M] for b in range(NIMG)])
            d_t, d_c = up(part("tabs").view(np.int32)), up(part("center"))
            assert d_t.shape == (sum(n) * M, S1)                         # the last image's last row ends the buffer
            keep.append((d_t, d_c))
            table[l].tables, table[l].center, table[l].c0, table[l].M = d_t.data_ptr(), d_c.data_ptr(), c0, M
            starts |= {first[b] * M * S1 % 4 for b in range(NIMG) if n[b]}
        before = staged[5].cpu().numpy().copy()
        rc = lib.lic_rans_decode_step_layers_ragged(
            *[F_._ptr(a) for a in staged], table, len(split), F_._ptr(seg), NIMG, G, sum(n), W, F_._ptr(dst),
            F_._ptr(ypad), F_._ptr(d_ybase), F_._ptr(d_pixels), size, y_pix, F_._stream())
        assert rc == 0
        if per_layer:
            for l, ((st, plane, _, d_base), (d_t, d_c), (_, M)) in enumerate(zip(own, keep, split)):
                rc = lib.lic_rans_decode_step_ragged(*[F_._ptr(a) for a in st], F_._ptr(d_t), F_._ptr(d_c), F_._ptr(seg),
                                                     NIMG, G, sum(n), M, W, F_._ptr(dst), F_._ptr(plane), F_._ptr(d_base),
                                                     F_._ptr(d_pixels), plane.numel(), F_._stream())
                assert rc == 0
        torch.cuda.synchronize()
        got, y = staged[5].cpu().numpy(), ypad.cpu().numpy()
        for l, ((c0, M), (st, plane, base_l, _)) in enumerate(zip(split, own)):
            blocks = slice(l * NIMG * G, (l + 1) * NIMG * G)
            if per_layer:
                assert np.array_equal(got[blocks], st[5].cpu().numpy()), f"step {t}, layer {l}: state blocks"
                p = plane.cpu().numpy()
                for b, (npx, _) in enumerate(dests):
                    mine = y[y_base[b]:y_base[b] + npx * y_pix].reshape(npx, y_pix)[:, c0:c0 + M]
                    assert np.array_equal(mine, p[base_l[b]:base_l[b] + npx * M].reshape(npx, M)), f"step {t}, layer {l}"
            for b in range(NIMG):
                rounds = (n[b] * M + 63) // 64
                idle = [blocks.start + b * G + g for g in range(G) if g >= rounds]       # the whole image when n[b] == 0
                assert np.array_equal(got[idle], before[idle]), f"step {t}, layer {l}: a block that sat out was written"
                if rounds and shorten is None:
                    assert not np.array_equal(got[blocks.start + b * G], before[blocks.start + b * G])
        for b in range(NIMG):
            row_at[b] += n[b]
    return ypad.cpu().numpy(), y_base, staged[5].cpu().numpy().view(np.uint32), starts


def _expected(rows, split, y_pix, W, case, size, y_base, which=range(NIMG), centre_of=()):
    """from the symbols the Python decoder returned: idx + centre - W at (dest pixel, c0 + channel), the sentinel
    elsewhere; `centre_of`: (layer, image) pairs decoded as the table centre instead"""
    want = np.full(size, SENTINEL, np.float32)
    dests = _dests(rows)
    for l, ((c0, M), imgs) in enumerate(zip(split, case)):
        for b in which:
            im = imgs[b]
            idx = np.full_like(im["idx"], W) if (l, b) in centre_of else im["idx"]
            v = (idx.astype(np.int64) + im["center"] - W).astype(np.float32).reshape(-1, M)
            for k, d in enumerate(dests[b][1]):
                at = y_base[b] + d * y_pix + c0
                want[at:at + M] = v[k]
    return want


CASES = [([(0, 20), (20, 12)], 32, 24, 1), ([(0, 20), (20, 12)], 32, 24, 3), ([(0, 20), (20, 12)], 32, 24, 8),
         ([(0, 17), (17, 13)], 30, 24, 1), ([(0, 17), (17, 13)], 33, 24, 3), ([(0, 17), (17, 13)], 30, 24, 8),
         ([(0, 8), (8, 4), (12, 4)], 16, 24, 3), ([(0, 20), (20, 12)], 32, 1, 3), ([(0, 17), (17, 13)], 30, 64, 3),
         ([(5, 12)], 20, 24, 3)]                                  # one layer, c0 > 0, y_pix > M_l


def _check_final(case, state):
    streams, escs = _all_blocks(case)
    assert (state[:, 66] == 0).all(), state[:, 66]
    for i in range(len(streams)):
        assert state[i, 64] == (len(streams[i]) - 256) // 2 and state[i, 65] == len(escs[i]) // 4, i
    assert (state[:, :64] == 1 << 16).all()


@pytest.mark.parametrize("split,y_pix,W,G", CASES)
def test_layers_of_ragged_images_in_one_launch(env, split, y_pix, W, G):
    y, y_base, state, starts = _run(env, RAGGED, split, y_pix, W, G)
    case = _case(RAGGED, split, W, G)
    want = _expected(RAGGED, split, y_pix, W, case, y.size, y_base)
    assert np.array_equal(y, want), "decoded values, or elements no layer owns (channels, guards), differ"
    assert (y == SENTINEL).sum() == (want == SENTINEL).sum() > 2 * GAP
    _check_final(case, state)
    assert sum(len(e) for im in case[0] for e in im["escs"]) >= 4 * 4 * NIMG          # layer 0's escapes were coded
    if any(M % 2 for _, M in split) and W != 1:
        assert starts == {0, 2}                                                     # both reachable table offsets mod 4
    else:
        assert starts <= {0, 2}


def test_one_layer_over_the_whole_plane_is_the_ragged_entry(env):
    """L = 1, c0 = 0, y_pix = M: `_run` compares with lic_rans_decode_step_ragged after every step, into equal planes"""
    y, y_base, state, _ = _run(env, RAGGED, [(0, 13)], 13, 24, 3)
    case = _case(RAGGED, [(0, 13)], 24, 3)
    assert np.array_equal(y, _expected(RAGGED, [(0, 13)], 13, 24, case, y.size, y_base))
    _check_final(case, state)


@pytest.mark.parametrize("split,y_pix,W,G", [CASES[1], CASES[4], CASES[8]])
def test_equal_images_are_the_layered_entry(env, split, y_pix, W, G):
    """every image at seg[b] = (b n, n) and y_base[b] = b * pixels * y_pix: planes and state blocks of
    lic_rans_decode_step_layers"""
    _lib, F_, dev = env
    lib, case = _lib.load(), _case(EQUAL, split, W, G)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    npx = sum(EQUAL[0]) + 3
    dest = np.random.RandomState(9).permutation(npx)[:sum(EQUAL[0])].astype(np.int64)
    runs = {}
    for which in ("ragged", "layers"):
        staged, _ = _stage(env, *_all_blocks(case))
        ypad = torch.full((NIMG * npx * y_pix,), SENTINEL, device=dev)
        d_ybase, d_pixels = up(np.arange(NIMG, dtype=np.int64) * npx * y_pix), up(np.full(NIMG, npx, np.int64))
        at = 0
        for n in EQUAL[0]:
            table, keep = (_lib.RansLayer * len(split))(), []
            for l, (imgs, (c0, M)) in enumerate(zip(case, split)):
                part = lambda key: np.concatenate([im[key][at * M:(at + n) * M] for im in imgs])
                keep.append((up(part("tabs").view(np.int32)), up(part("center"))))
                table[l].tables, table[l].center, table[l].c0, table[l].M = keep[-1][0].data_ptr(), keep[-1][1].data_ptr(), c0, M
            front = [F_._ptr(a) for a in staged]
            if which == "layers":
                d_dest = up(dest[at:at + n])
                rc = lib.lic_rans_decode_step_layers(*front, table, len(split), NIMG, G, n, W, F_._ptr(d_dest),
                                                     F_._ptr(ypad), npx, y_pix, F_._stream())
            else:
                d_dest = up(np.tile(dest[at:at + n], NIMG))
                seg = up(np.array([[b * n, n] for b in range(NIMG)], np.int32))
                rc = lib.lic_rans_decode_step_layers_ragged(*front, table, len(split), F_._ptr(seg), NIMG, G, NIMG * n, W,
                                                            F_._ptr(d_dest), F_._ptr(ypad), F_._ptr(d_ybase),
                                                            F_._ptr(d_pixels), ypad.numel(), y_pix, F_._stream())
            assert rc == 0
            torch.cuda.synchronize()
            at += n
        runs[which] = (ypad.cpu().numpy(), staged[5].cpu().numpy().view(np.uint32))
    assert np.array_equal(runs["ragged"][0], runs["layers"][0]) and np.array_equal(runs["ragged"][1], runs["layers"][1])
    assert (runs["ragged"][0] != SENTINEL).any()
    _check_final(case, runs["ragged"][1])


def test_a_sub_stream_one_word_short_reports_for_itself_alone(env):
    """block (layer 1, image 0, group 1) is given one word short: the cursor rule refuses the word, that block's error
    word is set and no other; every other layer and image is exact, image 0 of layer 1 decodes right values or the
    table centre, and the same elements are written"""
    split, y_pix, W, G = [(0, 20), (20, 12)], 32, 24, 3
    case = _case(RAGGED, split, W, G)
    blk = (1 * NIMG + 0) * G + 1
    assert len(case[1][0]["streams"][1]) > 256                          # the sub-stream has a word to lose
    y, y_base, state, _ = _run(env, RAGGED, split, y_pix, W, G, shorten=blk)        # equal to the per-layer runs throughout
    assert state[blk, 66] != 0 and (np.delete(state[:, 66], blk) == 0).all(), state[:, 66]
    full = _expected(RAGGED, split, y_pix, W, case, y.size, y_base)
    centre = _expected(RAGGED, split, y_pix, W, case, y.size, y_base, centre_of={(1, 0)})
    assert np.array_equal(y == SENTINEL, full == SENTINEL)
    assert ((y == full) | (y == centre)).all()
    differs = np.flatnonzero(y != full)
    npx = _dests(RAGGED)[0][0]
    assert all(y_base[0] <= k < y_base[0] + npx * y_pix and 20 <= (k - y_base[0]) % y_pix for k in differs)


def test_segments_and_planes_are_checked_on_the_device(env):
    """a segment that leaves the step, a plane that leaves the buffer: LIC_RANS_ERR_RANGE in that image's blocks of
    every layer, nothing of it written, the other images exact.  Compared before anything is addressed."""
    _lib, F_, dev = env
    split, y_pix, W, G = [(0, 17), (17, 13)], 30, 24, 1
    lib, case = _lib.load(), _case(RAGGED, split, W, G)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = [RAGGED[b][0] for b in range(NIMG)]
    dests, good_base, size = _layout(RAGGED, y_pix, GAP)
    dst = up(np.concatenate([dests[b][1][:n[b]] for b in range(NIMG)]))
    table, keep = (_lib.RansLayer * 2)(), []
    for l, (imgs, (c0, M)) in enumerate(zip(case, split)):
        keep.append((up(np.concatenate([imgs[b]["tabs"][:n[b] * M] for b in range(NIMG)]).view(np.int32)),
                     up(np.concatenate([imgs[b]["center"][:n[b] * M] for b in range(NIMG)]))))
        table[l].tables, table[l].center, table[l].c0, table[l].M = keep[-1][0].data_ptr(), keep[-1][1].data_ptr(), c0, M
    good_px = np.array([npx for npx, _ in dests], np.int64)
    good_seg = np.array([[0, n[0]], [n[0], n[1]], [n[0] + n[1], n[2]]], np.int32)
    step0 = [[dict(im, idx=im["idx"][:n[b] * M], center=im["center"][:n[b] * M]) for b, im in enumerate(imgs)]
             for imgs, (_, M) in zip(case, split)]
    cases = [(dict(seg=(1, [n[0], n[1] + n[2] + 1])), 1), (dict(seg=(1, [-1, 3])), 1), (dict(seg=(2, [5, -2])), 2),
             (dict(base=(0, -1)), 0), (dict(base=(2, size - 3)), 2), (dict(px=(1, -4)), 1), (dict(px=(1, 1 << 50)), 1),
             (dict(base=(1, 1 << 50)), 1), (dict(px=(2, (size - good_base[2]) // y_pix + 1)), 2)]
    for change, hit in cases:
        seg, base, px = good_seg.copy(), np.array(good_base, np.int64), good_px.copy()
        for key, (b, v) in change.items():
            {"seg": seg, "base": base, "px": px}[key][b] = v
        st, seed = _stage(env, *_all_blocks(case))
        ypad = torch.full((size,), SENTINEL, device=dev)
        d_seg, d_base, d_px = up(seg), up(base), up(px)
        rc = lib.lic_rans_decode_step_layers_ragged(*[F_._ptr(a) for a in st], table, 2, F_._ptr(d_seg), NIMG, G, sum(n),
                                                    W, F_._ptr(dst), F_._ptr(ypad), F_._ptr(d_base), F_._ptr(d_px), size,
                                                    y_pix, F_._stream())
        assert rc == 0
        torch.cuda.synchronize()
        state, y = st[5].cpu().numpy().view(np.uint32), ypad.cpu().numpy()
        hits = [l * NIMG + hit for l in range(2)]
        assert (state[hits, 66] == 1).all() and (np.delete(state[:, 66], hits) == 0).all(), (change, state[:, 66])
        others = [b for b in range(NIMG) if b != hit]
        want = np.full(size, SENTINEL, np.float32)
        for l, ((c0, M), imgs) in enumerate(zip(split, step0)):
            for b in others:
                v = (imgs[b]["idx"].astype(np.int64) + imgs[b]["center"] - W).astype(np.float32).reshape(-1, M)
                for k, d in enumerate(dests[b][1][:n[b]]):
                    want[good_base[b] + d * y_pix + c0:good_base[b] + d * y_pix + c0 + M] = v[k]
        assert np.array_equal(y, want), change
        if "seg" in change:
            assert np.array_equal(np.delete(state[hits], 66, axis=1), np.delete(seed[hits], 66, axis=1))
