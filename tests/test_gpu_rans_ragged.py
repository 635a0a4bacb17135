"""lic_rans_decode_step_ragged on an MI355X: three images that bring different numbers of rows, or none, to four
consecutive steps.  After every step the state blocks (all 67 words), the decoded values (one flat buffer, canaries
around every plane) and the blocks of images that sat the step out are compared with lic_rans_decode_step_groups run
on every image alone with the same tables; after the last step with the host encoder's symbols as well.  Streams come
from codec.rans_encode_grouped; escapes are placed by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

import rans_groups_ref as GR

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
GAP = 5                                            # sentinel floats in front of every plane and behind the last
# rows per (image, step).  M = 1: 5, 64, 65 and 130 symbols, image 0 finishes early, image 1 is idle in step 1;
# M = 3: 3, 66 and 129 symbols, and with S + 1 = 6 image 1's tables of step 0 start at dword 18 = 2 mod 4
ROWS = {1: [[5, 64, 0, 0], [65, 0, 130, 5], [130, 65, 64, 130]],
        3: [[1, 22, 0, 0], [22, 0, 43, 2], [43, 22, 21, 43]]}
CONFIGS = [(1, 24, 1), (1, 24, 3), (3, 2, 1), (3, 2, 3), (1, 33, 3)]         # (M, W, G); W = 33: the wide variant


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import _lib, codec
    from neural_image_compression_amd import functional as F_
    return codec, _lib, F_, torch.device("cuda:0")


_SYN = {}


def _synthetic(codec, M, W, G):
    """tables, symbols, centres, destinations and the encoded sub-streams of the three images, made once"""
    if (M, W, G) in _SYN:
        return _SYN[M, W, G]
    from oracle import codec_ref as CR
    S, rows = 2 * W + 1, ROWS[M]
    r = np.random.RandomState(100 * M + W)
    imgs = []
    for b, shape in enumerate((0.3, 0.05, 2.0)):
        steps = [n * M for n in rows[b]]
        nsym = sum(steps)
        f = r.gamma(shape, 1.0, size=(nsym, S)) + 1e-9
        F = np.concatenate([np.zeros((nsym, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
        F[:, -1] = 1.0
        t = CR.quantize_cdf(F).astype(np.uint32)
        u = r.randint(0, 65536, size=nsym)
        idx = np.array([np.searchsorted(t[k], u[k], side="right") - 1 for k in range(nsym)], np.int32).clip(1, S - 2)
        # escapes and edge symbols by hand: first symbol, the last lane of a full round, the middle, the last symbol
        for k, v in ((0, -3), (min(63, nsym - 1), S + 100000), (nsym // 2, -100000), (nsym // 2 + 1, 0),
                     (nsym - 2, S - 1), (nsym - 1, S + 7)):
            idx[k] = v
        if b == 1:
            # image 1 ends in every table's most probable symbol: with these peaked tables such a symbol costs no word
            # as a rule, so a sub-stream reads its last word well before it ends and, cut by one word, has symbols left
            # to get wrong (rans_groups_ref.symbols_after_the_last_word counts them)
            late = np.arange(nsym * 3 // 5, nsym)
            idx[late] = np.diff(t[late].astype(np.int64), axis=1).argmax(1)
        npx = sum(rows[b]) + 3
        dest = r.permutation(npx)[:sum(rows[b])].astype(np.int64)                # distinct over the whole call
        streams, escs = codec.rans_encode_grouped(t, idx, steps, G)
        assert (codec.rans_decode_grouped(streams, escs, t, steps) == idx).all()
        imgs.append(dict(steps=steps, tabs=t, idx=idx, center=r.randint(-10, 11, size=nsym).astype(np.int32), dest=dest,
                         pixels=npx, streams=streams, escs=escs))
    _SYN[M, W, G] = imgs
    return imgs


def _stage(_lib, imgs, shorten=None):
    streams = [s for im in imgs for s in im["streams"]]
    escs = [e for im in imgs for e in im["escs"]]
    nb = len(streams)
    s_off = np.zeros(nb + 1, np.int64)
    for i in range(nb):
        s_off[i + 1] = s_off[i] + (len(streams[i]) + 3) // 4 * 4
    s_len = np.array([len(s) for s in streams], np.int64)
    if shorten is not None:
        s_len[shorten] -= 2
    buf = np.zeros(int(s_off[nb]), np.uint8)
    state = np.zeros((nb, _lib.RANS_STATE_WORDS), np.uint32)
    for i in range(nb):
        buf[s_off[i]:s_off[i] + len(streams[i])] = np.frombuffer(streams[i], np.uint8)
        state[i, :64] = np.frombuffer(streams[i][:256], "<u4")
    e_off = np.concatenate([[0], np.cumsum([len(e) // 4 for e in escs])]).astype(np.int64)
    e_all = np.frombuffer(b"".join(escs) + bytes(4), "<u4").astype(np.uint32)
    return buf, s_off, s_len, e_all.view(np.int32), e_off, state.view(np.int32)


def _run(env, M, W, G, shorten=None):
    """the four steps, ragged against per-image, compared after every step
    -> (flat latent buffer, y_base, state blocks [3 * G][67]) of the ragged run"""
    codec, _lib, F_, dev = env
    lib, imgs, rows, S1 = _lib.load(), _synthetic(codec, M, W, G), ROWS[M], 2 * W + 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    host = _stage(_lib, imgs, shorten)
    staged = {k: [up(a) for a in host] for k in ("ragged", "single")}           # each run carries its own blocks
    y_base, at = [], 0
    for im in imgs:
        y_base.append(at + GAP)
        at += GAP + im["pixels"] * M
    ypad = {k: torch.full((at + GAP,), SENTINEL, device=dev) for k in staged}
    d_ybase, d_pixels = up(np.array(y_base, np.int64)), up(np.array([im["pixels"] for im in imgs], np.int64))
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)
    sym_at, row_at = [0, 0, 0], [0, 0, 0]
    for t in range(4):
        n = [rows[b][t] for b in range(3)]
        first = [sum(n[:b]) for b in range(3)]
        part = lambda key, at, per: np.concatenate([imgs[b][key][at[b]:at[b] + per * n[b]] for b in range(3)])
        tabs, cen = up(part("tabs", sym_at, M).view(np.int32)), up(part("center", sym_at, M))
        dst = up(part("dest", row_at, 1))
        assert tabs.shape == (sum(n) * M, S1)                                    # the last image's last row ends the buffer
        seg = up(np.array([[first[b], n[b]] for b in range(3)], np.int32))
        before = staged["ragged"][5].cpu().numpy().copy()
        rc = lib.lic_rans_decode_step_ragged(*(F_._ptr(x) for x in staged["ragged"]), F_._ptr(tabs), F_._ptr(cen),
                                             F_._ptr(seg), 3, G, sum(n), M, W, F_._ptr(dst), F_._ptr(ypad["ragged"]),
                                             F_._ptr(d_ybase), F_._ptr(d_pixels), ypad["ragged"].numel(), F_._stream())
        assert rc == 0
        d_buf, d_soff, d_slen, d_esc, d_eoff, d_state = staged["single"]
        for b in range(3):
            if n[b] == 0:
                continue
            own_t = tabs[first[b] * M:(first[b] + n[b]) * M].clone()             # the same tables, 16-byte aligned
            own_c = cen[first[b] * M:(first[b] + n[b]) * M].clone()
            own_d = dst[first[b]:first[b] + n[b]].clone()
            rc = lib.lic_rans_decode_step_groups(F_._ptr(d_buf), off(d_soff, 8 * b * G), off(d_slen, 8 * b * G),
                                                 F_._ptr(d_esc), off(d_eoff, 8 * b * G), off(d_state, 4 * 67 * b * G),
                                                 F_._ptr(own_t), F_._ptr(own_c), 1, G, n[b], M, W, F_._ptr(own_d),
                                                 off(ypad["single"], 4 * y_base[b]), imgs[b]["pixels"], F_._stream())
            assert rc == 0
        torch.cuda.synchronize()
        got, want = staged["ragged"][5].cpu().numpy(), d_state.cpu().numpy()
        assert np.array_equal(got, want), f"step {t}: state blocks differ from the per-image kernel's"
        assert np.array_equal(ypad["ragged"].cpu().numpy(), ypad["single"].cpu().numpy()), f"step {t}: values differ"
        for b in range(3):
            rounds = (n[b] * M + 63) // 64
            idle = [b * G + g for g in range(G) if g >= rounds]                  # the whole image when n[b] == 0
            assert np.array_equal(got[idle], before[idle]), f"step {t}: a block that sat out was written"
            if rounds and shorten is None:
                assert not np.array_equal(got[b * G], before[b * G])                # group 0 did decode
        for b in range(3):
            sym_at[b] += n[b] * M
            row_at[b] += n[b]
    return ypad["ragged"].cpu().numpy(), y_base, staged["ragged"][5].cpu().numpy().view(np.uint32)


def _expected(imgs, M, W, y_base, size, which, idx_of=lambda im: im["idx"]):
    want = np.full(size, SENTINEL, np.float32)
    for b in which:
        im = imgs[b]
        v = (idx_of(im).astype(np.int64) + im["center"] - W).astype(np.float32).reshape(-1, M)
        for k, d in enumerate(im["dest"]):
            want[y_base[b] + d * M:y_base[b] + (d + 1) * M] = v[k]
    return want


@pytest.mark.parametrize("M,W,G", CONFIGS)
def test_ragged_steps_match_the_per_image_kernel_and_the_host_coder(env, M, W, G):
    codec = env[0]
    y, y_base, state = _run(env, M, W, G)
    imgs = _synthetic(codec, M, W, G)
    assert np.array_equal(y, _expected(imgs, M, W, y_base, y.size, range(3))), "values, or an element outside the planes"
    assert (state[:, 66] == 0).all(), state[:, 66]
    streams = [s for im in imgs for s in im["streams"]]
    escs = [e for im in imgs for e in im["escs"]]
    for i in range(3 * G):
        assert state[i, 64] == (len(streams[i]) - 256) // 2 and state[i, 65] == len(escs[i]) // 4
    assert (state[:, :64] == 1 << 16).all()
    assert sum(len(e) for e in escs) >= 4 * 4 * 3                                # the hand-placed escapes were coded


@pytest.mark.parametrize("M,W,G,blk", [(1, 24, 3, 1 * 3 + 0), (3, 2, 1, 1)])
def test_a_sub_stream_one_word_short_stops_that_image_only(env, M, W, G, blk):
    """the cursor rule refuses the last word although it is allocated memory: that block's error word is set, its
    later symbols decode as the table centre, every other image is exact"""
    codec = env[0]
    imgs = _synthetic(codec, M, W, G)
    # the input's part: the sub-stream reads its last word before its last symbols, and one of those is not the centre
    im = imgs[blk // G]
    pos, lens = codec.rans_deal(im["steps"], G)[blk % G]
    left = GR.symbols_after_the_last_word(im["streams"][blk % G], im["tabs"][pos], lens)
    assert left >= 1 and (im["idx"][pos][-left:] != W).any()
    y, y_base, state = _run(env, M, W, G, shorten=blk)                           # equal to the per-image kernel throughout
    assert state[blk, 66] != 0 and (np.delete(state[:, 66], blk) == 0).all(), state[:, 66]
    hit = blk // G
    others = [b for b in range(3) if b != hit]
    lo, hi = y_base[hit], y_base[hit] + imgs[hit]["pixels"] * M
    want = _expected(imgs, M, W, y_base, y.size, others)
    keep = np.ones(y.size, bool)
    keep[lo:hi] = False
    assert np.array_equal(y[keep], want[keep])
    full = _expected(imgs, M, W, y_base, y.size, [hit])
    centre = _expected(imgs, M, W, y_base, y.size, [hit], lambda im: np.full_like(im["idx"], W))
    assert np.array_equal(y[lo:hi] == SENTINEL, full[lo:hi] == SENTINEL)
    assert ((y[lo:hi] == full[lo:hi]) | (y[lo:hi] == centre[lo:hi])).all()
    assert (y[lo:hi] != full[lo:hi]).any()


def test_segments_and_planes_are_checked_on_the_device(env):
    """a segment that leaves the step, a plane that leaves the buffer: the image's error word, nothing written"""
    codec, _lib, F_, dev = env
    M, W, G = 1, 24, 1
    lib, imgs = _lib.load(), _synthetic(codec, M, W, G)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = [ROWS[1][b][0] for b in range(3)]
    tabs = up(np.concatenate([imgs[b]["tabs"][:n[b]] for b in range(3)]).view(np.int32))
    cen = up(np.concatenate([imgs[b]["center"][:n[b]] for b in range(3)]))
    dst = up(np.concatenate([imgs[b]["dest"][:n[b]] for b in range(3)]))
    size = sum(im["pixels"] for im in imgs)
    good_base = np.cumsum([0] + [im["pixels"] for im in imgs[:2]]).astype(np.int64)
    good_px = np.array([im["pixels"] for im in imgs], np.int64)
    good_seg = np.array([[0, n[0]], [n[0], n[1]], [n[0] + n[1], n[2]]], np.int32)
    cases = [(dict(seg=(1, [n[0], n[1] + n[2] + 1])), 1), (dict(seg=(1, [-1, 3])), 1), (dict(seg=(2, [5, -2])), 2),
             (dict(base=(0, -1)), 0), (dict(base=(2, size - 3)), 2), (dict(px=(1, -4)), 1), (dict(px=(1, 1 << 50)), 1),
             (dict(base=(1, 1 << 50)), 1)]
    for change, hit in cases:
        seg, base, px = good_seg.copy(), good_base.copy(), good_px.copy()
        for key, (b, v) in change.items():
            {"seg": seg, "base": base, "px": px}[key][b] = v
        st = [up(a) for a in _stage(_lib, imgs)]
        seed = st[5].cpu().numpy().copy()
        ypad = torch.full((size,), SENTINEL, device=dev)
        d_seg, d_base, d_px = up(seg), up(base), up(px)
        rc = lib.lic_rans_decode_step_ragged(*(F_._ptr(x) for x in st), F_._ptr(tabs), F_._ptr(cen), F_._ptr(d_seg), 3,
                                             G, sum(n), M, W, F_._ptr(dst), F_._ptr(ypad), F_._ptr(d_base),
                                             F_._ptr(d_px), size, F_._stream())
        assert rc == 0
        torch.cuda.synchronize()
        state, y = st[5].cpu().numpy().view(np.uint32), ypad.cpu().numpy()
        assert state[hit, 66] != 0 and (np.delete(state[:, 66], hit) == 0).all(), change
        lo, hi = int(good_base[hit]), int(good_base[hit] + good_px[hit])
        assert (y[lo:hi] == SENTINEL).all(), change
        for b in range(3):
            if b != hit:
                v = (imgs[b]["idx"][:n[b]].astype(np.int64) + imgs[b]["center"][:n[b]] - W).astype(np.float32)
                assert np.array_equal(y[good_base[b] + imgs[b]["dest"][:n[b]]], v), change
        if "seg" in change:
            assert np.array_equal(np.delete(state[hit], 66), np.delete(seed.view(np.uint32)[hit], 66))


def test_bad_arguments_are_refused_without_a_launch(env):
    """every other argument is step 0 of the three images, which a launch would decode: after a refusal the planes
    still hold their sentinels and the state blocks their seeds; the same arguments unchanged then do decode"""
    codec, _lib, F_, dev = env
    M, W, G = 1, 24, 1
    lib, imgs = _lib.load(), _synthetic(codec, M, W, G)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = [ROWS[1][b][0] for b in range(3)]
    st = [up(a) for a in _stage(_lib, imgs)]
    seed = st[5].cpu().numpy().copy()
    px = [im["pixels"] for im in imgs]
    size = sum(px)
    ypad = torch.full((size,), SENTINEL, device=dev)
    live = dict(zip(["streams", "stream_off", "stream_bytes", "escapes", "esc_off", "state"], st))
    live.update(tables=up(np.concatenate([imgs[b]["tabs"][:n[b]] for b in range(3)]).view(np.int32)),
                center=up(np.concatenate([imgs[b]["center"][:n[b]] for b in range(3)])),
                seg=up(np.array([[0, n[0]], [n[0], n[1]], [n[0] + n[1], n[2]]], np.int32)),
                dest=up(np.concatenate([imgs[b]["dest"][:n[b]] for b in range(3)])), ypad=ypad,
                y_base=up(np.cumsum([0] + px[:2]).astype(np.int64)), pixels=up(np.array(px, np.int64)))
    names = ["streams", "stream_off", "stream_bytes", "escapes", "esc_off", "state", "tables", "center", "seg", "nimg",
             "G", "total_rows", "M", "W", "dest", "ypad", "y_base", "pixels", "ypad_len", "stream"]
    good = {k: F_._ptr(live[k]) if k in live else None for k in names}
    good.update(nimg=3, G=G, total_rows=sum(n), M=M, W=W, ypad_len=size, stream=F_._stream())
    off = lambda k, nbytes: C.c_void_p(live[k].data_ptr() + nbytes)

    def refused(status, **bad):
        assert lib.lic_rans_decode_step_ragged(*dict(good, **bad).values()) == status, bad
        torch.cuda.synchronize()
        assert (ypad == SENTINEL).all() and np.array_equal(st[5].cpu().numpy(), seed), bad

    for name in live:
        refused(-1, **{name: None})
    for bad in (dict(nimg=0), dict(G=0), dict(G=9), dict(total_rows=0), dict(total_rows=-3), dict(M=0), dict(W=0),
                dict(ypad_len=0), dict(tables=off("tables", 4)), dict(tables=off("tables", 8)),
                dict(streams=off("streams", 2)), dict(dest=off("dest", 4)), dict(y_base=off("y_base", 4)),
                dict(pixels=off("pixels", 12)), dict(seg=off("seg", 2)), dict(center=off("center", 1)),
                dict(state=off("state", 2)), dict(ypad=off("ypad", 2))):
        refused(-1, **bad)
    for bad in (dict(W=65), dict(total_rows=1 << 31), dict(total_rows=1 << 20, M=1 << 12), dict(nimg=30000, G=3),
                dict(ypad_len=(1 << 40) + 1)):
        refused(-2, **bad)
    assert lib.lic_rans_decode_step_ragged(*good.values()) == 0                  # and the launch does leave its mark
    torch.cuda.synchronize()
    assert int((ypad != SENTINEL).sum()) == sum(n) and not np.array_equal(st[5].cpu().numpy(), seed)
