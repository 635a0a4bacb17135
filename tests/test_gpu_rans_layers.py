"""lic_rans_decode_step_layers on an MI355X: all layers of a step in one launch, bit for bit what
lic_rans_decode_step_groups gives when it is run per layer into a plane of that layer's own, and what the Python
decoder of tests/rans_groups_ref.py gives.  Streams come from that file's Python coder over synthetic tables
(`synthetic_images` is the recipe); eleven consecutive launches of n = 1 .. 11 pixels carry the state blocks."""
import numpy as np
import pytest
import torch

import rans_groups_ref as GR

pytestmark = pytest.mark.gpu

B = 2
SENTINEL = -777.0
NS = list(range(1, 12))                          # pixels per step: with M_l = 20, 12, 17, 13, 8 the steps have 8 .. 220 symbols,
PIXELS = 40                                      # 64 (8 x 8), 65 (13 x 5) and more than 64 G for G = 1, 3 among them


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    return _lib, F_, torch.device("cuda:0")


_DATA = {}


def _layer_data(M, W, escapes, seed):
    """two images of layer data: tables [B][nsym][S+1], idx [B][nsym], centres; escapes only if asked for"""
    key = (M, W, escapes, seed)
    if key not in _DATA:
        steps = [n * M for n in NS]
        tabs, idx = GR.synthetic_images(W, steps, seed)
        S = 2 * W + 1
        if escapes:
            tabs, idx = tabs[[0, 2]], idx[[0, 2]]                 # the two images with hand-placed edge symbols
            assert ((idx <= 0) | (idx >= S - 1)).any()
        else:
            tabs, idx = tabs[[0, 1]], idx[[0, 1]].clip(1, max(S - 2, 1))
        cen = np.random.RandomState(seed + 1).randint(-10, 11, size=idx.shape).astype(np.int32)
        _DATA[key] = (np.ascontiguousarray(tabs), np.ascontiguousarray(idx), cen, steps)
    return _DATA[key]


_CODED = {}


def _coded(M, W, escapes, seed, G):
    """the layer's B * G sub-streams and escape lists by the Python coder, image-major, checked by its decoder"""
    key = (M, W, escapes, seed, G)
    if key not in _CODED:
        tabs, idx, _, steps = _layer_data(M, W, escapes, seed)
        streams, escs = [], []
        for b in range(B):
            s, e = GR.encode(tabs[b], idx[b], steps, G)
            assert (GR.decode(s, e, tabs[b], steps) == idx[b]).all()
            streams += s
            escs += e
        if not escapes:
            assert all(len(e) == 0 for e in escs)
        _CODED[key] = (streams, escs)
    return _CODED[key]


def _stage(env, streams, escs, shorten=None):
    """streams and escape lists -> the six staging tensors of the decode entries (kept alive by the caller)"""
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


def _dests():
    r = np.random.RandomState(3)
    return [r.permutation(PIXELS)[:n].astype(np.int64) for n in NS]


def _run_layers(env, split, y_pix, W, G, datas, codeds, shorten=None):
    """the eleven launches of the layered entry -> (plane [B][PIXELS][y_pix], state blocks, blocks after step 0, seed)"""
    _lib, F_, dev = env
    lib = _lib.load()
    streams = [s for c in codeds for s in c[0]]                   # layer-major
    escs = [e for c in codeds for e in c[1]]
    staged, seed = _stage(env, streams, escs, shorten)
    ypad = torch.full((B, PIXELS, y_pix), SENTINEL, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = [0] * len(split)
    first = None
    for t, (n, dest) in enumerate(zip(NS, _dests())):
        table = (_lib.RansLayer * len(split))()
        keep = []
        for l, ((c0, M), (tabs, _, cen, _)) in enumerate(zip(split, datas)):
            ns = n * M
            d_t, d_c = up(tabs[:, base[l]:base[l] + ns].view(np.int32)), up(cen[:, base[l]:base[l] + ns])
            keep += [d_t, d_c]
            table[l].tables, table[l].center, table[l].c0, table[l].M = d_t.data_ptr(), d_c.data_ptr(), c0, M
            base[l] += ns
        d_dest = up(dest)
        rc = lib.lic_rans_decode_step_layers(*[F_._ptr(a) for a in staged], table, len(split), B, G, n, W,
                                             F_._ptr(d_dest), F_._ptr(ypad), PIXELS, y_pix, F_._stream())
        assert rc == 0
        torch.cuda.synchronize()
        if t == 0:
            first = staged[5].cpu().numpy().view(np.uint32).copy()
    return ypad.cpu().numpy(), staged[5].cpu().numpy().view(np.uint32), first, seed


def _run_per_layer(env, M, W, G, data, coded):
    """lic_rans_decode_step_groups on one layer alone, into a plane of M channels -> (plane, state blocks)"""
    _lib, F_, dev = env
    lib = _lib.load()
    staged, _ = _stage(env, *coded)
    ypad = torch.full((B, PIXELS, M), SENTINEL, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tabs, _, cen, _ = data
    base = 0
    for n, dest in zip(NS, _dests()):
        ns = n * M
        d_t, d_c, d_dest = up(tabs[:, base:base + ns].view(np.int32)), up(cen[:, base:base + ns]), up(dest)
        rc = lib.lic_rans_decode_step_groups(*[F_._ptr(a) for a in staged], F_._ptr(d_t), F_._ptr(d_c), B, G, n, M, W,
                                             F_._ptr(d_dest), F_._ptr(ypad), PIXELS, F_._stream())
        assert rc == 0
        torch.cuda.synchronize()
        base += ns
    return ypad.cpu().numpy(), staged[5].cpu().numpy().view(np.uint32)


def _expected_plane(split, y_pix, W, datas):
    """from the symbols the Python decoder returns: value = idx + centre - W at (dest pixel, c0 + channel)"""
    want = np.full((B, PIXELS, y_pix), SENTINEL, np.float32)
    for (c0, M), (_, idx, cen, _) in zip(split, datas):
        base = 0
        for n, dest in zip(NS, _dests()):
            v = idx[:, base:base + n * M].astype(np.int64) + cen[:, base:base + n * M] - W
            want[:, dest, c0:c0 + M] = v.astype(np.float32).reshape(B, n, M)
            base += n * M
    return want


def _case(split, W, G):
    """layer data and streams: escapes in layer 0 only"""
    datas = [_layer_data(M, W, l == 0, 40 + 7 * l) for l, (_, M) in enumerate(split)]
    codeds = [_coded(M, W, l == 0, 40 + 7 * l, G) for l, (_, M) in enumerate(split)]
    return datas, codeds


CASES = [([(0, 20), (20, 12)], 32, 24, 1), ([(0, 20), (20, 12)], 32, 24, 3), ([(0, 20), (20, 12)], 32, 24, 8),
         ([(0, 17), (17, 13)], 30, 24, 1), ([(0, 17), (17, 13)], 33, 24, 3), ([(0, 17), (17, 13)], 30, 24, 8),
         ([(0, 8), (8, 4), (12, 4)], 16, 24, 3), ([(0, 20), (20, 12)], 32, 1, 3), ([(0, 17), (17, 13)], 30, 64, 3),
         ([(5, 12)], 20, 24, 3)]                                  # one layer, c0 > 0, y_pix > M_l


@pytest.mark.parametrize("split,y_pix,W,G", CASES)
def test_layers_in_one_launch_are_the_layers_one_by_one(env, split, y_pix, W, G):
    datas, codeds = _case(split, W, G)
    got, state, first, seed = _run_layers(env, split, y_pix, W, G, datas, codeds)
    want = _expected_plane(split, y_pix, W, datas)
    assert np.array_equal(got, want), "decoded values, or elements no layer owns, differ from the Python decoder's"
    owned = np.zeros(y_pix, bool)
    for c0, M in split:
        owned[c0:c0 + M] = True
    assert (got[:, :, ~owned] == SENTINEL).all()
    streams = [s for c in codeds for s in c[0]]
    escs = [e for c in codeds for e in c[1]]
    assert (state[:, 66] == 0).all(), state[:, 66]
    for i in range(len(streams)):
        assert state[i, 64] == (len(streams[i]) - 256) // 2 and state[i, 65] == len(escs[i]) // 4, i
    assert (state[:, :64] == 1 << 16).all()
    # per layer through the one-layer entry: the same planes, the same state blocks
    for l, ((c0, M), data, coded) in enumerate(zip(split, datas, codeds)):
        plane, st = _run_per_layer(env, M, W, G, data, coded)
        assert np.array_equal(plane, got[:, :, c0:c0 + M]), f"layer {l}"
        assert np.array_equal(st, state[l * B * G:(l + 1) * B * G]), f"layer {l}: state blocks"
    # step 0 has n = 1 pixel: M_l symbols, one round, so every block of a group >= 1 sat it out, bit for bit
    sat_out = [i for i in range(len(streams)) if i % G >= 1]
    assert np.array_equal(first[sat_out], seed[sat_out])
    assert not np.array_equal(first[::G], seed[::G])


def test_a_truncated_sub_stream_of_layer_1_reports_for_itself_alone(env):
    """block (layer 1, image 0, group 1) is given one word short: the cursor rule refuses the word, that block's error
    word is set and no other; layer 0's values and state blocks are those of the intact run"""
    split, y_pix, W, G = [(0, 20), (20, 12)], 32, 24, 3
    datas, codeds = _case(split, W, G)
    blk = (1 * B + 0) * G + 1
    assert len(codeds[1][0][1]) > 256                              # the sub-stream has a word to lose
    good, good_state, _, _ = _run_layers(env, split, y_pix, W, G, datas, codeds)
    got, state, _, _ = _run_layers(env, split, y_pix, W, G, datas, codeds, shorten=blk)
    assert state[blk, 66] != 0
    assert (np.delete(state[:, 66], blk) == 0).all(), state[:, 66]
    assert np.array_equal(got[:, :, :20], good[:, :, :20])
    assert np.array_equal(state[:B * G], good_state[:B * G])
    assert np.array_equal(got[1], good[1])                          # image 1 of layer 1 is not touched by it either
    # image 0 of layer 1: right values or the table centre, and the same elements written
    cen = _expected_plane(split, y_pix, W, [datas[0], (datas[1][0], np.full_like(datas[1][1], W), datas[1][2], None)])
    assert np.array_equal(got[0] == SENTINEL, good[0] == SENTINEL)
    assert ((got[0] == good[0]) | (got[0] == cen[0])).all()
