"""lic_rans_z_pick (+ lic_rans_encode_ragged) and lic_rans_z_decode on an MI355X, through the C ABI with synthetic
tables: the encoder's bytes against the host coder's (which tests/test_rans_z_host.py holds to the restatement of the
format), the decoder's values against the symbols, both table paths against each other, and damaged input.  Every output
has canaries on both sides."""
import numpy as np
import pytest
import torch

import rans_z_cases as ZC

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
GAP = 5


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    from neural_image_compression_amd import _lib, codec
    from neural_image_compression_amd import functional as F_
    return codec, _lib, F_, torch.device("cuda:0")


_TABLES = {}


def _tables(M, S):
    if (M, S) not in _TABLES:
        _TABLES[M, S] = ZC.shared_tables(M, S, 11 * M + S)
        if S == 2:                                         # two symbols of about one bit each: a state takes 15 of them
            _TABLES[M, S] = np.array([[0, 30000 + 1000 * c, 65536] for c in range(M)], np.uint32)
    return _TABLES[M, S]


def _host_streams(codec, t, idxs, G):
    """-> ([stream], [escape list]) image-major, by the host coder"""
    M, streams, escs = len(t), [], []
    for idx in idxs:
        for pos, steps_g in codec.rans_deal([len(idx)], G):
            s, e = codec.rans_encode_shared(t, idx[pos], steps_g, (pos % M).astype(np.int32))
            streams.append(s)
            escs.append(e)
    return streams, escs


def _images(S, counts, seed):
    return [ZC.symbols(S, n, seed + 13 * i, far=n >= 8) if n else np.zeros(0, np.int32) for i, n in enumerate(counts)]


# ---- pick + encode ------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (1, 2, 8))
@pytest.mark.parametrize("M,S,pixels", [(5, 4, (1, 7, 40)), (192, 129, (1, 6))])
def test_pick_and_encode_write_the_host_bytes(env, M, S, pixels, G):
    codec, _lib, F_, dev = env
    lib, t, lo = _lib.load(), _tables(M, S), -(S // 2)
    idxs = _images(S, [P * M for P in pixels], 5)
    want_s, want_e = _host_streams(codec, t, idxs, G)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    images, blocks, step_len, rows, words_len, esc_len = codec.z_encode_plan(pixels, M, G)
    nimg, n = len(pixels), rows * M
    z = up((np.concatenate(idxs).astype(np.int64) + lo).astype(np.int32))
    canary = 0x5A5A5A5A
    sf = torch.full((n + 2,), canary, device=dev, dtype=torch.int32)
    exc = torch.full((n + 2,), canary, device=dev, dtype=torch.int32)
    words = torch.full((words_len + 8,), 0xA5, device=dev, dtype=torch.uint8)
    esc = torch.full((esc_len + 2,), canary, device=dev, dtype=torch.int32)
    state = torch.zeros((nimg * G + 2, _lib.RANS_STATE_WORDS), device=dev, dtype=torch.int32)
    state[nimg * G + 1] = canary
    d_t, d_images, d_blocks, d_steps = up(t.view(np.int32)), up(images), up(blocks), up(step_len)
    assert lib.lic_rans_z_pick(F_._ptr(d_t), M, lo, S, F_._ptr(z), n, F_._ptr(sf[1:]), F_._ptr(exc[1:]),
                               F_._ptr(state[nimg * G:]), F_._stream()) == 0
    assert lib.lic_rans_encode_ragged(F_._ptr(sf[1:]), F_._ptr(exc[1:]), F_._ptr(d_steps), nimg, F_._ptr(d_images),
                                      F_._ptr(d_blocks), nimg, G, rows, M, F_._ptr(words[4:]), words_len,
                                      F_._ptr(esc[1:]), esc_len, F_._ptr(state), F_._stream()) == 0
    torch.cuda.synchronize()
    h_state = state.cpu().numpy().view(np.uint32)
    assert (h_state[nimg * G] == 0).all() and (h_state[nimg * G + 1] == canary).all()      # pick's word, the canary row
    assert (h_state[:nimg * G, 66] == 0).all()
    for a in (sf, exc, esc):
        assert int(a[0]) == canary and int(a[-1]) == canary
    # sf / exc are lic_rans_encode_pick's words
    flat = np.concatenate(idxs).astype(np.int64)
    k = np.arange(n)
    s = flat.clip(0, S - 1)
    assert np.array_equal(sf[1:-1].cpu().numpy().view(np.uint32),
                          ((t[k % M, s] << 16) | (t[k % M, s + 1] - t[k % M, s])).astype(np.uint32))
    want_exc = np.where(flat <= 0, -flat, np.where(flat >= S - 1, flat - (S - 1), 0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(exc[1:-1].cpu().numpy().view(np.uint32), want_exc)
    h_words, h_esc = words.cpu().numpy(), esc.cpu().numpy().view(np.uint32)
    untouched = np.ones(words_len + 8, bool)
    for i in range(nimg * G):
        nw, ne = int(h_state[i, 64]), int(h_state[i, 65])
        end = int(blocks[i, 0] + blocks[i, 1]) + 4
        assert 2 * nw <= blocks[i, 1] and ne <= blocks[i, 3]
        got = h_state[i, :64].astype("<u4").tobytes() + h_words[end - 2 * nw:end].tobytes()
        assert got == want_s[i], f"block {i}: stream differs from the host coder's"
        e0 = int(blocks[i, 2]) + 1
        assert h_esc[e0:e0 + ne].astype("<u4").tobytes() == want_e[i], f"block {i}: escape list differs"
        assert (h_esc[e0 + ne:e0 + int(blocks[i, 3])] == canary).all()
        untouched[end - 2 * nw:end] = False
    assert (h_words[untouched] == 0xA5).all()
    assert sum(map(len, want_e)) > 0


def test_pick_reports_a_malformed_table_in_its_call_level_word(env):
    codec, _lib, F_, dev = env
    lib, M, S, lo = _lib.load(), 5, 4, -1
    t = _tables(M, S).copy()
    t[3, 2] = t[3, 1]                                                             # a zero frequency of table 3, symbol 1
    z = torch.full((10,), 1 + lo, device=dev, dtype=torch.int32)                  # every symbol codes idx 1
    sf, exc = torch.zeros(10, device=dev, dtype=torch.int32), torch.zeros(10, device=dev, dtype=torch.int32)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    d_t = torch.from_numpy(t.view(np.int32)).to(dev)
    assert lib.lic_rans_z_pick(F_._ptr(d_t), M, lo, S, F_._ptr(z), 10, F_._ptr(sf), F_._ptr(exc), F_._ptr(err),
                               F_._stream()) == 0
    assert int(err[0]) == 1                                                       # LIC_RANS_ERR_RANGE
    got = sf.cpu().numpy().view(np.uint32)
    assert got[3] == 1 and got[8] == 1 and (got[[0, 1, 2, 4]] != 1).all()         # (start 0, freq 1) where the table is bad


# ---- decode -------------------------------------------------------------------------------------
def _decode(env, t, lo, G, idxs, path=0, z_len_cut=0, mutate=None, planes=None):
    """stage the host coder's streams of `idxs` (one array per image; empty: nsym = 0) and decode them in one launch
    -> (flat z buffer with GAP canaries around every plane, plane starts, state blocks before, after, rc)"""
    codec, _lib, F_, dev = env
    lib, M, S = _lib.load(), len(t), t.shape[1] - 1
    streams, escs = _host_streams(codec, t, idxs, G)
    staged = codec._RansStaging(streams, escs, len(idxs), G)
    buf, s_off, s_len, e_all, e_off, state = staged.host
    # blocks that must stay bit for bit -- an image without symbols, a group without a round -- get cursors no decoder
    # would leave
    for b, idx in enumerate(idxs):
        for g in range(G):
            if g >= (len(idx) + 63) // 64:
                state[b * G + g, 64:66] = (0x1234, 0x77)
    tabs = t.view(np.int32).copy()
    if mutate:
        mutate(dict(s_len=s_len, tables=tabs.view(np.uint32), state=state))
    before = state.copy().view(np.uint32)
    base, at = [], 0
    for idx in idxs:
        base.append(at + GAP)
        at += GAP + len(idx)
    size = at + GAP
    if planes:
        base = planes(base)
    z = torch.full((size,), SENTINEL, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dev_args = [up(a) for a in (buf, s_off, s_len, e_all, e_off, state)]
    d_t, d_n, d_base = up(tabs), up(np.array([len(i) for i in idxs], np.int64)), up(np.array(base, np.int64))
    rc = lib.lic_rans_z_decode(*(F_._ptr(a) for a in dev_args), F_._ptr(d_t), M, lo, S, len(idxs), G, F_._ptr(d_n),
                               F_._ptr(d_base), F_._ptr(z), size - z_len_cut, path, F_._stream())
    torch.cuda.synchronize()
    return z.cpu().numpy(), base, before, dev_args[5].cpu().numpy().view(np.uint32), rc, (streams, escs)


def _expected(idxs, lo, base, size, skip=()):
    want = np.full(size, SENTINEL, np.float32)
    for b, idx in enumerate(idxs):
        if b not in skip:
            want[base[b]:base[b] + len(idx)] = (idx.astype(np.int64) + lo).astype(np.float32)
    return want


def _check_intact(idxs, G, before, after, streams, escs):
    for b, idx in enumerate(idxs):
        for g in range(G):
            i = b * G + g
            if g >= (len(idx) + 63) // 64:
                assert np.array_equal(after[i], before[i]), f"block {i} has no round and was written"
            else:
                assert after[i, 66] == 0 and (after[i, :64] == 1 << 16).all(), f"block {i}"
                assert after[i, 64] == (len(streams[i]) - 256) // 2 and after[i, 65] == len(escs[i]) // 4, f"block {i}"


DECODE = [(5, 4, [5, 35, 200]), (192, 129, [192, 1152, 576]),
          (1, 9, "edges"),                                                        # n around one round and around G rounds
          (5, 4, [35, 0, 200]),                                                   # an image without symbols between two
          (3, 2, [130, 3, 66]),                                                   # S = 2: every symbol escapes
          (7, 6, [64 * 7, 1, 449])]                                               # even S, a round that ends a row


@pytest.mark.parametrize("G", (1, 2, 8))
@pytest.mark.parametrize("M,S,counts", DECODE, ids=lambda v: str(v).replace(" ", ""))
def test_decode_gives_the_symbols(env, M, S, counts, G):
    if counts == "edges":
        counts = [1, 63, 64, 65, 64 * G - 1, 64 * G + 1]
    t, lo = _tables(M, S), -(S // 2)
    idxs = _images(S, counts, 40 + M)
    z, base, before, after, rc, (streams, escs) = _decode(env, t, lo, G, idxs)
    assert rc == 0
    assert np.array_equal(z, _expected(idxs, lo, base, z.size)), "values, or an element outside the planes"
    _check_intact(idxs, G, before, after, streams, escs)
    if S == 2:
        n_esc = sum(len(e) // 4 for e in escs)
        assert n_esc == sum(counts)                                               # every symbol is an edge symbol
        assert all(len(s) == 256 for s in streams)                                # and so few of them cost no word


@pytest.mark.parametrize("M,S", [(192, 129), (5, 4)])
def test_forced_paths_write_the_same_bytes(env, M, S):
    _lib = env[1]
    t, lo, G = _tables(M, S), -(S // 2), 2
    idxs = _images(S, [M * 3, M * 9, M], 9)
    assert _lib.load().lic_rans_z_decode_path(M, S) == _lib.RANS_Z_RESIDENT
    runs = [_decode(env, t, lo, G, idxs, path) for path in (_lib.RANS_Z_AUTO, _lib.RANS_Z_RESIDENT, _lib.RANS_Z_GLOBAL)]
    for z, base, before, after, rc, _ in runs:
        assert rc == 0
        assert np.array_equal(z, runs[0][0]) and np.array_equal(after, runs[0][3])
    assert np.array_equal(runs[0][0], _expected(idxs, lo, runs[0][1], runs[0][0].size))


def test_auto_takes_the_global_path_beyond_the_lds_budget(env):
    _lib = env[1]
    M, S, G = 1024, 129, 2
    t, lo = _tables(M, S), -64
    assert _lib.load().lic_rans_z_decode_path(M, S) == _lib.RANS_Z_GLOBAL
    idxs = _images(S, [M, 2 * M], 3)
    z, base, before, after, rc, (streams, escs) = _decode(env, t, lo, G, idxs, _lib.RANS_Z_AUTO)
    assert rc == 0 and np.array_equal(z, _expected(idxs, lo, base, z.size))
    _check_intact(idxs, G, before, after, streams, escs)
    assert _decode(env, t, lo, G, idxs, _lib.RANS_Z_RESIDENT)[4] == -1            # cannot be forced on chip


# ---- damage: handed damaged input; every read is bounds-checked first --------------------------------------
@pytest.mark.parametrize("path", (1, 2))
def test_a_stream_one_word_short_stops_that_block_only(env, path):
    M, S, G, blk = 5, 4, 2, 1 * 2 + 0
    t, lo = _tables(M, S), -2
    idxs = _images(S, [200, 1500, 300], 2)

    def cut(a):
        assert a["s_len"][blk] > 256
        a["s_len"][blk] -= 2
    z, base, before, after, rc, _ = _decode(env, t, lo, G, idxs, path, mutate=cut)
    assert rc == 0
    assert after[blk, 66] == 1 and (np.delete(after[:, 66], blk) == 0).all(), after[:, 66]
    want = _expected(idxs, lo, base, z.size)
    plane = slice(base[1], base[1] + len(idxs[1]))
    keep = np.ones(z.size, bool)
    keep[plane] = False
    assert np.array_equal(z[keep], want[keep])                                    # other images, and every canary
    # inside the image: the other group's rounds are exact; the cut block's symbols are exact or lo + S / 2
    k = np.arange(len(idxs[1]))
    mine = (k // 64) % G == blk % G
    assert np.array_equal(z[plane][~mine], want[plane][~mine])
    ok = (z[plane][mine] == want[plane][mine]) | (z[plane][mine] == lo + S // 2)
    assert ok.all()


def test_a_stream_shorter_than_its_states_is_refused(env):
    M, S, G = 5, 4, 1
    t, lo = _tables(M, S), -2
    idxs = _images(S, [200, 100], 2)

    def cut(a):
        a["s_len"][1] = 252
    z, base, before, after, rc, _ = _decode(env, t, lo, G, idxs, mutate=cut)
    assert rc == 0 and after[1, 66] & 2 and after[0, 66] == 0                     # LIC_RANS_ERR_STREAM, that block only
    want = _expected(idxs, lo, base, z.size)
    assert np.array_equal(z[:base[1]], want[:base[1]])
    assert (z[base[1]:base[1] + 100] == lo + S // 2).all() and (z[base[1] + 100:] == SENTINEL).all()


@pytest.mark.parametrize("path", (1, 2))
@pytest.mark.parametrize("what", ("last", "zero_freq", "first"))
def test_a_malformed_table_decodes_nothing(env, what, path):
    M, S, G = 5, 4, 2
    t, lo = _tables(M, S), -2
    idxs = _images(S, [200, 70], 2)

    def spoil(a):
        if what == "last":
            a["tables"][4, S] = 65535
        elif what == "first":
            a["tables"][0, 0] = 1
        else:
            a["tables"][2, 3] = a["tables"][2, 2]
    z, base, before, after, rc, _ = _decode(env, t, lo, G, idxs, path, mutate=spoil)
    assert rc == 0
    assert (after[:, 66] == 1).all()                                              # every block says so
    assert np.array_equal(after[:, :66], before[:, :66])                          # and has not moved
    assert (z == SENTINEL).all()                                                  # no z element was written


def test_a_plane_beyond_z_len_writes_nothing(env):
    M, S, G = 5, 4, 2
    t, lo = _tables(M, S), -2
    idxs = _images(S, [200, 70], 2)
    # the buffer is said to end inside the second image's plane; then a negative and a far base
    for kw in (dict(z_len_cut=GAP + 1), dict(planes=lambda b: [b[0], -1]), dict(planes=lambda b: [b[0], 1 << 41])):
        z, base, before, after, rc, _ = _decode(env, t, lo, G, idxs, **kw)
        assert rc == 0
        assert (after[:G, 66] == 0).all() and (after[G:, 66] == 1).all(), after[:, 66]
        want = _expected(idxs, lo, [base[0], 0], z.size, skip=(1,))
        assert np.array_equal(z, want)
