"""The "rANS-64 x G" y streams on an MI355X: lic_rans_decode_step_groups against the host decoder over five
consecutive launches, the cursor rule on one shortened sub-stream, lic_rans_encode_groups against
codec.rans_encode_grouped byte for byte, ContextCodec(coder="rans", groups=G) with both encoders, and the LICBITS3
container at a size that is no multiple of 64."""
import numpy as np
import pytest
import torch

import golden_recipe as R
import rans_groups_ref as GR
import test_rans_encode_host as EH

pytestmark = pytest.mark.gpu

W_, S_ = 24, 49
SENTINEL = -777.0
LAUNCHES = GR.LAUNCHES                         # 32, 96, 327, 1 and 576 symbols per image: 1, 2, 6, 1 and 9 rounds
PIXELS = {32: 8, 1: 400, 192: 5}               # pixels per image of the latent buffer each M writes into
CANARY = 0xA5
PAD = 256                                      # canary bytes in front of and behind every output buffer


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib, codec
    return nic, codec, _lib, torch.device("cuda:0")


def _model(nic, kind, M, K, seed, dev):
    model = (nic.JointAutoregressiveHierarchical if kind == "jah" else nic.HierarchicalMixtureResidual)(M, K)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.to(dev).eval()


# ---- the decode kernel ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(env):
    """three images, their sub-streams for every G by the host encoder, decoded back by the host decoder"""
    codec = env[1]
    tabs, idx = GR.synthetic_images(W_)
    r = np.random.RandomState(22)
    nsym = sum(GR.STEPS)
    syn = {"B": 3, "W": W_, "tabs": tabs, "idx": idx, "center": r.randint(-10, 11, size=(3, nsym)).astype(np.int32),
           "dest": {0: np.array([5]), 1: np.array([0, 7, 2]), 2: r.permutation(399)[:327], 3: np.array([399]),
                    4: np.array([4, 0, 2])}}
    for G in (1, 2, 3, 4, 8):
        pairs = [codec.rans_encode_grouped(tabs[b], idx[b], GR.STEPS, G) for b in range(3)]
        for b in range(3):
            assert (codec.rans_decode_grouped(*pairs[b], tabs[b], GR.STEPS) == idx[b]).all()
        syn[G] = ([s for p in pairs for s in p[0]], [e for p in pairs for e in p[1]])      # image-major
    return syn


def _seed(_lib, streams):
    state = np.zeros((len(streams), _lib.RANS_STATE_WORDS), np.uint32)
    for i, s in enumerate(streams):
        state[i, :64] = np.frombuffer(s[:256], "<u4")
    return state


def _run_launches(env, syn, G, shorten=None, entry="groups"):
    """the five launches on one stream, the state blocks carried between them.  `shorten`: block whose stream length
    is given as one word less.  -> ({M: latent buffer}, state blocks [B*G][67], the blocks after the first launch)"""
    _, codec, _lib, dev = env
    from neural_image_compression_amd import functional as F_
    lib, B = _lib.load(), syn["B"]
    streams, escs = syn[G]
    nb = B * G
    assert len(streams) == nb
    s_off = np.zeros(nb + 1, np.int64)
    for i in range(nb):
        s_off[i + 1] = s_off[i] + (len(streams[i]) + 3) // 4 * 4
    s_len = np.array([len(s) for s in streams], np.int64)
    if shorten is not None:
        s_len[shorten] -= 2
    buf = np.zeros(int(s_off[nb]) + 64, np.uint8)                  # slack behind the last stream as well
    for i in range(nb):
        buf[s_off[i]:s_off[i] + len(streams[i])] = np.frombuffer(streams[i], np.uint8)
    state = _seed(_lib, streams)
    e_off = np.concatenate([[0], np.cumsum([len(e) // 4 for e in escs])]).astype(np.int64)
    e_all = np.frombuffer(b"".join(escs) + bytes(4), "<u4").astype(np.uint32)
    up = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_soff, d_slen, d_eoff = up(buf), up(s_off), up(s_len), up(e_off)
    d_esc, d_state = up(e_all.view(np.int32)), up(state.view(np.int32))
    ybuf = {M: torch.full((B, P, M), SENTINEL, device=dev) for M, P in PIXELS.items()}
    base, first = 0, None
    for li, (M, n) in enumerate(LAUNCHES):
        ns = M * n
        tabs = up(np.ascontiguousarray(syn["tabs"][:, base:base + ns]).view(np.int32))
        cen = up(np.ascontiguousarray(syn["center"][:, base:base + ns]))
        dst = up(syn["dest"][li].astype(np.int64))
        args = (F_._ptr(d_buf), F_._ptr(d_soff), F_._ptr(d_slen), F_._ptr(d_esc), F_._ptr(d_eoff), F_._ptr(d_state),
                F_._ptr(tabs), F_._ptr(cen), B)
        tail = (n, M, syn["W"], F_._ptr(dst), F_._ptr(ybuf[M]), PIXELS[M], F_._stream())
        if entry == "groups":
            rc = lib.lic_rans_decode_step_groups(*args, G, *tail)
        else:
            assert G == 1
            rc = lib.lic_rans_decode_step(*args, *tail)
        assert rc == 0
        if li == 0:
            first = d_state.cpu().numpy().view(np.uint32).copy()
        base += ns
    torch.cuda.synchronize()
    return {M: y.cpu().numpy() for M, y in ybuf.items()}, d_state.cpu().numpy().view(np.uint32), first


def _expected(syn, images, idx=None):
    idx = syn["idx"] if idx is None else idx
    want = {M: np.full((syn["B"], P, M), SENTINEL, np.float32) for M, P in PIXELS.items()}
    base = 0
    for li, (M, n) in enumerate(LAUNCHES):
        ns = M * n
        for b in images:
            v = idx[b, base:base + ns].astype(np.int64) + syn["center"][b, base:base + ns] - syn["W"]
            want[M][b, syn["dest"][li]] = v.astype(np.float32).reshape(n, M)
        base += ns
    return want


@pytest.mark.parametrize("G", [2, 3, 4, 8])
def test_kernel_matches_host_decoder_over_consecutive_launches(env, synthetic, G):
    """values, untouched elements, error words, both cursors and the final states of every block against the host
    decoder's; the first launch has one round, so every block of a group >= 1 sits it out and must not change"""
    _, _, _lib, _ = env
    got, state, first = _run_launches(env, synthetic, G)
    want = _expected(synthetic, range(3))
    for M in PIXELS:
        assert np.array_equal(got[M], want[M]), f"M = {M}: destinations or untouched elements differ"
    streams, escs = synthetic[G]
    assert (state[:, 66] == 0).all(), state[:, 66]
    for i in range(3 * G):
        assert state[i, 64] == (len(streams[i]) - 256) // 2, f"block {i}: words left over or used twice"
        assert state[i, 65] == len(escs[i]) // 4
    assert (state[:, :64] == 1 << 16).all()                                   # the encoder's initial states
    seed = _seed(_lib, streams)
    sat_out = [i for i in range(3 * G) if i % G >= 1]
    assert np.array_equal(first[sat_out], seed[sat_out]), "a block without a round in the launch was written"
    assert not np.array_equal(first[::G], seed[::G])                          # group 0 did decode


def test_one_group_through_the_new_entry_is_the_old_entry(env, synthetic):
    new = _run_launches(env, synthetic, 1, entry="groups")
    old = _run_launches(env, synthetic, 1, entry="step")
    for M in PIXELS:
        assert np.array_equal(new[0][M], old[0][M])
    assert np.array_equal(new[1], old[1]) and np.array_equal(new[2], old[2])
    want = _expected(synthetic, range(3))
    for M in PIXELS:
        assert np.array_equal(new[0][M], want[M])
    assert (new[1][:, 66] == 0).all() and (new[1][:, :64] == 1 << 16).all()


@pytest.mark.parametrize("G", [2, 4])
def test_kernel_stops_at_the_given_sub_stream_length(env, synthetic, G):
    """block (1, 1)'s length is given as one word less: the cursor rule refuses that word although it is allocated
    memory (the next block's stream follows it), sets that block's error word and no other; the other images are
    exact, and image 1 holds right values (its other groups, and group 1 before the missing word was needed) or the
    table centre"""
    _, codec, _, _ = env
    blk = 1 * G + 1
    # the input's part: the sub-stream reads its last word at least a round before its end, and some symbol after
    # that is not the table centre (the format's restatement says so, not the kernel)
    pos, lens = codec.rans_deal(GR.STEPS, G)[1]
    left = GR.symbols_after_the_last_word(synthetic[G][0][blk], synthetic["tabs"][1][pos], lens)
    assert left >= 64 and (synthetic["idx"][1][pos][-left:] != W_).any()
    got, state, _ = _run_launches(env, synthetic, G, shorten=blk)
    want = _expected(synthetic, (0, 2))
    assert state[blk, 66] != 0
    assert (np.delete(state[:, 66], blk) == 0).all(), state[:, 66]
    for M in PIXELS:
        assert np.array_equal(got[M][[0, 2]], want[M][[0, 2]])
    full = _expected(synthetic, (1,))
    cen = _expected(synthetic, (1,), idx=np.full_like(synthetic["idx"], synthetic["W"]))
    wrong = 0
    for M in PIXELS:
        assert np.array_equal(got[M][1] == SENTINEL, full[M][1] == SENTINEL)
        assert ((got[M][1] == full[M][1]) | (got[M][1] == cen[M][1])).all()
        wrong += int((got[M][1] != full[M][1]).sum())
    assert wrong > 0


# ---- the encode kernel ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_synthetic(env):
    """the five images of tests/test_gpu_rans_encode.py in coding order (gamma tables, frequency 1 everywhere,
    frequency 65536 - 48 everywhere; empty, one-symbol, partial and long steps; escapes up to 2^31), M = 1"""
    tabs, idx = EH.make_images(W=W_)
    n = sum(EH.STEPS)
    r = np.random.RandomState(33)
    syn = {"M": 1, "P": n, "W": W_, "steps": EH.STEPS, "tabs": tabs, "idx": idx,
           "order": r.permutation(n).astype(np.int64), "center": r.randint(-10, 11, size=(5, n)).astype(np.int64)}
    syn["center"][idx == -2 ** 31] = W_                    # y = idx + center - W must be an int32
    return syn


def _raster(syn):
    """coding order -> what lic_gmm_cdf_tables would have left, in RASTER pixel order (M = 1)"""
    P, order, tabs = syn["P"], syn["order"], syn["tabs"]
    B, S1 = tabs.shape[0], tabs.shape[-1]
    t_r, c_r, y_r = np.zeros((B, P, S1), np.uint32), np.zeros((B, P), np.int32), np.zeros((B, P), np.int32)
    for b in range(B):
        y = syn["idx"][b] + syn["center"][b] - syn["W"]
        assert (y >= -2 ** 31).all() and (y < 2 ** 31).all()
        t_r[b, order], c_r[b, order], y_r[b, order] = tabs[b], syn["center"][b], y
    return t_r, c_r.reshape(B * P, 1), y_r.reshape(B, P, 1)


def _encode(env, syn, G, slot, cap, steps=None, entry="groups"):
    """pick + encode on buffers framed by canaries -> (state [B*G][67] uint32, words, escape and state buffers with
    their frames, as bytes)"""
    _, _, _lib, dev = env
    from neural_image_compression_amd import functional as F_
    lib, B, nsym = _lib.load(), 5, syn["P"]
    steps = syn["steps"] if steps is None else steps
    t_r, c_r, y_r = _raster(syn)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_t, d_c, d_y = up(t_r.view(np.int32)), up(c_r), up(y_r)
    d_order, d_steps = up(syn["order"]), up(np.array(steps, np.int64))
    sf = torch.empty((B, nsym), device=dev, dtype=torch.int32)
    exc = torch.empty_like(sf)
    nb = B * G
    words = torch.full((PAD + nb * slot + PAD,), CANARY, device=dev, dtype=torch.uint8)
    esc = torch.full((PAD + 4 * nb * cap + PAD,), CANARY, device=dev, dtype=torch.uint8)
    state = torch.full((PAD + 4 * nb * 67 + PAD,), CANARY, device=dev, dtype=torch.uint8)
    state[PAD:PAD + 4 * nb * 67].view(torch.int32).view(nb, 67)[:, 66] = 0      # the caller zeroes the error words
    picked = torch.zeros((B, 67), device=dev, dtype=torch.int32)
    off = lambda t: t.data_ptr() + PAD
    rc = lib.lic_rans_encode_pick(F_._ptr(d_t), F_._ptr(d_c), F_._ptr(d_y), F_._ptr(d_order), B, nsym, 1, syn["W"],
                                  F_._ptr(sf), F_._ptr(exc), F_._ptr(picked), F_._stream())
    assert rc == 0
    if entry == "groups":
        rc = lib.lic_rans_encode_groups(F_._ptr(sf), F_._ptr(exc), F_._ptr(d_steps), len(steps), B, G, nsym, off(words),
                                        slot, off(esc), cap, off(state), F_._stream())
    else:
        assert G == 1 and cap == nsym
        rc = lib.lic_rans_encode(F_._ptr(sf), F_._ptr(exc), F_._ptr(d_steps), len(steps), B, nsym, off(words), slot,
                                 off(esc), off(state), F_._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (picked.cpu().numpy()[:, 66] == 0).all()
    st = state.cpu().numpy()
    return st[PAD:PAD + 4 * nb * 67].view(np.uint32).reshape(nb, 67), words.cpu().numpy(), esc.cpu().numpy(), st


def _stream_of(st, slot, cap, words, esc, i):
    """block i's stream and escape list, assembled as the host does"""
    nw, ne = int(st[i, 64]), int(st[i, 65])
    assert 2 * nw <= slot and ne <= cap
    end = PAD + (i + 1) * slot
    e0 = PAD + 4 * i * cap
    return st[i, :64].astype("<u4").tobytes() + words[end - 2 * nw:end].tobytes(), esc[e0:e0 + 4 * ne].tobytes()


def _host(codec, syn, G):
    pairs = [codec.rans_encode_grouped(syn["tabs"][b], syn["idx"][b].astype(np.int32), syn["steps"], G) for b in range(5)]
    return [s for p in pairs for s in p[0]], [e for p in pairs for e in p[1]]


@pytest.mark.parametrize("sizes", ["smallest", "roomy"])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_encode_kernel_matches_the_grouped_host_encoder(env, enc_synthetic, G, sizes):
    """five images in one launch, byte for byte, with the smallest slot and escape list lic.h allows (the fullest
    sub-stream's symbol count: image 3 codes one word per symbol and fills it) and with 2 * nsym / nsym; nothing
    but [slot end - 2 * count, slot end) and the first `count` escape entries of any block is written"""
    _, codec, _, _ = env
    syn, nsym = enc_synthetic, enc_synthetic["P"]
    fullest = max(len(pos) for pos, _ in codec.rans_deal(syn["steps"], G))
    slot, cap = ((2 * fullest + 3) // 4 * 4, fullest) if sizes == "smallest" else ((2 * nsym + 3) // 4 * 4, nsym)
    st, words, esc, state = _encode(env, syn, G, slot, cap)
    streams, escs = _host(codec, syn, G)
    assert (st[:, 66] == 0).all(), st[:, 66]
    keep_w, keep_e = np.ones(words.size, bool), np.ones(esc.size, bool)
    for i in range(5 * G):
        stream, elist = _stream_of(st, slot, cap, words, esc, i)
        assert stream == streams[i], f"image {i // G} ({EH.KINDS[i // G]}) group {i % G}: stream differs"
        assert elist == escs[i], f"image {i // G} group {i % G}: escape list differs"
        end = PAD + (i + 1) * slot
        keep_w[end - 2 * int(st[i, 64]):end] = False
        keep_e[PAD + 4 * i * cap:PAD + 4 * (i * cap + int(st[i, 65]))] = False
    # both ends of the word cursor: image 3 one word per symbol, image 4 none
    counts = [len(pos) for pos, _ in codec.rans_deal(syn["steps"], G)]
    assert [int(v) for v in st[3 * G:4 * G, 64]] == counts and (st[4 * G:, 64] == 0).all()
    assert sum(int(v) for v in st[:G, 65]) == 7                              # image 0's hand-placed escapes
    assert keep_w.sum() >= 2 * PAD and keep_e.sum() > 2 * PAD
    assert (words[keep_w] == CANARY).all(), "bytes outside [slot end - 2 * count, slot end) were written"
    assert (esc[keep_e] == CANARY).all(), "escape entries beyond the count were written"
    assert (state[:PAD] == CANARY).all() and (state[PAD + 4 * 5 * G * 67:] == CANARY).all()


def test_one_group_through_the_new_encode_entry_is_the_old_entry(env, enc_synthetic):
    syn, nsym = enc_synthetic, enc_synthetic["P"]
    slot = (256 + 2 * nsym + 3) // 4 * 4
    new = _encode(env, syn, 1, slot, nsym, entry="groups")
    old = _encode(env, syn, 1, slot, nsym, entry="image")
    for a, b in zip(new, old):
        assert np.array_equal(a, b)
    streams, escs = _host(env[1], syn, 1)
    for b in range(5):
        assert _stream_of(new[0], slot, nsym, new[1], new[2], b) == (streams[b], escs[b])


@pytest.mark.parametrize("G", [2, 8])
def test_bad_step_lengths_mark_every_block(env, enc_synthetic, G):
    syn, nsym = enc_synthetic, enc_synthetic["P"]
    for steps in (syn["steps"][:-1] + [syn["steps"][-1] - 1], [nsym + 64, -64]):
        st, words, esc, _ = _encode(env, syn, G, (2 * nsym + 3) // 4 * 4, nsym, steps=steps)
        assert (st[:, 66] != 0).all(), st[:, 66]
        assert (st[:, :64] == 1 << 16).all() and (st[:, 64] == 0).all() and (st[:, 65] == 0).all()
        assert (words == CANARY).all() and (esc == CANARY).all()


def test_a_slot_that_is_too_small_is_reported_not_overrun(env, enc_synthetic):
    """half the words and escapes the fullest sub-stream needs: the blocks that run out say so and write nothing
    outside their slot or list"""
    _, codec, _, _ = env
    syn, G = enc_synthetic, 2
    fullest = max(len(pos) for pos, _ in codec.rans_deal(syn["steps"], G))
    slot, cap = fullest // 4 * 4, 2
    st, words, esc, state = _encode(env, syn, G, slot, cap)
    assert st[3 * G, 66] != 0 and st[0, 66] != 0                             # one word per symbol; 7 escapes in 2 lists
    assert (st[4 * G:, 66] == 0).all()                                       # no word, no escape
    assert (st[:, 64] * 2 <= slot).all() and (st[:, 65] <= cap).all()
    for buf in (words, esc, state):
        assert (buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all()
    streams, escs = _host(codec, syn, G)
    for i in range(4 * G, 5 * G):
        assert _stream_of(st, slot, cap, words, esc, i) == (streams[i], escs[i])


# ---- the codec ------------------------------------------------------------------------------------
CASES = [(1, 1, 64, 128, "jah", 192), (3, 3, 128, 64, "hmr", 64), (3, 2, 64, 128, "jah", 32)]
_KW = dict(z_lo=-32, z_S=65, y_W=24)


@pytest.fixture(scope="module")
def one_group(env):
    """the groups = 1 decode of every case, computed once"""
    nic, codec, _, dev = env
    out = {}
    for K, B, H, W, kind, M in CASES:
        model = _model(nic, kind, M, K, 51, dev)
        x = torch.from_numpy(R.make_image(B, H, W, 52)).to(dev).contiguous(memory_format=torch.channels_last)
        cc = codec.ContextCodec(model, coder="rans", **_KW)
        enc = cc.compress(x)
        assert "groups" not in enc["strings"]
        dec = cc.decompress(enc["strings"], enc["shape"], enc["z_shape"])
        with torch.no_grad():
            ref = model(x, training=False)["x_hat"]
        out[(K, B, H, W, kind, M)] = (model, x, enc, dec, ref)
    return out


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("K,B,H,W,kind,M", CASES)
def test_context_codec_with_groups(env, one_group, K, B, H, W, kind, M, G):
    nic, codec, _, dev = env
    model, x, enc1, dec1, ref = one_group[(K, B, H, W, kind, M)]
    host = codec.ContextCodec(model, coder="rans", encoder="host", groups=G, **_KW).compress(x)
    cc = codec.ContextCodec(model, coder="rans", encoder="device", groups=G, **_KW)
    enc = cc.compress(x)
    s, hs = enc["strings"], host["strings"]
    assert set(s) == set(hs) == {"y", "y_esc", "y_crc32", "z", "coder", "groups"}
    for key in ("y", "y_esc", "y_crc32", "z", "coder", "groups"):
        assert s[key] == hs[key], key
    assert s["groups"] == G and len(s["y"]) == B * G and len(s["y_esc"]) == B * G and len(s["y_crc32"]) == B
    assert s["y_crc32"] == enc1["strings"]["y_crc32"] and s["z"] == enc1["strings"]["z"]
    assert all(isinstance(v, bytes) for v in s["y"] + s["y_esc"])
    assert enc["bpp_coded"] == 8.0 * (len(s["z"]) + sum(map(len, s["y"])) + sum(map(len, s["y_esc"]))) / (B * H * W)
    assert enc["bpp_coded"] == host["bpp_coded"] and enc["shape"] == host["shape"] == enc1["shape"]
    # any codec decodes them: the strings say how they are grouped
    dec = codec.ContextCodec(model, coder="rans", **_KW).decompress(s, enc["shape"], enc["z_shape"])
    assert torch.equal(dec["z_hat"], enc["z_in"])
    assert torch.equal(dec["y_hat"], enc["y_in"]), "decoder tables diverged from the encoder's"
    assert torch.equal(dec["x_hat"], ref)
    assert torch.equal(dec["y_hat"], dec1["y_hat"]) and torch.equal(dec["x_hat"], dec1["x_hat"])
    with pytest.raises(codec.CodecError):
        cc.decompress(dict(s, y_crc32=[c ^ 1 for c in s["y_crc32"]]), enc["shape"], enc["z_shape"])
    with pytest.raises(codec.CodecError):
        cc.decompress(dict(s, groups=1), enc["shape"], enc["z_shape"])       # the list lengths no longer fit
    if B > 1:
        # image 1's last sub-stream that has words (with M = 64 a step has three rounds at the most: at G = 4 the
        # last sub-stream of every image is its 256 bytes of states)
        i = max(j for j in range(G, 2 * G) if len(s["y"][j]) > 256)
        assert i > G
        cut = dict(s, y=s["y"][:i] + [s["y"][i][:-2]] + s["y"][i + 1:])
        with pytest.raises(codec.CodecError, match="image 1"):
            cc.decompress(cut, enc["shape"], enc["z_shape"])


def test_any_size_container_with_groups(env):
    nic, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    model = _model(nic, "jah", 32, 3, 51, dev)
    B, H, W, G = 1, 70, 100, 4
    x = torch.from_numpy(R.make_image(B, H, W, 54)).to(dev)
    g4 = codec.ContextCodec(model, coder="rans", groups=G, **_KW)
    blob = g4.compress_image(x)
    assert blob[:8] == b"LICBITS3"
    assert blob == codec.ContextCodec(model, coder="rans", encoder="device", groups=G, **_KW).compress_image(x)
    want = nic.padded_forward(model, x)["x_hat"]
    x_hat = g4.decompress_image(blob)
    assert x_hat.shape == x.shape and torch.equal(x_hat, want)
    # the magic and the header say how to decode, whatever the codec was constructed with
    plain = codec.ContextCodec(model, coder="rans", **_KW)
    for other in (plain, codec.ContextCodec(model, coder="rans", groups=1, **_KW),
                  codec.ContextCodec(model, coder="rans", groups=2, **_KW), codec.ContextCodec(model, **_KW),
                  codec.ContextCodec(model, z_lo=-64, z_S=129, y_W=32, coder="range")):
        assert torch.equal(other.decompress_image(blob), want)
    # size: the padded run's streams and escape lists plus the container's overhead, nothing else
    enc = g4.compress(F_.pad_to_multiple(x))
    head, z, ys, es, crcs, groups = codec.unpack_bitstream_grouped(blob)
    assert groups == G and head["y_W"] == 24 and (head["H"], head["W"]) == (H, W)
    assert (z, ys, es, crcs) == (enc["strings"]["z"], enc["strings"]["y"], enc["strings"]["y_esc"],
                                 enc["strings"]["y_crc32"])
    overhead = 8 + 13 * 4 + 4 * B + 8 * B * G + 4      # magic, 11 fields + z length + lanes, CRCs, rows, trailing CRC
    assert len(blob) == overhead + len(z) + sum(map(len, ys)) + sum(map(len, es))
    assert 8.0 * (len(blob) - overhead) / (B * 128 * 128) == enc["bpp_coded"]
    # groups = 1 is the container and the bytes of a codec that was never told about groups
    blob1 = codec.ContextCodec(model, coder="rans", groups=1, **_KW).compress_image(x)
    assert blob1[:8] == b"LICBITS2" and blob1 == plain.compress_image(x)
    assert codec.ContextCodec(model, **_KW).compress_image(x, coder="rans") == blob1
    assert g4.compress_image(x, coder="range") == codec.ContextCodec(model, **_KW).compress_image(x)
    assert torch.equal(g4.decompress_image(blob1), want)
    with pytest.raises(codec.CodecError):
        g4.decompress_image(blob[:-1])
