"""The device decoder of the "rANS-64" y streams (lic_rans_decode_step) and ContextCodec(coder="rans") on an MI355X:
the kernel against the host decoder on synthetic tables over consecutive launches, the cursor rule on a shortened
stream, full round trips at the shapes of test_codec.py's range-coder round trip, the two coders against each other,
and the LICBITS2 container at a size that is no multiple of 64."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_recipe as R
from oracle import codec_ref as CR

pytestmark = pytest.mark.gpu

W_, S_ = 24, 49
SENTINEL = -777.0
# (M, pixels of the step): 32, 96, 327 and 1 symbols per image; every step ends in a partial round
LAUNCHES = [(32, 1), (32, 3), (1, 327), (1, 1)]
PIXELS = {32: 8, 1: 400}                      # pixels per image of the latent buffer each M writes into


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


def make_synthetic(codec, W=W_):
    """B = 3 images of different entropy (so different stream lengths), escapes in images 0 and 2, coded by the host
    encoder and decoded back by the host decoder, for the window half-width W: the reference of the kernel tests"""
    S = 2 * W + 1
    r = np.random.RandomState(21)
    B, steps = 3, [M * n for M, n in LAUNCHES]
    nsym = sum(steps)
    tabs, idx = [], []
    for b, shape in enumerate((0.3, 0.02, 2.0)):
        f = r.gamma(shape, 1.0, size=(nsym, S)) + 1e-9
        F = np.concatenate([np.zeros((nsym, 1)), np.cumsum(f / f.sum(1, keepdims=True), 1)], 1)
        F[:, -1] = 1.0
        t = CR.quantize_cdf(F)
        u = r.randint(0, 65536, size=nsym)
        # interior symbols drawn from the tables; the edge symbols are placed by hand below
        i = np.array([np.searchsorted(t[k], u[k], side="right") - 1 for k in range(nsym)], np.int32).clip(1, S - 2)
        tabs.append(t)
        idx.append(i)
    idx[0][[3, 40, 130, 131, 454, 455]] = [0, -1, S - 1, S + 100000, -100000, S]
    idx[2][[31, 127, 128 + 64 * 5 + 6]] = [-7, S - 1, 0]              # last lanes of partial rounds
    streams, escs = zip(*[codec.rans_encode(tabs[b], idx[b], steps) for b in range(B)])
    # the escape lists by the format's rule (idx <= 0 or idx >= S - 1): 6, 0 and 3 entries
    n_esc = [int(((idx[b] <= 0) | (idx[b] >= S - 1)).sum()) for b in range(B)]
    assert n_esc == [6, 0, 3] and [len(e) for e in escs] == [4 * c for c in n_esc]
    assert len({len(s) for s in streams}) == 3
    host = [codec.rans_decode(streams[b], escs[b], tabs[b], steps) for b in range(B)]
    assert all((host[b] == idx[b]).all() for b in range(B))
    center = r.randint(-10, 11, size=(B, nsym)).astype(np.int32)
    dest = {0: np.array([5]), 1: np.array([0, 7, 2]), 2: r.permutation(399)[:327], 3: np.array([399])}
    return {"B": B, "W": W, "steps": steps, "tabs": np.stack(tabs), "idx": np.stack(host), "streams": streams,
            "escs": escs, "center": center, "dest": dest}


@pytest.fixture(scope="module")
def synthetic(env):
    """the W = 24 reference of both kernel tests, computed once"""
    return make_synthetic(env[1])


def _run_launches(env, syn, shorten=None):
    """the four launches on one stream, the state block carried between them.  `shorten`: image whose stream length
    is given as one word less.  -> ({M: latent buffer}, state blocks [B][67])"""
    _, codec, _lib, dev = env
    from neural_image_compression_amd import functional as F_
    lib, B = _lib.load(), syn["B"]
    streams, escs = syn["streams"], syn["escs"]
    s_off = np.zeros(B + 1, np.int64)
    for b in range(B):
        s_off[b + 1] = s_off[b] + (len(streams[b]) + 3) // 4 * 4
    s_len = np.array([len(s) for s in streams], np.int64)
    if shorten is not None:
        s_len[shorten] -= 2
    buf = np.zeros(int(s_off[B]) + 64, np.uint8)                   # slack behind the last stream as well
    state = np.zeros((B, _lib.RANS_STATE_WORDS), np.uint32)
    for b in range(B):
        buf[s_off[b]:s_off[b] + len(streams[b])] = np.frombuffer(streams[b], np.uint8)
        state[b, :64] = np.frombuffer(streams[b][:256], "<u4")
    e_off = np.concatenate([[0], np.cumsum([len(e) // 4 for e in escs])]).astype(np.int64)
    e_all = np.frombuffer(b"".join(escs) + bytes(4), "<u4").astype(np.uint32)
    up = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_soff, d_slen, d_eoff = up(buf), up(s_off), up(s_len), up(e_off)
    d_esc, d_state = up(e_all.view(np.int32)), up(state.view(np.int32))
    ybuf = {M: torch.full((B, P, M), SENTINEL, device=dev) for M, P in PIXELS.items()}
    base = 0
    for li, (M, n) in enumerate(LAUNCHES):
        ns = M * n
        tabs = up(np.ascontiguousarray(syn["tabs"][:, base:base + ns]).view(np.int32))
        cen = up(np.ascontiguousarray(syn["center"][:, base:base + ns]))
        dst = up(syn["dest"][li].astype(np.int64))
        rc = lib.lic_rans_decode_step(F_._ptr(d_buf), F_._ptr(d_soff), F_._ptr(d_slen), F_._ptr(d_esc), F_._ptr(d_eoff),
                                      F_._ptr(d_state), F_._ptr(tabs), F_._ptr(cen), B, n, M, syn["W"], F_._ptr(dst),
                                      F_._ptr(ybuf[M]), PIXELS[M], F_._stream())
        assert rc == 0
        base += ns
    torch.cuda.synchronize()
    return {M: y.cpu().numpy() for M, y in ybuf.items()}, d_state.cpu().numpy().view(np.uint32)


def _expected(syn, images):
    want = {M: np.full((syn["B"], P, M), SENTINEL, np.float32) for M, P in PIXELS.items()}
    base = 0
    for li, (M, n) in enumerate(LAUNCHES):
        ns = M * n
        for b in images:
            v = (syn["idx"][b, base:base + ns].astype(np.int64) + syn["center"][b, base:base + ns] - syn["W"])
            want[M][b, syn["dest"][li]] = v.astype(np.float32).reshape(n, M)
        base += ns
    return want


def check_consecutive_launches(env, synthetic):
    """values, untouched elements, error words, both cursors and the final states against the host decoder's"""
    got, state = _run_launches(env, synthetic)
    want = _expected(synthetic, range(3))
    for M in PIXELS:
        assert np.array_equal(got[M], want[M]), f"M = {M}: destinations or untouched elements differ"
    assert (state[:, 66] == 0).all(), state[:, 66]
    for b in range(3):
        assert state[b, 64] == (len(synthetic["streams"][b]) - 256) // 2      # every word used, none twice
        assert state[b, 65] == len(synthetic["escs"][b]) // 4
    assert (state[:, :64] == 1 << 16).all()                                   # the encoder's initial states


def test_kernel_matches_host_decoder_over_consecutive_launches(env, synthetic):
    check_consecutive_launches(env, synthetic)


def check_stops_at_the_given_stream_length(env, synthetic):
    """image 1's length is given as one word less: the cursor rule refuses that word although it is allocated memory
    (the next image's stream follows it), sets image 1's error word and leaves the other images alone"""
    got, state = _run_launches(env, synthetic, shorten=1)
    want = _expected(synthetic, (0, 2))
    assert state[1, 66] != 0 and state[0, 66] == 0 and state[2, 66] == 0
    for M in PIXELS:
        assert np.array_equal(got[M][[0, 2]], want[M][[0, 2]])
    # image 1 still wrote its destinations and nothing else; each holds the right value (decoded before the missing
    # word was needed) or the table centre (idx = W, decoded after it), and some are not the right value
    full = _expected(synthetic, (1,))
    centre = dict(synthetic, idx=np.full_like(synthetic["idx"], synthetic["W"]))
    cen = _expected(centre, (1,))
    wrong = 0
    for M in PIXELS:
        assert np.array_equal(got[M][1] == SENTINEL, full[M][1] == SENTINEL)
        assert ((got[M][1] == full[M][1]) | (got[M][1] == cen[M][1])).all()
        wrong += int((got[M][1] != full[M][1]).sum())
    assert wrong > 0


def test_kernel_stops_at_the_given_stream_length(env, synthetic):
    check_stops_at_the_given_stream_length(env, synthetic)


CASES = [(1, 2, 64, 128, "jah", 32), (3, 1, 128, 64, "jah", 32), (3, 2, 64, 192, "hmr", 32),
         (1, 3, 128, 128, "jah", 64), (3, 1, 192, 64, "jah", 64), (3, 4, 64, 256, "jah", 64),
         (1, 1, 64, 128, "jah", 192)]


@pytest.mark.parametrize("K,B,H,W,kind,M", CASES)
def test_context_codec_rans_round_trip(env, K, B, H, W, kind, M):
    nic, codec, _, dev = env
    model = _model(nic, kind, M, K, 51, dev)
    x = torch.from_numpy(R.make_image(B, H, W, 52)).to(dev).contiguous(memory_format=torch.channels_last)
    cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder="rans")
    enc = cc.compress(x)
    s = enc["strings"]
    assert s["coder"] == "rans" and len(s["y"]) == B and len(s["y_esc"]) == B and len(s["y_crc32"]) == B
    npix = B * H * W
    assert enc["bpp_coded"] == 8.0 * (len(s["z"]) + sum(map(len, s["y"])) + sum(map(len, s["y_esc"]))) / npix
    dec = cc.decompress(s, enc["shape"], enc["z_shape"])
    assert torch.equal(dec["z_hat"], enc["z_in"])
    assert torch.equal(dec["y_hat"], enc["y_in"]), "decoder tables diverged from the encoder's"
    with torch.no_grad():
        ref = model(x, training=False)
    assert torch.equal(dec["x_hat"], ref["x_hat"])
    bad = dict(s, y_crc32=[c ^ 1 for c in s["y_crc32"]])
    with pytest.raises(codec.CodecError):
        cc.decompress(bad, enc["shape"], enc["z_shape"])


def test_range_and_rans_decoders_agree(env):
    nic, codec, _, dev = env
    model = _model(nic, "jah", 32, 3, 51, dev)
    x = torch.from_numpy(R.make_image(2, 64, 128, 53)).to(dev).contiguous(memory_format=torch.channels_last)
    outs = {}
    for coder in ("range", "rans"):
        cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder=coder)
        enc = cc.compress(x)
        assert enc["strings"].get("coder", "range") == coder
        outs[coder] = cc.decompress(enc["strings"], enc["shape"], enc["z_shape"])
        assert torch.equal(outs[coder]["y_hat"], enc["y_in"])
    assert torch.equal(outs["range"]["y_hat"], outs["rans"]["y_hat"])
    assert torch.equal(outs["range"]["x_hat"], outs["rans"]["x_hat"])
    # a damaged rANS stream is reported with the image's number, by the error word or by the checksum
    cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder="rans")
    enc = cc.compress(x)
    cut = dict(enc["strings"], y=[enc["strings"]["y"][0], enc["strings"]["y"][1][:-2]])
    with pytest.raises(codec.CodecError, match="image 1"):
        cc.decompress(cut, enc["shape"], enc["z_shape"])


def test_any_size_container(env):
    nic, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    model = _model(nic, "jah", 32, 3, 51, dev)
    B, H, W = 1, 70, 100
    x = torch.from_numpy(R.make_image(B, H, W, 54)).to(dev)
    rng = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24)
    rans = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder="rans")
    blob1, blob2 = rng.compress_image(x), rans.compress_image(x)
    assert blob1[:8] == b"LICBITS1" and blob2[:8] == b"LICBITS2"
    assert rng.compress_image(x, coder="rans") == blob2 and rans.compress_image(x, coder="range") == blob1
    x1 = rng.decompress_image(blob1)
    x2 = rans.decompress_image(blob2)
    assert x2.shape == x.shape and torch.equal(x1, x2)
    assert torch.equal(x2, nic.padded_forward(model, x)["x_hat"])
    # the magic picks the coder, whatever the codec was constructed with
    assert torch.equal(rans.decompress_image(blob1), x1) and torch.equal(rng.decompress_image(blob2), x1)
    # bits per pixel: the padded run's streams and escape lists plus the container's overhead, nothing else
    enc = rans.compress(F_.pad_to_multiple(x))
    head, z, ys, es, crcs = codec.unpack_bitstream_rans(blob2)
    assert (z, ys, es, crcs) == (enc["strings"]["z"], enc["strings"]["y"], enc["strings"]["y_esc"],
                                 enc["strings"]["y_crc32"])
    overhead = 8 + 13 * 4 + 12 * B + 4
    assert len(blob2) == overhead + len(z) + sum(map(len, ys)) + sum(map(len, es))
    assert 8.0 * (len(blob2) - overhead) / (B * 128 * 128) == enc["bpp_coded"]
    with pytest.raises(codec.CodecError):
        rans.decompress_image(blob2[:-1])
