"""The device encoder of the "rANS-64" y streams (lic_rans_encode_pick + lic_rans_encode) and
ContextCodec(coder="rans", encoder="device") on an MI355X.  The bitstream does not change, so every check is
byte identity: with the host encoder (codec.rans_encode) and with the format's restatement (tests/rans_ref.py).
The kernels on synthetic tables (images, steps and hand-placed edge symbols of tests/test_rans_encode_host.py),
canaries around everything they write, malformed tables, full codecs against the host path, the container."""
import numpy as np
import pytest
import torch

import golden_recipe as R
import rans_ref as RR
import test_rans_encode_host as EH

pytestmark = pytest.mark.gpu

W_, S_ = EH.W_, EH.S_
CANARY = 0xA5
PAD = 256                                       # canary bytes in front of and behind every output buffer


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
    """the five images in coding order with both references for the window half-width W: M = 1 on the whole step
    list, and the M = 32 rerun on the first 128 symbols"""
    tabs, idx = EH.make_images(W=W)
    out = {}
    for M, steps in ((1, EH.STEPS), (32, [32, 96])):
        n = sum(steps)
        t, i = tabs[:, :n], idx[:, :n]
        host = [codec.rans_encode(t[b], i[b].astype(np.int32), steps) for b in range(5)]
        assert host == [RR.encode(t[b], i[b], steps) for b in range(5)]
        r = np.random.RandomState(32 + M)
        P = n // M
        out[M] = {"M": M, "P": P, "W": W, "steps": steps, "tabs": t, "idx": i, "host": host,
                  "order": r.permutation(P).astype(np.int64),          # a fixed permutation, not the identity
                  "center": r.randint(-10, 11, size=(5, n)).astype(np.int64)}
        assert (out[M]["order"] != np.arange(P)).any()
        # y = idx + center - W must be an int32: the one symbol with idx = -2^31 gets center = W
        out[M]["center"][i == -2 ** 31] = W
    return out


@pytest.fixture(scope="module")
def synthetic(env):
    """the W = 24 references, computed once"""
    return make_synthetic(env[1])


def _raster(syn, images, tabs=None):
    """coding order -> what lic_gmm_cdf_tables would have left: tables [B][P*M][S+1], center [B*P][M], y [B][P][M]
    in RASTER pixel order (coded position p is pixel order[p])"""
    M, P, order = syn["M"], syn["P"], syn["order"]
    tabs = syn["tabs"] if tabs is None else tabs
    B, W, S1 = len(images), syn["W"], tabs.shape[-1]
    assert S1 == 2 * W + 2
    t_r = np.zeros((B, P, M, S1), np.uint32)
    c_r, y_r = np.zeros((B, P, M), np.int32), np.zeros((B, P, M), np.int32)
    for j, b in enumerate(images):
        y = syn["idx"][b] + syn["center"][b] - W
        assert (y >= -2 ** 31).all() and (y < 2 ** 31).all()
        t_r[j, order] = tabs[b].reshape(P, M, S1)
        c_r[j, order] = syn["center"][b].reshape(P, M)
        y_r[j, order] = y.reshape(P, M)
    return t_r.reshape(B, P * M, S1), c_r.reshape(B * P, M), y_r


def _launch(env, syn, t_r, c_r, y_r):
    """pick + encode on buffers framed by canaries -> (state [B][67] uint32, slot, and the whole words / escape /
    state buffers, frames included, as bytes / uint32)"""
    _, _, _lib, dev = env
    from neural_image_compression_amd import functional as F_
    lib, B, M, P = _lib.load(), t_r.shape[0], syn["M"], syn["P"]
    nsym = P * M
    slot = (256 + 2 * nsym + 3) // 4 * 4
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_t, d_c, d_y = up(t_r.view(np.int32)), up(c_r), up(y_r)
    d_order, d_steps = up(syn["order"]), up(np.array(syn["steps"], np.int64))
    sf = torch.empty((B, nsym), device=dev, dtype=torch.int32)
    exc = torch.empty_like(sf)
    words = torch.full((PAD + B * slot + PAD,), CANARY, device=dev, dtype=torch.uint8)
    esc = torch.full((PAD + 4 * B * nsym + PAD,), CANARY, device=dev, dtype=torch.uint8)
    state = torch.full((PAD + 4 * B * 67 + PAD,), CANARY, device=dev, dtype=torch.uint8)
    sview = state[PAD:PAD + 4 * B * 67].view(torch.int32).view(B, 67)
    sview[:, 66] = 0                                                   # the caller zeroes the error words
    off = lambda t: t.data_ptr() + PAD
    rc = lib.lic_rans_encode_pick(F_._ptr(d_t), F_._ptr(d_c), F_._ptr(d_y), F_._ptr(d_order), B, P, M, syn["W"], F_._ptr(sf),
                                  F_._ptr(exc), off(state), F_._stream())
    assert rc == 0
    rc = lib.lic_rans_encode(F_._ptr(sf), F_._ptr(exc), F_._ptr(d_steps), len(syn["steps"]), B, nsym, off(words), slot,
                             off(esc), off(state), F_._stream())
    assert rc == 0
    torch.cuda.synchronize()
    st = state.cpu().numpy()
    return (st[PAD:PAD + 4 * B * 67].view(np.uint32).reshape(B, 67), slot, words.cpu().numpy(), esc.cpu().numpy(), st)


def _stream_of(st, slot, words, esc, j, nsym):
    """image j's stream and escape list, assembled as the host does"""
    nw, ne = int(st[j, 64]), int(st[j, 65])
    assert 2 * nw <= slot and ne <= nsym
    end = PAD + (j + 1) * slot
    e0 = PAD + 4 * j * nsym
    return st[j, :64].astype("<u4").tobytes() + words[end - 2 * nw:end].tobytes(), esc[e0:e0 + 4 * ne].tobytes()


def check_kernels_match_the_host_encoder(env, syn):
    """streams, escape lists and counts of the five images against the host encoder's, whatever the window"""
    _, codec, _, _ = env
    M = syn["M"]
    nsym = syn["P"] * M
    st, slot, words, esc, _ = _launch(env, syn, *_raster(syn, range(5)))
    assert (st[:, 66] == 0).all(), st[:, 66]
    for b in range(5):
        stream, elist = _stream_of(st, slot, words, esc, b, nsym)
        ref_stream, ref_esc = syn["host"][b]
        assert stream == ref_stream, f"image {b} ({EH.KINDS[b]}): stream differs from the host encoder's"
        assert elist == ref_esc, f"image {b}: escape list differs"
        assert st[b, 64] == (len(ref_stream) - 256) // 2 and st[b, 65] == len(ref_esc) // 4
        back = codec.rans_decode(stream, elist, syn["tabs"][b], syn["steps"])
        assert (back == syn["idx"][b]).all()
    # the two ends of the word cursor: one word per symbol, and none
    assert st[3, 64] == nsym and st[4, 64] == 0
    if M == 1:
        # the escape lists by the format's rule (idx <= 0 or idx >= S - 1): 7, 0 and 3 entries
        n_esc = [EH.escape_count(syn["idx"][b], 2 * syn["W"] + 1) for b in range(3)]
        assert n_esc == [7, 0, 3] and [len(syn["host"][b][1]) for b in range(3)] == [4 * c for c in n_esc]


@pytest.mark.parametrize("M", [1, 32])
def test_kernels_match_the_host_encoder(env, synthetic, M):
    check_kernels_match_the_host_encoder(env, synthetic[M])


def check_nothing_outside_the_slots_is_written(env, syn):
    nsym, B = syn["P"] * syn["M"], 5
    st, slot, words, esc, state = _launch(env, syn, *_raster(syn, range(5)))
    keep_w, keep_e = np.ones(words.size, bool), np.ones(esc.size, bool)
    for b in range(B):
        end = PAD + (b + 1) * slot
        keep_w[end - 2 * int(st[b, 64]):end] = False
        keep_e[PAD + 4 * b * nsym:PAD + 4 * (b * nsym + int(st[b, 65]))] = False
    assert keep_w.sum() > 2 * PAD and keep_e.sum() > 2 * PAD                # frames, and slack between the images
    assert (words[keep_w] == CANARY).all(), "bytes outside [slot_end - 2 * count, slot_end) were written"
    assert (esc[keep_e] == CANARY).all(), "escape entries beyond the count were written"
    assert (state[:PAD] == CANARY).all() and (state[PAD + 4 * B * 67:] == CANARY).all()


def test_nothing_outside_the_slots_is_written(env, synthetic):
    check_nothing_outside_the_slots_is_written(env, synthetic[1])


@pytest.mark.parametrize("damage", ["last entry 65535", "frequency 0"])
def test_malformed_table_sets_that_images_error_word(env, synthetic, damage):
    """argument validation: the launch succeeds, image 1 reports, images 0 and 2 are coded as if nothing had happened"""
    syn = synthetic[1]
    tabs = syn["tabs"].copy()
    k = 200
    if damage == "last entry 65535":
        tabs[1, k, S_] = 65535
    else:
        s = int(syn["idx"][1, k])
        assert 0 < s < S_ - 1
        tabs[1, k, s + 1] = tabs[1, k, s]
    st, slot, words, esc, _ = _launch(env, syn, *_raster(syn, range(3), tabs))
    assert st[1, 66] != 0 and st[0, 66] == 0 and st[2, 66] == 0
    for b in (0, 2):
        assert _stream_of(st, slot, words, esc, b, syn["P"]) == syn["host"][b]


CASES = [(1, 2, 64, 128, "jah", 32), (3, 2, 64, 192, "hmr", 32), (3, 4, 64, 256, "jah", 64),
         (1, 1, 64, 128, "jah", 192)]


@pytest.mark.parametrize("K,B,H,W,kind,M", CASES)
def test_context_codec_device_encoder_writes_the_host_bytes(env, K, B, H, W, kind, M):
    nic, codec, _, dev = env
    model = _model(nic, kind, M, K, 51, dev)
    x = torch.from_numpy(R.make_image(B, H, W, 52)).to(dev).contiguous(memory_format=torch.channels_last)
    host = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder="rans", encoder="host").compress(x)
    cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24, coder="rans", encoder="device")
    enc = cc.compress(x)
    s, hs = enc["strings"], host["strings"]
    assert set(s) == set(hs) == {"y", "y_esc", "y_crc32", "z", "coder"}
    for key in ("y", "y_esc", "y_crc32", "z", "coder"):
        assert s[key] == hs[key], key
    assert all(isinstance(v, bytes) for v in s["y"] + s["y_esc"])
    assert enc["bpp_coded"] == host["bpp_coded"] and enc["shape"] == host["shape"] and enc["z_shape"] == host["z_shape"]
    dec = cc.decompress(s, enc["shape"], enc["z_shape"])
    assert torch.equal(dec["y_hat"], enc["y_in"])
    with torch.no_grad():
        ref = model(x, training=False)
    assert torch.equal(dec["x_hat"], ref["x_hat"])


def test_container_with_the_device_encoder(env):
    nic, codec, _, dev = env
    model = _model(nic, "jah", 32, 3, 51, dev)
    x = torch.from_numpy(R.make_image(1, 70, 100, 54)).to(dev)
    kw = dict(z_lo=-32, z_S=65, y_W=24)
    host = codec.ContextCodec(model, coder="rans", encoder="host", **kw)
    device = codec.ContextCodec(model, coder="rans", encoder="device", **kw)
    blob = device.compress_image(x)
    assert blob[:8] == b"LICBITS2" and blob == host.compress_image(x)
    x_hat = device.decompress_image(blob)
    assert x_hat.shape == x.shape and torch.equal(x_hat, nic.padded_forward(model, x)["x_hat"])
    # the other coder has no device encoder: the temporary codec falls back to the host's, and back again
    rng = codec.ContextCodec(model, **kw)
    assert device.compress_image(x, coder="range") == rng.compress_image(x)
    assert rng.compress_image(x, coder="rans") == blob
