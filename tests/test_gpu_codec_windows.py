"""The device codec over its whole window range on an MI355X, not only at W = 24.

Every kernel of the y-stream path takes a window half-width W (S = 2W + 1 symbols) or a symbol count S and has code
that runs only for some values of it: lic_rans_decode_step launches rans_step_kernel<17, 66> up to W = 32 and
<33, 130> from 33 to 64 (registers, LDS size, row pitch, reciprocal, search depth), and its table fetch is
misaligned by two dwords only for even W; lic_gmm_cdf_tables' wave kernel carries a running maximum from one
64-entry chunk to the next only for S > 65; lic_factorized_cdf_tables takes a second trip through its strided loop
only for S >= 256.  This file runs the kernels against the host coder, tests/rans_ref.py, oracle/codec_ref.py and a
float64 restatement on both sides of each of those thresholds and at the ends of the accepted ranges, and the full
codecs at the windows people use (the defaults among them)."""
import math

import numpy as np
import pytest
import torch

import golden_recipe as R
import table_edges as TE
import test_gpu_rans as GR
import test_gpu_rans_encode as GE
from oracle import codec_ref as CR
from test_rans_windows_host import WINDOWS

pytestmark = pytest.mark.gpu

LIC_ERR_INVALID = -1


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib, codec
    return nic, codec, _lib, torch.device("cuda:0")


# ---- (a) the decode kernel, both instantiations ----------------------------------------------------
def _fetch_paths(B, W):
    """(gbase % 4, total % 4) of every (image, launch) of GR.LAUNCHES, as lic_rans_decode_step computes them"""
    S1 = 2 * W + 2
    return [((b * M * n * S1) % 4, (B * M * n * S1) % 4) for M, n in GR.LAUNCHES for b in range(B)]


@pytest.mark.parametrize("W", WINDOWS)
def test_decode_kernel_matches_host_decoder_at_every_window(env, W):
    syn = GR.make_synthetic(env[1], W)
    assert syn["B"] == 3 and syn["tabs"].shape[-1] == 2 * W + 2
    # the table fetch: a round's first dword sits 0 or 2 dwords past a 16-byte boundary, and the buffer's last
    # piece is partial when its length is no multiple of 4 dwords.  Both happen for even W only, in image 1 of the
    # launches with an odd symbol count; for odd W every row starts a 16-byte piece
    paths = _fetch_paths(syn["B"], W)
    if W % 2 == 0:
        assert (2, 2) in paths and (0, 2) in paths and (0, 0) in paths
    else:
        assert set(paths) == {(0, 0)}
    GR.check_consecutive_launches(env, syn)


def test_decode_kernel_stops_at_the_given_stream_length_at_the_widest_window(env):
    GR.check_stops_at_the_given_stream_length(env, GR.make_synthetic(env[1], 64))


# ---- (b) the encoder kernels ------------------------------------------------------------------------
_ENC = {}


def _enc_synthetic(codec, W):
    if W not in _ENC:
        _ENC[W] = GE.make_synthetic(codec, W)
    return _ENC[W]


@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("W", WINDOWS)
def test_encoder_kernels_match_the_host_encoder_at_every_window(env, W, M):
    """byte identity with the host encoder and rans_ref, word count nsym for the frequency-1 image and 0 for the
    near-certain one (GE.check_kernels_match_the_host_encoder), for M = 1 on the whole step list and M = 32"""
    GE.check_kernels_match_the_host_encoder(env, _enc_synthetic(env[1], W)[M])


@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("W", WINDOWS)
def test_encoder_kernels_write_nothing_outside_the_slots_at_every_window(env, W, M):
    GE.check_nothing_outside_the_slots_is_written(env, _enc_synthetic(env[1], W)[M])


# ---- (c) lic_gmm_cdf_tables beyond one chunk -------------------------------------------------------
TABLE_M, TABLE_P = 64, 514                       # 32896 elements: one more pixel row than the wave kernel takes
FLOAT64_BAND = 2                                 # counts; the project's band for these tables (erf + floor in fp32)


def _erf64(a):
    """erf of a float64 array (torch's double-precision erf; pinned to math.erf in _check_erf64)"""
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def _check_erf64():
    r = np.random.RandomState(7)
    a = np.concatenate([r.randn(4000) * 2, r.uniform(-6.5, 6.5, 4000), [0.0, -0.0, 1e-300, 40.0, -40.0, 5e5, -5e5]])
    want = np.array([math.erf(v) for v in a])
    assert np.abs(_erf64(a) - want).max() <= 4e-16


def _tables64(w_, mu_, sg_, center, W):
    """lic_gmm_cdf_tables restated in float64 from the fp32 parameters, the window placed on the DEVICE's centre:
    cum[i] = max_{j <= i} floor(clip(F_j, 0, 1) (65536 - S)) + i, F_j = sum_k w_k Phi((c - W + j - 0.5 - mu_k) / s_k)"""
    S = 2 * W + 1
    x = center.astype(np.float64)[:, None] - W + np.arange(S + 1, dtype=np.float64)[None, :] - 0.5
    F = np.zeros_like(x)
    for k in range(mu_.shape[0]):
        t = (x - mu_[k].astype(np.float64)[:, None]) / sg_[k].astype(np.float64)[:, None]
        F += w_[k].astype(np.float64)[:, None] * (0.5 * (1.0 + _erf64(t / math.sqrt(2.0))))
    c = np.floor(np.clip(F, 0.0, 1.0) * (65536 - S)).astype(np.int64)
    c[:, 0] = 0
    c = np.maximum.accumulate(np.minimum(c, 65536 - S), axis=1)
    c[:, S] = 65536 - S
    return c + np.arange(S + 1)


def _loop_and_wave(codec, act, K, W):
    """the same parameters through the loop kernel (all 514 pixels) and the wave kernel (slices of 512 and 2 pixels)
    -> (centre [P*M], tables [P*M][S+1] int64), after asserting that the two agree bit for bit"""
    M, P = TABLE_M, TABLE_P
    assert P * M > 32768 and 512 * M <= 32768
    center, tabs = codec.gmm_tables(act, M, K, W)
    parts = [codec.gmm_tables(act[:, :, p0:p1], M, K, W) for p0, p1 in ((0, 512), (512, P))]
    assert torch.equal(center.view(-1), torch.cat([c.view(-1) for c, _ in parts]))
    assert torch.equal(tabs, torch.cat([t for _, t in parts])), "loop and wave kernels built different tables"
    t = tabs.cpu().numpy().view(np.uint32).astype(np.int64)
    S = 2 * W + 1
    assert t.shape == (P * M, S + 1)
    assert (t[:, 0] == 0).all() and (t[:, S] == 65536).all() and (np.diff(t, axis=1) >= 1).all()
    return center.cpu().numpy().ravel(), t


@pytest.mark.parametrize("W", [1, 33, 64, 65, 200])
@pytest.mark.parametrize("K", [1, 3])
def test_gmm_tables_beyond_one_chunk(env, K, W):
    """Loop and wave kernels bit for bit, the table invariants, oracle/codec_ref.py under test_codec.py's conditions
    and a float64 restatement within FLOAT64_BAND counts (fp32 erf plus floor: a value that sits within an fp32
    rounding of an integer may floor to either side, and K components may do so one after the other), at windows of
    one chunk (W = 1), two (33, 64), three (65) and seven (200).

    The rows whose sigma sits at its 1e-6 floor are a step at the centre: 0 up to entry W or W + 1, the cap
    65536 - S from there on.  Where a chunk boundary lies behind that step (entry 65 for W = 33, 129 for W = 65, 257
    for W = 200; W = 64 has its only boundary, 65, exactly at the step) a share of rows enters the next chunk with
    the maximum already at the cap, and every later entry must be cap + i.  A mixture CDF with positive weights is
    monotone up to erff's last bit, so on these rows a lost carry would not show: the next test builds CDFs that
    step back."""
    _, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    M, P, S = TABLE_M, TABLE_P, 2 * W + 1
    _check_erf64()
    r = np.random.RandomState(190 + 10 * K + W)
    raw = torch.from_numpy(TE.edge_raw(r, K, M, P, W)).to(dev).contiguous(memory_format=torch.channels_last)
    act = F_.entropy_params_activation(raw, M, K)
    c, t = _loop_and_wave(codec, act, K, W)
    a = act.detach().permute(0, 2, 3, 1).reshape(P, -1).cpu().numpy()
    w_, mu_, sg_ = TE.split_act(a, K, M)
    assert (sg_ <= 1.0001e-6).mean() > 0.05 and (sg_ > 1e3).mean() > 0.03          # the edges are really there
    # saturated before a chunk boundary, and the cap held from there to the end
    cap = 65536 - S
    bounds = [b for b in range(65, S, 64) if b > W + 2]
    if W >= 33:
        assert (bounds[:1] == [65]) == (W == 33) and (bounds == []) == (W == 64)
    for b in bounds[:1]:
        sat = t[:, b - 1] == cap + b - 1
        print(f"K = {K}, W = {W}: {sat.mean():.3f} of the rows are saturated before entry {b}")
        assert sat.mean() > 0.05
        assert (t[sat][:, b - 1:S] == cap + np.arange(b - 1, S)[None, :]).all()
    # oracle/codec_ref.py, fp32 on the host: the conditions of test_codec.py
    c_ref, t_ref = CR.gmm_tables(w_, mu_, sg_, W)
    same = c == c_ref
    assert same.mean() > 0.99
    d = np.abs(t[same] - t_ref[same].astype(np.int64))
    print(f"K = {K}, W = {W}: max |device - codec_ref| = {d.max()} counts")
    assert d.max() <= 2, d.max()
    # float64, on the device's own centres: every row counts
    d64 = np.abs(t - _tables64(w_, mu_, sg_, c, W))
    print(f"K = {K}, W = {W}: max |device - float64| = {d64.max()} counts, {(d64 > 1).sum()} entries above 1")
    assert d64.max() <= FLOAT64_BAND, d64.max()


@pytest.mark.parametrize("W", [1, 33, 64, 65, 200])
def test_gmm_tables_hold_the_maximum_across_chunks(env, W):
    """The table kernels promise a non-decreasing table whatever F does ("F is forced non-decreasing").  With
    positive weights F is monotone by construction, so only a CDF that steps back shows whether the wave kernel's
    running maximum survives a chunk boundary: K = 2 with weights (1, -0.5) and narrow components is 0 up to entry
    u, 1 from u to d, 0.5 behind d.  u lies in the first chunk and d anywhere behind it, so the cap reached in chunk
    one has to be carried through every later chunk.  The means are chosen so that the window centre
    rint(mu_0 - mu_1 / 2) is exact.  W = 1 (one chunk, nothing to carry) is the control."""
    _, codec, _, dev = env
    M, P, K, S = TABLE_M, TABLE_P, 2, 2 * W + 1
    n = P * M
    r = np.random.RandomState(290 + W)
    u = r.randint(1, min(S - 1, 64), size=n) if S > 3 else np.ones(n, np.int64)       # first entry with F = 1
    d = np.array([r.randint(max(ui + 1, min(65, S - 1)), S) for ui in u]) if S > 3 else np.full(n, 2)
    aa = 2 * u - d - 1 - 2 * W                                                         # centre - W
    mu = np.stack([aa + u - 1, aa + d - 1]).astype(np.float32)                         # [K, n], between two entries
    w = np.stack([np.ones(n), np.full(n, -0.5)]).astype(np.float32)
    sg = np.full((K, n), 0.01, np.float32)
    to_act = lambda v: v.reshape(K, P, M).transpose(1, 0, 2).reshape(P, K * M)
    act = np.concatenate([to_act(w), to_act(mu), to_act(sg)], 1)                       # [P, 3KM]
    act = torch.from_numpy(np.ascontiguousarray(act.T).reshape(1, 3 * K * M, P, 1)).to(dev)
    act = act.contiguous(memory_format=torch.channels_last)
    c, t = _loop_and_wave(codec, act, K, W)
    assert (c == aa + W).all()
    cap = 65536 - S
    i = np.arange(S + 1)[None, :]
    half = math.floor(0.5 * cap)
    want = np.where(i < u[:, None], 0, cap) + i
    want[:, 0], want[:, S] = 0, 65536
    assert (half < cap) and np.array_equal(t, want), "the running maximum was lost behind the step back"
    if W >= 33:
        assert (d >= 65).all() and (u <= 64).all()
        for b in range(65, S, 64):                                # every boundary has rows that step back before it
            assert ((d < b).mean() > 0.02) or b == 65
    assert np.array_equal(t, _tables64(w, mu, sg, c, W))
    c_ref, t_ref = CR.gmm_tables(w, mu, sg, W)
    assert np.array_equal(c, c_ref) and np.array_equal(t, t_ref.astype(np.int64))


# ---- (d) lic_factorized_cdf_tables beyond one trip ---------------------------------------------------
@pytest.fixture(scope="module")
def fe_model(env):
    nic, _, _, dev = env
    model = nic.JointAutoregressiveHierarchical(16, 1)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.to(dev)


@pytest.mark.parametrize("lo,S", [(-1, 2), (-1, 3), (-127, 255), (-128, 256), (-128, 257), (-500, 1000),
                                  (-2048, 4096)])
def test_factorized_tables_beyond_one_trip(env, fe_model, lo, S):
    """the smallest tables, S + 1 = 256 entries (exactly one trip of the 256-thread loop), 257 and 258 (the second
    trip is one and two entries long), four trips, and the largest table the entry accepts"""
    _, codec, _, dev = env
    fe = fe_model.factorized_entropy_model
    got = codec.factorized_tables(fe, lo, S).cpu().numpy().view(np.uint32).astype(np.int64)

    class _Dev:  # channel_cdf through the parity-tested device path, returned on the host
        channels = 16

        @staticmethod
        def channel_cdf(c, xs):
            return fe.channel_cdf(c, xs.to(dev)).cpu()
    ref = CR.factorized_tables(_Dev, lo, S).astype(np.int64)
    assert got.shape == ref.shape == (16, S + 1)
    d = np.abs(got - ref)
    print(f"lo = {lo}, S = {S}: max |device - codec_ref| = {d.max()} counts")
    assert d.max() <= 1                                                # floor() of an fp32 product: +-1 count
    assert (got[:, 0] == 0).all() and (got[:, S] == 65536).all() and (np.diff(got, axis=1) >= 1).all()


@pytest.mark.parametrize("S", [1, 4097])
def test_factorized_tables_refuse_sizes_outside_their_range(env, fe_model, S):
    _, _, _lib, dev = env
    from neural_image_compression_amd import functional as F_
    params = fe_model.factorized_entropy_model.packed_params().detach().contiguous()
    out = torch.full((16, S + 1), -5, device=dev, dtype=torch.int32)
    rc = _lib.load().lic_factorized_cdf_tables(F_._ptr(params), 16, -1, S, F_._ptr(out), F_._stream())
    torch.cuda.synchronize()
    assert rc == LIC_ERR_INVALID
    assert (out == -5).all()                                           # no launch: nothing was written


# ---- (e) full codecs at the windows people use -----------------------------------------------------
_MODELS = {}


def _jah(env, K):
    nic, _, _, dev = env
    if K not in _MODELS:
        model = nic.JointAutoregressiveHierarchical(32, K)
        st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 51)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        _MODELS[K] = model.to(dev).eval()
    return _MODELS[K]


@pytest.mark.parametrize("K,B,H,W,y_W", [(1, 2, 64, 128, 2), (1, 2, 64, 128, 32), (1, 2, 64, 128, 33),
                                         (1, 2, 64, 128, 64), (3, 1, 64, 128, 32), (3, 1, 64, 128, 64)])
def test_context_codecs_round_trip_at_the_window(env, K, B, H, W, y_W):
    nic, codec, _, dev = env
    model = _jah(env, K)
    x = torch.from_numpy(R.make_image(B, H, W, 52)).to(dev).contiguous(memory_format=torch.channels_last)
    kw = dict(z_lo=-32, z_S=65, y_W=y_W)
    host = codec.ContextCodec(model, coder="rans", encoder="host", **kw).compress(x)
    cc = codec.ContextCodec(model, coder="rans", encoder="device", **kw)
    enc = cc.compress(x)
    s, hs = enc["strings"], host["strings"]
    assert set(s) == set(hs) == {"y", "y_esc", "y_crc32", "z", "coder"}
    for key in ("y", "y_esc", "y_crc32", "z", "coder"):
        assert s[key] == hs[key], key
    with torch.no_grad():
        ref = model(x, training=False)
    dec = cc.decompress(s, enc["shape"], enc["z_shape"])
    assert torch.equal(dec["z_hat"], enc["z_in"])
    assert torch.equal(dec["y_hat"], enc["y_in"]), "decoder tables diverged from the encoder's"
    assert torch.equal(dec["x_hat"], ref["x_hat"])
    # the range coder at the same window decodes the same latents
    rc = codec.ContextCodec(model, **kw)
    renc = rc.compress(x)
    rdec = rc.decompress(renc["strings"], renc["shape"], renc["z_shape"])
    assert torch.equal(rdec["y_hat"], dec["y_hat"]) and torch.equal(rdec["z_hat"], dec["z_hat"])
    assert torch.equal(rdec["x_hat"], dec["x_hat"])
    npix = B * H * W
    n_esc = [len(e) // 4 for e in s["y_esc"]]
    print(f"K = {K}, y_W = {y_W}: escapes per image {n_esc}, |y| max {float(enc['y_in'].abs().max())}, "
          f"coded {renc['bpp_coded']:.4f} bpp, estimated {renc['bpp_est']:.4f} bpp")
    if y_W >= 32:
        # test_context_codec_full_round_trip's bound, on the coder it was written for
        assert abs(renc["bpp_coded"] - renc["bpp_est"]) <= 0.02 * renc["bpp_est"] + (64.0 * (B + 1)) / npix
    else:
        # a window of five symbols: escapes dominate the size, and every image has some
        assert all(c > 0 for c in n_esc), n_esc


def test_container_at_the_default_windows_with_the_device_encoder(env):
    """ContextCodec's own defaults (y_W = 32, z_S = 129), which the rANS coder had never run at, at a ragged size"""
    nic, codec, _, dev = env
    model = _jah(env, 3)
    x = torch.from_numpy(R.make_image(1, 70, 100, 54)).to(dev)
    cc = codec.ContextCodec(model, coder="rans", encoder="device")
    assert (cc.y_W, cc.z_lo, cc.z_S) == (32, -64, 129)
    blob = cc.compress_image(x)
    head = codec.unpack_bitstream_rans(blob)[0]
    assert blob[:8] == b"LICBITS2" and head["y_W"] == 32 and head["z_S"] == 129 and (head["H"], head["W"]) == (70, 100)
    assert blob == codec.ContextCodec(model, coder="rans").compress_image(x)
    x_hat = cc.decompress_image(blob)
    assert x_hat.shape == x.shape and torch.equal(x_hat, nic.padded_forward(model, x)["x_hat"])
    # a codec constructed with other windows reads them from the header
    other = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24)
    assert torch.equal(other.decompress_image(blob), x_hat)


def test_range_coder_above_the_rans_limit(env):
    nic, codec, _, dev = env
    model = _jah(env, 1)
    x = torch.from_numpy(R.make_image(1, 64, 128, 52)).to(dev).contiguous(memory_format=torch.channels_last)
    cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=100)
    enc = cc.compress(x)
    dec = cc.decompress(enc["strings"], enc["shape"], enc["z_shape"])
    assert torch.equal(dec["z_hat"], enc["z_in"]) and torch.equal(dec["y_hat"], enc["y_in"])
    with torch.no_grad():
        ref = model(x, training=False)
    assert torch.equal(dec["x_hat"], ref["x_hat"])
    with pytest.raises(codec.CodecError, match="64"):
        codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=100, coder="rans")
