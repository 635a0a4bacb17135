"""ContextCodec(coder="rans", slice_rows=R) on an MI355X: small seeded models on 128 x 192 images, whose 8 x 12 latents
give single-row slices (R = 1), whole slices (2), a ragged last slice (3) and the one-slice case (8 >= h).  Round trips
with both encoders and G in {1, 4}, the reconstruction against the codec without slices, the step count, the LICBITS4
container at a size that is no multiple of 64, and the refusals."""
import numpy as np
import pytest
import torch

import ctx_slices_ref as SR
import golden_recipe as GRc

pytestmark = pytest.mark.gpu

CASES = [(1, 1, "jah", 32), (3, 2, "hmr", 64)]                # K, B, family, M
H, W = 128, 192
LH, LW = H // 16, W // 16
_KW = dict(z_lo=-32, z_S=65, y_W=24)
RS = [1, 2, 3, 8]


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
    st = GRc.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def unsliced(env):
    """per case and G: the model, the image and the compress / decompress of the codec without slices, computed once"""
    nic, codec, _, dev = env
    out = {}
    for K, B, kind, M in CASES:
        model = _model(nic, kind, M, K, 51, dev)
        x = torch.from_numpy(GRc.make_image(B, H, W, 52)).to(dev).contiguous(memory_format=torch.channels_last)
        for G in (1, 4):
            cc = codec.ContextCodec(model, coder="rans", groups=G, **_KW)
            enc = cc.compress(x)
            assert "slice_rows" not in enc["strings"] and enc["shape"] == (B, M, LH, LW)
            out[(K, G)] = (model, x, enc, cc.decompress(enc["strings"], enc["shape"], enc["z_shape"]))
    return out


def _counted_decompress(_lib, cc, strings, shape, z_shape):
    """-> (decompress's result, calls of lic_rans_decode_step_groups = decode steps taken, lic_ctx_gather calls)"""
    lib, calls = _lib.load(), {"lic_rans_decode_step_groups": 0, "lic_ctx_gather": 0}
    entries = {name: getattr(lib, name) for name in calls}

    def counting(name):
        def call(*args):
            calls[name] += 1
            return entries[name](*args)
        return call

    for name in calls:
        setattr(lib, name, counting(name))
    try:
        out = cc.decompress(strings, shape, z_shape)
    finally:
        for name, fn in entries.items():
            setattr(lib, name, fn)
    return out, calls["lic_rans_decode_step_groups"], calls["lic_ctx_gather"]


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("K,B,kind,M", CASES)
def test_sliced_round_trip(env, unsliced, K, B, kind, M, R, G):
    nic, codec, _lib, dev = env
    model, x, enc0, dec0 = unsliced[(K, G)]
    host = codec.ContextCodec(model, coder="rans", encoder="host", groups=G, slice_rows=R, **_KW).compress(x)
    cc = codec.ContextCodec(model, coder="rans", encoder="device", groups=G, slice_rows=R, **_KW)
    enc = cc.compress(x)
    s, hs = enc["strings"], host["strings"]
    keys = {"y", "y_esc", "y_crc32", "z", "coder", "slice_rows"} | ({"groups"} if G > 1 else set())
    assert set(s) == set(hs) == keys
    for key in keys:
        assert s[key] == hs[key], key                                   # host and device encoders: the same bytes
    assert s["slice_rows"] == R and len(s["y"]) == B * G
    # what is coded does not change, only how: the same latents, checksums and z stream as without slices
    assert torch.equal(enc["y_in"], enc0["y_in"]) and s["y_crc32"] == enc0["strings"]["y_crc32"]
    assert s["z"] == enc0["strings"]["z"]
    if R >= LH:
        assert s["y"] == enc0["strings"]["y"] and s["y_esc"] == enc0["strings"]["y_esc"]   # one slice: byte for byte
    else:
        assert s["y"] != enc0["strings"]["y"]
    # a codec that was never told about slices decodes them: the strings say so
    fresh = codec.ContextCodec(model, coder="rans", **_KW)
    dec, steps, gathers = _counted_decompress(_lib, fresh, s, enc["shape"], enc["z_shape"])
    assert steps == gathers == SR.n_steps(LH, LW, R) == LW + 3 * (min(R, LH) - 1)
    assert torch.equal(dec["y_hat"], enc["y_in"]), "decoder tables diverged from the encoder's"
    assert torch.equal(dec["z_hat"], enc["z_in"])
    assert torch.equal(dec["x_hat"], dec0["x_hat"]) and torch.equal(dec["y_hat"], dec0["y_hat"])
    # the strings carry the rule: decoded as if unsliced, or with another slice height, the checksum or the stream
    # check refuses them
    if R < LH:
        for wrong in ({k: v for k, v in s.items() if k != "slice_rows"}, dict(s, slice_rows=R + 1)):
            with pytest.raises(codec.CodecError):
                fresh.decompress(wrong, enc["shape"], enc["z_shape"])


def test_windows_all_is_the_restated_gather(env, unsliced):
    """the encoder's windows for every pixel against the numpy restatement, with and without slices"""
    nic, codec, _, dev = env
    model, x, enc0, _ = unsliced[(1, 1)]
    y = enc0["y_in"]
    y_np = y.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    for R in (None, 1, 3):
        cc = codec.ContextCodec(model, coder="rans", slice_rows=R, **_KW)
        assert [t for t in SR.TAPS] == [(r - cc.pad, s - cc.pad) for r, s in cc.taps]
        win = cc._windows_all(y, R)
        want, _ = SR.gather(y_np, LH if R is None else R, list(range(LH * LW)))
        assert win.shape == (LH * LW, 12 * 32, 1, 1) and np.array_equal(win.reshape(LH * LW, -1).cpu().numpy(), want)


def test_any_size_container_with_slices(env):
    nic, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    model = _model(nic, "jah", 32, 3, 51, dev)
    Bi, Hi, Wi, G, R = 1, 70, 100, 4, 3                                 # padded to 128 x 128: 8 latent rows, ragged
    x = torch.from_numpy(GRc.make_image(Bi, Hi, Wi, 54)).to(dev)
    cc = codec.ContextCodec(model, coder="rans", groups=G, slice_rows=R, **_KW)
    blob = cc.compress_image(x)
    assert blob[:8] == b"LICBITS4"
    assert blob == codec.ContextCodec(model, coder="rans", encoder="device", groups=G, slice_rows=R, **_KW).compress_image(x)
    want = nic.padded_forward(model, x)["x_hat"]
    got = cc.decompress_image(blob)
    assert got.shape == x.shape and torch.equal(got, want)
    for other in (codec.ContextCodec(model), codec.ContextCodec(model, coder="rans", **_KW),
                  codec.ContextCodec(model, coder="rans", groups=2, slice_rows=5, **_KW)):
        assert torch.equal(other.decompress_image(blob), want)         # the header says how to decode
    enc = cc.compress(F_.pad_to_multiple(x))
    head, z, ys, es, crcs, groups, rows = codec.unpack_bitstream_sliced(blob)
    assert (groups, rows, head["slice_rows"]) == (G, R, R)
    assert (z, ys, es, crcs) == (enc["strings"]["z"], enc["strings"]["y"], enc["strings"]["y_esc"],
                                 enc["strings"]["y_crc32"])
    # one group is written as LICBITS4 too; a codec without slices keeps writing what it wrote
    one = codec.ContextCodec(model, coder="rans", slice_rows=R, **_KW)
    blob1 = one.compress_image(x)
    assert blob1[:8] == b"LICBITS4" and torch.equal(codec.ContextCodec(model).decompress_image(blob1), want)
    assert one.compress_image(x, coder="range") == codec.ContextCodec(model, **_KW).compress_image(x)
    assert codec.ContextCodec(model, coder="rans", groups=G, **_KW).compress_image(x)[:8] == b"LICBITS3"
    # damage and another model
    with pytest.raises(codec.CodecError):
        cc.decompress_image(blob[:200] + bytes([blob[200] ^ 1]) + blob[201:])
    with pytest.raises(codec.CodecError):
        cc.decompress_image(blob[:-9])
    with pytest.raises(codec.CodecError, match="written by family 1"):
        codec.ContextCodec(_model(nic, "hmr", 32, 3, 51, dev)).decompress_image(blob)


def test_refusals(env, unsliced):
    nic, codec, _, dev = env
    model, x, enc0, _ = unsliced[(1, 1)]
    with pytest.raises(codec.CodecError, match="needs coder='rans'"):
        codec.ContextCodec(model, coder="range", slice_rows=4)
    for bad in (0, -2, 2.5, True):
        with pytest.raises(codec.CodecError, match="slice_rows"):
            codec.ContextCodec(model, coder="rans", slice_rows=bad)
    enc = codec.ContextCodec(model, coder="rans", slice_rows=2, **_KW).compress(x)
    cc = codec.ContextCodec(model, coder="rans", **_KW)
    for bad in (0, "2"):
        with pytest.raises(codec.CodecError, match="slice_rows"):
            cc.decompress(dict(enc["strings"], slice_rows=bad), enc["shape"], enc["z_shape"])
    with pytest.raises(codec.CodecError, match="slice_rows"):
        cc.decompress(dict(enc["strings"], coder="range"), enc["shape"], enc["z_shape"])
