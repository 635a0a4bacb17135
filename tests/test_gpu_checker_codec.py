"""ContextCodec on a checkerboard context model: two decode steps whatever the size, host and device encoder byte for
byte, every entry point bit for bit against `decompress`, the container LICBITS7 and its refusals.

Images are 64 x 64, 64 x 128 and 128 x 64 (latent 4 x 4, 4 x 8, 8 x 4: both parities of the row length's start, more
rows than columns and the reverse) and one 70 x 100 through `compress_image` (padding); K in {1, 3}, groups in {1, 3},
y_W in {2, 32} (y_W = 2 puts most symbols into the escape lists).

Coded against estimated size.  The existing statement (tests/test_codec.py, test_context_codec_round_trip_*; applied by
tests/test_gpu_codec_windows.py "on the coder it was written for") is
    |bpp_coded - bpp_est| <= 0.02 bpp_est + 64 (B + 1) / npix
for the RANGE coder's B y streams and one z stream: 64 bits of flush per stream.  A checkerboard codec has the "rans"
coder only, whose every sub-stream starts with 64 states of 32 bits, which that margin does not know at these sizes
(nor does it for a raster codec).  So the statement is made as there: the symbols and tables the checkerboard codec
codes go through the range coder, image by image in `two_pass` order, z through LatentCodec.encode_z, and that size is
held to the bound with its own margin.  The rANS sizes are printed beside it.

Run on the MI355X box:  python -m pytest tests/test_gpu_checker_codec.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

M = 32
IMAGES = [(64, 64), (64, 128), (128, 64)]
CONFIGS = [(K, G, y_W) for K in (1, 3) for G in (1, 3) for y_W in (2, 32)]
_MODELS = {}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import codec
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, codec, torch.device("cuda:0")


def _model(nic, dev, K, context="checkerboard"):
    if (K, context) not in _MODELS:
        model = nic.JointAutoregressiveHierarchical(M, K, context=context)
        own = model.state_dict()
        st = R.make_state([(k, tuple(v.shape)) for k, v in own.items()], 51)
        st = {k: (own[k].numpy().copy() if k.endswith(".mask") else v) for k, v in st.items()}   # the model's own mask
        model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        _MODELS[K, context] = model.to(dev).eval()
    return _MODELS[K, context]


def _image(H, W, dev, B=1):
    return torch.from_numpy(R.make_image(B, H, W, 54 + H + W)).to(dev).contiguous(memory_format=torch.channels_last)


def _codecs(codec, model, G, y_W, z_coder="rans"):
    return {enc: codec.ContextCodec(model, y_W=y_W, coder="rans", encoder=enc, groups=G, z_coder=z_coder)
            for enc in ("host", "device")}


def test_the_codec_constructs_and_refuses_what_it_cannot_code(env):
    """on the parent commit the first line raises "context mask is not causal in raster order" """
    nic, codec, dev = env
    model = _model(nic, dev, 1)
    cc = codec.ContextCodec(model, coder="rans")
    assert cc.schedule == "checkerboard"
    for h, w in ((4, 4), (4, 8), (32, 48)):
        assert len(cc._wavefront(h, w)) == 2
    with pytest.raises(codec.CodecError, match="coder='range'"):
        codec.ContextCodec(model, coder="range")
    with pytest.raises(codec.CodecError, match="coder='range'"):
        codec.ContextCodec(model)
    with pytest.raises(codec.CodecError, match="slice_rows=4"):
        codec.ContextCodec(model, coder="rans", slice_rows=4)
    with pytest.raises(codec.CodecError, match="z_coder='range'"):
        cc.compress_image(_image(64, 64, dev))
    with pytest.raises(codec.CodecError, match="z_coder='range'"):
        codec.ContextCodec(model, coder="rans", encoder="device").compress_images([_image(64, 64, dev)])
    assert codec.ContextCodec(_model(nic, dev, 1, "raster"), coder="rans").schedule == "raster"


@pytest.mark.parametrize("K,G,y_W", CONFIGS)
def test_round_trip_in_two_steps(env, K, G, y_W):
    nic, codec, dev = env
    model = _model(nic, dev, K)
    ccs = _codecs(codec, model, G, y_W)
    for H, W in IMAGES:
        x = _image(H, W, dev)
        enc = {k: cc.compress(x) for k, cc in ccs.items()}
        s = enc["device"]["strings"]
        assert s == enc["host"]["strings"], "host and device encoder differ"
        assert s["schedule"] == "checkerboard" and s["coder"] == "rans" and s["z_coder"] == "rans"
        assert len(s["y"]) == G and len(s["y_crc32"]) == 1 and s.get("groups", 1) == G
        B, _, h, w = enc["device"]["shape"]
        assert (h, w) == (H // 16, W // 16) and len(ccs["device"]._wavefront(h, w)) == 2
        calls = []
        lib = codec.L.load()
        real = lib.lic_rans_decode_step_groups
        try:
            lib.lic_rans_decode_step_groups = lambda *a: (calls.append(1), real(*a))[1]
            dec = ccs["device"].decompress(s, enc["device"]["shape"], enc["device"]["z_shape"])   # raises on a CRC
        finally:
            lib.lic_rans_decode_step_groups = real
        assert len(calls) == 2                                            # one decode launch per step: two
        assert torch.equal(dec["y_hat"], enc["device"]["y_in"]), "decoder tables diverged from the encoder's"
        assert torch.equal(dec["z_hat"], enc["device"]["z_in"])
        with torch.no_grad():
            assert torch.equal(dec["x_hat"], model.decoder(dec["y_hat"]))
            assert torch.equal(dec["x_hat"], model(x, training=False)["x_hat"])
        bad = dict(s, y_crc32=[c ^ 1 for c in s["y_crc32"]])
        with pytest.raises(codec.CodecError):
            ccs["device"].decompress(bad, enc["device"]["shape"], enc["device"]["z_shape"])
        many = ccs["device"].decompress_many([(s, enc["device"]["shape"], enc["device"]["z_shape"])] * 2)
        assert all(torch.equal(m[k], dec[k]) for m in many for k in ("x_hat", "y_hat", "z_hat"))
        (cm,) = ccs["device"].compress_many([x])
        assert cm["strings"] == s


@pytest.mark.parametrize("K,G,y_W", CONFIGS)
def test_containers_one_by_one_and_batched(env, K, G, y_W):
    nic, codec, dev = env
    model = _model(nic, dev, K)
    ccs = _codecs(codec, model, G, y_W)
    images = [_image(64, 64, dev), _image(64, 128, dev), _image(70, 100, dev)]
    blobs = [ccs["device"].compress_image(x) for x in images]
    assert [ccs["host"].compress_image(x) for x in images] == blobs
    assert ccs["device"].compress_images(images) == blobs
    singles = [ccs["device"].decompress_image(b) for b in blobs]
    batched = ccs["device"].decompress_images(blobs)
    for x, blob, one, got in zip(images, blobs, singles, batched):
        assert blob[:8] == b"LICBITS7"
        head = codec.unpack_bitstream_checker(blob)[0]                    # the CRC passes
        assert (head["H"], head["W"], head["y_W"], head["M"], head["K"]) == (x.shape[2], x.shape[3], y_W, M, K)
        assert one.shape == x.shape and torch.equal(one, got)
        with torch.no_grad():
            assert torch.equal(one, nic.padded_forward(model, x)["x_hat"])
    # a codec with other windows reads the header's
    other = codec.ContextCodec(model, y_W=7, z_lo=-20, z_S=41, coder="rans", z_coder="rans")
    assert torch.equal(other.decompress_image(blobs[2]), singles[2])


@pytest.mark.parametrize("K", [1, 3])
def test_coded_size_against_the_estimate(env, K):
    """module docstring: the existing bound, on the coder it was written for, over the checkerboard codec's own tables"""
    nic, codec, dev = env
    model = _model(nic, dev, K)
    cc = codec.ContextCodec(model, coder="rans", encoder="device", z_coder="rans")           # y_W = 32, the default
    for H, W in IMAGES:
        x = _image(H, W, dev, B=2)
        enc = cc.compress(x)
        with torch.no_grad():
            out = model.analysis_hyperprior(x, training=False)
            psi = model.hyper_decoder(out["z_in"]).float()
            win, comb = cc._windows_all(cc._context_plane(out["y_in"]), None, psi)
            center, tables = cc._params_at(win, None, cc._prepack(), comb)
        B, _, h, w = enc["shape"]
        y_sym = out["y_in"].permute(0, 2, 3, 1).reshape(B * h * w, M).round().to(torch.int32)
        order = np.concatenate([ii * w + jj for ii, jj in codec.two_pass(h, w)])
        idx = (y_sym - center + cc.y_W).view(B, h * w, M).cpu().numpy()[:, order].reshape(B, -1)
        tabs = tables.view(B, h * w, M, -1).cpu().numpy().view(np.uint32)[:, order].reshape(B, h * w * M, -1)
        assert idx.min() >= 0 and idx.max() <= 2 * cc.y_W, "a symbol left the window: the range coder has no escapes"
        y_bytes = sum(len(codec.rc_encode(np.ascontiguousarray(tabs[b]), np.ascontiguousarray(idx[b]).astype(np.int32)))
                      for b in range(B))
        z_bytes = len(codec.LatentCodec(model, cc.z_lo, cc.z_S, cc.y_W).encode_z(out["z_in"]))
        npix = B * H * W
        coded = 8.0 * (y_bytes + z_bytes) / npix
        est = float(-(out["logp_y"].double().sum() + out["logp_z"].double().sum()) / np.log(2.0) / npix)
        assert abs(est - enc["bpp_est"]) <= 1e-9 * est
        print(f"FIGURE K{K} {H}x{W}: range-coded {coded:.4f} bpp, estimated {est:.4f} bpp, rANS strings "
              f"{enc['bpp_coded']:.4f} bpp; margin used {abs(coded - est) / (0.02 * est + 64.0 * (B + 1) / npix):.3f}")
        assert abs(coded - est) <= 0.02 * est + (64.0 * (B + 1)) / npix, (coded, est)


def test_schedule_mismatches_are_refused_before_any_launch(env, monkeypatch):
    nic, codec, dev = env
    from neural_image_compression_amd import functional as F_
    checker, raster = _model(nic, dev, 1), _model(nic, dev, 1, "raster")
    cc = codec.ContextCodec(checker, coder="rans", encoder="device", z_coder="rans")
    rc = codec.ContextCodec(raster, coder="rans", encoder="device", z_coder="rans")
    x = _image(64, 64, dev)
    seven, five = cc.compress_image(x), rc.compress_image(x)
    two = codec.ContextCodec(raster, coder="rans").compress_image(x)
    one = codec.ContextCodec(raster).compress_image(x)
    assert (seven[:8], five[:8], two[:8], one[:8]) == (b"LICBITS7", b"LICBITS5", b"LICBITS2", b"LICBITS1")
    enc_c, enc_r = cc.compress(x), rc.compress(x)

    def launched():
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(F_, "_stream", launched)                           # every launch asks for the stream first
    for codec_, blobs in ((rc, [seven]), (cc, [five, two, one])):
        for blob in blobs:
            with pytest.raises(codec.CodecError, match="schedule mismatch"):
                codec_.decompress_image(blob)
            with pytest.raises(codec.CodecError, match="blob 0: schedule mismatch"):
                codec_.decompress_images([blob])
    for codec_, enc in ((rc, enc_c), (cc, enc_r)):
        with pytest.raises(codec.CodecError, match="schedule mismatch"):
            codec_.decompress(enc["strings"], enc["shape"], enc["z_shape"])
        with pytest.raises(codec.CodecError, match="item 0: schedule mismatch"):
            codec_.decompress_many([(enc["strings"], enc["shape"], enc["z_shape"])])
    with pytest.raises(codec.CodecError, match="z_coder='range'"):
        codec.ContextCodec(checker, coder="rans").compress_image(x)
    monkeypatch.undo()
    # the raster model's bytes do not depend on the new code path being there: its blob decodes as before
    assert torch.equal(rc.decompress_image(five), rc.decompress_images([five])[0])
