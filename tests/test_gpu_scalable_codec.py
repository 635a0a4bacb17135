"""codec.ScalableCodec end to end on an MI355X: the two layers of a ScalableImageCoding latent round-trip exactly, the
base layer decodes alone from the first base_bytes of the blob, host and device encoders write the same bytes, and
layer 0's bytes do not depend on layer 1's model."""
import struct
import zlib

import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

MODELS = [(32, 20, 1), (32, 12, 3)]
IMAGES = [(1, 64, 64), (2, 64, 192)]
CASES = [(m, G, rows) for m in MODELS for G in (1, 4) for rows in (None, 2)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import codec
    return nic, codec, torch.device("cuda:0")


def _build(nic, m, dev):
    model = nic.ScalableImageCoding(*m)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 77)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    with torch.no_grad():                                      # spread z over its window, as test_gpu_codec_zrans.py does
        for p in model.hyper_encoder.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def models(env):
    nic, _, dev = env
    return {m: _build(nic, m, dev) for m in MODELS}


def _image(shape, dev, seed=3):
    return torch.from_numpy(R.make_image(*shape, seed=seed)).to(dev)


@pytest.mark.parametrize("m,G,rows", CASES)
def test_round_trip_base_alone_and_encoders(env, models, m, G, rows):
    nic, codec, dev = env
    model = models[m]
    M, M1, K = m
    cc = codec.ScalableCodec(model, groups=G, slice_rows=rows)
    host = codec.ScalableCodec(model, groups=G, slice_rows=rows, encoder="host")
    for shape in IMAGES:
        x = _image(shape, dev)
        r = cc.compress(x)
        s = r["strings"]
        B = shape[0]
        assert len(s["layers"]) == 2 and all(len(ly["y"]) == B * G == len(ly["y_esc"]) and len(ly["y_crc32"]) == B
                                             for ly in s["layers"])
        assert s.get("groups", 1) == G and s.get("slice_rows") == rows and s["z_coder"] == "rans"
        out = cc.decompress(s, r["shape"], r["z_shape"])
        assert torch.equal(out["y_hat"], r["y_in"].round()) and torch.equal(out["z_hat"], r["z_in"].round())
        assert torch.equal(out["x_hat"], model.decoder(out["y_hat"]))
        assert torch.equal(out["F_tilde"], model.LST(out["y_hat"][:, :M1]))
        # the base layer alone, with layer 1's strings gone
        base_strings = dict(s, layers=s["layers"][:1])
        base = cc.decompress_base(base_strings, r["shape"], r["z_shape"])
        assert torch.equal(base["y1_hat"], out["y_hat"][:, :M1]) and torch.equal(base["z_hat"], out["z_hat"])
        assert torch.equal(base["F_tilde"], out["F_tilde"])
        # the container and the ledger
        blob = cc.compress_image(x)
        base_bytes = cc.base_bytes_of(blob)
        npix = B * shape[1] * shape[2]
        assert 8.0 * len(blob) / npix == r["bpp_coded"] and 8.0 * base_bytes / npix == r["bpp_coded_base"]
        assert 0 < r["bpp_coded_base"] < r["bpp_coded"] and r["bpp_est"] > 0
        assert host.compress_image(x) == blob
        assert torch.equal(cc.decompress_image(blob), out["x_hat"])
        y1, F_tilde = cc.decompress_base_image(blob[:base_bytes])
        assert torch.equal(y1, base["y1_hat"]) and torch.equal(F_tilde, base["F_tilde"])
        y1, F_tilde = cc.decompress_base_image(blob[:base_bytes] + b"\x5a" * 33)
        assert torch.equal(y1, base["y1_hat"]) and torch.equal(F_tilde, base["F_tilde"])
        y1, _ = cc.decompress_base_image(blob)
        assert torch.equal(y1, base["y1_hat"])
        with pytest.raises(codec.CodecError, match="truncated"):
            cc.decompress_image(blob[:base_bytes])


def test_any_size_goes_through_the_container(env, models):
    nic, codec, dev = env
    model = models[MODELS[0]]
    cc = codec.ScalableCodec(model, groups=4)
    x = _image((1, 100, 75), dev)
    blob = cc.compress_image(x)
    x_hat = cc.decompress_image(blob)
    assert tuple(x_hat.shape) == (1, 3, 100, 75)
    from neural_image_compression_amd import functional as F_
    r = cc.compress(F_.pad_to_multiple(x, 64, "replicate", "topleft"))
    out = cc.decompress(r["strings"], r["shape"], r["z_shape"])
    assert torch.equal(x_hat, F_.crop_window(out["x_hat"], 0, 0, 100, 75))
    assert torch.equal(out["y_hat"], r["y_in"].round())
    y1, F_tilde = cc.decompress_base_image(blob[:cc.base_bytes_of(blob)])
    assert torch.equal(y1, out["y_hat"][:, :model.M1]) and torch.equal(F_tilde, out["F_tilde"])
    assert cc.decompress_images(cc.compress_images([x, x[:, :, :64, :64]]))[0].equal(x_hat)
    # the layered entries launched once per layer instead of once per step (the benchmark's comparison): the same
    per_layer = codec.ScalableCodec(model, groups=4)
    per_layer.merge_layers = False
    assert per_layer.compress_image(x) == blob and torch.equal(per_layer.decompress_image(blob), x_hat)


def test_layer_0_does_not_depend_on_layer_1(env, models):
    """the enhancement layer's context model and MLP scaled by 1.5: the first base_bytes of the blob do not move, the
    enhancement section does"""
    nic, codec, dev = env
    model = models[MODELS[0]]
    other = _build(nic, MODELS[0], dev)
    with torch.no_grad():
        for mod in (other.context_model_2, other.entropy_parameters_2):
            for p in mod.parameters():
                p.mul_(1.5)
    x = _image((1, 64, 64), dev)
    a = codec.ScalableCodec(model, groups=4).compress_image(x)
    b = codec.ScalableCodec(other, groups=4).compress_image(x)
    nb = codec.ScalableCodec.base_bytes_of(a)
    assert codec.ScalableCodec.base_bytes_of(b) == nb and a[:nb] == b[:nb] and a[nb:] != b[nb:]
    y1a, _ = codec.ScalableCodec(model).decompress_base_image(a[:nb])
    y1b, _ = codec.ScalableCodec(other).decompress_base_image(b[:nb])
    assert torch.equal(y1a, y1b)


def test_refusals(env, models):
    nic, codec, dev = env
    model = models[MODELS[0]]
    cc = codec.ScalableCodec(model, groups=4)
    x = _image((1, 64, 64), dev)
    blob = cc.compress_image(x)
    nb = cc.base_bytes_of(blob)
    # a codec for another split of the same latent: the header check
    wrong = codec.ScalableCodec(nic.ScalableImageCoding(32, 12, 1).to(dev).eval(), groups=4)
    for call in (wrong.decompress_image, wrong.decompress_base_image):
        with pytest.raises(codec.CodecError, match="M1=20"):
            call(blob)
    # a flipped byte in a layer-1 sub-stream: the picture is refused, the base decodes
    bad = bytearray(blob)
    bad[nb + 8 * 4 + 300] ^= 0x10
    with pytest.raises(codec.CodecError):
        cc.decompress_image(bytes(bad))
    y1, _ = cc.decompress_base_image(bytes(bad))
    assert torch.equal(y1, cc.decompress_base_image(blob)[0])
    # ... and with both CRC-32 redone, so that the stream itself is what is wrong: the decoder's own checks speak
    struct.pack_into("<I", bad, len(bad) - 4, zlib.crc32(bytes(bad[:-4])) & 0xFFFFFFFF)
    with pytest.raises(codec.CodecError, match="damaged|checksum"):
        cc.decompress_image(bytes(bad))
    # a flipped byte in the base section is refused by both
    bad = bytearray(blob)
    bad[nb - 40] ^= 0x10
    for call in (cc.decompress_image, cc.decompress_base_image):
        with pytest.raises(codec.CodecError):
            call(bytes(bad))
    # constructor
    jah = nic.JointAutoregressiveHierarchical(8, 1)
    with pytest.raises(codec.CodecError, match="ScalableImageCoding"):
        codec.ScalableCodec(jah)
    with pytest.raises(codec.CodecError, match="y_W = 65"):
        codec.ScalableCodec(model, y_W=65)
    with pytest.raises(codec.CodecError, match="encoder"):
        codec.ScalableCodec(model, encoder="gpu")
    odd = nic.ScalableImageCoding(32, 20, 1)
    odd.context_model_2.masked._tap_mask = odd.context_model_1.masked._tap_mask & ~1
    with pytest.raises(codec.CodecError, match="live taps"):
        codec.ScalableCodec(odd)
    # the one-layer codec still has no use for a scalable model, and says so as before
    with pytest.raises(AttributeError):
        codec.ContextCodec(model)
