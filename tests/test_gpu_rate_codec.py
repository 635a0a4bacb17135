"""ContextCodec over a rate-level model (`rate_levels=3`, random gain tables): what a blob decodes to is bit
for bit the model's own evaluation forward at the blob's quality, for the default range coder, for the grouped device
rANS coder with rANS-coded z, and for a checkerboard model; the LICRATE1 envelope carries the quality; many images of
mixed quality and size encode byte for byte and decode bit for bit as the single calls; what cannot be right is refused
on the host; `compress_image_to` meets its budget.  No statement here is about size against quality: the weights are
random.

M = 16, q in {0, 0.5, 2}, images 64 x 64 and 80 x 120 (padded to 128 x 128).

Run on the MI355X box:  python -m pytest tests/test_gpu_rate_codec.py -m gpu -q"""
import numpy as np
import pytest
import torch

import gain_ref as G
import golden_recipe as R

pytestmark = pytest.mark.gpu

M, Q = 16, 3
QUALITIES = [0.0, 0.5, 2.0]
IMAGES = [(64, 64), (80, 120)]
TABLES = ("log_gain_y", "log_inv_gain_y", "log_gain_z", "log_inv_gain_z")
KINDS = {"range": ("raster", {}),
         "rans-device-G4-zrans": ("raster", dict(coder="rans", encoder="device", groups=4, z_coder="rans")),
         "checkerboard": ("checkerboard", dict(coder="rans", encoder="device", z_coder="rans"))}
INNER_MAGIC = {"range": b"LICBITS1", "rans-device-G4-zrans": b"LICBITS5", "checkerboard": b"LICBITS7"}
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


def _model(nic, dev, context="raster", rate_levels=Q):
    """weights of golden_recipe, gain tables uniform in +-0.7 (gains between 0.5 and 2); dev None: left on the host"""
    key = (context, rate_levels, dev is None)
    if key not in _MODELS:
        model = nic.JointAutoregressiveHierarchical(M, 1, context=context, rate_levels=rate_levels)
        own = model.state_dict()
        st = R.make_state([(k, tuple(v.shape)) for k, v in own.items() if k not in TABLES], 51)
        st = {k: (own[k].numpy().copy() if k.endswith(".mask") else v) for k, v in st.items()}   # the model's own mask
        if rate_levels is not None:
            r = np.random.RandomState(52)
            st.update({k: r.uniform(-0.7, 0.7, (rate_levels, M)).astype(np.float32) for k in TABLES})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        _MODELS[key] = (model if dev is None else model.to(dev)).eval()
    return _MODELS[key]


def _codec(env, kind):
    nic, codec, dev = env
    context, kw = KINDS[kind]
    model = _model(nic, dev, context)
    return model, codec.ContextCodec(model, **kw)


def _image(H, W, dev, B=1):
    return torch.from_numpy(R.make_image(B, H, W, 54 + H + W)).to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("size", IMAGES, ids=str)
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_blob_decodes_to_the_models_own_forward(env, kind, q, size):
    nic, codec, dev = env
    from neural_image_compression_amd import bitstream as bs
    model, cc = _codec(env, kind)
    img = _image(*size, dev)
    blob = cc.compress_image(img, quality=q)
    assert bs.quality_of(blob) == q
    got_q, got_Q, pad, n, inner, crc_ok = G.read_envelope(blob)
    assert (got_q, got_Q, pad, crc_ok) == (q, Q, 0, True) and inner[:8] == INNER_MAGIC[kind] and len(blob) == n + 24
    x_hat = cc.decompress_image(blob)                    # raises CodecError if the decoded symbols miss their CRC-32
    want = nic.padded_forward(model, img, quality=q)
    assert x_hat.shape == img.shape and torch.equal(x_hat, want["x_hat"])
    # the strings route, with the quality given by hand
    from neural_image_compression_amd import functional as F_
    res = cc.compress(F_.pad_to_multiple(img, 64, "replicate", "topleft"), q)
    assert res["strings"]["quality"] == q and torch.equal(res["y_in"], want["y_in"])
    bare = {k: v for k, v in res["strings"].items() if k != "quality"}
    with pytest.raises(codec.CodecError, match="a quality in"):
        cc.decompress(bare, res["shape"], res["z_shape"])
    dec = cc.decompress(bare, res["shape"], res["z_shape"], quality=q)
    assert torch.equal(dec["y_hat"], want["y_in"]) and torch.equal(dec["z_hat"], want["z_in"])
    assert torch.equal(dec["x_hat"][:, :, :size[0], :size[1]], want["x_hat"])


@pytest.mark.parametrize("kind", ["rans-device-G4-zrans", "checkerboard"])
def test_many_images_of_mixed_quality_and_size(env, kind):
    nic, codec, dev = env
    model, cc = _codec(env, kind)
    images = [_image(64, 64, dev), _image(80, 120, dev), _image(64, 64, dev, B=2), _image(80, 120, dev)]
    qs = [0.0, 0.5, 2.0, 1.25]
    singles = [cc.compress_image(x, quality=q) for x, q in zip(images, qs)]
    blobs = cc.compress_images(images, quality=qs)
    assert blobs == singles                                                   # byte for byte
    assert cc.compress_images(images[:2], quality=0.5) == [cc.compress_image(x, quality=0.5) for x in images[:2]]
    one_by_one = [cc.decompress_image(b) for b in blobs]
    together = cc.decompress_images(blobs)
    for a, b, x, q in zip(together, one_by_one, images, qs):
        assert torch.equal(a, b) and torch.equal(a, nic.padded_forward(model, x, quality=q)["x_hat"])
    # refusals of the list, before any launch: named
    with pytest.raises(codec.CodecError, match="3 qualities for 4 images"):
        cc.compress_images(images, quality=qs[:3])
    with pytest.raises(codec.CodecError, match="image 2: .*outside"):
        cc.compress_images(images, quality=[0.0, 1.0, 2.5, 1.0])
    with pytest.raises(codec.CodecError, match="a quality in"):
        cc.compress_images(images)
    bad = bytearray(blobs[1])
    bad[9] ^= 0x40                                                            # inside q
    with pytest.raises(codec.CodecError, match="blob 1: .*CRC-32"):
        cc.decompress_images([blobs[0], bytes(bad), blobs[2]])


def test_what_the_host_refuses_needs_no_device(env):
    """the refusing codecs sit over models that were never moved to the GPU: a launch would raise LicError, not CodecError"""
    nic, codec, dev = env
    from neural_image_compression_amd import bitstream as bs
    _, cc = _codec(env, "rans-device-G4-zrans")
    blob = cc.compress_image(_image(64, 64, dev), quality=0.5)
    q, _, inner = bs.unpack_rate_envelope(blob, Q)
    kw = KINDS["rans-device-G4-zrans"][1]
    host_same = codec.ContextCodec(_model(nic, None), **kw)
    host_q4 = codec.ContextCodec(_model(nic, None, rate_levels=4), **kw)
    host_plain = codec.ContextCodec(_model(nic, None, rate_levels=None), **kw)
    cases = [(host_q4, blob, "3 rate levels; this model has 4"),
             (host_same, inner, "bad magic"),                                                  # a bare blob
             (host_plain, blob, "no rate levels"),                                             # an envelope, plain codec
             (host_same, G.make_envelope(inner, 2.5, Q), "outside"),
             (host_same, G.make_envelope(inner, 0.5, Q, pad=7), "pad"),
             (host_same, G.make_envelope(inner, 0.5, Q, length=len(inner) + 4), "length"),
             (host_same, G.make_envelope(inner, 0.5, Q, crc=1), "CRC-32"),
             (host_same, blob[:-3], "length"),
             (host_same, G.make_envelope(inner[:-1] + bytes([inner[-1] ^ 1]), 0.5, Q), "CRC-32 mismatch")]  # the inner blob's
    for dec, data, names in cases:
        with pytest.raises(codec.CodecError, match=names):
            dec.decompress_image(data)
        with pytest.raises(codec.CodecError, match="blob 0: .*" + names):
            dec.decompress_images([data])
    # the plain codec still reads its own blobs, and the rate-level one refuses them
    plain_dev = codec.ContextCodec(_model(nic, dev, rate_levels=None), **kw)
    img = _image(64, 64, dev)
    plain_blob = plain_dev.compress_image(img)
    assert plain_blob[:8] == b"LICBITS5"
    assert torch.equal(plain_dev.decompress_image(plain_blob), nic.padded_forward(plain_dev.model, img)["x_hat"])
    with pytest.raises(codec.CodecError, match="bad magic"):
        cc.decompress_image(plain_blob)
    with pytest.raises(codec.CodecError, match="no rate levels"):
        plain_dev.compress_image(img, quality=1.0)


def test_compress_image_to_meets_its_budget(env):
    nic, codec, dev = env
    model, cc = _codec(env, "rans-device-G4-zrans")
    img = _image(80, 120, dev)
    steps = 4
    grid = [k * (Q - 1) / steps for k in range(steps + 1)]
    sizes = [len(cc.compress_image(img, quality=q)) for q in grid]
    print("sizes on the grid:", dict(zip(grid, sizes)))
    for budget in sorted(set(sizes)) + [max(sizes) + 1000]:
        blob, q = cc.compress_image_to(img, budget, steps=steps)
        assert len(blob) <= budget and q in grid and blob == cc.compress_image(img, quality=q)
        assert torch.equal(cc.decompress_image(blob), nic.padded_forward(model, img, quality=q)["x_hat"])
    blob, q = cc.compress_image_to(img, max(sizes) + 1000, steps=steps)
    assert q == grid[-1]                                                      # everything fits: the top of the grid
    with pytest.raises(codec.CodecError, match="does not fit"):
        cc.compress_image_to(img, min(sizes) - 1, steps=steps)
    with pytest.raises(codec.CodecError, match="steps"):
        cc.compress_image_to(img, 10 ** 6, steps=0)
