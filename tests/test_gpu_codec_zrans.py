"""ContextCodec(z_coder="rans") end to end on an MI355X: the hyper-latent coded by lic_rans_z_pick +
lic_rans_encode_ragged and decoded by lic_rans_z_decode, against the same codec with z_coder="range".  Only the z
bytes may differ: y streams, checksums and z_hat, y_hat, x_hat are compared bit for bit; host and device encoders and the
batched entries must give the same blobs; a damaged z sub-stream must raise."""
import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

MODELS = [("jah", 8, 1), ("hmr", 8, 3)]
IMAGES = [(1, 64, 64), (1, 100, 75), (1, 64, 192)]          # z planes 1x1, 2x2 (padded to 128x128) and 1x3
Z_WINDOWS = [None, (-1, 4)]                                 # the default window; one so narrow that z really escapes
CASES = [(m, zw, G, rows) for m in MODELS for zw in Z_WINDOWS for G in (1, 4) for rows in (None, 2)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import codec
    return nic, codec, torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(env):
    nic, _, dev = env
    out = {}
    for kind, M, K in MODELS:
        model = (nic.JointAutoregressiveHierarchical if kind == "jah" else nic.HierarchicalMixtureResidual)(M, K)
        st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 77)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        # the recipe's weights leave z at 0 almost everywhere; three times the hyper-encoder's weights spread it over
        # about -30 .. 22: inside the default window, well outside (-1, 4)
        with torch.no_grad():
            for p in model.hyper_encoder.parameters():
                if p.dim() > 1:
                    p.mul_(3.0)
        out[kind, M, K] = model.to(dev).eval()
    return out


@pytest.fixture(scope="module")
def xs(env):
    return [torch.from_numpy(R.make_image(B, H, W, 30 + i)).to(env[2]) for i, (B, H, W) in enumerate(IMAGES)]


def _codecs(codec, model, zw, G, rows):
    kw = dict(coder="rans", groups=G, slice_rows=rows, **({} if zw is None else dict(z_lo=zw[0], z_S=zw[1])))
    return (codec.ContextCodec(model, encoder="device", **kw),
            codec.ContextCodec(model, encoder="device", z_coder="rans", **kw),
            codec.ContextCodec(model, encoder="host", z_coder="rans", **kw))


def _y_part(codec, blob):
    """(y streams, y escape lists, symbol checksums, G, slice_rows) of a blob of any rANS container"""
    head, _, ys, es, crcs, G = codec._unpack(codec._format_of_magic(blob[:8]), blob)
    return ys, es, crcs, G, head.get("slice_rows")


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}-z{c[1]}-G{c[2]}-R{c[3]}".replace(" ", ""))
def test_only_the_z_bytes_differ_from_the_range_coder(env, models, xs, case):
    _, codec, _ = env
    model_key, zw, G, rows = case
    by_range, by_rans, by_host = _codecs(codec, models[model_key], zw, G, rows)
    blobs, hats = [], []
    for i, x in enumerate(xs):
        ref, blob = by_range.compress_image(x), by_rans.compress_image(x)
        assert blob[:8] == b"LICBITS5" and ref[:8] != b"LICBITS5"
        assert by_host.compress_image(x) == blob, f"image {i}: host and device encoders differ"
        assert _y_part(codec, blob) == _y_part(codec, ref), f"image {i}: y streams or checksums moved"
        head, zs, zes, _, _, _, g, r = codec.unpack_bitstream_zrans(blob)
        assert (g, r) == (G, rows) and len(zs) == len(zes) == G and all(len(s) >= 256 for s in zs)
        if zw is not None:
            assert sum(map(len, zes)) > 0, f"image {i}: the narrow window was meant to make z escape"
        want, got = by_range.decompress_image(ref), by_rans.decompress_image(blob)
        assert got.shape == x.shape and torch.equal(got, want), f"image {i}: x_hat differs from z_coder='range'"
        blobs.append(blob)
        hats.append(got)
    many = by_rans.compress_images(xs)
    assert many == blobs
    for i, got in enumerate(by_rans.decompress_images(blobs)):
        assert torch.equal(got, hats[i]), f"image {i}: decompress_images differs from decompress_image"


@pytest.mark.parametrize("model_key", MODELS, ids=lambda m: m[0])
def test_latents_are_bit_for_bit_those_of_the_range_coder(env, models, xs, model_key):
    """through compress / decompress, where z_hat and y_hat are returned: a batch of two 64x192 images"""
    _, codec, _ = env
    by_range, by_rans, by_host = _codecs(codec, models[model_key], (-1, 4), 4, 2)
    x = torch.cat([xs[2], xs[2].flip(3)])
    a, b, c = by_range.compress(x), by_rans.compress(x), by_host.compress(x)
    sa, sb = a["strings"], b["strings"]
    assert sb["z_coder"] == "rans" and "z_coder" not in sa and isinstance(sa["z"], bytes)
    assert len(sb["z"]) == len(sb["z_esc"]) == 2 * 4 and sb["z"] == c["strings"]["z"] and sb["z_esc"] == c["strings"]["z_esc"]
    assert sb["y"] == sa["y"] and sb["y_esc"] == sa["y_esc"] and sb["y_crc32"] == sa["y_crc32"]
    want = by_range.decompress(sa, a["shape"], a["z_shape"])
    got = by_rans.decompress(sb, b["shape"], b["z_shape"])
    many = by_rans.decompress_many([(sb, b["shape"], b["z_shape"]), (sa, a["shape"], a["z_shape"])])
    for k in ("z_hat", "y_hat", "x_hat"):
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(many[0][k], want[k]) and torch.equal(many[1][k], want[k]), k
    assert torch.equal(got["z_hat"], a["z_in"].round())
    one = by_rans.compress_many([x, xs[0]])
    assert one[0]["strings"] == sb and one[0]["bpp_coded"] == b["bpp_coded"]


def test_blobs_of_different_containers_and_z_windows_decode_together(env, models, xs):
    _, codec, _ = env
    model = models["jah", 8, 1]
    plain, by_rans, _ = _codecs(codec, model, None, 1, None)
    _, narrow, _ = _codecs(codec, model, (-1, 4), 1, None)
    _, sliced, _ = _codecs(codec, model, (-1, 4), 1, 2)
    blobs = [plain.compress_image(xs[0]), by_rans.compress_image(xs[1]), narrow.compress_image(xs[2]),
             sliced.compress_image(xs[1])]
    assert [b[:8] for b in blobs] == [b"LICBITS2", b"LICBITS5", b"LICBITS5", b"LICBITS5"]
    each = [plain.decompress_image(b) for b in blobs]
    for i, got in enumerate(plain.decompress_images(blobs)):
        assert torch.equal(got, each[i]), f"blob {i}"


@pytest.mark.parametrize("G", (1, 4))
def test_a_damaged_z_sub_stream_raises_naming_the_image(env, models, xs, G):
    """one byte inside a z sub-stream flipped and the container's CRC recomputed, so that the blob still opens"""
    _, codec, _ = env
    _, by_rans, _ = _codecs(codec, models["jah", 8, 1], None, G, None)
    x = torch.cat([xs[1], xs[1].flip(2)])                                        # two images: the second one is hit
    blob = by_rans.compress_image(x)
    head, zs, zes, ys, es, crcs, g, r = codec.unpack_bitstream_zrans(blob)
    hit = 1 * G + 0
    zs[hit] = bytes([zs[hit][0] ^ 0x40]) + zs[hit][1:]                           # lane 0's state: another slot
    bad = codec.pack_bitstream_zrans(head, zs, zes, ys, es, crcs, g, r)
    assert len(bad) == len(blob) and bad != blob
    with pytest.raises(codec.CodecError, match="image 1"):
        by_rans.decompress_image(bad)
    with pytest.raises(codec.CodecError, match="blob 1: image 1"):
        by_rans.decompress_images([blob, bad])
    assert torch.equal(by_rans.decompress_images([blob])[0], by_rans.decompress_image(blob))
