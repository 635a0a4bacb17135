"""ScalableCodec.decompress_images / decompress_base_images on an MI355X: LICBITS6 blobs of different sizes, batches,
slice heights and z windows decoded in one step loop, `torch.equal` to decompress_image / decompress_base_image blob by
blob, base prefixes and whole blobs mixed; the launches the loop takes; a damaged escape entry behind a resealed
container, chosen on the host so that only the latent checksum of its layer can notice."""
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

_KW = dict(z_lo=-32, z_S=65, y_W=24)
MODELS = [(32, 20, 1), (32, 12, 3)]
CASES = [(m, G) for m in MODELS for G in (1, 4)]
# (B, H, W, slice_rows, z window or None for _KW's)
BLOBS = [(1, 64, 64, None, None), (1, 70, 100, 2, None), (2, 96, 64, None, (-64, 129))]
T = 25                                            # 96x64 is coded as 128x64: an 8 x 4 latent without slices, 4 + 3 * 7 steps


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib, codec
    return nic, codec, _lib, torch.device("cuda:0")


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
def worlds(env):
    """per case: the model, a decoder, the blobs and the single-blob decodes of every blob, computed once"""
    nic, codec, _, dev = env
    out, models = {}, {}
    for m, G in CASES:
        if m not in models:
            models[m] = _build(nic, m, dev)
        model = models[m]
        blobs = []
        for i, (B, H, W, rows, zwin) in enumerate(BLOBS):
            kw = dict(_KW) if zwin is None else dict(_KW, z_lo=zwin[0], z_S=zwin[1])
            x = torch.from_numpy(R.make_image(B, H, W, 60 + i)).to(dev)
            blobs.append(codec.ScalableCodec(model, groups=G, slice_rows=rows, **kw).compress_image(x))
        cc = codec.ScalableCodec(model, **_KW)
        out[m, G] = (model, cc, blobs, [cc.decompress_image(b) for b in blobs], [cc.decompress_base_image(b) for b in blobs])
    return out


NEW = ("lic_ctx_gather_layers_ragged", "lic_rans_decode_step_layers_ragged")
OLD = ("lic_ctx_gather_layers", "lic_rans_decode_step_layers", "lic_ctx_gather", "lic_ctx_gather_ragged",
       "lic_rans_decode_step", "lic_rans_decode_step_groups", "lic_rans_decode_step_ragged")


def _counted(_lib, fn):
    lib, calls = _lib.load(), {name: 0 for name in NEW + OLD}
    entries = {name: getattr(lib, name) for name in calls}

    def counting(name):
        def call(*args):
            calls[name] += 1
            return entries[name](*args)
        return call

    for name in calls:
        setattr(lib, name, counting(name))
    try:
        out = fn()
    finally:
        for name, fn_ in entries.items():
            setattr(lib, name, fn_)
    return out, calls


def _prefixes(cc, blobs):
    """base prefixes and whole blobs mixed: a prefix, a whole blob, a prefix with other bytes behind it"""
    cut = [b[:cc.base_bytes_of(b)] for b in blobs]
    return [cut[0], blobs[1], cut[2] + b"\x5a" * 33]


def test_the_schedule_has_25_steps(env):
    codec = env[1]
    shapes = [(4, 4), (8, 8), (8, 4), (8, 4)]
    assert codec.merged_wavefront(shapes, 2, [None, 2, None, None]).T == T


@pytest.mark.parametrize("m,G", CASES)
def test_every_entry_is_the_single_decode_bit_for_bit(env, worlds, m, G):
    _, codec, _lib, _ = env
    model, cc, blobs, single, base = worlds[m, G]
    many, calls = _counted(_lib, lambda: cc.decompress_images(blobs))
    assert len(many) == len(blobs)
    for i, (got, want, (B, H, W, _, _)) in enumerate(zip(many, single, BLOBS)):
        assert got.shape == want.shape == (B, 3, H, W), i
        assert got.is_contiguous(memory_format=torch.channels_last), i
        assert torch.equal(got, want), f"blob {i} differs from decompress_image"
    # one gather and one decode launch per step of the longest image, for both layers; no other gather or decode entry
    assert calls == dict({name: T for name in NEW}, **{name: 0 for name in OLD})
    for given in (blobs, _prefixes(cc, blobs), [b[:cc.base_bytes_of(b)] for b in blobs]):
        many, calls = _counted(_lib, lambda: cc.decompress_base_images(given))
        assert calls == dict({name: T for name in NEW}, **{name: 0 for name in OLD})
        assert len(many) == len(blobs)
        for i, ((y1, F_tilde), (want_y1, want_F)) in enumerate(zip(many, base)):
            assert y1.shape[1] == model.M1 and y1.is_contiguous(memory_format=torch.channels_last), i
            assert torch.equal(y1, want_y1) and torch.equal(F_tilde, want_F), f"blob {i} differs from decompress_base_image"


@pytest.mark.parametrize("m,G", [CASES[0], CASES[3]])
def test_order_and_company_do_not_matter(env, worlds, m, G):
    _, codec, _, _ = env
    model, cc, blobs, single, base = worlds[m, G]
    for i in (0, 2):
        (alone,) = cc.decompress_images([blobs[i]])
        assert torch.equal(alone, single[i])
        ((y1, F_tilde),) = cc.decompress_base_images([blobs[i][:cc.base_bytes_of(blobs[i])]])
        assert torch.equal(y1, base[i][0]) and torch.equal(F_tilde, base[i][1])
    for got, want in zip(cc.decompress_images(blobs[::-1]), single[::-1]):
        assert torch.equal(got, want)
    for (y1, F_tilde), want in zip(cc.decompress_base_images(_prefixes(cc, blobs)[::-1]), base[::-1]):
        assert torch.equal(y1, want[0]) and torch.equal(F_tilde, want[1])
    twice = cc.decompress_images([blobs[1], blobs[1]])
    assert torch.equal(twice[0], single[1]) and torch.equal(twice[1], single[1])
    twice = cc.decompress_base_images([blobs[1], blobs[1][:cc.base_bytes_of(blobs[1])]])
    assert all(torch.equal(y1, base[1][0]) and torch.equal(F_tilde, base[1][1]) for y1, F_tilde in twice)
    # a decoder constructed with other windows and groups reads everything from the blobs
    other = codec.ScalableCodec(model, z_lo=-64, z_S=129, y_W=32, groups=2, slice_rows=3)
    for got, want in zip(other.decompress_images(blobs[:2]), single):
        assert torch.equal(got, want)
    for (y1, F_tilde), want in zip(other.decompress_base_images(blobs[1:]), base[1:]):
        assert torch.equal(y1, want[0]) and torch.equal(F_tilde, want[1])


def _last_pixel_escapes(cc, r, W):
    """per layer, how many of the LAST coded pixel's symbols are edge symbols, i.e. own the last entries of the layer's
    escape list (one image, G = 1, no slices): from the encoder's own tables, for what `compress` returned"""
    y_in = r["y_in"]
    psi = cc.model.hyper_decoder(r["z_in"]).float()
    last = y_in.permute(0, 2, 3, 1).reshape(-1, y_in.shape[1])[-1].round().to(torch.int32)
    counts = []
    for ly, (win, comb) in zip(cc.layers, cc._windows_layers(y_in, None, psi)):
        center, _ = ly.params_at(win, None, ly.prepack(), comb, W)
        sym = last[ly.c0:ly.c0 + ly.M] - center[-1] + W
        counts.append(int(((sym <= 0) | (sym >= 2 * W)).sum()))
    return counts


def test_a_damaged_escape_entry_fails_the_checksum_of_its_blob_and_layer(env, worlds):
    """y_W = 1: every symbol but the table centre is an edge symbol with an escape entry.  The entry of the last pixel's
    last edge symbol of a layer changes that value alone -- no later pixel reads it as context -- so cursors and final
    states stay right and only that layer's latent checksum can notice (the precondition comes from the encoder's own
    tables, not from a trial decode).  A flipped stream word is noticed sooner; either way a CodecError that names the
    blob, and the blobs decode again afterwards."""
    nic, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd.bitstream import pack_bitstream_layered, unpack_bitstream_layered
    model = worlds[MODELS[0], 1][0]
    cc = codec.ScalableCodec(model, z_lo=-32, z_S=65, y_W=1)
    xs = [torch.from_numpy(R.make_image(1, H, W, 70 + i)).to(dev) for i, (H, W) in enumerate([(64, 64), (70, 100), (64, 128)])]
    blobs = [cc.compress_image(x) for x in xs]
    single = [cc.decompress_image(b) for b in blobs]
    base = [cc.decompress_base_image(b) for b in blobs]
    with torch.no_grad():
        counts = _last_pixel_escapes(cc, cc.compress(F_.pad_to_multiple(xs[1], 64)), 1)
    assert min(counts) >= 1                                                      # the input's part
    head, zs, zes, layers, G, rows = unpack_bitstream_layered(blobs[1])
    for l in (0, 1):
        esc = bytearray(layers[l]["y_esc"][0])
        assert len(esc) >= 4
        esc[-4] ^= 0x04                                                          # the last entry's excess, by 4
        hurt_layers = [dict(ly) for ly in layers]
        hurt_layers[l]["y_esc"] = [bytes(esc)]
        hurt = pack_bitstream_layered(head, zs, zes, hurt_layers, G, rows)       # resealed: the container is intact
        assert len(hurt) == len(blobs[1]) and hurt != blobs[1]
        with pytest.raises(codec.CodecError, match=rf"^blob 1: image 0, layer {l}: decoded latents do not match"):
            cc.decompress_images([blobs[0], hurt, blobs[2]])
        with pytest.raises(codec.CodecError, match=rf"^image 0, layer {l}: decoded latents do not match"):
            cc.decompress_image(hurt)
        if l == 0:
            with pytest.raises(codec.CodecError, match=r"^blob 2: image 0, layer 0: decoded latents do not match"):
                cc.decompress_base_images([blobs[0], blobs[2], hurt[:cc.base_bytes_of(hurt)]])
        else:                                                                    # the base layer of that blob is whole
            got = cc.decompress_base_images([blobs[0], hurt])
            assert torch.equal(got[1][0], base[1][0]) and torch.equal(got[1][1], base[1][1])
    words = bytearray(layers[1]["y"][0])
    words[256 + (len(words) - 256) // 2 // 2 * 2] ^= 0x10                        # a stream word in the middle
    cut_layers = [layers[0], dict(layers[1], y=[bytes(words)])]
    cut = pack_bitstream_layered(head, zs, zes, cut_layers, G, rows)
    with pytest.raises(codec.CodecError, match=r"^blob 2: image 0, layer 1: "):
        cc.decompress_images([blobs[0], blobs[2], cut])
    for got, want in zip(cc.decompress_images(blobs), single):
        assert torch.equal(got, want)
