"""ContextCodec.decompress_images on an MI355X: blobs of different sizes, batches, slice heights, z windows and
containers decoded in one step loop, `torch.equal` to decompress_image blob by blob; the launches the loop takes; a
damaged escape entry behind a resealed container, chosen on the host so that only the latent checksum can notice."""
import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

_KW = dict(z_lo=-32, z_S=65, y_W=24)
# (model, M, K, groups)
CASES = [("jah", 32, 3, 1), ("jah", 32, 3, 4), ("hmr", 64, 3, 4)]
# (B, H, W, slice_rows, z window or None for _KW's)
BLOBS = [(1, 64, 64, None, None), (1, 70, 100, 2, None), (1, 128, 192, 8, None), (2, 96, 64, None, (-64, 129))]


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


@pytest.fixture(scope="module")
def worlds(env):
    """per case: the model, a decoder, the blobs (device encoder) and decompress_image of every blob, computed once"""
    nic, codec, _, dev = env
    out, models = {}, {}
    for kind, M, K, G in CASES:
        if (kind, M, K) not in models:
            models[kind, M, K] = _model(nic, kind, M, K, 51, dev)
        model = models[kind, M, K]
        blobs = []
        for i, (B, H, W, rows, zwin) in enumerate(BLOBS):
            kw = dict(_KW) if zwin is None else dict(_KW, z_lo=zwin[0], z_S=zwin[1])
            x = torch.from_numpy(R.make_image(B, H, W, 60 + i)).to(dev)
            enc = codec.ContextCodec(model, coder="rans", encoder="device", groups=G, slice_rows=rows, **kw)
            blobs.append(enc.compress_image(x))
        magics = [b[:8] for b in blobs]
        assert magics == [b"LICBITS2" if G == 1 else b"LICBITS3", b"LICBITS4", b"LICBITS4", magics[0]]
        if G == 1:
            # LICBITS3 holds one group as well, though compress_image never writes it: blob 0's payload in that container
            blobs.append(codec.pack_bitstream_grouped(*codec.unpack_bitstream_rans(blobs[0]), 1))
            assert blobs[-1][:8] == b"LICBITS3"
        cc = codec.ContextCodec(model, coder="rans", **_KW)
        out[kind, M, K, G] = (model, cc, blobs, [cc.decompress_image(b) for b in blobs])
    return out


def _counted(_lib, fn):
    lib, calls = _lib.load(), {"lic_rans_decode_step_ragged": 0, "lic_ctx_gather_ragged": 0,
                               "lic_rans_decode_step_groups": 0, "lic_rans_decode_step": 0, "lic_ctx_gather": 0}
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


@pytest.mark.parametrize("kind,M,K,G", CASES)
def test_every_entry_is_the_single_decode_bit_for_bit(env, worlds, kind, M, K, G):
    _, codec, _lib, _ = env
    model, cc, blobs, single = worlds[kind, M, K, G]
    many, calls = _counted(_lib, lambda: cc.decompress_images(blobs))
    assert len(many) == len(blobs)
    for i, (got, want, (B, H, W, _, _)) in enumerate(zip(many, single, BLOBS + BLOBS[:1])):
        assert got.shape == want.shape == (B, 3, H, W), i
        assert got.is_contiguous(memory_format=torch.channels_last), i
        assert torch.equal(got, want), f"blob {i} differs from decompress_image"
    # one gather and one decode launch per step of the longest image: 128x192 in slices of 8 rows is 12 + 3 * 7 steps,
    # 96x64 (coded as 128x64) without slices 4 + 3 * 7, 70x100 (128x128) in slices of 2 rows 8 + 3
    assert calls == {"lic_rans_decode_step_ragged": 33, "lic_ctx_gather_ragged": 33, "lic_rans_decode_step_groups": 0,
                     "lic_rans_decode_step": 0, "lic_ctx_gather": 0}


@pytest.mark.parametrize("kind,M,K,G", CASES[:2])
def test_order_and_company_do_not_matter(env, worlds, kind, M, K, G):
    _, codec, _, _ = env
    model, cc, blobs, single = worlds[kind, M, K, G]
    for i in (0, 3):
        (alone,) = cc.decompress_images([blobs[i]])
        assert torch.equal(alone, single[i])
    back = cc.decompress_images(blobs[::-1])
    for got, want in zip(back, single[::-1]):
        assert torch.equal(got, want)
    twice = cc.decompress_images([blobs[1], blobs[1]])
    assert torch.equal(twice[0], single[1]) and torch.equal(twice[1], single[1])
    # a decoder constructed with other windows and groups reads everything from the blobs
    other = codec.ContextCodec(model, z_lo=-64, z_S=129, y_W=32, coder="range")
    for got, want in zip(other.decompress_images(blobs[:2]), single):
        assert torch.equal(got, want)


def test_the_decoded_latents_pass_their_checksums(env, worlds):
    import zlib
    _, codec, _, _ = env
    model, cc, blobs, _ = worlds["jah", 32, 3, 4]
    opened = [cc._open_blob(b) for b in blobs]
    items = []
    for head, strings in opened:
        Hp, Wp = -(-head["H"] // 64) * 64, -(-head["W"] // 64) * 64
        items.append((strings, (head["B"], 32, Hp // 16, Wp // 16), (head["B"], 32, Hp // 64, Wp // 64)))
    outs = cc.decompress_many(items, [(h["z_lo"], h["z_S"]) for h, _ in opened])
    for (head, strings), out, item in zip(opened, outs, items):
        assert tuple(out["y_hat"].shape) == item[1]
        sym = out["y_hat"].permute(0, 2, 3, 1).reshape(head["B"], -1).round().to(torch.int32).cpu().numpy()
        assert [zlib.crc32(np.ascontiguousarray(s).tobytes()) & 0xFFFFFFFF for s in sym] == strings["y_crc32"]
    # without the checksums in the strings nothing else complains either: the streams were used up exactly
    bare = [({k: v for k, v in s.items() if k != "y_crc32"}, a, b) for s, a, b in items]
    for out, ref in zip(cc.decompress_many(bare, [(h["z_lo"], h["z_S"]) for h, _ in opened]), outs):
        assert torch.equal(out["x_hat"], ref["x_hat"])


def _last_pixel_escapes(cc, model, x, W):
    """how many of the LAST coded pixel's symbols are edge symbols, i.e. own the last entries of the image's escape
    list (G = 1, no slices): from the encoder's own tables, for the padded image x"""
    out = model.analysis_hyperprior(x, training=False)
    y_in = out["y_in"].contiguous()
    psi = model.hyper_decoder(out["z_in"]).float()
    win, comb = cc._windows_all(out["y_in"], None, psi)
    center, _ = cc._params_at(win, None, cc._prepack(), comb)
    sym = y_in.permute(0, 2, 3, 1).reshape(-1, y_in.shape[1]).round().to(torch.int32)[-1] - center[-1] + W
    return int(((sym <= 0) | (sym >= 2 * W)).sum())


def test_a_damaged_escape_entry_fails_the_checksum_of_its_blob(env, worlds):
    """The named case is a flipped y-stream byte that the checksum, not a cursor, catches.  No byte of the rANS words
    or states can be chosen for that on the host: any change there moves the coder states, and the read-back of the
    state blocks (final states, cursors) speaks before the checksum is computed.  So this test reads "y-stream byte"
    as a byte of the image's y payload in the container, which is its stream followed by its escape list, and damages
    the escape list; the precondition below comes from the encoder's own tables, evaluated by the model on the device,
    not from a trial decode.
    y_W = 1: every symbol but the table centre is an edge symbol with an escape entry.  The entry of the last
    pixel's last edge symbol changes that value alone -- no later pixel reads it as context -- so cursors and final
    states stay right and only the latent checksum can notice.  A flipped stream word is noticed sooner; either way a
    CodecError that names the blob, and the blobs decode again afterwards."""
    nic, codec, _, dev = env
    from neural_image_compression_amd import functional as F_
    model = worlds["jah", 32, 3, 1][0]
    kw = dict(z_lo=-32, z_S=65, y_W=1)
    cc = codec.ContextCodec(model, coder="rans", encoder="device", **kw)
    xs = [torch.from_numpy(R.make_image(1, H, W, 70 + i)).to(dev)
          for i, (H, W) in enumerate([(64, 64), (70, 100), (64, 128)])]
    blobs = [cc.compress_image(x) for x in xs]
    single = [cc.decompress_image(b) for b in blobs]
    with torch.no_grad():
        assert _last_pixel_escapes(cc, model, F_.pad_to_multiple(xs[1], 64), 1) >= 1      # the input's part
    head, z, ys, escs, crcs = codec.unpack_bitstream_rans(blobs[1])
    assert len(escs[0]) >= 4
    esc = bytearray(escs[0])
    esc[-4] ^= 0x04                                                              # the last entry's excess, by 4
    hurt = codec.pack_bitstream_rans(head, z, ys, [bytes(esc)], crcs)            # resealed: the container is intact
    assert len(hurt) == len(blobs[1]) and hurt != blobs[1]
    with pytest.raises(codec.CodecError, match=r"^blob 1: image 0: decoded latents do not match the encoder's checksum"):
        cc.decompress_images([blobs[0], hurt, blobs[2]])
    with pytest.raises(codec.CodecError, match=r"^image 0: decoded latents do not match"):
        cc.decompress_image(hurt)
    words = bytearray(ys[0])
    words[256 + (len(words) - 256) // 2 // 2 * 2] ^= 0x10                        # a stream word in the middle
    cut = codec.pack_bitstream_rans(head, z, [bytes(words)], escs, crcs)
    with pytest.raises(codec.CodecError, match=r"^blob 2: image 0: "):
        cc.decompress_images([blobs[0], blobs[2], cut])
    # a z stream that is not the encoder's: whichever check notices first names the blob
    with pytest.raises(codec.CodecError, match=r"^blob 1: "):
        cc.decompress_images([blobs[0], codec.pack_bitstream_rans(head, b"", ys, escs, crcs)])
    for got, want in zip(cc.decompress_images(blobs), single):
        assert torch.equal(got, want)
