"""The encode paths of codec.py on an MI355X, pinned against each other: the host and the device rANS encoder write the
same strings for every G, slice_rows and z coder; compress_many is compress item by item; both encoders of the scalable
codec agree; every blob decodes; the single-item paths launch what they always launched; an encoder refusal names its
image.  The CRC-32 of every configuration's blobs is printed (-s), so two trees can be compared by their bytes."""
import zlib

import pytest
import torch

import golden_recipe as R
import test_gpu_compress_many as CM
import test_gpu_scalable_codec as SC

pytestmark = pytest.mark.gpu

_KW = dict(z_lo=-32, z_S=65, y_W=24)
# a 4x4 latent (most wavefront steps hold one pixel, G = 4 leaves sub-streams empty), a batch of two, a larger plane
IMAGES = [(1, 64, 64), (2, 64, 128), (1, 128, 192)]
CONFIGS = [(G, rows, z) for G in (1, 4) for rows in (None, 2) for z in ("range", "rans")]
SCALABLE = (32, 20, 1)
EXTRA = ("lic_rans_z_pick", "lic_ctx_gather_layers")
RAGGED = ("lic_ctx_gather_ragged", "lic_rans_encode_pick_ragged", "lic_rans_encode_ragged")
MALFORMED = "the rANS encoder met a malformed table, a pixel index outside the image or step lengths that do not add up"


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib, codec
    return nic, codec, _lib, torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(env):
    nic, _, _, dev = env
    m = nic.JointAutoregressiveHierarchical(32, 3)
    st = R.make_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 51)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def scalable(env):
    nic, _, _, dev = env
    return SC._build(nic, SCALABLE, dev)


@pytest.fixture(scope="module")
def xs(env):
    dev = env[3]
    return [torch.from_numpy(R.make_image(B, H, W, 80 + i)).to(dev) for i, (B, H, W) in enumerate(IMAGES)]


def _decoded(model, r):
    """what the decoder must give back for `compress`'s result r: the synthesis of the rounded latents"""
    return model.decoder(r["y_in"].round().contiguous(memory_format=torch.channels_last))


@pytest.fixture(scope="module")
def coded(env, model, xs):
    """{(encoder, G, rows, z_coder): (codec, [compress(x)], [compress_image(x)])}, computed once"""
    codec = env[1]
    out = {}
    for enc in ("host", "device"):
        for G, rows, z in CONFIGS:
            cc = codec.ContextCodec(model, coder="rans", encoder=enc, groups=G, slice_rows=rows, z_coder=z, **_KW)
            out[enc, G, rows, z] = (cc, [cc.compress(x) for x in xs], [cc.compress_image(x) for x in xs])
    return out


@pytest.fixture(scope="module")
def coded_scalable(env, scalable, xs):
    """{(encoder, G): (codec, [compress(x)], [compress_image(x)])} of the scalable codec"""
    codec = env[1]
    out = {}
    for enc in ("host", "device"):
        for G in (1, 4):
            cc = codec.ScalableCodec(scalable, groups=G, encoder=enc)
            out[enc, G] = (cc, [cc.compress(x) for x in xs], [cc.compress_image(x) for x in xs])
    return out


def _crc(blobs) -> int:
    return zlib.crc32(b"".join(blobs)) & 0xFFFFFFFF


@pytest.mark.parametrize("G,rows,z", CONFIGS)
def test_host_and_device_encoders_agree_and_the_blobs_decode(coded, model, xs, G, rows, z):
    (_, host, host_blobs), (cc, dev, dev_blobs) = coded["host", G, rows, z], coded["device", G, rows, z]
    for enc, blobs in (("host", host_blobs), ("device", dev_blobs)):
        print(f"crc32 context encoder={enc} G={G} slice_rows={rows} z_coder={z}: {_crc(blobs):08x}")
    for i, (a, b) in enumerate(zip(host, dev)):
        assert set(a["strings"]) == set(b["strings"])
        assert a["strings"] == b["strings"], f"image {i}: the encoders' strings differ"
        assert a["strings"].get("groups", 1) == G and a["strings"].get("slice_rows") == rows
        assert a["strings"].get("z_coder", "range") == z and a["strings"]["coder"] == "rans"
        assert len(a["strings"]["y"]) == len(a["strings"]["y_esc"]) == IMAGES[i][0] * G
    assert host_blobs == dev_blobs
    for x, r, blob in zip(xs, dev, dev_blobs):                     # the host encoder's blobs are these very bytes
        got = cc.decompress_image(blob)
        assert got.shape == x.shape and torch.equal(got, _decoded(model, r))


@pytest.mark.parametrize("G,rows,z", CONFIGS)
def test_compress_many_is_compress(coded, xs, G, rows, z):
    cc, single, _ = coded["device", G, rows, z]
    many = cc.compress_many(xs)
    assert len(many) == len(xs)
    for i, (got, ref) in enumerate(zip(many, single)):
        assert set(got) == set(ref) and set(got["strings"]) == set(ref["strings"])
        assert got["strings"] == ref["strings"], f"item {i}: compress_many's strings differ from compress's"
        assert got["shape"] == ref["shape"] and got["z_shape"] == ref["z_shape"]
        assert got["bpp_coded"] == ref["bpp_coded"]
        print(f"bpp_est G={G} slice_rows={rows} z_coder={z} item {i}: many {got['bpp_est']!r} single {ref['bpp_est']!r} "
              f"equal {got['bpp_est'] == ref['bpp_est']}")
        assert abs(got["bpp_est"] - ref["bpp_est"]) <= 1e-12 * abs(ref["bpp_est"])


@pytest.mark.parametrize("G", (1, 4))
def test_scalable_encoders_agree_and_the_blobs_decode(coded_scalable, scalable, xs, G):
    (_, host, host_blobs), (cc, dev, dev_blobs) = coded_scalable["host", G], coded_scalable["device", G]
    for enc, blobs in (("host", host_blobs), ("device", dev_blobs)):
        print(f"crc32 scalable encoder={enc} G={G}: {_crc(blobs):08x}")
    for i, (a, b) in enumerate(zip(host, dev)):
        assert a["strings"] == b["strings"], f"image {i}: the encoders' strings differ"
        assert len(a["strings"]["layers"]) == 2 and a["strings"].get("groups", 1) == G
        assert a["bpp_coded"] == b["bpp_coded"] and a["bpp_coded_base"] == b["bpp_coded_base"]
    assert host_blobs == dev_blobs
    for x, r, blob in zip(xs, dev, dev_blobs):
        got = cc.decompress_image(blob)
        assert got.shape == x.shape and torch.equal(got, _decoded(scalable, r))


def _counted(_lib, fn):
    """`test_gpu_compress_many._counted` with the z pick and the layered gather counted as well"""
    lib, extra = _lib.load(), {name: 0 for name in EXTRA}
    entries = {name: getattr(lib, name) for name in EXTRA}

    def counting(name):
        def call(*args):
            extra[name] += 1
            return entries[name](*args)
        return call

    for name in EXTRA:
        setattr(lib, name, counting(name))
    try:
        out, calls = CM._counted(_lib, fn)
    finally:
        for name, fn_ in entries.items():
            setattr(lib, name, fn_)
    return out, dict(calls, **extra)


@pytest.mark.parametrize("G,rows,z", CONFIGS)
def test_launches_of_a_single_compress(env, coded, xs, G, rows, z):
    _lib = env[2]
    cc = coded["device", G, rows, z][0]
    for x in xs:
        _, calls = _counted(_lib, lambda: cc.compress(x))
        want = dict.fromkeys(CM.SHARED + CM.SINGLE + EXTRA, 0)
        want.update(lic_ctx_gather=1, lic_gmm_cdf_tables=1, lic_rans_encode_pick=1)
        want["lic_rans_encode" if G == 1 else "lic_rans_encode_groups"] = 1
        if z == "rans":                                            # z: its own pick, and the ragged encoder once
            want.update(lic_rans_z_pick=1, lic_rans_encode_ragged=1)
        assert calls == want
        assert all(calls[name] == 0 for name in RAGGED if not (z == "rans" and name == "lic_rans_encode_ragged"))


@pytest.mark.parametrize("G", (1, 4))
def test_launches_of_a_scalable_compress(env, coded_scalable, xs, G):
    _lib = env[2]
    cc = coded_scalable["device", G][0]
    _, calls = _counted(_lib, lambda: cc.compress(xs[1]))
    want = dict.fromkeys(CM.SHARED + CM.SINGLE + EXTRA, 0)
    want.update(lic_ctx_gather_layers=1, lic_gmm_cdf_tables=2, lic_rans_encode_pick=2, lic_rans_z_pick=1,
                lic_rans_encode_ragged=1)                          # pick and encode once per layer; z as above
    want["lic_rans_encode" if G == 1 else "lic_rans_encode_groups"] = 2
    assert calls == want


@pytest.mark.parametrize("G", (1, 4))
def test_an_encoder_refusal_names_its_image(env, coded, xs, G):
    """pick's error word of image 1 is set behind the real call (a host-side wrapper around the entry: the kernels run
    as always, only the word the host reads differs): compress must refuse, naming image 1"""
    _, codec, _lib, _ = env
    from neural_image_compression_amd import functional as F_
    cc = coded["device", G, None, "range"][0]
    lib, pick, ptr_of = _lib.load(), _lib.load().lic_rans_encode_pick, F_._ptr
    seen = {}

    def remembering(t):
        p = ptr_of(t)
        if t is not None:
            seen[p.value] = t
        return p

    def spoiled(*args):
        rc = pick(*args)
        blocks = seen[args[10].value].reshape(-1)                  # pick's blocks, one per image
        blocks[1 * _lib.RANS_STATE_WORDS + _lib.RANS_LANES + 2] |= 4
        return rc

    F_._ptr, lib.lic_rans_encode_pick = remembering, spoiled
    try:
        with pytest.raises(codec.CodecError) as err:
            cc.compress(xs[1])
    finally:
        F_._ptr, lib.lic_rans_encode_pick = ptr_of, pick
    assert str(err.value).startswith(f"image 1: {MALFORMED} (error word 4)")
    assert cc.compress(xs[1])["strings"] == coded["device", G, None, "range"][1][1]["strings"]
