"""ContextCodec.compress_images / compress_many on an MI355X: images of different sizes and batches encoded in one
pass, byte for byte compress_image entry by entry, for every container (LICBITS2 / 3 / 4); the launches a chunk takes;
chunking, order and company change no byte; the round trip through decompress_images; refusals before any launch."""
import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

_KW = dict(z_lo=-32, z_S=65, y_W=24)
# (model, M, K, groups): the models and windows of test_gpu_decode_many.py
CASES = [("jah", 32, 3, 1), ("jah", 32, 3, 4), ("hmr", 64, 3, 4)]
IMAGES = [(1, 64, 64), (1, 70, 100), (1, 128, 192), (2, 96, 64)]
SLICE_ROWS = [None, 2, 8]
SHARED = ("lic_ctx_gather_ragged", "lic_gmm_cdf_tables", "lic_rans_encode_pick_ragged", "lic_rans_encode_ragged")
SINGLE = ("lic_ctx_gather", "lic_rans_encode_pick", "lic_rans_encode", "lic_rans_encode_groups")


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
def models(env):
    nic, _, _, dev = env
    out = {}
    for kind, M, K, _ in CASES:
        if (kind, M, K) not in out:
            model = (nic.JointAutoregressiveHierarchical if kind == "jah" else nic.HierarchicalMixtureResidual)(M, K)
            st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 51)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
            out[kind, M, K] = model.to(dev).eval()
    return out


@pytest.fixture(scope="module")
def xs(env):
    dev = env[3]
    return [torch.from_numpy(R.make_image(B, H, W, 60 + i)).to(dev) for i, (B, H, W) in enumerate(IMAGES)]


def _counted(_lib, fn):
    lib, calls = _lib.load(), {name: 0 for name in SHARED + SINGLE}
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


def _launches(per_shared):
    return dict({name: per_shared for name in SHARED}, **{name: 0 for name in SINGLE})


@pytest.fixture(scope="module")
def singles(env, models, xs):
    """compress_image of every image for every codec, computed once: {(case, slice_rows): (codec, [blob])}"""
    _, codec, _, _ = env
    out = {}
    for kind, M, K, G in CASES:
        for rows in SLICE_ROWS:
            cc = codec.ContextCodec(models[kind, M, K], coder="rans", encoder="device", groups=G, slice_rows=rows, **_KW)
            out[(kind, M, K, G), rows] = (cc, [cc.compress_image(x) for x in xs])
    return out


@pytest.mark.parametrize("rows", SLICE_ROWS)
@pytest.mark.parametrize("case", CASES)
def test_every_entry_is_compress_image_byte_for_byte(env, singles, xs, case, rows):
    _, codec, _lib, _ = env
    cc, want = singles[case, rows]
    magic = b"LICBITS4" if rows is not None else (b"LICBITS3" if case[3] > 1 else b"LICBITS2")
    assert all(b[:8] == magic for b in want)
    many, calls = _counted(_lib, lambda: cc.compress_images(xs))
    assert len(many) == len(xs) and all(isinstance(b, bytes) for b in many)
    for i, (got, ref) in enumerate(zip(many, want)):
        assert got == ref, f"image {i} differs from compress_image"
    assert calls == _launches(1)                                              # one chunk: one launch of each
    each, calls = _counted(_lib, lambda: cc.compress_images(xs, table_budget_bytes=0))
    assert each == want and calls == _launches(len(xs))                       # one item per chunk
    # two chunks: the budget holds the first three images' tables (4 + 8 * 8 + 8 * 12 latent pixels) and no more
    budget = (16 + 64 + 96) * case[1] * (2 * _KW["y_W"] + 2) * 4
    two, calls = _counted(_lib, lambda: cc.compress_images(xs, table_budget_bytes=budget))
    assert two == want and calls == _launches(2)


@pytest.mark.parametrize("rows", SLICE_ROWS)
@pytest.mark.parametrize("case", CASES)
def test_order_and_company_do_not_matter(env, singles, xs, case, rows):
    cc, want = singles[case, rows]
    assert cc.compress_images(xs[::-1]) == want[::-1]
    for i in (0, 3):
        assert cc.compress_images([xs[i]]) == [want[i]]
    assert cc.compress_images([xs[1], xs[3], xs[1]]) == [want[1], want[3], want[1]]
    assert cc.compress_images(iter(xs[:2]), "replicate", "topleft") == want[:2]
    other = cc.compress_images(xs[1:3], mode="reflect", align="center")
    assert other == [cc.compress_image(x, "reflect", "center") for x in xs[1:3]] and other != want[1:3]


@pytest.mark.parametrize("rows", [None, 2])
@pytest.mark.parametrize("case", CASES[1:])
def test_compress_many_is_compress_item_by_item(env, singles, xs, case, rows):
    from neural_image_compression_amd import functional as F_
    cc, _ = singles[case, rows]
    padded = [F_.pad_to_multiple(x, 64) for x in xs]
    many = cc.compress_many(padded)
    assert len(many) == len(padded)
    for x, got in zip(padded, many):
        ref = cc.compress(x)
        assert set(got) == set(ref) == {"strings", "shape", "z_shape", "bpp_coded", "bpp_est", "y_in", "z_in"}
        assert set(got["strings"]) == set(ref["strings"])
        assert got["strings"] == ref["strings"]
        assert got["strings"].get("groups", 1) == case[3] and got["strings"].get("slice_rows") == rows
        assert got["shape"] == ref["shape"] and got["z_shape"] == ref["z_shape"]
        assert got["bpp_coded"] == ref["bpp_coded"]
        print("bpp_est", got["bpp_est"], ref["bpp_est"])
        # the same fp64 sums of the same log-likelihoods, divided on the host instead of on the device
        assert abs(got["bpp_est"] - ref["bpp_est"]) <= 1e-12 * abs(ref["bpp_est"])
        assert torch.equal(got["y_in"], ref["y_in"]) and torch.equal(got["z_in"], ref["z_in"])


@pytest.mark.parametrize("rows", [None, 8])
@pytest.mark.parametrize("case", CASES)
def test_round_trip_through_the_batched_decoder(env, singles, xs, case, rows):
    cc, want = singles[case, rows]
    back = cc.decompress_images(cc.compress_images(xs))
    for x, got, blob in zip(xs, back, want):
        assert got.shape == x.shape and torch.equal(got, cc.decompress_image(blob))


def test_refusals_name_their_entry_and_launch_nothing(env, models, xs):
    _, codec, _lib, _ = env
    model = models["jah", 32, 3]
    cc = codec.ContextCodec(model, coder="rans", encoder="device", groups=4, **_KW)
    bad = [
        (cc, [xs[0], xs[1], xs[2][0]], r"^image 2: expected a \[B,3,H,W\] tensor"),
        (cc, [xs[0], xs[1].cpu(), xs[2]], r"^image 1: expected a tensor on the GPU"),
        (codec.ContextCodec(model, coder="rans", groups=4, **_KW), xs, r"^image 0: .*encoder='host'"),
        (codec.ContextCodec(model, **_KW), xs, r"^image 0: .*coder='range'"),
    ]
    for c, images, message in bad:
        def refused():
            with pytest.raises(codec.CodecError, match=message):
                c.compress_images(images)
        _, calls = _counted(_lib, refused)
        assert calls == _launches(0)
    _, calls = _counted(_lib, lambda: cc.compress_images([]))
    assert calls == _launches(0)
    with pytest.raises(codec.CodecError, match=r"^item 1: expected a tensor on the GPU"):
        cc.compress_many([xs[0], xs[0].cpu()])
