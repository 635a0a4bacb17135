"""Whole `compress_image` byte strings pinned on an MI355X: the codec has no floating-point reduction whose order may
vary between runs, so the blob is a fixed function of model, image and windows on a given machine and build.  For
the inputs of test_any_size_container (JAH, M = 32, K = 3, a 70 x 100 image) and the five (coder, encoder, groups)
configurations below, the SHA-256 of the blob is compared with tests/golden/bitstream_containers.json, key
"compress_image_gfx950"; every blob decodes to padded_forward's x_hat, and device and host encoders agree.  The same
key holds the MFMA kernel variants one `decompress` launches per coder (functional.KERNEL_TRACE), and the test counts
the lic_rans_decode_step_groups calls: one per wavefront step.

Regenerating the fixture: only for a DELIBERATE change of the coded bytes or of the decoder's launches.  Build the tree
whose output is to be pinned and run, on the GPU,

    python tests/test_gpu_codec_blobs.py COMMIT [output.json]        (default: the fixture itself; keeps other keys)

The module uses ContextCodec's public methods, padded_forward and KERNEL_TRACE only, so it runs unchanged on older
trees: a refactor generates the fixture on its parent's build."""
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_recipe as R  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bitstream_containers.json")
KEY = "compress_image_gfx950"
CONFIGS = [("range", "host", 1), ("rans", "host", 1), ("rans", "device", 1), ("rans", "host", 4), ("rans", "device", 4)]
MAGIC = {("range", 1): b"LICBITS1", ("rans", 1): b"LICBITS2", ("rans", 4): b"LICBITS3"}
WINDOWS = dict(z_lo=-32, z_S=65, y_W=24)
H, W = 70, 100
# the latent of the padded 128 x 128 image is 8 x 8; the 5 x 5 mask (pad 2) gives w + 3 (h - 1) wavefront steps
STEPS = 8 + 3 * (8 - 1)


def _name(cfg):
    return "%s,%s,%d" % cfg


def _setup():
    import __graft_entry__ as g
    g.build_codec()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import codec
    dev = torch.device("cuda:0")
    model = nic.JointAutoregressiveHierarchical(32, 3)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 51)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(dev).eval()
    x = torch.from_numpy(R.make_image(1, H, W, 54)).to(dev)
    codecs = {cfg: codec.ContextCodec(model, coder=cfg[0], encoder=cfg[1], groups=cfg[2], **WINDOWS) for cfg in CONFIGS}
    return nic, codec, model, x, codecs


def _traced_decompress(cc, x, counted=None):
    """one `decompress` of the padded image's strings -> (MFMA variant names, calls of the `counted` entry)"""
    from neural_image_compression_amd import _lib
    from neural_image_compression_amd import functional as F_
    enc = cc.compress(F_.pad_to_multiple(x))
    lib, calls = _lib.load(), [0]
    entry = getattr(lib, counted) if counted else None

    def counting(*args):
        calls[0] += 1
        return entry(*args)

    if counted:
        setattr(lib, counted, counting)
    F_.KERNEL_TRACE = set()
    try:
        out = cc.decompress(enc["strings"], enc["shape"], enc["z_shape"])
        names = sorted(F_.KERNEL_TRACE)
    finally:
        F_.KERNEL_TRACE = None
        if counted:
            setattr(lib, counted, entry)
    assert torch.equal(out["y_hat"], enc["y_in"])
    return names, calls[0]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    nic, codec, model, x, codecs = _setup()
    blobs = {cfg: cc.compress_image(x) for cfg, cc in codecs.items()}
    with open(FIXTURE) as f:
        golden = json.load(f)[KEY]
    return nic, model, x, codecs, blobs, golden


def test_blobs_are_the_pinned_ones(env):
    _, _, _, _, blobs, golden = env
    for cfg, blob in blobs.items():
        assert blob[:8] == MAGIC[cfg[0], cfg[2]]
        print(_name(cfg), len(blob), "bytes", hashlib.sha256(blob).hexdigest())
    assert {_name(cfg): hashlib.sha256(blob).hexdigest() for cfg, blob in blobs.items()} == golden["sha256"]


def test_device_and_host_encoders_write_the_same_blob(env):
    _, _, _, _, blobs, _ = env
    for G in (1, 4):
        assert blobs["rans", "device", G] == blobs["rans", "host", G]


def test_every_blob_decodes_to_the_padded_forward(env):
    nic, model, x, codecs, blobs, _ = env
    want = nic.padded_forward(model, x)["x_hat"]
    for cfg, blob in blobs.items():
        got = codecs[cfg].decompress_image(blob)
        assert got.shape == x.shape and torch.equal(got, want), _name(cfg)
    # the magic selects the format, whatever the codec was constructed with
    assert torch.equal(codecs["range", "host", 1].decompress_image(blobs["rans", "device", 4]), want)


def test_decompress_launches_the_pinned_kernels_once_per_step(env):
    _, _, x, codecs, _, golden = env
    names, _ = _traced_decompress(codecs["range", "host", 1], x)
    assert names and names == golden["decompress_mfma_variants"]["range"]
    for G in (1, 4):
        names, calls = _traced_decompress(codecs["rans", "host", G], x, "lic_rans_decode_step_groups")
        assert names and names == golden["decompress_mfma_variants"]["rans"]
        assert calls == STEPS


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out_path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    _, _, _, x_, codecs_ = _setup()
    rec = {"comment": "SHA-256 of compress_image's blob per 'coder,encoder,groups' and the MFMA variants of one "
                      "decompress per coder, on an MI355X at commit %s (python tests/test_gpu_codec_blobs.py COMMIT)"
                      % sys.argv[1],
           "sha256": {_name(cfg): hashlib.sha256(cc.compress_image(x_)).hexdigest() for cfg, cc in codecs_.items()},
           "decompress_mfma_variants": {
               "range": _traced_decompress(codecs_["range", "host", 1], x_)[0],
               "rans": _traced_decompress(codecs_["rans", "host", 1], x_)[0]}}
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc[KEY] = rec
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1))
