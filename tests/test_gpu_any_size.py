"""Images of any size end to end: the random-crop loader, padded_forward, the self-describing bitstream and the
padded evaluation.  Bitwise comparisons throughout: the padded paths run the same kernels on the same shapes
as a hand-padded call."""
import numpy as np
import pytest
import torch

import golden_recipe as R
import window_ref as WR

pytestmark = pytest.mark.gpu

SHAPES = [(375, 501), (256, 256), (257, 301), (300, 259), (512, 767), (260, 256), (256, 333), (411, 289), (290, 290)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import codec, data
    import __graft_entry__ as g
    g.build_codec()
    return nic, data, codec, torch.device("cuda:0")


def _model(nic, kind, M, K, seed, dev):
    model = (nic.JointAutoregressiveHierarchical if kind == "jah" else nic.HierarchicalMixtureResidual)(M, K)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return model.to(dev).eval()


def _ragged(tmp_path, data):
    imgs = [np.random.RandomState(200 + i).randint(0, 256, (h, w, 3)).astype(np.uint8) for i, (h, w) in enumerate(SHAPES)]
    a, b = str(tmp_path / "a.lic2"), str(tmp_path / "b.lic2")
    data.write_ragged_shard(a, imgs[:5])
    data.write_ragged_shard(b, imgs[5:])
    return data.RaggedShardDataset([a, b]), imgs


def test_random_crop_loader_resident_and_staged_agree_with_the_reference(env, tmp_path):
    nic, data, codec, dev = env
    ds, imgs = _ragged(tmp_path, data)
    res = data.RandomCropLoader(ds, 4, crop=256, device=dev, seed=3, hflip=True, resident=True)
    stg = data.RandomCropLoader(ds, 4, crop=256, device=dev, seed=3, hflip=True, resident=False)
    assert len(res) == len(stg) == 2
    epochs = []
    for epoch in range(2):
        sched = res.schedule(epoch)
        assert np.array_equal(sched, stg.schedule(epoch)) and sched.shape == (8, 4)
        a, b = list(res), list(stg)
        assert len(a) == len(b) == 2
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.shape == (4, 3, 256, 256) and x.dtype == torch.float32 and x.device.type == "cuda"
            assert x.is_contiguous(memory_format=torch.channels_last)
            ref = WR.batch_ref(imgs, sched[4 * k:4 * k + 4], 256)
            assert np.array_equal(x.permute(0, 2, 3, 1).cpu().numpy(), ref)
            assert torch.equal(x, y)
        epochs.append(torch.cat(a))
    assert not torch.equal(epochs[0], epochs[1])
    # the last, short batch and the rank slices
    tail = data.RandomCropLoader(ds, 4, crop=256, device=dev, seed=3, drop_last=False)
    assert [t.shape[0] for t in tail] == [4, 4, 1]
    r1 = data.RandomCropLoader(ds, 2, crop=256, device=dev, seed=3, rank=1, world_size=2)
    got = torch.cat(list(r1))
    assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy(), WR.batch_ref(imgs, r1.schedule(0), 256))
    with pytest.raises(ValueError, match="7 of 9"):
        data.RandomCropLoader(ds, 4, crop=300, device=dev)
    with pytest.raises(nic._lib.LicError):
        data.RandomCropLoader(ds, 4, crop=256, device="cpu")


def test_trainer_runs_on_the_random_crop_loader(env, tmp_path):
    nic, data, codec, dev = env
    from neural_image_compression_amd.trainer import Trainer
    ds, _ = _ragged(tmp_path, data)
    loader = data.RandomCropLoader(ds, 2, crop=256, device=dev, seed=1, hflip=True)
    model = _model(nic, "jah", 16, 1, 5, dev).train()
    opt = nic.FusedAdam(model.parameters(), lr=1e-4)
    losses = []

    class Rec:
        def add_scalar(self, tag, value, step):
            if tag == "losses/bpp_total":
                losses.append(value)

        def close(self):
            pass

    tr = Trainer(model, opt, loader, rd_loss=nic.rd_loss, lambda_val=0.01, max_steps=2, log_interval=10 ** 6,
                 val_interval=10 ** 6, checkpoint_path=None, device=dev, writer=Rec(), distributed=False)
    tr.log_statistics = False
    tr.train()
    assert tr.step == 2 and len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses)
    _, res = tr.train_step(next(iter(loader)))
    assert np.isfinite(float(res["loss"].detach()))


CASES = [("jah", 1, 1, 375, 500), ("hmr", 3, 2, 200, 328), ("jah", 3, 2, 200, 328), ("hmr", 1, 1, 375, 500)]


@pytest.mark.parametrize("kind,K,B,H,W", CASES)
def test_padded_forward_is_the_hand_padded_run_cropped(env, kind, K, B, H, W):
    nic, data, codec, dev = env
    model = _model(nic, kind, 32, K, 31, dev)
    x = torch.from_numpy(R.make_image(B, H, W, 32)).to(dev)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        model(x, training=False)
    out = nic.padded_forward(model, x)
    Hp, Wp = -(-H // 64) * 64, -(-W // 64) * 64
    assert out["x_hat"].shape == x.shape and out["padded_hw"] == (Hp, Wp) and out["window"] == (0, 0, H, W)
    with torch.no_grad():
        ref = model(torch.nn.functional.pad(x, (0, Wp - W, 0, Hp - H), mode="replicate"), training=False)
    assert torch.equal(out["x_hat"], ref["x_hat"][:, :, :H, :W])
    rates = [k for k, v in ref.items() if torch.is_tensor(v) and k != "x_hat"]
    assert {"logp_y", "logp_z"} <= set(rates)
    for k in rates:
        assert torch.equal(out[k], ref[k]), k
    rd = nic.rd_loss(out, x, 0.01)
    rd_pad = nic.rd_loss(ref, torch.nn.functional.pad(x, (0, Wp - W, 0, Hp - H), mode="replicate"), 0.01)
    assert rd["bits_total"] == rd_pad["bits_total"]
    # bpp_total = fl(fl(mean_b fl(bits_y_b / n)) + fl(mean_b fl(bits_z_b / n))) and bits_total = fl(mean_b bits_b): at most
    # five fp32 roundings (2^-24 relative each) separate it from bits_total / n in exact arithmetic; 6 allows for the
    # second-order terms
    want = float(np.float64(rd["bits_total"]) / np.float64(H * W))
    print(f"bpp_total {rd['bpp_total']!r} expected {want!r} rel {abs(rd['bpp_total'] - want) / want:.3e}")
    assert abs(rd["bpp_total"] - want) <= 6 * 2.0 ** -24 * want
    assert rd["bpp_total"] > rd_pad["bpp_total"]          # the same bits over fewer pixels
    # centre alignment and another border, against the same hand-made padding
    top, left = (Hp - H) // 2, (Wp - W) // 2
    out_c = nic.padded_forward(model, x, mode="reflect", align="center")
    with torch.no_grad():
        ref_c = model(torch.nn.functional.pad(x, (left, Wp - W - left, top, Hp - H - top), mode="reflect"), training=False)
    assert out_c["window"] == (top, left, H, W)
    assert torch.equal(out_c["x_hat"], ref_c["x_hat"][:, :, top:top + H, left:left + W])
    assert torch.equal(out_c["logp_y"], ref_c["logp_y"])


def test_padded_forward_scalable(env):
    nic, data, codec, dev = env
    model = nic.ScalableImageCoding(32, 16, 1)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 71)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(dev).eval()
    x = torch.from_numpy(R.make_image(1, 100, 150, 72)).to(dev)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        model(x, training=False)
    out = nic.padded_forward(model, x)
    with torch.no_grad():
        ref = model(torch.nn.functional.pad(x, (0, 42, 0, 28), mode="replicate"), training=False)
    assert out["x_hat"].shape == x.shape and torch.equal(out["x_hat"], ref["x_hat"][:, :, :100, :150])
    assert torch.equal(out["logp_y1"], ref["logp_y1"]) and torch.equal(out["logp_z"], ref["logp_z"])


@pytest.mark.parametrize("kind,K,B,H,W", CASES[:3])
def test_compress_image_round_trip(env, kind, K, B, H, W):
    nic, data, codec, dev = env
    from neural_image_compression_amd import functional as F_
    model = _model(nic, kind, 32, K, 51, dev)
    x = torch.from_numpy(R.make_image(B, H, W, 52)).to(dev)
    cc = codec.ContextCodec(model, z_lo=-32, z_S=65, y_W=24)
    blob = cc.compress_image(x)
    assert isinstance(blob, bytes)
    x_hat = cc.decompress_image(blob)
    want = nic.padded_forward(model, x)
    assert x_hat.shape == x.shape and torch.equal(x_hat, want["x_hat"])
    # a decoder with other window defaults reads them from the header
    assert torch.equal(codec.ContextCodec(model).decompress_image(blob), x_hat)
    # the payload is compress(x_pad)'s streams
    enc = cc.compress(F_.pad_to_multiple(x))
    head, z, ys, crcs = codec.unpack_bitstream(blob)
    assert z == enc["strings"]["z"] and ys == enc["strings"]["y"] and crcs == enc["strings"]["y_crc32"]
    assert (head["B"], head["H"], head["W"], head["top"], head["left"]) == (B, H, W, 0, 0)
    assert (head["M"], head["K"], head["z_lo"], head["z_S"], head["y_W"]) == (32, K, -32, 65, 24)
    assert head["family"] == (1 if kind == "jah" else 2)
    overhead = 8 + 12 * 4 + 8 * B + 4
    assert len(blob) == overhead + len(z) + sum(map(len, ys))
    # bits per ORIGINAL pixel: the padded run's streams plus the container's overhead, over B * H * W
    Hp, Wp = -(-H // 64) * 64, -(-W // 64) * 64
    assert 8.0 * (len(blob) - overhead) / (B * Hp * Wp) == enc["bpp_coded"]
    assert 8.0 * len(blob) / (B * H * W) > enc["bpp_coded"]
    # damage anywhere is refused
    at = len(blob) // 2
    with pytest.raises(codec.CodecError):
        cc.decompress_image(blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:])
    with pytest.raises(codec.CodecError):
        cc.decompress_image(blob[:-1])
    other = _model(nic, kind, 16, K, 51, dev)
    with pytest.raises(codec.CodecError, match="this model"):
        codec.ContextCodec(other).decompress_image(blob)
    # centre alignment round-trips too
    blob_c = cc.compress_image(x, mode="reflect", align="center")
    assert torch.equal(cc.decompress_image(blob_c), nic.padded_forward(model, x, mode="reflect", align="center")["x_hat"])


def test_evaluator_with_pad_mode_averages_per_image_values(env, tmp_path):
    nic, data, codec, dev = env
    from neural_image_compression_amd.evaluator import CompressionEvaluator
    model = _model(nic, "jah", 32, 3, 61, dev)
    batches = [torch.from_numpy(R.make_image(1, h, w, 62 + i)) for i, (h, w) in enumerate([(375, 500), (200, 328), (256, 256)])]
    ev = CompressionEvaluator(model, batches, dev, 0.01, save_dir=str(tmp_path))
    report, ins, recs = ev.evaluate(nic.rd_loss, coded=True, pad_mode="replicate")
    cc = codec.ContextCodec(model)
    per = []
    for b in batches:
        x = b.to(dev)
        out = nic.padded_forward(model, x, mode="replicate")
        rd = nic.rd_loss(out, x, 0.01)
        row = dict(ev.compute_metrics(x, out["x_hat"].clamp(0, 1)))
        row.update({"BPP": rd["bpp_y"], "BPP(y)": rd["bpp_y"], "BPP(z)": rd["bpp_z"], "BPP(total)": rd["bpp_total"],
                    "BPP(coded)": 8.0 * len(cc.compress_image(x)) / (x.shape[2] * x.shape[3])})
        per.append(row)
    assert set(report) == set(per[0])
    for k in report:
        assert report[k] == (per[0][k] + per[1][k] + per[2][k]) / 3, k
    assert len(ins) == len(recs) == 3 and [tuple(t.shape) for t in recs] == [tuple(b.shape[1:]) for b in batches]
    assert report["BPP(coded)"] > report["BPP(total)"] * 0.9
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ev.evaluate(nic.rd_loss, coded=True, pad_mode=None)
