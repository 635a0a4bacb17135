"""VisionCompressionEvaluator on an MI355X: every key of its report against the value computed directly from the model,
vision_rd_loss, compute_metrics and ScalableCodec.compress on a two-batch loader, and the result file's format."""
import numpy as np
import pytest
import torch

import golden_recipe as R

pytestmark = pytest.mark.gpu

LAMBDA, GAMMA = 0.01, 0.0


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as G
    G.build_codec()
    import neural_image_compression_amd as nic
    dev = torch.device("cuda:0")
    model = nic.ScalableImageCoding(32, 20, 1)
    st = R.make_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 77)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(dev).eval()
    # 192 x 192: MS-SSIM, one of the five metrics, needs sides above 160 (four 2x downsamplings of an 11-tap window),
    # and the model multiples of 64
    loader = [torch.from_numpy(R.make_image(1, 192, 192, seed=s)) for s in (5, 6)]
    return nic, model, loader, dev


def test_report_keys_equal_the_directly_computed_values(setup, tmp_path):
    nic, model, loader, dev = setup
    from neural_image_compression_amd.codec import ScalableCodec
    from neural_image_compression_amd.evaluator import VisionCompressionEvaluator
    from compat.Evaluator import VisionCompressionEvaluator as exported
    assert exported is VisionCompressionEvaluator
    ev = VisionCompressionEvaluator(model, loader, dev, LAMBDA, GAMMA, save_dir=str(tmp_path))
    report, inputs, recons = ev.evaluate(nic.vision_rd_loss, coded=True)
    plain, _, _ = ev.evaluate(nic.vision_rd_loss)
    assert "BPP(coded)" not in plain and "BPP(coded base)" not in plain
    assert {k: v for k, v in report.items() if not k.startswith("BPP(coded")} == plain

    want, codec = {}, ScalableCodec(model)
    with torch.no_grad():
        for batch in loader:
            batch = batch.to(dev)
            out = model(batch, training=False)
            rd = nic.vision_rd_loss(out, batch, LAMBDA, GAMMA)
            r = codec.compress(batch)
            row = dict(ev.compute_metrics(batch, out["x_hat"].clamp(0, 1)))
            row.update({"BPP": rd["bpp_y"], "BPP(y)": rd["bpp_y"], "BPP(y1)": rd["bpp_y1"], "BPP(y2)": rd["bpp_y2"],
                        "BPP(z)": rd["bpp_z"], "BPP(total)": rd["bpp_total"], "BPP(coded)": r["bpp_coded"],
                        "BPP(coded base)": r["bpp_coded_base"]})
            for k, v in row.items():
                want.setdefault(k, []).append(float(v))
    assert list(report) == ["MSE(255)", "PSNR(RGB)", "MS-SSIM(RGB)", "PSNR(Y)", "MS-SSIM(Y)", "BPP", "BPP(y)", "BPP(y1)",
                            "BPP(y2)", "BPP(z)", "BPP(total)", "BPP(coded)", "BPP(coded base)"]
    for k, vals in want.items():
        assert report[k] == sum(vals) / len(vals), k             # the same arithmetic mean of the same per-batch values
    assert report["BPP"] == report["BPP(y)"] != report["BPP(total)"]
    assert 0 < report["BPP(coded base)"] < report["BPP(coded)"]
    assert len(inputs) == len(recons) == 2 and tuple(recons[0].shape) == (3, 192, 192)

    path = ev.save_results(report, 1234, caption="vision")
    lines = open(path).read().splitlines()
    assert path.endswith(f"eval_results_{LAMBDA}_lambda_vision.txt")
    assert lines[:2] == [f"Lambda: {LAMBDA}", "Trained for: 1234 steps"]
    assert lines[2:] == [f"{k}: {v:.6f}" for k, v in report.items()]
