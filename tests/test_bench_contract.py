"""bench.py's output contract: one JSON line with the driver's keys, plus `roofline` and `cpu_baseline` with --full.
CPU: the newest committed line under profiles/ has every key with a sane type, bench.py refuses to run
without a GPU (no CPU fallback).  GPU: a short live run prints a conforming line, and --dump-outputs writes
the same arrays in every run."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTRACT = {"metric": str, "value": (int, float), "unit": str, "n_gpus": int, "steps": int, "warmup": int,
            "ms_per_step": (int, float), "higher_is_better": bool, "scaling": str, "dtype": str, "data": str,
            "config": dict}
ROOFLINE = {"bound": str, "achieved": (int, float), "peak": (int, float), "unit": str, "frac": (int, float)}
CPU_BASELINE = {"value": (int, float), "unit": str, "cores": int, "kind": str, "sample": str}


def check_line(d, want_cpu, full=True):
    for k, t in CONTRACT.items():
        assert k in d and isinstance(d[k], t), k
    assert "vs_baseline" in d and d["vs_baseline"] is None      # BASELINE.md publishes no number for this metric
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["unit"] == "images/s" and d["value"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["config"]["loss"] == d["config"]["loss"] and abs(d["config"]["loss"]) < 1e6, "non-finite loss in a bench line"
    assert abs(d["value"] - d["config"]["global_batch"] / d["ms_per_step"] * 1e3) <= 0.01 * d["value"]
    if not full:
        assert not {"roofline", "kernels", "analysis_hyperprior_fwd", "cpu_baseline"} & set(d), "a plain run measured extras"
        return
    r = d["roofline"]
    for k, t in ROOFLINE.items():
        assert k in r and isinstance(r[k], t), k
    assert r["bound"] in ("hbm", "mfma") and "traffic" in r
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if want_cpu:
        c = d["cpu_baseline"]
        for k, t in CPU_BASELINE.items():
            assert k in c and isinstance(c[k], t), k
        assert c["kind"] in ("reference", "port") and c["cores"] >= 1


def test_committed_bench_line_follows_the_contract():
    lines = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_line.json")))
    assert lines, "no bench line committed under profiles/"
    d = json.loads(open(lines[-1]).read().strip().splitlines()[-1])
    check_line(d, want_cpu=True)
    assert d["n_gpus"] == 1 and d["dtype"] == "f32" and "cfg2" in d["config"]["workload"]
    # the rocprofv3 summary of the same command is committed next to it and names the same kernel
    stats = lines[-1].replace("_bench_line.json", "_kernel_stats_bench_cfg2.csv")
    assert os.path.exists(stats) and d["roofline"]["kernel"] in open(stats).read()


def test_bench_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "no CPU fallback" in (p.stderr + p.stdout)


def test_bench_configs_cover_baseline_json():
    sys.path.insert(0, ROOT)
    import bench
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert len(base["configs"]) == 5
    for k in ("2", "3", "4", "5"):
        assert k in bench.CONFIGS
    kind, M, K, B, H, W, lam = bench.CONFIGS["2"]
    assert (kind, M, K, B, H, W) == ("jah", 192, 1, 32, 256, 256)


def test_dump_arrays_are_float32_seeded_samples_within_the_limit():
    """output_arrays on host tensors: large arrays become the same fixed sample in every call, taken in logical
    order (a channels_last copy gives the same values), small ones stay whole; private result keys are left out."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    model = torch.nn.Linear(1000, 1000)   # (1001000 values: below DUMP_SAMPLE, kept whole)
    model.weight.grad = torch.rand_like(model.weight)
    x_hat = torch.rand(4, 3, 300, 300)
    res = {"loss": torch.tensor(2.5), "psnr_per_image": torch.rand(4), "_buffer": torch.zeros(8)}
    a = bench.output_arrays({"x_hat": x_hat, "training": True}, res, model)
    b = bench.output_arrays({"x_hat": x_hat.contiguous(memory_format=torch.channels_last), "training": True}, res, model)
    assert sorted(a) == ["gradients", "loss", "parameters", "psnr_per_image", "x_hat"]
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    assert a["x_hat"].shape == (bench.DUMP_SAMPLE,) and np.isin(a["x_hat"], x_hat.numpy()).all()
    assert a["loss"] == np.float32(2.5) and a["psnr_per_image"].shape == (4,)
    assert a["gradients"][-1000:].sum() == 0.0   # (the bias has no gradient: zeros)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_live_bench_line():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--full",
                        "--no-cpu-baseline", "--no-analysis-fwd"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    check_line(d, want_cpu=False)
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["2", "3", "2h"])
def test_two_stream_training_step_is_finite_and_repeatable(cfg):
    """The whole two-stream training step (every kernel variant the config dispatches, at full size, beside each
    other) run twice from the same seed: the loss after the steps is finite and bit-identical.  This is the net that
    catches a race between workgroups or wave groups -- one such race passed every parity test and showed up only
    here, as NaNs (config 2h dispatches the 8-wave tile, config 3 the fused bf16 launches and the K split)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    losses = []
    for _ in range(2):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", cfg, "--steps", "6", "--warmup", "2",
                            "--no-cpu-baseline", "--no-analysis-fwd", "--no-profile-events"], capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
        losses.append(json.loads(p.stdout.strip().splitlines()[-1])["config"]["loss"])
    assert losses[0] == losses[0] and abs(losses[0]) < 1e6, losses
    assert losses[0] == losses[1], losses


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    """A plain run (no --full) prints the headline line and nothing else; two runs with the same arguments write
    bit-identical --dump-outputs (seeded inputs, deterministic kernels), float32, at most 64 MB."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        check_line(line, want_cpu=False, full=False)
        assert line["steps"] == 3 and line["warmup"] == 1
        arrays = {f.name[:-4]: np.load(f) for f in d.iterdir()}
        assert {"x_hat", "y_in", "logp_y", "loss", "parameters", "gradients"} <= set(arrays), sorted(arrays)
        assert all(a.dtype == np.float32 for a in arrays.values())
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
        assert abs(float(arrays["loss"]) - line["config"]["loss"]) <= 1e-5 * abs(line["config"]["loss"])
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
