"""parallel.GradientAllReducer against the plain step in every model mode, on one MI355X (tests/dp_modes_worker.py):

  S1  one rank, reducer forced (gloo without the overlap, RCCL with it): gradients, and parameters after the optimizer
      step, bit for bit those of the plain run -- bf16 storage, the 3x3 residual model, the checkerboard context, rate
      levels, the MS-SSIM loss and ScalableImageCoding included;
  S2  two gloo ranks on cuda:0: every rank holds exactly (g0 + g1) * 0.5 of the plain shard gradients (for GDN
      parameters below their bound: of the gradients in front of the one-sided pass-through, which the ranks apply
      to the mean -- see the worker), beside the whole-batch band of tests/dp_worker.py; Trainer(distributed=True)
      against a hand loop.

As in tests/test_00_dp_two_rank_gpu.py the children are started before THIS process initialises the GPU (the file name
sorts in front of every test that does); started later the tests skip.  A child that ends by signal, abort or timeout
stops the file: the tests behind it start no further GPU program and fail naming the first failure."""
import os
import re
import socket
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dp_modes_worker.py")
# Measured on the MI355X inside the whole suite: the one-rank children take 8.7 s (gloo, 9 modes) and 8.9 s (RCCL, 7
# modes), the two-rank child 10-15 s; the existing two-rank test (tests/dp_worker.py) takes 5.1 s there.  A mode costs
# 0.4-1 s (the first of a child 2.7 s); process start, the imports and the first launch of every kernel are the rest,
# twice over for two ranks.  The limit is ten times the slowest: room for a cold file cache and a busy host, well
# short of the ten minutes a hang would otherwise take.
CHILD_LIMIT = 150
_STOPPED = []   # why no further GPU program is started from this file (the first child that died, if any)


def _need_fresh_gpu():
    if torch.cuda.device_count() == 0:
        pytest.skip("needs an MI355X")
    if torch.cuda.is_initialized():
        pytest.skip("this process already initialised the GPU: the rank programs must be started before that "
                    "(run `pytest tests -m gpu`, where this file comes first, or this file alone)")
    if _STOPPED:
        pytest.fail(f"not started: {_STOPPED[0]}")


def _child(name, cmd, timeout, ok_line):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GPU_MAX_HW_QUEUES="8", OMP_NUM_THREADS="2")
    t0 = time.time()
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _STOPPED.append(f"the {name} child did not end within {timeout} s")
        pytest.fail(_STOPPED[0] + "\n" + (e.stdout or b"").decode(errors="replace")[-4000:])
    text = r.stdout.decode(errors="replace")
    print(f"\n[{name}] child wall time {time.time() - t0:.1f} s")
    print("\n".join(ln for ln in text.splitlines() if ln.startswith(("MODE ", "TRAINER ", "DP_MODES_OK"))))
    # (a rank that torch.distributed.run lost to a signal shows as a negative exit code in the launcher's report)
    died = r.returncode < 0 or r.returncode in (124, 134, 137, 139) or re.search(r"exitcode\s*:\s*-\d+", text)
    if died:
        _STOPPED.append(f"the {name} child ended by signal or abort (exit code {r.returncode})")
        pytest.fail(_STOPPED[0] + "\n" + text[-4000:])
    assert r.returncode == 0 and ok_line in text, text[-4000:]
    return text


@pytest.mark.gpu
def test_one_rank_gloo_reducer_is_the_plain_step_in_every_mode(tmp_path):
    _need_fresh_gpu()
    text = _child("one rank, gloo", [sys.executable, WORKER, "--backend", "gloo", "--store", str(tmp_path / "store")],
                  CHILD_LIMIT, "DP_MODES_OK backend=gloo world=1 modes=9")
    assert len(re.findall(r"^MODE \w+ ", text, re.M)) == 9


@pytest.mark.gpu
def test_one_rank_rccl_reducer_with_overlap_is_the_plain_step_in_every_mode(tmp_path):
    _need_fresh_gpu()
    text = _child("one rank, RCCL", [sys.executable, WORKER, "--backend", "nccl", "--store", str(tmp_path / "store")],
                  CHILD_LIMIT, "DP_MODES_OK backend=nccl world=1 modes=7")
    assert len(re.findall(r"^MODE \w+ ", text, re.M)) == 7


@pytest.mark.gpu
def test_two_gloo_ranks_hold_the_exact_mean_of_the_shard_gradients():
    _need_fresh_gpu()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), WORKER]
    text = _child("two ranks, gloo", cmd, CHILD_LIMIT, "DP_MODES_OK backend=gloo world=2 modes=3")
    for mode in ("a", "c", "e"):
        assert len(re.findall(rf"^MODE {mode} .* S2 gloo world=2 rank [01]:", text, re.M)) == 2, text[-4000:]
    assert len(re.findall(r"^TRAINER rank [01]:", text, re.M)) == 2, text[-4000:]
