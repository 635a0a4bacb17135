"""Gradient clipping without a GPU: the numpy restatement (clip_ref.py) against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam, the argument validation of lic_grad_norm_partial / lic_grad_norm_finish / lic_adam_run_scaled, and
the torch path of FusedAdam / Trainer on CPU parameters."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import clip_ref as R

LR, STEPS = 3e-3, 4


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restatement_matches_torch_clip_and_adam(wd):
    g = torch.Generator().manual_seed(3)
    shapes = [(5,), (4097,), (33, 7), (1,)]
    pt = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    opt = torch.optim.Adam(pt, lr=LR, weight_decay=wd)
    pn = [p.detach().numpy().copy() for p in pt]
    mn, vn = [np.zeros_like(p) for p in pn], [np.zeros_like(p) for p in pn]
    grads0 = [torch.randn(s, generator=g) for s in shapes]
    max_norm = 0.5 * float(torch.linalg.vector_norm(torch.cat([x.flatten() for x in grads0])))
    clipped = 0
    for step in range(1, STEPS + 1):
        grads = grads0 if step == 1 else [torch.randn(s, generator=g) * (0.2 if step == 3 else 1.0) for s in shapes]
        for p, x in zip(pt, grads):
            p.grad = x.clone()
        norm_t = torch.nn.utils.clip_grad_norm_(pt, max_norm)
        opt.step()
        norm, coef, skipped = R.clipped_step(pn, [x.numpy() for x in grads], mn, vn, step, LR, max_norm=max_norm,
                                             weight_decay=wd)
        assert not skipped
        assert abs(float(norm) - float(norm_t)) <= 4 * np.spacing(np.float32(norm_t))   # (torch sums in fp32)
        clipped += bool(coef < 1.0)
    assert 1 <= clipped < STEPS     # (both branches of the clamp were taken)
    for p, q in zip(pt, pn):
        # test_gpu_optim.py's bound between two Adam implementations: STEPS updates of ~lr each
        assert float(np.abs(p.detach().numpy() - q).max()) <= 1e-5 * (STEPS * LR) + 1e-6 * float(p.detach().abs().max())


def test_norm_and_coefficient_of_the_restatement():
    g = [np.array([3.0, -4.0], np.float32), np.array([12.0], np.float32)]
    assert R.grad_norm(g) == np.float32(13.0)
    assert R.coefficient(np.float32(13.0), math.inf) == np.float32(1.0)
    assert R.coefficient(np.float32(13.0), 26.0) == np.float32(1.0)
    assert R.coefficient(np.float32(13.0), 6.5) == np.float32(6.5) / (np.float32(13.0) + np.float32(1e-6))
    assert np.isnan(R.coefficient(np.float32(np.nan), 1.0)) and R.coefficient(np.float32(np.inf), 1.0) == 0.0
    p, m, v = (np.ones(2, np.float32) for _ in range(3))
    norm, _, skipped = R.clipped_step([p], [np.array([np.inf, 1.0], np.float32)], [m], [v], 1, LR, skip_nonfinite=True)
    assert skipped and np.isinf(norm) and (p == 1).all() and (m == 1).all() and (v == 1).all()


def test_argument_validation_without_gpu(lib):
    L = lib.load()
    INVALID, UNSUPPORTED = -1, -2
    buf = ctypes.create_string_buffer(64)          # stands for device memory: never dereferenced by a refused call
    dev = ctypes.c_void_p(ctypes.addressof(buf))
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    null_entry = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    many = (ctypes.c_void_p * 449)()

    assert L.lic_grad_norm_partial(None, 1, 1, one, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 1, 1, None, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 1, 1, one, None, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 0, 1, one, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 1, 0, one, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 1, 1 << 31, one, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 2, 2, null_entry, dev, None) == INVALID
    assert L.lic_grad_norm_partial(dev, 449, 449, many, dev, None) == UNSUPPORTED

    assert L.lic_grad_norm_finish(None, 1, 1.0, 0, dev, None) == INVALID
    assert L.lic_grad_norm_finish(dev, 1, 1.0, 0, None, None) == INVALID
    assert L.lic_grad_norm_finish(dev, 0, 1.0, 0, dev, None) == INVALID
    assert L.lic_grad_norm_finish(dev, -3, 1.0, 0, dev, None) == INVALID
    assert L.lic_grad_norm_finish(dev, 1, -1.0, 0, dev, None) == INVALID
    assert L.lic_grad_norm_finish(dev, 1, math.nan, 0, dev, None) == INVALID

    adam = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001)
    assert L.lic_adam_run_scaled(None, 1, 1, one, *adam, dev, 0, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 1, 1, None, *adam, dev, 0, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 1, 1, one, *adam, None, 0, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 0, 1, one, *adam, dev, 0, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 1, 0, one, *adam, dev, 0, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 2, 2, null_entry, *adam, dev, 1, None) == INVALID
    assert L.lic_adam_run_scaled(dev, 1, 1, one, *adam[:5], 0.0, 0.001, dev, 0, None) == INVALID   # bias correction
    assert L.lic_adam_run_scaled(dev, 449, 449, many, *adam, dev, 0, None) == UNSUPPORTED
    assert L.lic_version() == 4      # the ABI only grew


class _Rows:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))

    def close(self):
        pass


def _toy(seed=4):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def _toy_loss(scale):
    def rd_loss(out, imgs, lam):
        return {"loss": scale * (out ** 2).sum() * lam, "lam": float(lam)}
    return rd_loss


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_clips_on_the_torch_path(fused):
    """CPU parameters: a plain torch.optim.Adam gets clip_grad_norm_ in front of its step; a FusedAdam is given the
    options and, the kernel not covering CPU tensors, does the same through its fallback"""
    from neural_image_compression_amd.optim import FusedAdam
    from neural_image_compression_amd.trainer import Trainer
    x = torch.randn(8, 6, generator=torch.Generator().manual_seed(5))
    ma, mb = _toy(), _toy()
    # by hand
    oa = torch.optim.Adam(ma.parameters(), lr=1e-2)
    oa.zero_grad()
    (_toy_loss(50.0)(ma(x), x, 0.5)["loss"]).backward()
    ref_norm = torch.nn.utils.clip_grad_norm_(ma.parameters(), 0.25)
    assert float(ref_norm) > 0.25        # (clipping is active)
    oa.step()
    # the trainer
    ob = (FusedAdam if fused else torch.optim.Adam)(mb.parameters(), lr=1e-2)
    log = _Rows()
    tr = Trainer(mb, ob, [x], rd_loss=_toy_loss(50.0), lambda_val=0.5, max_steps=1, checkpoint_path=None, device="cpu",
                 distributed=False, writer=log, log_interval=1, img_interval=1, val_interval=1, clip_max_norm=0.25)
    tr.log_statistics = False
    tr.train()
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
    assert [(t, v) for t, v, s in log.rows if t == "train/grad_norm"] == [("train/grad_norm", float(ref_norm))]
    assert not [r for r in log.rows if r[0] == "train/skipped_steps"]     # (only logged when skipping is on)
    if fused:
        assert ob.max_grad_norm == 0.25 and ob.fused_steps == 0 and float(ob.grad_norm()) == float(ref_norm)
        assert "max_grad_norm" not in ob.state_dict()["param_groups"][0]


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_skips_a_nonfinite_step_on_the_torch_path(fused):
    from neural_image_compression_amd.optim import FusedAdam
    from neural_image_compression_amd.trainer import Trainer
    x = torch.randn(8, 6, generator=torch.Generator().manual_seed(6))
    m = _toy()
    before = [p.detach().clone() for p in m.parameters()]
    opt = (FusedAdam if fused else torch.optim.Adam)(m.parameters(), lr=1e-2)
    log = _Rows()
    tr = Trainer(m, opt, [x], rd_loss=_toy_loss(float("inf")), lambda_val=0.5, max_steps=1, checkpoint_path=None,
                 device="cpu", distributed=False, writer=log, log_interval=1, img_interval=1, val_interval=1,
                 skip_nonfinite=True)
    tr.log_statistics = False
    tr.train()
    for p, q in zip(m.parameters(), before):
        assert torch.equal(p.detach(), q)
    assert ("train/skipped_steps", 1.0, 0) in log.rows
    assert not math.isfinite([v for t, v, s in log.rows if t == "train/grad_norm"][0])
    if fused:
        assert opt.skipped_steps() == 1


def test_fused_adam_without_the_options_has_no_norm():
    from neural_image_compression_amd.optim import FusedAdam
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and opt.skipped_steps() == 0
    with pytest.raises(RuntimeError, match="clipping is off"):
        opt.grad_norm()
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=-1.0)
