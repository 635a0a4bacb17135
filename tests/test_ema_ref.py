"""The moving average without a GPU: the numpy restatement (ema_ref.py) against its own definition in float64, the
warm-up schedule, the cases that must be exact, and the torch path of FusedAdam(ema_decay=...), the Trainer's checkpoint
and the evaluator's loader on CPU parameters."""
import math

import numpy as np
import pytest
import torch

import ema_ref as E

F = np.float32


def test_warmup_schedule_and_its_crossover_with_the_decay():
    d = 0.999
    for t, want in ((1, 2.0 / 11.0), (9, 10.0 / 19.0), (10, 11.0 / 20.0), (10 ** 6, d)):
        assert E.ema_weight(t, d) == 1.0 - min(d, want), t
        assert E.ema_weight(t, d, warmup=False) == 1.0 - d
    # (1 + t) / (10 + t) = 0.999 at t = 8990 (8991 / 9000): the warm-up rules below it, the decay from there on
    assert (1.0 + 8989) / (10.0 + 8989) < d <= (1.0 + 8990) / (10.0 + 8990)
    assert E.ema_weight(8989, d) == 1.0 - 8990.0 / 8999.0 and E.ema_weight(8989, d) > 1.0 - d
    assert E.ema_weight(8990, d) == 1.0 - d and E.ema_weight(8991, d) == 1.0 - d
    assert E.ema_weight(1, 0.0) == 1.0 and E.ema_weight(10 ** 6, 0.0) == 1.0      # d = 0 wins the min at once
    ws = [E.ema_weight(t, d) for t in range(1, 10000)]
    assert all(a >= b for a, b in zip(ws, ws[1:]))                                 # the weight only falls


@pytest.mark.parametrize("w", [1.0 - 0.999, 9.0 / 19.0, 0.5, 1.0 - 2.0 / 11.0])
def test_update_is_within_one_and_a_half_ulp_of_float64(w):
    r = np.random.RandomState(5)
    e = r.randn(20000).astype(np.float32)
    p = (e + r.randn(20000).astype(np.float32) * np.float32(1e-2)).astype(np.float32)
    got = E.ema_update(e, p, w)
    assert got.dtype == np.float32
    wf = float(F(w))
    exact = e.astype(np.float64) + wf * (p.astype(np.float64) - e.astype(np.float64))
    # three roundings of half an ulp each: of p - e, of its product with w (the error of p - e comes through times
    # w <= 1), of the sum.  With `ulp` the spacing of fp32 at the largest of the three rounded values, that is 1.5 ulp
    diff = (p - e).astype(np.float32)
    largest = np.maximum(np.maximum(np.abs(diff), np.abs(F(w) * diff)), np.abs(got))
    ulp = np.spacing(largest.astype(np.float32)).astype(np.float64)
    assert float((np.abs(got.astype(np.float64) - exact) / ulp).max()) <= 1.5


def test_decay_zero_gives_the_parameter_exactly():
    """w = 1 with data as it occurs (the parameter a small step away from its average, so p - e is exact by
    Sterbenz' lemma): e + 1 * (p - e) is p, bit for bit"""
    r = np.random.RandomState(6)
    e = (r.rand(5000).astype(np.float32) + F(1.0)).astype(np.float32)
    p = (e * F(1.0 + 2.0 ** -10)).astype(np.float32)
    assert E.ema_weight(7, 0.0) == 1.0
    assert np.array_equal(E.ema_update(e, p, E.ema_weight(7, 0.0)).view(np.int32), p.view(np.int32))
    # and where the state starts: e = p gives p whatever the weight
    assert np.array_equal(E.ema_update(p, p, 0.37).view(np.int32), p.view(np.int32))


def test_weight_zero_leaves_the_average_bit_for_bit():
    r = np.random.RandomState(7)
    e = r.randn(5000).astype(np.float32)
    e[:3] = [0.0, -0.0, np.float32(1e-42)]             # zeros of both signs and a subnormal
    p = r.randn(5000).astype(np.float32)
    got = E.ema_update(e, p, 0.0)
    same = got.view(np.int32) == e.view(np.int32)
    assert same[2:].all() and got[0] == 0.0 and got[1] == 0.0    # (-0 + 0 is +0 in IEEE: the value, not the sign)


def test_skipped_step_leaves_the_average_bit_for_bit():
    r = np.random.RandomState(8)
    shapes = (5, 4097)
    ps = [r.randn(n).astype(np.float32) for n in shapes]
    ms, vs = [np.zeros(n, np.float32) for n in shapes], [np.zeros(n, np.float32) for n in shapes]
    es = [p.copy() for p in ps]
    gs = [r.randn(n).astype(np.float32) for n in shapes]
    assert E.ema_step(ps, gs, ms, vs, es, 1, 1e-2, 0.999, max_norm=1.0, skip_nonfinite=True)[2] is False
    assert not np.array_equal(es[1], ps[1]) and not np.array_equal(es[1], es[1] * 0)
    before = [[a.copy() for a in group] for group in (ps, ms, vs, es)]
    gs[1][-1] = np.inf
    norm, coef, skipped = E.ema_step(ps, gs, ms, vs, es, 2, 1e-2, 0.999, max_norm=1.0, skip_nonfinite=True)
    assert skipped and not math.isfinite(float(norm))
    for group, kept in zip((ps, ms, vs, es), before):
        for a, b in zip(group, kept):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_step_moves_the_average_towards_the_new_parameter():
    r = np.random.RandomState(9)
    p = [r.randn(33).astype(np.float32)]
    m, v, e = [np.zeros(33, np.float32)], [np.zeros(33, np.float32)], [p[0].copy()]
    p0 = p[0].copy()
    E.ema_step(p, [r.randn(33).astype(np.float32)], m, v, e, 1, 1e-2, 0.999)
    want = E.ema_update(p0, p[0], 1.0 - 2.0 / 11.0)           # step 1 of the warm-up
    assert np.array_equal(e[0].view(np.int32), want.view(np.int32))


# ---- the torch path of FusedAdam on CPU parameters: the same three roundings ----------------------------------------
def _cpu_run(steps, **kw):
    import neural_image_compression_amd as nic
    g = torch.Generator().manual_seed(4)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 4097, 1)]
    opt = nic.FusedAdam(ps, lr=1e-2, **kw)
    trail = []
    for step in range(1, steps + 1):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        before = [opt.state[p]["ema"].numpy().copy() if "ema" in opt.state.get(p, {}) else p.detach().numpy().copy()
                  for p in ps]
        opt.step()
        trail.append((step, before, [p.detach().numpy().copy() for p in ps]))
    return ps, opt, trail


@pytest.mark.parametrize("warmup", [True, False])
def test_torch_path_applies_the_restatement_bit_for_bit(warmup):
    ps, opt, trail = _cpu_run(3, ema_decay=0.99, ema_warmup=warmup)
    assert opt.fused_steps == 0
    # replay: every step's average from the one before it and the parameter the step left
    es = [t.copy() for t in trail[0][1]]
    for step, before, after in trail:
        for i in range(len(es)):
            assert np.array_equal(es[i].view(np.int32), before[i].view(np.int32)), (step, i)
            es[i] = E.ema_update(es[i], after[i], E.ema_weight(step, 0.99, warmup))
    for p, e in zip(ps, es):
        assert np.array_equal(opt.state[p]["ema"].numpy().view(np.int32), e.view(np.int32))
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}


def test_arguments_states_and_swapping_on_the_torch_path():
    import neural_image_compression_amd as nic
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            nic.FusedAdam([torch.nn.Parameter(torch.zeros(3))], ema_decay=bad)
    ps, plain, _ = _cpu_run(2)
    assert set(plain.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}     # torch's, key for key
    assert plain.ema_decay is None
    with pytest.raises(RuntimeError, match="moving average is off"):
        plain.swap_ema()
    ps, opt, _ = _cpu_run(2, ema_decay=0.9)
    live = [p.detach().clone() for p in ps]
    avg = [opt.state[p]["ema"].clone() for p in ps]
    versions = [p._version for p in ps]
    assert not opt.swapped and not any(torch.equal(a, b) for a, b in zip(live, avg))
    with opt.ema_weights():
        assert opt.swapped
        assert all(torch.equal(p.detach(), a) for p, a in zip(ps, avg))
        assert all(torch.equal(opt.state[p]["ema"], b) for p, b in zip(ps, live))
        assert all(p._version > v for p, v in zip(ps, versions))        # whatever is keyed on versions sees the swap
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
    assert not opt.swapped
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, live))
    assert all(torch.equal(opt.state[p]["ema"], a) for p, a in zip(ps, avg))
    # the state dict carries the averages; a torch-Adam state dict (none) starts them from the parameters
    sd = opt.state_dict()
    ps2, opt2, _ = _cpu_run(0, ema_decay=0.9)
    opt2.load_state_dict(sd)
    assert all(torch.equal(opt2.state[q]["ema"], a) for q, a in zip(ps2, avg))
    ps3, opt3, _ = _cpu_run(0, ema_decay=0.9)
    opt3.load_state_dict(plain.state_dict())
    assert "ema" not in opt3.state[ps3[0]]
    start = [q.detach().numpy().copy() for q in ps3]
    for q in ps3:
        q.grad = torch.ones_like(q)
    opt3.step()
    for q, p0 in zip(ps3, start):
        want = E.ema_update(p0, q.detach().numpy(), E.ema_weight(3, 0.9))       # the loaded count was 2
        assert np.array_equal(opt3.state[q]["ema"].numpy().view(np.int32), want.view(np.int32))


def test_ema_state_dict_names_the_averages_and_leaves_the_model():
    import neural_image_compression_amd as nic
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    opt = nic.FusedAdam(model.parameters(), lr=1e-2, ema_decay=0.5, ema_warmup=False)
    for _ in range(2):
        opt.zero_grad()
        model(torch.randn(8, 3)).square().mean().backward()
        opt.step()
    live = {k: v.clone() for k, v in model.state_dict().items()}
    sd = opt.ema_state_dict(model)
    assert list(sd) == list(live)
    for k, v in model.state_dict().items():
        assert torch.equal(v, live[k])                                           # the model is as it was
    for name, p in model.named_parameters():
        assert torch.equal(sd[name], opt.state[p]["ema"]) and not torch.equal(sd[name], live[name])
    assert torch.equal(sd["1.running_mean"], live["1.running_mean"])              # buffers as they are
    with opt.ema_weights():
        inside = opt.ema_state_dict(model)
    assert all(torch.equal(inside[k], sd[k]) for k in sd)
    torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4)).load_state_dict(sd)


def test_trainer_checkpoint_and_evaluator_loader_on_the_torch_path(tmp_path):
    """CPU model, torch path: the checkpoint holds the averaged model next to the reference's keys, the evaluator's
    loader prefers it, validation under ema_eval runs on it and leaves the trained weights in place"""
    import neural_image_compression_amd as nic
    from neural_image_compression_amd.evaluator import load_checkpoint_weights
    from neural_image_compression_amd.trainer import Trainer

    def loss_fn(out, x, lam, **kw):
        mse = (out - x).square().mean()
        return {"loss": mse, "bpp_total": 0.0, "psnr": float(mse.detach())}

    class Log:
        def add_scalar(self, *a):
            pass

        def close(self):
            pass

    torch.manual_seed(1)
    build = lambda: torch.nn.Sequential(torch.nn.Linear(4, 4))     # noqa: E731
    model = build()
    _forward = model.forward
    model.forward = lambda x, training=True: _forward(x)
    opt = nic.FusedAdam(model.parameters(), lr=1e-1, ema_decay=0.5, ema_warmup=False)
    batches = [torch.randn(8, 4) for _ in range(2)]
    path = str(tmp_path / "c.pth")
    tr = Trainer(model, opt, batches, val_loader=batches[:1], rd_loss=loss_fn, max_steps=2, checkpoint_path=path,
                 device="cpu", writer=Log(), log_interval=100, img_interval=100, val_interval=100, ema_eval=True)
    tr.log_statistics = False
    tr.train()
    live = {k: v.clone() for k, v in model.state_dict().items()}
    on_average = tr.validate()
    assert not opt.swapped and all(torch.equal(v, live[k]) for k, v in model.state_dict().items())
    tr.ema_eval = False
    assert tr.validate() != on_average
    state = torch.load(path)
    assert set(state) == {"model", "optimizer", "step", "scheduler", "ema_state_dict"}
    shipped, plain = build(), build()
    assert load_checkpoint_weights(shipped, path) == "ema_state_dict"
    assert load_checkpoint_weights(plain, state, ema=False) == "model"
    for (name, p), q, r in zip(model.named_parameters(), shipped.parameters(), plain.parameters()):
        assert torch.equal(q.detach(), opt.state[p]["ema"]) and torch.equal(r.detach(), p.detach()), name
    with torch.no_grad():
        assert float(loss_fn(shipped(batches[0]), batches[0], 0.0)["loss"]) == on_average
    del state["ema_state_dict"]                                     # a checkpoint of before: the trained weights
    assert load_checkpoint_weights(build(), state) == "model"
    # a Trainer whose optimizer does not average writes the reference's four keys and nothing else
    other = build()
    tr2 = Trainer(other, nic.FusedAdam(other.parameters(), lr=1e-1), batches, rd_loss=loss_fn, max_steps=1,
                  checkpoint_path=str(tmp_path / "d.pth"), device="cpu", writer=Log(), log_interval=100, img_interval=100,
                  val_interval=100, ema_eval=True)
    tr2.log_statistics = False
    tr2.train()
    assert set(torch.load(str(tmp_path / "d.pth"))) == {"model", "optimizer", "step", "scheduler"}
