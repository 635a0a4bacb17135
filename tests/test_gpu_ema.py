"""The moving average of the weights inside FusedAdam's launch (lic_adam_run_ema), its exchange with the live weights
(lic_swap_run) and what hangs on them, on the GPU: the average bit for bit against ema_ref.py with everything else
bit for bit what a FusedAdam without it computes, the guard, the torch path, the swap and the caches it must reach,
the state dict, and the Trainer.

Shapes: lengths around the 4096-element block of the lic_adam_plan partition (1, 3, 4095, 4096, 4097, 8193,
3 * 4096 + 5: one and several blocks, scalar tails of 1 to 3 elements behind the 16-byte stores), a parameter that is
not 16-byte aligned (element-wise path), an average that is not (element-wise average inside the 16-byte path), a
tensor without an average, 449 tensors (one more than a launch takes)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ema_ref as E
from guarded import Guarded

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4095, 4096, 4097, 8193, 3 * 4096 + 5)
UNALIGNED_P, UNALIGNED_E = 4, 5      # the parameter of 4097 / the average of 8193 elements: 4 bytes off the 16-byte grid
LR, DECAY = 1e-2, 0.999


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _off_grid(values):
    big = torch.zeros(values.numel() + 1, dtype=values.dtype, device=values.device)
    big[1:] = values
    out = big[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _params(dev, seed, lengths=LENGTHS, unaligned=UNALIGNED_P):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for i, n in enumerate(lengths):
        v = torch.randn(n, generator=g).to(dev)
        out.append(torch.nn.Parameter(_off_grid(v) if i == unaligned else v))
    return out


def _grads(seed, lengths=LENGTHS, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in lengths]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.to(p.device).clone()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _guarded_averages(opt, params):
    """the optimizer's state with every average inside NaN-patterned guard bands (guarded.py), one of them 4 bytes off
    the 16-byte grid: the state torch's _init_group would create, entered by hand so that the first step already
    writes into the guarded buffers"""
    guards = []
    for i, p in enumerate(params):
        g = Guarded(1, p.numel(), p.device, shift=1 if i == UNALIGNED_E else 0)
        g.t.copy_(p.detach().view(1, -1))
        e = g.t[0]
        assert e.is_contiguous() and e.data_ptr() % 16 == (4 if i == UNALIGNED_E else 0)
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p),
                        "ema": e}
        guards.append(g)
    return guards


# ---- 1. arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 0.75])
@pytest.mark.parametrize("warmup", [True, False])
def test_average_is_the_restatement_and_changes_nothing_else(clip, warmup):
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    pa, pb = _params(dev, 3), _params(dev, 3)
    kw = {} if clip is None else {"max_grad_norm": clip, "skip_nonfinite": True}
    oa = nic.FusedAdam(pa, lr=LR, weight_decay=0.01, ema_decay=DECAY, ema_warmup=warmup, **kw)
    ob = nic.FusedAdam(pb, lr=LR, weight_decay=0.01, **kw)
    guards = _guarded_averages(oa, pa)
    for step in (1, 2, 3):
        grads = _grads(40 + step, scale=1e-3 if step == 2 else 1.0)
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        before = [oa.state[p]["ema"].cpu().numpy().copy() for p in pa]
        oa.step()
        ob.step()
        w = E.ema_weight(step, DECAY, warmup)
        for i, (a, b) in enumerate(zip(pa, pb)):
            want = E.ema_update(before[i], a.detach().cpu().numpy(), w)
            got = oa.state[a]["ema"].cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (step, i)
            assert not np.array_equal(got, before[i]), (step, i)      # (it moved)
            assert _same_bits(a, b), (step, i)
            for k in ("exp_avg", "exp_avg_sq"):
                assert _same_bits(oa.state[a][k], ob.state[b][k]), (step, i, k)
    assert oa.fused_steps == ob.fused_steps == 3 and oa._fast is not None      # (the third step: the cached plan)
    if clip is not None:
        assert oa.skipped_steps() == 0 and _same_bits(oa.grad_norm(), ob.grad_norm())
    for i, g in enumerate(guards):
        g.check(f"average {i}")
        assert g.unwritten() == 0


@pytest.mark.parametrize("clip", [False, True])
def test_raw_entry_with_a_tensor_that_has_no_average(clip):
    """lic_adam_run_ema driven directly: entry 2 of ema_device is NULL -- that tensor is updated as lic_adam_run /
    lic_adam_run_scaled update it and nothing else happens; the others get their averages"""
    dev = _need_gpu()
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()
    n, hole = len(LENGTHS), 2
    sets = []
    for _ in range(2):
        ps = [p.detach() for p in _params(dev, 5)]
        sets.append((ps, [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]))
    tables = []
    for ps, ms, vs in sets:
        arr = (L.AdamJob * n)()
        for j, p, m, v in zip(arr, ps, ms, vs):
            j.p, j.m, j.v, j.n = p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        blocks = lib.lic_adam_plan(arr, n)
        assert blocks == sum((x + 4095) // 4096 for x in LENGTHS)
        tables.append(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev))
    guards = [Guarded.holding(p.view(1, -1), dev, shift=1 if i == UNALIGNED_E else 0) for i, p in enumerate(sets[0][0])]
    etab = torch.tensor([0 if i == hole else g.ptr() for i, g in enumerate(guards)], dtype=torch.int64).to(dev)
    state = torch.zeros(4, dtype=torch.float32, device=dev)
    state[1] = 0.625                                       # (a coefficient as lic_grad_norm_finish leaves it)
    clip_ptr = C.c_void_p(state.data_ptr()) if clip else None
    for step in (1, 2, 3):
        grads = [g.to(dev) for g in _grads(60 + step)]
        gptrs = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
        before = [g.cpu().numpy().reshape(-1).copy() for g in guards]
        hyper = (LR, 0.9, 0.999, 1e-8, 0.0, 1.0 - 0.9 ** step, 1.0 - 0.999 ** step)
        w = E.ema_weight(step, DECAY)
        L.check(lib.lic_adam_run_ema(C.c_void_p(tables[0].data_ptr()), n, blocks, gptrs, *hyper,
                                     C.c_void_p(etab.data_ptr()), w, clip_ptr, 0, F_._stream()), "lic_adam_run_ema")
        if clip:
            L.check(lib.lic_adam_run_scaled(C.c_void_p(tables[1].data_ptr()), n, blocks, gptrs, *hyper, clip_ptr, 0,
                                            F_._stream()), "lic_adam_run_scaled")
        else:
            L.check(lib.lic_adam_run(C.c_void_p(tables[1].data_ptr()), n, blocks, gptrs, *hyper, F_._stream()),
                    "lic_adam_run")
        torch.cuda.synchronize()
        for i in range(n):
            for a, b in zip((sets[0][0][i], sets[0][1][i], sets[0][2][i]), (sets[1][0][i], sets[1][1][i], sets[1][2][i])):
                assert _same_bits(a, b), (step, i)
            got = guards[i].cpu().numpy().reshape(-1)
            want = before[i] if i == hole else E.ema_update(before[i], sets[0][0][i].cpu().numpy(), w)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (step, i)
    for i, g in enumerate(guards):
        g.check(f"average {i}")


# ---- 2. guard --------------------------------------------------------------------------------------------------------
def test_nonfinite_step_leaves_the_average_untouched():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    params = _params(dev, 7)
    opt = nic.FusedAdam(params, lr=LR, ema_decay=DECAY, max_grad_norm=1.0, skip_nonfinite=True)
    guards = _guarded_averages(opt, params)
    _set_grads(params, _grads(70))
    opt.step()
    keys = ("exp_avg", "exp_avg_sq", "ema")
    before = [[p.detach().clone()] + [opt.state[p][k].clone() for k in keys] for p in params]
    bad = _grads(71)
    bad[-1][-1] = math.inf
    _set_grads(params, bad)
    opt.step()
    assert opt.fused_steps == 2 and not math.isfinite(float(opt.grad_norm()))
    for p, kept in zip(params, before):
        for got, want in zip([p] + [opt.state[p][k] for k in keys], kept):
            assert _same_bits(got, want)
    assert opt.skipped_steps() == 1
    _set_grads(params, _grads(72))
    prev = [opt.state[p]["ema"].cpu().numpy().copy() for p in params]
    opt.step()                                              # the count went on: this is step 3 of the schedule
    for p, e0 in zip(params, prev):
        want = E.ema_update(e0, p.detach().cpu().numpy(), E.ema_weight(3, DECAY))
        assert np.array_equal(opt.state[p]["ema"].cpu().numpy().view(np.int32), want.view(np.int32))
    for g in guards:
        g.check("average")


# ---- 3. the torch path -----------------------------------------------------------------------------------------------
def _replay(opt, params, steps, seed, lengths, decay, scale=1.0):
    """`steps` steps; after each, every average must be ema_update(average before, parameter after, w(t))"""
    for step in range(1, steps + 1):
        _set_grads(params, _grads(seed + step, lengths, scale))
        before = [opt.state[p]["ema"].cpu().numpy().copy() if "ema" in opt.state.get(p, {})
                  else p.detach().cpu().numpy().copy() for p in params]
        opt.step()
        w = E.ema_weight(step, decay)
        for i, p in enumerate(params):
            want = E.ema_update(before[i], p.detach().cpu().numpy(), w)
            assert np.array_equal(opt.state[p]["ema"].cpu().numpy().view(np.int32), want.view(np.int32)), (step, i)


def test_449_tensors_take_the_torch_path_and_give_the_same_bits():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    lengths = tuple((1, 3, 5, 64, 127)[i % 5] for i in range(449))
    params = _params(dev, 9, lengths, unaligned=-1)
    opt = nic.FusedAdam(params, lr=LR, ema_decay=DECAY)
    _replay(opt, params, 2, 80, lengths, DECAY)
    assert opt.fused_steps == 0
    # ... and the launch, given the same tensors in two groups it can take (224 and 225 of them: the two larger
    # kernel-argument blocks), holds the same statement for the parameters IT computes
    twins = _params(dev, 9, lengths, unaligned=-1)
    fused = nic.FusedAdam([{"params": twins[:224]}, {"params": twins[224:]}], lr=LR, ema_decay=DECAY)
    _replay(fused, twins, 2, 80, lengths, DECAY)
    assert fused.fused_steps == 2
    # swapping 449 tensors goes through torch as well, and back
    live = [p.detach().clone() for p in params]
    avg = [opt.state[p]["ema"].clone() for p in params]
    opt.swap_ema()
    assert opt.swapped and all(_same_bits(p, a) for p, a in zip(params, avg))
    opt.swap_ema()
    assert all(_same_bits(p, b) for p, b in zip(params, live)) and all(_same_bits(opt.state[p]["ema"], a)
                                                                      for p, a in zip(params, avg))


def test_two_groups_one_fused_one_not_stay_consistent():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    small = tuple((1, 3, 5, 64, 127)[i % 5] for i in range(449))
    lengths = LENGTHS + small
    params = _params(dev, 10, lengths)
    opt = nic.FusedAdam([{"params": params[:len(LENGTHS)]}, {"params": params[len(LENGTHS):]}], lr=LR, ema_decay=DECAY,
                        max_grad_norm=1.0)
    _replay(opt, params, 2, 90, lengths, DECAY)
    counts = {float(s["step"]) for s in opt.state_dict()["state"].values()}
    assert counts == {2.0}
    live = [p.detach().clone() for p in params]
    avg = [opt.state[p]["ema"].clone() for p in params]
    with opt.ema_weights():             # group 0 through lic_swap_run, group 1 through torch
        assert all(_same_bits(p, a) for p, a in zip(params, avg))
        assert all(_same_bits(opt.state[p]["ema"], b) for p, b in zip(params, live))
    assert all(_same_bits(p, b) for p, b in zip(params, live))
    assert all(_same_bits(opt.state[p]["ema"], a) for p, a in zip(params, avg))
    _set_grads(params, _grads(99, lengths))
    opt.step()                          # and training goes on


# ---- 4. swap ---------------------------------------------------------------------------------------------------------
def test_swap_twice_is_the_identity_and_stays_inside_its_buffers():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    params = _params(dev, 11)
    opt = nic.FusedAdam(params, lr=LR, ema_decay=0.9, ema_warmup=False)
    guards = _guarded_averages(opt, params)
    for step in (1, 2):
        _set_grads(params, _grads(100 + step))
        opt.step()
    live = [p.detach().clone() for p in params]
    avg = [opt.state[p]["ema"].clone() for p in params]
    assert not any(_same_bits(a, b) for a, b in zip(live, avg))
    versions = [p._version for p in params]
    opt.swap_ema()
    assert opt.swapped
    assert all(_same_bits(p, a) for p, a in zip(params, avg))
    assert all(_same_bits(opt.state[p]["ema"], b) for p, b in zip(params, live))
    assert all(p._version > v for p, v in zip(params, versions))
    with pytest.raises(RuntimeError, match="swapped"):
        opt.step()
    assert all(_same_bits(p, a) for p, a in zip(params, avg))          # (the refused step touched nothing)
    opt.swap_ema()
    assert not opt.swapped
    assert all(_same_bits(p, b) for p, b in zip(params, live))
    assert all(_same_bits(opt.state[p]["ema"], a) for p, a in zip(params, avg))
    for g in guards:
        g.check("average")
    opt.step()                                                         # and a step is taken again


# ---- 5. stale caches -------------------------------------------------------------------------------------------------
# 8 latent channels in fp32; the bf16 convolutions refuse a model that narrow (lic_igemm_bf16: LIC_ERR_UNSUPPORTED in
# the first forward, with or without an average), so the bf16 case has the 64 the other bf16 model tests use
WIDTH = {"fp32": 8, "bf16": 64}


def _forward(model, x):
    with torch.no_grad():
        out = model(x, training=False)
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _equal_outputs(a, b):
    assert a.keys() == b.keys()
    return all(_same_bits(a[k].float(), b[k].float()) for k in a)


@pytest.mark.parametrize("precision,context", [("fp32", "raster"), ("bf16", "raster"), ("fp32", "checkerboard")])
def test_swapped_weights_reach_every_derived_buffer(precision, context):
    """step preparation, functional.PREPARED, the masked context weight and the bf16 packs are all derived from the
    parameters and keyed on their version counters: inside ema_weights() the model must compute with the averages,
    behind it with the trained weights again.  The reference inside is a fresh model loaded from ema_state_dict()."""
    dev = _need_gpu()
    import neural_image_compression_amd as nic

    def build():
        m = nic.JointAutoregressiveHierarchical(WIDTH[precision], K=1, context=context).to(dev)
        if precision == "bf16":
            m.set_precision("bf16")
        assert m.use_step_prep
        return m

    torch.manual_seed(4)
    model = build()
    opt = nic.FusedAdam(model.parameters(), lr=1e-2, ema_decay=0.9, ema_warmup=False)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(1, 3, 64, 64, generator=g).to(dev)
    for _ in range(3):
        opt.zero_grad()
        nic.rd_loss(model(x), x, 0.01, sync=False)["loss"].backward()
        opt.step()
    assert opt.fused_steps == 3
    trained = _forward(model, x)                       # (fills every cache from the trained weights)
    launches = model.step_prep().launches
    fresh = build()
    fresh.load_state_dict(opt.ema_state_dict(model))
    want = _forward(fresh, x)
    assert not _equal_outputs(trained, want)           # the averages are other weights: the comparison can fail
    with opt.ema_weights():
        inside = _forward(model, x)
        assert model.step_prep().launches == launches + 1
        assert _equal_outputs(inside, want)
    assert not opt.swapped
    assert _equal_outputs(_forward(model, x), trained)
    assert model.step_prep().launches == launches + 2


# ---- 6. state --------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_on_the_same_bits():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    pa, pb = _params(dev, 12), _params(dev, 12)
    oa = nic.FusedAdam(pa, lr=LR, ema_decay=DECAY, max_grad_norm=1.0)
    ob = nic.FusedAdam(pb, lr=LR, ema_decay=DECAY, max_grad_norm=1.0)
    for step in (1, 2):
        for ps, o in ((pa, oa), (pb, ob)):
            _set_grads(ps, _grads(110 + step))
            o.step()
    sd = ob.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    # (the copy of the off-grid parameter is off the grid as well: the element-wise path rounds the update otherwise
    # than the 16-byte path, tests/test_gpu_grad_clip.py)
    pc = [torch.nn.Parameter(_off_grid(p.detach()) if i == UNALIGNED_P else p.detach().clone()) for i, p in enumerate(pb)]
    oc = nic.FusedAdam(pc, lr=LR, ema_decay=DECAY, max_grad_norm=1.0)
    oc.load_state_dict(sd)
    for ps, o in ((pa, oa), (pc, oc)):
        _set_grads(ps, _grads(113))
        o.step()
    assert oc.fused_steps == 1
    for a, c in zip(pa, pc):
        assert _same_bits(a, c)
        for k in ("exp_avg", "exp_avg_sq", "ema"):
            assert _same_bits(oa.state[a][k], oc.state[c][k]), k


def test_torch_adam_state_starts_the_average_from_the_parameters_and_plain_state_is_torchs():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    pa, pb = _params(dev, 13), _params(dev, 13)
    ta = torch.optim.Adam(pa, lr=LR)
    plain = nic.FusedAdam(_params(dev, 13), lr=LR)
    for o in (ta, plain):
        _set_grads(o.param_groups[0]["params"], _grads(120))
        o.step()
    sa, sp = ta.state_dict(), plain.state_dict()
    assert sa["state"].keys() == sp["state"].keys() and all(set(sa["state"][k]) == set(sp["state"][k]) for k in sa["state"])
    assert sa["param_groups"][0].keys() == sp["param_groups"][0].keys()
    ob = nic.FusedAdam(pb, lr=LR, ema_decay=DECAY)
    for p, q in zip(pa, pb):
        q.data.copy_(p.detach())
    ob.load_state_dict(sa)
    assert all("ema" not in ob.state[q] for q in pb)
    start = [q.detach().cpu().numpy().copy() for q in pb]
    _set_grads(pb, _grads(121))
    ob.step()
    assert ob.fused_steps == 1
    for q, p0 in zip(pb, start):
        want = E.ema_update(p0, q.detach().cpu().numpy(), E.ema_weight(2, DECAY))      # the loaded count was 1
        assert np.array_equal(ob.state[q]["ema"].cpu().numpy().view(np.int32), want.view(np.int32))


# ---- 7. trainer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step_plan", [False, True])
def test_trainer_validates_on_the_average_and_checkpoints_it(tmp_path, step_plan):
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd.trainer import Trainer

    class Log:          # (train() closes its writer; validate() is called again behind it)
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, value, step))

        def close(self):
            pass

    g = torch.Generator(device="cpu").manual_seed(31)
    batches = [torch.rand(2, 3, 64, 64, generator=g) for _ in range(2)]
    torch.manual_seed(6)
    model = nic.JointAutoregressiveHierarchical(8, K=1).to(dev)
    opt = nic.FusedAdam(model.parameters(), lr=1e-2, ema_decay=0.9, ema_warmup=False)
    path = str(tmp_path / "ckpt.pth")
    tr = Trainer(model, opt, batches, val_loader=batches[:1], rd_loss=nic.rd_loss, lambda_val=0.01, max_steps=2,
                 checkpoint_path=path, writer=Log(), step_plan=step_plan, log_interval=100,
                 img_interval=100, val_interval=1, ema_eval=True)
    tr.log_statistics = False
    tr.train()
    assert opt.fused_steps == 2 and not opt.swapped
    assert len([r for r in tr.writer.rows if r[0] == "validation/validation_loss"]) == 2
    if step_plan:
        assert tr._plan is not None and tr._plan.replays == 2
    trained = {k: v.clone() for k, v in model.state_dict().items()}
    on_average = tr.validate()
    assert not opt.swapped and all(_same_bits(v, trained[k]) for k, v in model.state_dict().items())
    tr.ema_eval = False
    on_trained = tr.validate()
    assert math.isfinite(on_average) and math.isfinite(on_trained) and on_average != on_trained
    state = torch.load(path, map_location=dev)
    assert set(state) == {"model", "optimizer", "step", "scheduler", "ema_state_dict"}
    assert state["ema_state_dict"].keys() == state["model"].keys()
    named = dict(model.named_parameters())
    for k, v in state["ema_state_dict"].items():
        if k in named:
            assert _same_bits(v, opt.state[named[k]]["ema"]), k
    shipped = nic.JointAutoregressiveHierarchical(8, K=1).to(dev)
    shipped.load_state_dict(state["ema_state_dict"])
    x = batches[0].to(dev)
    with torch.no_grad():
        loss = float(nic.rd_loss(shipped(x, training=False), x, 0.01)["loss"])
    assert loss == on_average                                     # the shipped model IS what validation measured
    # the averages come back through the optimizer's state dict
    again = nic.FusedAdam(model.parameters(), lr=1e-2, ema_decay=0.9, ema_warmup=False)
    again.load_state_dict(state["optimizer"])
    for p in model.parameters():
        assert _same_bits(again.state[p]["ema"], opt.state[p]["ema"])
