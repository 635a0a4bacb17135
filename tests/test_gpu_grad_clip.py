"""Gradient clipping and non-finite step skipping inside FusedAdam (lic_grad_norm_partial / lic_grad_norm_finish /
lic_adam_run_scaled) on the GPU: the norm and the coefficient bit for bit against clip_ref.py on exact data, the fused
step bit for bit against `grad.mul_(coefficient)` + the plain step, the real model against torch.nn.utils.clip_grad_norm_
+ torch.optim.Adam, skipped steps, untouched defaults, and the Trainer.

The shapes are the smallest at which the kernels can go wrong: lengths around the 4096-element block, a gradient that
is not 16-byte aligned (scalar path), scalar tails, 3 / 97 / 225 tensors (one per kernel-argument block size), two
parameter groups."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clip_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4095, 4096, 4097, 2 * 4096 + 5)
LR = 1e-2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _unaligned(values):
    """the same numbers in a contiguous tensor that starts 4 bytes into an allocation: not 16-byte aligned"""
    big = torch.zeros(values.numel() + 1, dtype=values.dtype, device=values.device)
    big[1:] = values
    out = big[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _params(count, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(LENGTHS[i % len(LENGTHS)], generator=g).to(dev)) for i in range(count)]


def _set_grads(params, grads, unaligned=4):
    """gradient `unaligned` (length 4097: a scalar-path job of two blocks) is the 16-byte-unaligned one"""
    for i, (p, g) in enumerate(zip(params, grads)):
        g = g.to(p.device)
        p.grad = _unaligned(g) if i == unaligned % len(params) else g.clone()


def _int_grads(count, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randint(-8, 9, (LENGTHS[i % len(LENGTHS)],), generator=g).float() for i in range(count)]


def _rand_grads(count, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(LENGTHS[i % len(LENGTHS)], generator=g) * scale for i in range(count)]


def _bits(t):
    return int(t.detach().reshape(1).view(torch.int32).item())


def _fbits(x):
    return int(np.float32(x).view(np.int32))


def _guarded_norm(opt, max_norm):
    """lic_grad_norm_partial per group + lic_grad_norm_finish on the optimizer's own job tables and gradient
    pointers, into buffers with canaries on both sides.  Returns (norm bits, coefficient bits)."""
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()
    tabs = [opt._tables[gi] for gi in range(len(opt.param_groups))]
    total = sum(t[3] for t in tabs)
    pad, canary = 8, -12345.5
    pbuf = torch.full((total + 2 * pad,), canary, dtype=torch.float64, device="cuda:0")
    sbuf = torch.full((4 + 2 * pad,), canary, dtype=torch.float32, device="cuda:0")
    sbuf[pad:pad + 4] = 0.0
    at = 0
    for _, dev_tab, njobs, blocks, gptrs in tabs:
        L.check(lib.lic_grad_norm_partial(C.c_void_p(dev_tab.data_ptr()), njobs, blocks, gptrs,
                                          C.c_void_p(pbuf.data_ptr() + 8 * (pad + at)), F_._stream()), "partial")
        at += blocks
    L.check(lib.lic_grad_norm_finish(C.c_void_p(pbuf.data_ptr() + 8 * pad), total, float(max_norm), 1,
                                     C.c_void_p(sbuf.data_ptr() + 4 * pad), F_._stream()), "finish")
    torch.cuda.synchronize()
    for buf, n in ((pbuf, total), (sbuf, 4)):
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + n:] == canary).all())
    assert bool(torch.isfinite(pbuf[pad:pad + total]).all())      # (every partial was written)
    flags = sbuf[pad:pad + 4].view(torch.int32)
    assert int(flags[2]) == 0 and int(flags[3]) == 0
    return _bits(sbuf[pad]), _bits(sbuf[pad + 1])


@pytest.mark.parametrize("count", [3, 97, 225])
def test_norm_and_coefficient_are_exact_on_integer_data(count):
    """integers in [-8, 8]: every partial and the total are exact in double in any order, so the fp32 norm and the
    fp32 coefficient must be clip_ref's, bit for bit"""
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    grads = _int_grads(count, 100 + count)
    ref_norm = R.grad_norm([g.numpy() for g in grads])
    assert np.isfinite(ref_norm) and ref_norm > 0
    for max_norm in (0.5 * float(ref_norm), 2.0 * float(ref_norm), math.inf):
        ref_coef = R.coefficient(ref_norm, max_norm)
        assert (ref_coef < 1.0) == (max_norm < ref_norm)      # clipping active / coefficient exactly 1
        for split in (None, max(1, count // 3)):
            params = _params(count, dev, 7)
            _set_grads(params, grads)
            groups = [{"params": params}] if split is None else [{"params": params[:split]}, {"params": params[split:]}]
            opt = nic.FusedAdam(groups, lr=LR, max_grad_norm=max_norm)
            opt.step()
            assert opt.fused_steps == 1
            norm = opt.grad_norm()
            assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
            assert _bits(norm) == _fbits(ref_norm), (float(norm), float(ref_norm))
            assert _bits(opt._clip_state[1]) == _fbits(ref_coef), (float(opt._clip_state[1]), float(ref_coef))
            assert opt.skipped_steps() == 0
            assert _guarded_norm(opt, max_norm) == (_fbits(ref_norm), _fbits(ref_coef))
    # the stand-alone norm (no optimizer): the same two launches
    assert _bits(nic.grad_norm(params)) == _fbits(ref_norm)


def test_norm_of_random_data_is_within_one_ulp_and_repeats_bitwise():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    count = 97
    grads = _rand_grads(count, 11)
    ref_norm = R.grad_norm([g.numpy() for g in grads])
    params = _params(count, dev, 8)
    _set_grads(params, grads)
    seen = []
    for split in (None, None, 40):
        groups = [{"params": params}] if split is None else [{"params": params[:split]}, {"params": params[split:]}]
        opt = nic.FusedAdam(groups, lr=LR, max_grad_norm=math.inf)
        opt.step()
        seen.append(_bits(opt.grad_norm()))
    seen.append(_bits(nic.grad_norm(params)))
    seen.append(_bits(nic.grad_norm(params)))
    assert len(set(seen)) == 1, seen                        # run to run, one group or two: the same bits
    got = np.int32(seen[0]).view(np.float32)
    # the double sum is taken in another order than clip_ref's: the two doubles differ in their last bits, and ONE
    # rounding to fp32 follows -> at most one fp32 ulp
    assert abs(float(got) - float(ref_norm)) <= float(np.spacing(ref_norm)), (got, ref_norm)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_step_equals_scaled_gradients_and_plain_step_bitwise(wd):
    """copy A: every gradient multiplied by the coefficient with a torch fp32 mul_, then the plain step (lic_adam_run);
    copy B: the clipped step (lic_adam_run_scaled).  Same bits after 3 steps, the third through the cached fast path"""
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    count = 7
    pa, pb = _params(count, dev, 9), _params(count, dev, 9)
    oa = nic.FusedAdam(pa, lr=LR, weight_decay=wd)
    ob = nic.FusedAdam(pb, lr=LR, weight_decay=wd, max_grad_norm=0.75)
    coefs = []
    for step in range(3):
        grads = _rand_grads(count, 20 + step, scale=1e-3 if step == 1 else 1.0)
        _set_grads(pb, grads)
        ob.step()
        coef = ob._clip_state[1].clone()
        coefs.append(float(coef))
        _set_grads(pa, grads)               # (the same alignment as B's: the unaligned job takes the scalar path in both)
        for p in pa:
            p.grad.mul_(coef)
        oa.step()
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs
    assert oa.fused_steps == ob.fused_steps == 3 and oa._fast is not None and ob._fast is not None
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), i
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][k], ob.state[b][k]), (i, k)


def test_clipped_fused_adam_matches_torch_clip_and_adam_on_the_model():
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    torch.manual_seed(0)
    ma = nic.JointAutoregressiveHierarchical(64, 1).to(dev)
    mb = nic.JointAutoregressiveHierarchical(64, 1).to(dev)
    mb.load_state_dict(ma.state_dict())
    x = torch.rand(2, 3, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    oa = ob = None
    norms, max_norm, steps, lr = [], None, 4, 3e-3
    for step in range(steps):
        noise = (torch.rand(2, 64, 1, 1, device=dev), torch.rand(2, 64, 4, 4, device=dev))
        for m in (ma, mb):
            m.zero_grad(set_to_none=True)
            nic.rd_loss(m(x, noise=noise), x, 0.01, sync=False)["loss"].backward()
        for pa, pb in zip(ma.parameters(), mb.parameters()):   # identical inputs: identical gradients
            pb.grad.copy_(pa.grad)
        if step == 0:   # half of the first step's norm, as torch computes it
            max_norm = 0.5 * float(torch.nn.utils.get_total_norm([p.grad for p in ma.parameters()]))
            oa = torch.optim.Adam(ma.parameters(), lr=lr)
            ob = nic.FusedAdam(mb.parameters(), lr=lr, max_grad_norm=max_norm)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ma.parameters(), max_norm)))
        oa.step()
        ob.step()
        assert abs(float(ob.grad_norm()) - norms[-1]) <= 1e-5 * norms[-1]     # (torch sums squares in fp32)
    assert max(norms) > max_norm, (norms, max_norm)
    assert ob.fused_steps == steps
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        # test_fused_adam_matches_torch_adam's bound
        assert float((pa.detach() - pb.detach()).abs().max()) <= 1e-5 * (steps * lr) + 1e-6 * float(pa.detach().abs().max()), n
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()      # (the options are no group entries)
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == float(steps)
    ob.load_state_dict(sa)
    oa.load_state_dict(sb)


def _np_state(opt, params):
    return ([p.detach().cpu().numpy().copy() for p in params],
            [opt.state[p]["exp_avg"].cpu().numpy().copy() for p in params],
            [opt.state[p]["exp_avg_sq"].cpu().numpy().copy() for p in params])


def _assert_close_to_ref(params, opt, ref, steps_taken):
    got = _np_state(opt, params)
    for i in range(len(params)):
        for k in range(3):
            a, b = got[k][i], ref[k][i]
            # test_fused_adam_matches_torch_adam's bound (clip_ref does not fuse multiply-adds; the kernel does)
            assert float(np.abs(a - b).max()) <= 1e-5 * (steps_taken * LR) + 1e-6 * float(np.abs(b).max()), (i, k)


@pytest.mark.parametrize("bad,where", [(math.inf, "last"), (math.nan, "tail")])
def test_nonfinite_step_is_skipped_and_counted(bad, where):
    """one inf in the last element of the last tensor / one NaN in a scalar tail element (index 4096 of a 16-byte
    aligned gradient of 4097): p, m and v keep their bits, the count goes up, the step count advances, and the
    next finite step is an ordinary one.  Non-finite numbers only pass through arithmetic here."""
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    count, max_norm = 7, 0.75
    params = _params(count, dev, 12)
    opt = nic.FusedAdam(params, lr=LR, max_grad_norm=max_norm, skip_nonfinite=True)
    ref = ([p.detach().cpu().numpy().copy() for p in params], [np.zeros(p.numel(), np.float32) for p in params],
           [np.zeros(p.numel(), np.float32) for p in params])
    g1 = _rand_grads(count, 31)
    _set_grads(params, g1)
    opt.step()
    R.clipped_step(ref[0], [g.numpy() for g in g1], ref[1], ref[2], 1, LR, max_norm=max_norm, skip_nonfinite=True)
    _assert_close_to_ref(params, opt, ref, 1)
    assert opt.skipped_steps() == 0
    before = [[t.clone() for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])] for p in params]
    g2 = _rand_grads(count, 32)
    if where == "last":
        g2[-1][-1] = bad
    else:
        assert g2[5].numel() == 2 * 4096 + 5
        g2[5][-1] = bad                       # aligned gradient, vector path: the last of its 5 tail elements
    _set_grads(params, g2)
    opt.step()                                # second step: through the cached plan
    assert opt._fast is not None and opt.fused_steps == 2
    assert not math.isfinite(float(opt.grad_norm()))
    for p, (p0, m0, v0) in zip(params, before):
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32))
        assert torch.equal(opt.state[p]["exp_avg"].view(torch.int32), m0.view(torch.int32))
        assert torch.equal(opt.state[p]["exp_avg_sq"].view(torch.int32), v0.view(torch.int32))
    assert opt.skipped_steps() == 1
    assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {2.0}    # the count advanced all the same
    g3 = _rand_grads(count, 33)
    _set_grads(params, g3)
    opt.step()
    # the skipped step left the moments alone but took its place in the count: this is update number 3
    R.clipped_step(ref[0], [g.numpy() for g in g3], ref[1], ref[2], 3, LR, max_norm=max_norm, skip_nonfinite=True)
    _assert_close_to_ref(params, opt, ref, 2)
    assert opt.skipped_steps() == 1 and math.isfinite(float(opt.grad_norm()))


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_nonfinite_step_without_skipping_follows_torch(bad):
    """skip_nonfinite=False: what clip_grad_norm_ + torch.optim.Adam do with the same data -- an inf norm gives the
    coefficient 0 and a NaN where the inf was; a NaN norm gives a NaN coefficient and NaN everywhere"""
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    count = 7
    pa, pb = _params(count, dev, 13), _params(count, dev, 13)
    oa = torch.optim.Adam(pa, lr=LR)
    ob = nic.FusedAdam(pb, lr=LR, max_grad_norm=0.75)
    for step in range(2):
        grads = _rand_grads(count, 41 + step)
        if step == 1:
            grads[-1][-1] = bad
        _set_grads(pa, grads)
        _set_grads(pb, grads)
        torch.nn.utils.clip_grad_norm_(pa, 0.75)
        oa.step()
        ob.step()
    assert ob.fused_steps == 2 and ob.skipped_steps() == 0
    nans = 0
    for a, b in zip(pa, pb):
        a, b = a.detach(), b.detach()
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        nans += int(torch.isnan(b).sum())
        ok = ~torch.isnan(a)
        if bool(ok.any()):
            assert float((a[ok] - b[ok]).abs().max()) <= 1e-5 * (2 * LR) + 1e-6 * float(a[ok].abs().max())
    assert nans == (1 if math.isinf(bad) else sum(p.numel() for p in pb))


def test_defaults_launch_what_they_did():
    """no options: bitwise the parameters of lic_adam_run driven directly on a copy, nothing allocated for clipping,
    and grad_norm() says that clipping is off"""
    dev = _need_gpu()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    lib = L.load()
    count, wd = 7, 0.01
    params = _params(count, dev, 14)
    opt = nic.FusedAdam(params, lr=LR, weight_decay=wd)
    qs = [p.detach().clone() for p in params]
    ms, vs = [torch.zeros_like(q) for q in qs], [torch.zeros_like(q) for q in qs]
    arr = (L.AdamJob * count)()
    for j, q, m, v in zip(arr, qs, ms, vs):
        j.p, j.m, j.v, j.n = q.data_ptr(), m.data_ptr(), v.data_ptr(), q.numel()
    blocks = lib.lic_adam_plan(arr, count)
    assert blocks == sum((q.numel() + 4095) // 4096 for q in qs)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    for step in (1, 2, 3):
        _set_grads(params, _rand_grads(count, 50 + step))
        gptrs = (C.c_void_p * count)(*[p.grad.data_ptr() for p in params])
        L.check(lib.lic_adam_run(C.c_void_p(table.data_ptr()), count, blocks, gptrs, LR, 0.9, 0.999, 1e-8, wd,
                                 1.0 - 0.9 ** step, 1.0 - 0.999 ** step, F_._stream()), "lic_adam_run")
        opt.step()
    assert opt.fused_steps == 3 and opt._fast is not None
    for p, q, m, v in zip(params, qs, ms, vs):
        assert torch.equal(p.detach(), q)
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
    assert opt._clip_state is None and opt._partials is None
    with pytest.raises(RuntimeError, match="clipping is off"):
        opt.grad_norm()


def test_trainer_clips_with_and_without_the_step_plan(tmp_path):
    """the model and batches of test_gpu_plan.py's trainer test: Trainer(step_plan=True, clip_max_norm=m) and the eager
    Trainer(clip_max_norm=m) end 3 steps on the same bits; the JSONL writer holds train/grad_norm"""
    dev = _need_gpu()
    import json
    import neural_image_compression_amd as nic
    from neural_image_compression_amd.trainer import Trainer, _JsonlWriter
    g = torch.Generator(device="cpu").manual_seed(21)
    batches = [torch.rand(4, 3, 64, 64, generator=g) for _ in range(3)]
    max_norm = 1.0      # (the usual recipe's bound)

    def run(step_plan):
        torch.manual_seed(2)
        m = nic.JointAutoregressiveHierarchical(128, 3).to(dev)
        m.set_precision("bf16")
        folder = tmp_path / ("plan" if step_plan else "eager")
        tr = Trainer(m, nic.FusedAdam(m.parameters(), lr=1e-3), batches, rd_loss=nic.rd_loss, lambda_val=0.01, max_steps=3,
                     checkpoint_path=None, writer=_JsonlWriter(str(folder)), step_plan=step_plan, log_interval=1,
                     img_interval=100, val_interval=100, clip_max_norm=max_norm, skip_nonfinite=True)
        tr.log_statistics = False
        torch.cuda.manual_seed(9)
        tr.train()
        rows = [json.loads(line) for line in open(folder / "scalars.jsonl")]
        return m, rows, tr

    ma, rows_a, tra = run(False)
    mb, rows_b, trb = run(True)
    assert trb._plan is not None and trb._plan.replays == 3
    assert tra.optimizer.max_grad_norm == max_norm and tra.optimizer.fused_steps == 3 == trb.optimizer.fused_steps
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n
    for rows in (rows_a, rows_b):
        norms = [r["value"] for r in rows if r["tag"] == "train/grad_norm"]
        assert len(norms) == 3 and all(math.isfinite(v) and v > 0 for v in norms), norms
        assert [r["value"] for r in rows if r["tag"] == "train/skipped_steps"] == [0.0] * 3
    assert [r for r in rows_a if r["tag"] == "train/grad_norm"] == [r for r in rows_b if r["tag"] == "train/grad_norm"]
    print("train/grad_norm", [r["value"] for r in rows_a if r["tag"] == "train/grad_norm"])
