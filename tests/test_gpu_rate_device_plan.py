"""Rate levels with qualities and lambdas on the device (`device_quality=True`, a lambda tensor in `rd_loss`),
under launch plans and in the Trainer.  fp32 (M = 16) and bf16 (M = 64), raster and checkerboard contexts, x of
2..4 x 3 x 64 x 64; models, tables (|T| <= 0.7) and inputs as tests/test_gpu_rate_model.py builds them.

  * tables at zero: expf(0) = 1, so the device-quality run is the plain model bit for bit, out-dict and gradients;
  * device against host qualities at the same q: the two differ only in the exp of the gain rows (expf in the kernel,
    torch.exp on the host path; both within an ulp or two of the true rows), so x_hat agrees within 1e-4 of its
    maximum, the project's fp32 output band, and bpp_total within 1e-4 relative.  bf16: against the fp32 device-quality
    run of the same weights, at the project's bf16 bands (tests/test_gpu_variants.py BF16_BANDS, 2x the deviations of
    profiles/r03_bf16_deviations.json; of its two rows the one measured at the larger deviation, per quantity);
  * a mixed batch -- one quality and one lambda per image -- is the per-image runs, on the keys the host-quality test
    compares, and the per-image mse of the loss;
  * three FusedAdam steps, x, q[B] and lam[B] changing every step: eager (`device_quality=True`, lambda tensor) and planned
    (`StepPlan.step(x, quality=, lam=)`) give the same bits in losses, result buffers, every gradient (the four tables
    included) and the final weights; the record holds no memcpy node, and `step` does no host synchronisation;
  * Trainer(rate_per_image=True) with and without step_plan: same weights, B pairs per step, the draw resumes from a
    checkpoint; rate_points with step_plan=True and without the flag still raises;
  * ForwardPlan at two successive qualities is the eager device-quality forward;
  * `functional.gain_rows_device`: k views of one buffer, no gradient for q, the tables' gradients of the float32 statement;
  * `rd_loss_msssim` with a lambda tensor: rate + mean_b lam_b (1 - ms_b), and the scalar loss when all lambdas are equal.

Run on the MI355X box:  python -m pytest tests/test_gpu_rate_device_plan.py -m gpu -q"""
import numpy as np
import pytest
import torch

import rate_device_ref as RD

from test_gpu_rate_model import (CASES, OUT_KEYS, Q, TABLES, WIDTH, _build, _inputs, _param_keys, _same_tensors, _step,
                                 _tables)

pytestmark = pytest.mark.gpu

LAM = 0.01
# test_gpu_variants.BF16_BANDS: relative bpp_total and mse, y relative to max|y| -- per quantity the wider of its two rows
BF16_BAND = {"bpp_total": 2.5e-4, "mse": 7e-4, "y_rel_max": 0.015}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, torch.device("cuda:0")


def _dev(values, dev):
    return torch.tensor(values, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_zero_tables_on_the_device_path_are_the_plain_model(env, prec, ctx):
    nic, dev = env
    plain = _build(nic, dev, prec, ctx, K=3)
    rated = _build(nic, dev, prec, ctx, K=3, rate_levels=Q)
    x, noise = _inputs(plain.M, dev)
    q = _dev([0.0, 1.3], dev)
    out_p, grads_p = _step(nic, plain, x, noise)
    out_r, grads_r = _step(nic, rated, x, noise, quality=q, device_quality=True)
    assert list(out_r) == list(out_p) + ["quality"] and out_r["quality"] is not None and torch.equal(out_r["quality"], q)
    _same_tensors(out_r, out_p, list(out_p))
    assert set(grads_r) == set(grads_p) | set(TABLES)
    differ = [n for n in grads_p if not torch.equal(grads_r[n], grads_p[n])]
    assert not differ, differ
    for k in TABLES:
        assert grads_r[k] is not None and bool(torch.isfinite(grads_r[k]).all())
    with pytest.raises(ValueError, match="no rate levels"):
        plain(x, noise=noise, device_quality=True)
    for bad in (1.0, torch.tensor([0.0, 1.0]), _dev([0.0], dev), _dev([0.0, 1.0], dev).double()):
        with pytest.raises(ValueError, match="device_quality"):
            rated(x, noise=noise, quality=bad, device_quality=True)


@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_device_and_host_qualities_agree(env, prec, ctx):
    nic, dev = env
    M = WIDTH[prec]
    tables = _tables(M, 21)
    x, noise = _inputs(M, dev)
    qs = [0.5, 1.75]
    fp32 = _build(nic, dev, "fp32", ctx, rate_levels=Q, tables=tables) if prec == "fp32" else None
    if prec == "fp32":
        with torch.no_grad():
            host = fp32(x, noise=noise, quality=torch.tensor(qs))
            devq = fp32(x, noise=noise, quality=_dev(qs, dev), device_quality=True)
            bpp = [float(nic.rd_loss(o, x, LAM)["bpp_total"]) for o in (host, devq)]
        err = float((devq["x_hat"] - host["x_hat"]).abs().max() / host["x_hat"].abs().max())
        print(f"{ctx}: x_hat {err:.3e} of max, bpp_total {abs(bpp[1] - bpp[0]) / bpp[0]:.3e} relative")
        assert err <= 1e-4 and abs(bpp[1] - bpp[0]) <= 1e-4 * bpp[0]
        return
    # bf16 storage against the fp32 arithmetic of the same weights (width 64 on both sides), both on the device path
    ref = nic.JointAutoregressiveHierarchical(M, 1, context=ctx, rate_levels=Q).to(dev)
    low = _build(nic, dev, "bf16", ctx, rate_levels=Q, tables=tables)
    ref.load_state_dict(low.state_dict())
    with torch.no_grad():
        a = ref(x, noise=noise, quality=_dev(qs, dev), device_quality=True)
        b = low(x, noise=noise, quality=_dev(qs, dev), device_quality=True)
        ra, rb = nic.rd_loss(a, x, LAM), nic.rd_loss(b, x, LAM)
    dy = float((a["y"] - b["y"]).abs().max() / a["y"].abs().max())
    rel = {k: abs(rb[k] - ra[k]) / abs(ra[k]) for k in ("bpp_total", "mse")}
    print(f"{ctx}: y {dy:.3e} of max (band {BF16_BAND['y_rel_max']}), " +
          ", ".join(f"{k} {v:.3e} (band {BF16_BAND[k]})" for k, v in rel.items()))
    assert dy <= BF16_BAND["y_rel_max"] and all(rel[k] <= BF16_BAND[k] for k in rel)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_mixed_device_batch_is_the_per_image_runs(env, prec, ctx, training):
    nic, dev = env
    rated = _build(nic, dev, prec, ctx, rate_levels=Q, tables=_tables(WIDTH[prec], 22))
    x, (uz, uy) = _inputs(rated.M, dev)
    q, lam = _dev([0.5, 2.0], dev), _dev([0.002, 0.05], dev)
    with torch.no_grad():
        both = rated(x, training=training, noise=(uz, uy), quality=q, device_quality=True)
        res = nic.rd_loss(both, x, lam, sync=False)
        terms = []
        for b in range(2):
            one = rated(x[b:b + 1], training=training, noise=(uz[b:b + 1], uy[b:b + 1]), quality=q[b:b + 1].clone(),
                        device_quality=True)
            for k in OUT_KEYS + _param_keys(one):
                if torch.is_tensor(one[k]):
                    assert torch.equal(both[k][b:b + 1], one[k]), (k, b)
            r1 = nic.rd_loss(one, x[b:b + 1], lam[b:b + 1].clone(), sync=False)
            assert torch.equal(res["mse_per_image"][b:b + 1], r1["mse_per_image"]), b
            terms.append(float(r1["distortion_term"]))
    # mean_b lambda_b * 255^2 * mse_b: each image's own term is the B = 1 run's, within the final rounding to fp32
    want = sum(terms) / 2
    assert abs(float(res["distortion_term"]) - want) <= 2.0 ** -22 * want
    assert float(res["loss"]) == float(np.float32(float(res["bpp_total"])) + np.float32(float(res["distortion_term"])))


def _rate_points(steps, B):
    r = np.random.RandomState(31)
    return [(r.uniform(0, Q - 1, B).astype(np.float32), r.choice([0.002, 0.01, 0.05], B).astype(np.float32))
            for _ in range(steps)]


@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_step_plan_with_changing_rate_points_equals_eager_training(env, prec, ctx):
    nic, dev = env
    from neural_image_compression_amd.plan import StepPlan
    B, steps = 3, 3
    tables = _tables(WIDTH[prec], 23)
    xs = [_inputs(WIDTH[prec], dev, (B, 64, 64))[0] * s for s in (1.0, 0.9, 0.8)]
    points = _rate_points(steps, B)

    def build():
        m = _build(nic, dev, prec, ctx, rate_levels=Q, tables=tables)
        return m, nic.FusedAdam(m.parameters(), lr=1e-3)

    ma, oa = build()
    torch.cuda.manual_seed(5)
    eager = []
    for x, (q, lam) in zip(xs, points):
        oa.zero_grad(set_to_none=True)
        res = nic.rd_loss(ma(x, quality=_dev(q, dev), device_quality=True), x, _dev(lam, dev), sync=False)
        res["loss"].backward()
        eager.append((res["_buffer"].clone(), {n: p.grad.clone() for n, p in ma.named_parameters()}))
        oa.step()

    mb, ob = build()
    plan = StepPlan(mb, nic.rd_loss, _dev(points[0][1], dev), xs[0], quality=_dev(points[0][0], dev))
    assert plan.info["memcpys"] == 0, plan.info
    torch.cuda.manual_seed(5)
    for i, (x, (q, lam)) in enumerate(zip(xs, points)):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out, res = plan.step(x, quality=q, lam=lam)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        buf, grads = eager[i]
        assert torch.equal(res["_buffer"], buf), i                      # the loss and every reported number
        assert torch.equal(res["loss"].detach(), buf[0]) and torch.equal(out["quality"], _dev(q, dev))
        for n, p in mb.named_parameters():
            assert p.grad is not None and torch.equal(p.grad, grads[n]), (i, n)
        ob.step()
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n
    assert all(float(eager[-1][1][k].abs().max()) > 0 for k in TABLES)
    # omitted arguments keep the previous values; a plan without resident values refuses them
    before = (plan.quality.clone(), plan.lam.clone())
    plan.step(xs[0])
    assert torch.equal(plan.quality, before[0]) and torch.equal(plan.lam, before[1])
    plan.step(xs[0], lam=points[0][1])
    assert torch.equal(plan.quality, before[0]) and torch.equal(plan.lam, _dev(points[0][1], dev))
    plan.close()


def test_plan_without_resident_rate_points_refuses_them(env):
    nic, dev = env
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd.plan import StepPlan
    plain = _build(nic, dev, "fp32", "raster")
    x, _ = _inputs(plain.M, dev)
    plan = StepPlan(plain, nic.rd_loss, LAM, x)
    with pytest.raises(L.LicError, match="without a resident"):
        plan.step(x, lam=[0.01, 0.02])
    plan.close()


@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_trainer_per_image_rate_points_planned_and_eager(env, prec, ctx, tmp_path):
    nic, dev = env
    from neural_image_compression_amd.trainer import Trainer, draw_rate_points
    B = 2
    tables = _tables(WIDTH[prec], 24)
    x, _ = _inputs(WIDTH[prec], dev, (B, 64, 64))
    points = [(0.0, 0.002), (0.75, 0.005), (1.5, 0.02), (2.0, 0.05)]
    trained, drawn = {}, {}
    for planned in (False, True):
        model = _build(nic, dev, prec, ctx, rate_levels=Q, tables=tables)
        kw = dict(rd_loss=nic.rd_loss, rate_points=points, rate_seed=3, rate_per_image=True, step_plan=planned, max_steps=3,
                  device="cuda:0", writer=None, log_dir=str(tmp_path / f"log{planned}"),
                  checkpoint_path=str(tmp_path / f"ck{planned}.pth"), log_interval=100, val_interval=100)
        tr = Trainer(model, nic.FusedAdam(model.parameters(), lr=1e-4), [x.cpu()], **kw)
        torch.cuda.manual_seed(9)
        drawn[planned] = []
        for _ in range(3):
            out, res = tr.train_step(tr._next_batch())
            assert len(tr.last_rate_point) == B and all(p in points for p in tr.last_rate_point)
            assert torch.equal(out["quality"].cpu(), torch.tensor([p[0] for p in tr.last_rate_point]))
            assert np.isfinite(float(res["loss"].detach()))
            drawn[planned].append(list(tr.last_rate_point))
        trained[planned] = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert drawn[True] == drawn[False] and (tr._plan is not None and tr._plan.replays == 3)
    for n in trained[False]:
        assert torch.equal(trained[True][n], trained[False][n]), n
    # the draw sequence travels in the checkpoint
    tr.save_checkpoint()
    want = [draw_rate_points(tr._rate_rng, points, B) for _ in range(4)]
    again = Trainer(model, nic.FusedAdam(model.parameters(), lr=1e-4), [x.cpu()], resume=True, **dict(kw, rate_seed=77))
    assert [draw_rate_points(again._rate_rng, points, B) for _ in range(4)] == want
    with pytest.raises(ValueError, match="step_plan=True"):
        Trainer(model, nic.FusedAdam(model.parameters(), lr=1e-4), [x.cpu()], **dict(kw, rate_per_image=False))
    with pytest.raises(ValueError, match="needs rate_points"):
        Trainer(model, nic.FusedAdam(model.parameters(), lr=1e-4), [x.cpu()], **dict(kw, rate_points=None))


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_forward_plan_at_two_qualities_is_the_eager_forward(env, prec, ctx, training):
    nic, dev = env
    from neural_image_compression_amd.plan import ForwardPlan
    rated = _build(nic, dev, prec, ctx, rate_levels=Q, tables=_tables(WIDTH[prec], 25))
    x, _ = _inputs(rated.M, dev)
    qs = [[0.25, 2.0], [1.5, 0.0]]
    plan = ForwardPlan(rated, x, training=training, quality=_dev(qs[0], dev))
    assert plan.info["memcpys"] == 0, plan.info
    keys = [k for k in OUT_KEYS if k != "x_hat"]
    for q in qs:
        torch.cuda.manual_seed(13)
        got = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in plan(x, quality=q).items()}
        torch.cuda.manual_seed(13)
        with torch.no_grad():
            want = rated.analysis_hyperprior(x, training=training, quality=_dev(q, dev), device_quality=True)
        _same_tensors(got, want, keys + _param_keys(want))
    plan.close()


def test_gain_rows_device_function(env):
    nic, dev = env
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    M, B = 16, 5
    tabs = [torch.from_numpy(t).to(dev).requires_grad_() for t in _tables(M, 26).values()]
    q = _dev([0.0, 0.5, 0.5, 2.0, 1.25], dev).requires_grad_()
    rows = F_.gain_rows_device(q, *tabs)
    assert len(rows) == 4 and all(r.shape == (B, M) and r.is_contiguous() for r in rows)
    base = rows[0].untyped_storage().data_ptr()
    assert [r.data_ptr() - base for r in rows] == [4 * B * M * t for t in range(4)]     # views of one [4][B][M] buffer
    want = RD.rows64(q.detach().cpu().numpy(), np.stack([t.detach().cpu().numpy() for t in tabs]))
    got = torch.stack(rows).detach().cpu().numpy()
    assert (np.abs(got - want) / want).max() <= 2.0 ** -23 + 2.0 ** -24 * (1 + 3 * 0.7)
    g = [torch.from_numpy(np.random.RandomState(27 + t).standard_normal((B, M)).astype(np.float32)).to(dev) for t in range(4)]
    (rows[0] * g[0]).sum().add((rows[1] * g[1]).sum()).add((rows[3] * g[3]).sum()).backward()    # table 2: no gradient
    assert q.grad is None
    i, l = RD.levels(q.detach().cpu().numpy(), Q)
    want32, _ = RD.table_grad(i, l, got, [g[0].cpu().numpy(), g[1].cpu().numpy(), None, g[3].cpu().numpy()], Q, np.float32)
    for t in (0, 1, 3):
        assert np.array_equal(tabs[t].grad.cpu().numpy().view(np.int32), want32[t].view(np.int32)), t
    assert tabs[2].grad is None or not bool(tabs[2].grad.any())
    for bad in ((q.detach().cpu(), *tabs), (q.detach().double(), *tabs), (q.detach(),), (q.detach(), tabs[0], tabs[1][:, :8])):
        with pytest.raises(L.LicError):
            F_.gain_rows_device(*bad)


def test_msssim_loss_with_one_lambda_per_image(env):
    nic, dev = env
    B, H = 2, 192                                           # MS-SSIM needs sides above 160
    r = np.random.RandomState(28)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    x = up(r.rand(B, 3, H, H))
    noise = up(0.05 * r.standard_normal((B, 3, H, H)))

    def run(lam):
        x_hat = (x + noise).clamp(0, 1).requires_grad_()
        out = {"x_hat": x_hat, "logp_y": up(-r.gamma(2.0, 1.0, (B, 8, 12, 12))), "logp_z": up(-r.gamma(2.0, 1.0, (B, 8, 3, 3)))}
        r.seed(29)                                          # (the same rates for every run)
        res = nic.rd_loss_msssim(out, x, lam, sync=False)
        res["loss"].backward()
        return res, x_hat.grad

    r.seed(29)
    scalar, g_scalar = run(8.0)
    same, g_same = run(_dev([8.0, 8.0], dev))
    mixed, g_mixed = run(_dev([8.0, 2.0], dev))
    ms = mixed["ms_ssim_per_image"].double().cpu().numpy()
    rate = float(mixed["bpp_total"])
    eps = (2 * B + 8) * 2.0 ** -24                          # a handful of fp32 roundings on either side
    assert abs(float(same["loss"].detach()) - float(scalar["loss"].detach())) <= eps * (abs(rate) + 8.0)
    want = rate + float((np.array([8.0, 2.0]) * (1 - ms)).mean())
    assert abs(float(mixed["loss"].detach()) - want) <= eps * (abs(rate) + 8.0)
    assert abs(float(mixed["distortion_term"]) - (want - rate)) <= eps * 8.0
    assert set(mixed) == set(scalar) | {"distortion_term"}
    # the upstream gradient of image b is -lam_b / B either way, and the MS-SSIM backward is linear in it
    top = float(g_scalar.abs().max())
    assert float((g_same - g_scalar).abs().max()) <= 1e-6 * top
    assert float((g_mixed[0] - g_scalar[0]).abs().max()) <= 1e-6 * top
    assert float((g_mixed[1] * 4 - g_scalar[1]).abs().max()) <= 1e-6 * top
