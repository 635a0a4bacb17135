"""Training for MS-SSIM on the device: `functional.ms_ssim`'s gradient (lic_msssim_bwd) against the float64
reference of tests/msssim_ref64.py differentiated by torch.autograd on the CPU, `rd_loss_msssim` against the same
formula in torch, one whole training step against the torch-CPU path, and the upper layers (StepPlan, Trainer,
CompressionEvaluator) running with the new loss as they do with `rd_loss`.

Bands: gradients 5e-4 of the tensor's max |gradient| (the project's gradient band), values 2e-5 (tests/test_msssim.py),
loss outputs 1e-4 relative.  Every parity case has all per-scale terms above 0.05 (asserted on the float64 reference
before comparing; tests/test_msssim_ref64.py asserts the same on the CPU); no element is left out.

Measured on an MI355X (device dx against the float64 gradient, as a share of the 5e-4 band): see DESIGN.md 7."""
import numpy as np
import pytest
import torch

import golden_recipe as R
import msssim_ref64 as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import functional as F_
    return nic, F_, torch.device("cuda:0")


def _place(t, layout, dev):
    """the CPU tensor on the device in the case's memory layout"""
    d = t.to(dev)
    if layout == "nhwc":
        return d.contiguous(memory_format=torch.channels_last)
    if layout == "view":   # a window of a larger tensor: no dimension is dense
        B, C, H, W = d.shape
        big = torch.zeros(B, C + 1, H + 7, W + 9, device=dev)
        big[:, :C, 3:3 + H, 5:5 + W] = d
        v = big[:, :C, 3:3 + H, 5:5 + W]
        assert not v.is_contiguous() and not v.is_contiguous(memory_format=torch.channels_last)
        return v
    return d.contiguous()


def _device_value_and_grad(F_, x, y, data_range, layout, dev, size_average=True, upstream=None):
    dx = _place(x, layout, dev).requires_grad_(True)
    dy = _place(y, layout, dev)
    val = F_.ms_ssim(dx, dy, data_range=data_range, size_average=size_average)
    assert val.grad_fn is not None
    if upstream is None:
        val.backward()
    else:
        val.backward(upstream.to(dev))
    torch.cuda.synchronize()
    return val.detach(), dx.grad, dx, dy


@pytest.mark.parametrize("name", list(M.CASES))
def test_msssim_gradient_vs_float64(env, name):
    nic, F_, dev = env
    x, y, data_range, layout = M.case_inputs(name)
    v64, g64, tmin = M.value_and_grad(x, y, data_range)
    assert tmin > M.MIN_TERM, tmin
    val, grad, dx, dy = _device_value_and_grad(F_, x, y, data_range, layout, dev)
    assert grad.shape == x.shape and grad.dtype == torch.float32
    scale = float(g64.abs().max())
    err = float((grad.cpu().double() - g64).abs().max()) / scale
    verr = abs(float(val) - float(v64))
    print(f"{name}: value error {verr:.2e}, dx error {err:.2e} of max|g| = {err / M.GRAD_BAND:.3f} of the band")
    assert verr <= M.VALUE_BAND, (float(val), float(v64))
    assert err <= M.GRAD_BAND, err
    # the forward value is the no-grad path's, bit for bit
    with torch.no_grad():
        plain = F_.ms_ssim(dx, dy, data_range=data_range)
    assert plain.grad_fn is None and torch.equal(plain, val)
    assert torch.equal(F_.ms_ssim(dx.detach(), dy, data_range=data_range), val)
    # two runs, the same bits
    val2, grad2, _, _ = _device_value_and_grad(F_, x, y, data_range, layout, dev)
    assert torch.equal(val2, val) and torch.equal(grad2, grad)


def test_msssim_gradient_per_image_with_a_non_uniform_upstream(env):
    nic, F_, dev = env
    x, y, data_range, layout = M.case_inputs("crop_nhwc")
    up = torch.tensor([0.25, -1.5])
    v64, g64, tmin = M.value_and_grad(x, y, data_range, size_average=False, upstream=up)
    assert tmin > M.MIN_TERM
    val, grad, _, _ = _device_value_and_grad(F_, x, y, data_range, layout, dev, size_average=False, upstream=up)
    assert val.shape == (2,) and float((val.cpu().double() - v64).abs().max()) <= M.VALUE_BAND
    for b in range(2):   # each image against its own scale: the small upstream gradient is held to the band too
        err = float((grad[b].cpu().double() - g64[b]).abs().max()) / float(g64[b].abs().max())
        print(f"image {b}: dx error {err:.2e} of max|g|")
        assert err <= M.GRAD_BAND, (b, err)


def test_msssim_gradient_at_an_undefined_point_is_zero(env):
    nic, F_, dev = env
    x, y = M.undefined_pair()
    terms = M.scale_terms(x.double(), y.double(), 1.0)
    assert float(terms[:, 0].min()) <= 0.0 and float(terms[:, 1].min()) > M.MIN_TERM
    val, grad, _, _ = _device_value_and_grad(F_, x, y, 1.0, "nchw", dev, size_average=False, upstream=torch.ones(2))
    assert float(val[0]) == 0.0
    assert bool(torch.isfinite(grad).all()) and float(grad[0].abs().max()) == 0.0
    # the other image of the batch: its own gradient, within the band
    _, g64, _ = M.value_and_grad(x[1:], y[1:], 1.0, size_average=False)
    err = float((grad[1:].cpu().double() - g64).abs().max()) / float(g64.abs().max())
    assert err <= M.GRAD_BAND, err


def test_msssim_has_no_gradient_for_its_second_argument(env):
    nic, F_, dev = env
    x, y, _, _ = M.case_inputs("odd_sides")
    with pytest.raises(ValueError):
        F_.ms_ssim(x.to(dev), y.to(dev).requires_grad_(True), data_range=1.0)


# ---------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------
def _loss_reference(logp_y, logp_z, x_hat, x, lam):
    """loss = bpp_total + lam * (1 - ms_ssim(x_hat, x)) in float64 torch on the CPU, with the oracle's rate terms"""
    from oracle import torch_ref as TR
    ly, lz, xh = (t.double().requires_grad_(True) for t in (logp_y, logp_z, x_hat))
    rd = TR.rd_loss({"logp_y": ly, "logp_z": lz, "x_hat": xh}, x.double(), 0.0)
    ms_img = M.ms_ssim(xh, x.double(), 1.0, size_average=False)
    loss = rd["bpp_total"] + lam * (1.0 - ms_img.mean())
    loss.backward()
    ref = {k: float(rd[k].detach()) for k in ("bpp_y", "bpp_z", "bpp_total", "mse", "psnr", "bits_y", "bits_z")}
    ref.update(loss=float(loss.detach()), ms_ssim=float(ms_img.detach().mean()), bits_total=ref["bits_y"] + ref["bits_z"])
    return ref, ms_img.detach(), rd["mse_per_image"].detach(), (ly.grad, lz.grad, xh.grad)


def test_rd_loss_msssim_vs_torch(env):
    nic, F_, dev = env
    B, Mc, H, W, lam = 2, 8, 256, 256, 8.0
    x_hat, x = M.pair(B, 3, H, W, 31, 0.05)
    r = np.random.RandomState(32)
    logp_y = torch.from_numpy(-r.rand(B, Mc, H // 16, W // 16).astype(np.float32) * 3)
    logp_z = torch.from_numpy(-r.rand(B, Mc, H // 64, W // 64).astype(np.float32) * 3)
    assert float(M.scale_terms(x_hat.double(), x.double(), 1.0).min()) > M.MIN_TERM
    ref, ms_img, mse_img, (gy, gz, gx) = _loss_reference(logp_y, logp_z, x_hat, x, lam)

    def device_out():
        cl = torch.channels_last
        return {"logp_y": logp_y.to(dev).contiguous(memory_format=cl).requires_grad_(True),
                "logp_z": logp_z.to(dev).contiguous(memory_format=cl).requires_grad_(True),
                "x_hat": x_hat.to(dev).contiguous(memory_format=cl).requires_grad_(True)}

    out = device_out()
    tx = x.to(dev).contiguous(memory_format=torch.channels_last)
    res = nic.rd_loss_msssim(out, tx, lam)
    res["loss"].backward()
    for k, want in ref.items():
        got = float(res[k])
        print(f"{k}: {got:.8g} (reference {want:.8g})")
        assert isinstance(res[k], float) or k == "loss"
        assert abs(got - want) <= 1e-4 * abs(want), (k, got, want)
    assert float((res["ms_ssim_per_image"].cpu().double() - ms_img).abs().max()) <= M.VALUE_BAND
    assert float((res["mse_per_image"].cpu().double() - mse_img).abs().max()) <= 1e-4 * float(mse_img.max())
    for name, got, want in (("logp_y", out["logp_y"].grad, gy), ("logp_z", out["logp_z"].grad, gz),
                            ("x_hat", out["x_hat"].grad, gx)):
        err = float((got.cpu().double() - want).abs().max()) / float(want.abs().max())
        print(f"d loss / d {name}: {err:.2e} of max|g|")
        assert err <= M.GRAD_BAND, (name, err)
    # sync=False: the same numbers as device tensors, no host value anywhere in the result
    out2 = device_out()
    res2 = nic.rd_loss_msssim(out2, tx, lam, sync=False)
    for k, v in res2.items():
        assert torch.is_tensor(v) and v.is_cuda, k
    assert torch.equal(res2["loss"].detach(), res["loss"].detach())
    for k in ref:
        if k != "loss":
            assert float(res2[k]) == res[k], k


# ---------------------------------------------------------------------------------------------
# one whole training step against the torch-CPU path (the recipe of
# test_gpu_variants.test_full_size_config_step_vs_torch_cpu_path, with the new loss)
# ---------------------------------------------------------------------------------------------
X_HAT_OFFSET = 0.25


def _regular_state(st):
    """A random-weight model reconstructs nothing: its x_hat has mean 0 and no structure in common with x, so the
    MS-SSIM terms are negative or near 0 and the loss sits at (or next to) its undefined point.  A quarter of the last
    layer's weights and a bias put x_hat next to a low-contrast input, where every term is regular (asserted on the
    float64 reference before comparing).

    The bias is 0.25, not the input's mean of 0.5: the structure terms do not see a constant offset of x_hat and the
    luminance term is flat where the means agree, so with equal means the last layer's bias gradient -- the sum of
    d loss / d x_hat over 131,072 pixels -- is what 131,072 cancelling terms leave over: 3e-3 against 0.09 with the
    offset (float64, CPU), and the fp32 evaluation of the ORACLE is then off by 3e-4 of it, 60 % of the band, before any
    device arithmetic (1e-5 with the offset).  A model in training has unequal means; the comparison is made there."""
    st = dict(st)
    st["decoder.net.6.weight"] = (st["decoder.net.6.weight"] * 0.25).astype(np.float32)
    st["decoder.net.6.bias"] = (st["decoder.net.6.bias"] + X_HAT_OFFSET).astype(np.float32)
    return st


def _low_contrast(x):
    return (0.5 + 0.1 * (x - 0.5)).astype(np.float32)


def test_training_step_with_rd_loss_msssim_vs_torch_cpu_path(env):
    nic, F_, dev = env
    from oracle import torch_ref as TR
    from test_gpu_variants import _compare_fp32
    Mc, K, B, H, W, lam, seed = 16, 3, 2, 256, 256, 8.0, 40
    model = nic.JointAutoregressiveHierarchical(Mc, K)
    ks = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    st = _regular_state(R.make_state(ks, seed))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(dev)
    x = _low_contrast(R.make_image(B, H, W, seed + 1))
    uz, uy = R.make_noise((B, Mc, H // 64, W // 64), seed + 2), R.make_noise((B, Mc, H // 16, W // 16), seed + 3)
    tx = torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last)
    out = model(tx, noise=(torch.from_numpy(uz).to(dev), torch.from_numpy(uy).to(dev)))
    res = nic.rd_loss_msssim(out, tx, lam)
    res["loss"].backward()
    torch.cuda.synchronize()
    # the torch-CPU path: oracle/torch_ref's model, TR.ms_ssim in the loss
    P = {}
    for k, v in st.items():
        t = torch.as_tensor(np.asarray(v)).clone()
        if t.is_floating_point() and k.split(".")[-1] not in ("pedestal", "bound", "mask"):
            t.requires_grad_(True)
        P[k] = t
    xt = torch.as_tensor(x)
    t_o = TR.forward(P, xt, Mc, K, "5x5", True, (torch.as_tensor(uz), torch.as_tensor(uy)))
    terms = M.scale_terms(t_o["x_hat"].detach().double(), xt.double(), 1.0)
    assert float(terms.min()) > M.MIN_TERM, terms
    rd = TR.rd_loss(t_o, xt, 0.0)
    t_ms = TR.ms_ssim(t_o["x_hat"], xt, data_range=1.0)
    loss = rd["bpp_total"] + lam * (1.0 - t_ms)
    loss.backward()
    t_grads = {k: v.grad.numpy() for k, v in P.items() if v.requires_grad and v.grad is not None}
    t_loss = {k: float(rd[k]) for k in ("bpp_y", "bpp_z", "bpp_total", "mse", "psnr")}
    t_out = {k: v.detach().numpy() for k, v in t_o.items() if torch.is_tensor(v)}
    assert abs(float(res["loss"]) - float(loss)) <= 1e-4 * abs(float(loss)), (float(res["loss"]), float(loss))
    assert abs(res["ms_ssim"] - float(t_ms)) <= M.VALUE_BAND, (res["ms_ssim"], float(t_ms))
    # the decoder's gradients come from the MS-SSIM term alone: they must be there
    assert float(np.abs(t_grads["decoder.net.6.weight"]).max()) > 0.0
    _compare_fp32(model, out, res, t_out, t_loss, t_grads)


# ---------------------------------------------------------------------------------------------
# the upper layers
# ---------------------------------------------------------------------------------------------
def _regular_model(nic, Mc, K, precision, dev, seed):
    torch.manual_seed(seed)
    m = nic.JointAutoregressiveHierarchical(Mc, K)
    with torch.no_grad():   # (see _regular_state)
        m.decoder.net[6].weight.mul_(0.25)
        m.decoder.net[6].bias.add_(X_HAT_OFFSET)
    m = m.to(dev)
    if precision == "bf16":
        m.set_precision("bf16")
    return m


def _batches(n, B, H, W, seed, dev=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = [0.5 + 0.1 * (torch.rand(B, 3, H, W, generator=g) - 0.5) for _ in range(n)]
    return xs if dev is None else [x.to(dev).contiguous(memory_format=torch.channels_last) for x in xs]


@pytest.mark.parametrize("precision,Mc,K", [("bf16", 128, 3), ("fp32", 64, 1)])
def test_step_plan_with_rd_loss_msssim_equals_eager_training(env, precision, Mc, K):
    """four optimizer steps from the same seed, eager and planned: every loss and every parameter bit for bit (what
    test_gpu_plan.test_step_plan_equals_eager_training asserts for rd_loss)"""
    nic, F_, dev = env
    from neural_image_compression_amd.plan import StepPlan
    B, H, W, lam = 2, 192, 192, 8.0
    xs = _batches(2, B, H, W, 11, dev)

    def build():
        m = _regular_model(nic, Mc, K, precision, dev, 3)
        return m, nic.FusedAdam(m.parameters(), lr=1e-4)

    ma, oa = build()
    torch.cuda.manual_seed(5)
    losses_a, ms_a = [], []
    for i in range(4):
        oa.zero_grad(set_to_none=True)
        res = nic.rd_loss_msssim(ma(xs[i % 2]), xs[i % 2], lam, sync=False)
        res["loss"].backward()
        oa.step()
        losses_a.append(float(res["loss"].detach()))
        ms_a.append(float(res["ms_ssim"]))
    assert min(ms_a) > 0.0, ms_a   # (at 0 the MS-SSIM gradient is defined as 0 and the comparison would say little)

    mb, ob = build()
    plan = StepPlan(mb, nic.rd_loss_msssim, lam, xs[0])
    assert plan.info["memcpys"] == 0 and plan.info["kernels"] > 100, plan.info
    torch.cuda.manual_seed(5)
    losses_b, ms_b = [], []
    for i in range(4):
        out, res = plan.step(xs[i % 2])
        ob.step()
        losses_b.append(float(res["loss"].detach()))
        ms_b.append(float(res["ms_ssim"]))
    assert losses_a == losses_b and ms_a == ms_b, (losses_a, losses_b, ms_a, ms_b)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n
    plan.close()


def test_trainer_with_rd_loss_msssim_eager_and_planned(env):
    nic, F_, dev = env
    from neural_image_compression_amd.trainer import Trainer
    batches = _batches(3, 2, 192, 192, 21)

    class Log:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, value, step))

        def close(self):
            pass

    def run(step_plan):
        m = _regular_model(nic, 128, 3, "bf16", dev, 2)
        log = Log()
        tr = Trainer(m, nic.FusedAdam(m.parameters(), lr=1e-4), batches, rd_loss=nic.rd_loss_msssim, lambda_val=8.0,
                     max_steps=3, checkpoint_path=None, writer=log, step_plan=step_plan, log_interval=100,
                     img_interval=100, val_interval=100)
        tr.log_statistics = False
        torch.cuda.manual_seed(9)
        losses = []
        for x in batches:
            _, results = tr.train_step(x)
            tr._log_scalars(results)
            losses.append(float(results["loss"].detach()))
            assert float(results["ms_ssim"]) > 0.0
        return m, losses, log.rows, tr

    ma, losses_a, rows_a, _ = run(False)
    mb, losses_b, rows_b, trb = run(True)
    assert trb._plan is not None and trb._plan.replays == 3
    assert losses_a == losses_b, (losses_a, losses_b)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n
    # the eight plain numbers of rd_loss are logged by both; the eager step logs ms_ssim as a ninth
    common = [r for r in rows_a if r[0] != "losses/ms_ssim"]
    assert common == rows_b and len(rows_b) == 3 * 8 and len(rows_a) == 3 * 9


def test_evaluator_with_rd_loss_msssim_reports_the_reference_keys(env, tmp_path):
    nic, F_, dev = env
    from neural_image_compression_amd.evaluator import CompressionEvaluator
    model = _regular_model(nic, 16, 3, "fp32", dev, 6)
    batches = _batches(2, 1, 192, 256, 8)
    ev = CompressionEvaluator(model, batches, dev, 8.0, save_dir=str(tmp_path))
    rep_ms, ins, recs = ev.evaluate(nic.rd_loss_msssim)
    rep_mse, _, _ = ev.evaluate(nic.rd_loss)
    assert list(rep_ms) == list(rep_mse)
    for k in ("BPP", "BPP(y)", "BPP(z)", "BPP(total)", "MS-SSIM(RGB)", "PSNR(RGB)"):
        assert k in rep_ms, k
    for k in rep_mse:   # the rates and the metrics do not depend on which loss reported them
        assert abs(rep_ms[k] - rep_mse[k]) <= 1e-6 * abs(rep_mse[k]), k
    assert len(ins) == 2 and len(recs) == 2
