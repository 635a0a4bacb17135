"""The checkerboard context model (`context="checkerboard"`) on the GPU: phi = masked_conv(anchor(y_in)) against the
float64 statement of checker_ref.py, phi = bias at the anchors, the independence the two-pass format rests on, the
gradients of a whole training step against torch-CPU float64 autograd of the forward restated below, plan.StepPlan
against the eager step, and the raster model bit for bit what the default constructor builds.

Tolerances are the existing ones.  fp32 phi: 1e-4 |ref| + 1e-5, test_gpu_parity.test_masked_conv_golden's.  bf16 phi
(a bf16 slice of the entropy-parameter MLP's input): A_BAND * S + 2^-8 |ref| against the float64 convolution of the
bf16-rounded operands, test_gpu_latent_bf16's band for a bf16 slice.  fp32 gradients: 3e-4 * max(|ref|max, rms) + 1e-7,
what test_gpu_parity.test_model_vs_oracle holds every gradient of a training step to.  bf16 gradients: cosine >= 0.98,
test_gpu_bf16.test_model_bf16_vs_fp32's statement.  fp32 runs at M = 16 and bf16 at M = 64, the smallest widths the
existing fp32 / bf16 model tests use.

Run on the MI355X box:  python -m pytest tests/test_gpu_checker_model.py -m gpu -q"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import checker_ref as CR
import conv_bf16_ref as RB
import golden_recipe as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 64, 64), (2, 64, 128)]                    # latent 4 x 4 and 4 x 8
CASES = [(prec, K, size) for prec in ("fp32", "bf16") for K in (1, 3) for size in SIZES]
WIDTH = {"fp32": 16, "bf16": 64}
LAM = 0.01


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, torch.device("cuda:0")


def _state(model, seed):
    """golden_recipe's state for the model's keys; the mask buffer stays the model's own (the recipe writes type A)"""
    own = model.state_dict()
    st = R.make_state([(k, tuple(v.shape)) for k, v in own.items()], seed)
    return {k: (own[k].numpy().copy() if k.endswith(".mask") else v) for k, v in st.items()}


def _model(nic, dev, prec, K, context="checkerboard", seed=61):
    model = nic.JointAutoregressiveHierarchical(WIDTH[prec], K, context=context)
    st = _state(model, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    model = model.to(dev)
    if prec == "bf16":
        model.set_precision("bf16")
    return model, st


def _inputs(M, size, dev):
    B, H, W = size
    x = R.make_image(B, H, W, 62)
    uz, uy = R.make_noise((B, M, H // 64, W // 64), 63), R.make_noise((B, M, H // 16, W // 16), 64)
    cl = lambda a: torch.from_numpy(a).to(dev).contiguous(memory_format=torch.channels_last)
    return x, uz, uy, cl(x), cl(uz), cl(uy)


def _forward_with_phi(model, tx, noise, training=True):
    """-> (out, what the context model was given, what it returned)"""
    seen = {}
    hook = model.context_model.register_forward_hook(lambda mod, args, res: seen.update(inp=args[0], phi=res))
    try:
        out = model(tx, training=training, noise=noise)
    finally:
        hook.remove()
    return out, seen["inp"], seen["phi"]


def _host(t):
    return t.detach().float().cpu().contiguous().numpy()


@functools.lru_cache(maxsize=None)
def _run(prec, K, size):
    """one training forward + backward on the device, shared by the tests of a case (nothing below changes it)"""
    import neural_image_compression_amd as nic
    dev = torch.device("cuda:0")
    model, st = _model(nic, dev, prec, K)
    x, uz, uy, tx, tuz, tuy = _inputs(model.M, size, dev)
    out, inp, phi = _forward_with_phi(model, tx, (tuz, tuy))
    out["y"].retain_grad()
    nic.rd_loss(out, tx, LAM)["loss"].backward()
    mc = model.context_model.masked
    return dict(model=model, st=st, x=x, uz=uz, uy=uy, y_in=_host(out["y_in"]), inp=_host(inp), phi=_host(phi),
                weight=_host(mc.weight), bias=_host(mc.bias), dy=_host(out["y"].grad), dweight=_host(mc.weight.grad),
                inp_bf16=None if getattr(inp, "_lic_bf16", None) is None else inp._lic_bf16[1].float().cpu().numpy())


@pytest.mark.parametrize("prec,K,size", CASES, ids=str)
def test_phi_is_the_masked_conv_of_the_anchors(env, prec, K, size):
    r = _run(prec, K, size)
    assert (r["inp"].view(np.int32) == CR.anchor(r["y_in"]).view(np.int32)).all()      # anchor(y_in), +0.0 elsewhere
    dead = CR.mask(5) == 0
    assert np.abs(r["weight"][:, :, dead]).max() == 0                                  # masked in place
    if prec == "fp32":
        ref = CR.phi(r["y_in"], r["weight"], r["bias"])
        err, tol = np.abs(r["phi"] - ref), 1e-4 * np.abs(ref) + 1e-5
        print(f"FIGURE phi {prec} K{K} {size} worst err/tol {float((err / tol).max()):.4f}")
        assert (err <= tol).all(), float((err / tol).max())
        return
    # bf16: the kernel multiplies the bf16 copy of anchor(y_in), which the quantisation launch wrote, by bf16 weights
    assert r["inp_bf16"] is not None, "the quantisation launch attached no bf16 copy of anchor(y_in)"
    x16 = torch.from_numpy(r["inp_bf16"]).permute(0, 3, 1, 2)
    assert torch.equal(x16, RB.to_bf16_exact(r["inp"]))
    ref = RB.conv_ref(x16, RB.to_bf16_exact(r["weight"]), torch.from_numpy(r["bias"]), 5, 1, 2, tap_mask=CR.tap_mask(5))
    err = (RB.f64(r["phi"]) - ref.y).abs()
    tol = RB.A_BAND * ref.S + 2.0 ** -8 * ref.y.abs()
    print(f"FIGURE phi {prec} K{K} {size} worst err/tol {float((err / tol).max()):.4f}")
    assert bool((err <= tol).all()), float((err / tol).max())


@pytest.mark.parametrize("K,size", [(K, s) for K in (1, 3) for s in SIZES], ids=str)
def test_phi_at_the_anchors_is_the_bias_exactly(env, K, size):
    r = _run("fp32", K, size)
    anc = CR.is_anchor(*r["phi"].shape[2:])
    want = np.broadcast_to(r["bias"][None, :, None, None], r["phi"].shape)
    assert (r["phi"].view(np.int32)[:, :, anc] == np.ascontiguousarray(want).view(np.int32)[:, :, anc]).all()
    assert (r["phi"][:, :, ~anc] != want[:, :, ~anc]).any()


@pytest.mark.parametrize("prec,K,size", [c for c in CASES if c[2] == SIZES[1]], ids=str)
def test_phi_depends_on_the_anchors_alone(env, prec, K, size):
    """the property the format rests on: no non-anchor value reaches phi, and an anchor reaches only the non-anchors
    of its 5 x 5 neighbourhood"""
    nic, dev = env
    r = _run(prec, K, size)
    model = r["model"]
    _, _, _, tx, tuz, tuy = _inputs(model.M, size, dev)
    h, w = r["phi"].shape[2:]
    anc = CR.is_anchor(h, w)
    bits = lambda a: a.view(np.int32 if a.dtype == np.float32 else np.int16)
    with torch.no_grad():
        # every non-anchor at once, then one alone: another noise value there is another y_in there
        for where in (~anc, np.isin(np.arange(h * w).reshape(h, w), [1])):
            assert not anc[where].any()
            u2 = tuy.clone()
            u2[:, :, torch.from_numpy(where).to(dev)] = 0.987
            out, _, phi = _forward_with_phi(model, tx, (tuz, u2))
            assert (_host(out["y_in"])[:, :, where] != r["y_in"][:, :, where]).all()
            assert (bits(_host(phi)) == bits(r["phi"])).all()
        for i0, j0 in ((0, 0), (2, 4), (3, 7)):
            assert anc[i0, j0]
            u2 = tuy.clone()
            u2[:, :, i0, j0] = 0.987
            _, _, phi = _forward_with_phi(model, tx, (tuz, u2))
            changed = (bits(_host(phi)) != bits(r["phi"])).any(axis=(0, 1))
            i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            allowed = ~anc & (np.abs(i - i0) <= 2) & (np.abs(j - j0) <= 2)
            assert changed.any() and not (changed & ~allowed).any(), (i0, j0, changed)


def _reference_step(st, x, uz, uy, M, K):
    """the training step restated on the CPU in float64 with torch autograd: the reference's forward (oracle.torch_ref's
    stacks and likelihoods) with phi = conv(anchor(y_in), weight * checkerboard mask) -> (dL/dy, d context weight)"""
    from oracle import torch_ref as TR
    P = {}
    for k, v in st.items():
        t = torch.from_numpy(np.array(v))
        t = t.double() if t.is_floating_point() else t
        if t.is_floating_point() and k.split(".")[-1] not in ("pedestal", "bound", "mask"):
            t.requires_grad_(True)
        P[k] = t
    xt, uz, uy = (torch.from_numpy(a).double() for a in (x, uz, uy))
    y = TR.encoder(xt, P, "5x5")
    y.retain_grad()
    z = TR.hyper_encoder(y, P, "5x5")
    z_in, y_in = z + (uz - 0.5), y + (uy - 0.5)
    psi = TR.hyper_decoder(z_in, P, "5x5")
    wt = P["context_model.masked.weight"]
    with torch.no_grad():
        wt.mul_(torch.from_numpy(CR.mask(5)))              # in place, outside autograd: the gradient is not masked
    anc = torch.from_numpy(CR.is_anchor(y.shape[2], y.shape[3]))
    phi = TF.conv2d(torch.where(anc, y_in, torch.zeros((), dtype=torch.float64)), wt, P["context_model.masked.bias"],
                    padding=2)
    hdn = torch.cat([phi, psi], dim=1)
    ep = "entropy_parameters.net."
    hdn = TR._lrelu(TR._conv(hdn, P, ep + "0", 1, 0))
    hdn = TR._lrelu(TR._conv(hdn, P, ep + "2", 1, 0))
    raw = TR._conv(hdn, P, ep + "4", 1, 0)
    if K == 1:
        mu, sg = raw.chunk(2, dim=1)
        sg = TF.softplus(sg) + 1e-6
        p_y = TR._gcdf((y_in + 0.5 - mu) / sg) - TR._gcdf((y_in - 0.5 - mu) / sg)
    else:
        B, _, hh, ww = raw.shape
        wk, mus, sgs = (t.reshape(B, K, M, hh, ww) for t in raw.chunk(3, dim=1))
        wk, sgs, xe = TF.softmax(wk, dim=1), TF.softplus(sgs) + 1e-6, y_in.unsqueeze(1)
        p_y = (wk * (TR._gcdf((xe + 0.5 - mus) / sgs) - TR._gcdf((xe - 0.5 - mus) / sgs))).sum(dim=1)
    p_y = p_y.clamp_min(1e-9)
    p_z = TR._factorized(z_in, P).clamp_min(1e-9)
    out = {"x_hat": TR.decoder(y_in, P, "5x5"), "logp_y": torch.log(p_y), "logp_z": torch.log(p_z)}
    TR.rd_loss(out, xt, LAM)["loss"].backward()
    return y.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("prec,K,size", CASES, ids=str)
def test_gradients_against_float64_autograd(env, prec, K, size):
    r = _run(prec, K, size)
    dy, dw = _reference_step(r["st"], r["x"], r["uz"], r["uy"], r["model"].M, K)
    dead = CR.mask(5) == 0
    assert np.abs(dw[:, :, dead]).max() > 0 and np.abs(r["dweight"][:, :, dead]).max() > 0     # not masked
    for what, got, ref in (("dL/dy", r["dy"], dy), ("context weight gradient", r["dweight"], dw)):
        if prec == "fp32":
            scale = max(np.abs(ref).max(), np.sqrt((ref ** 2).mean()), 1e-12)
            err = np.abs(got - ref).max()
            print(f"FIGURE {what} {prec} K{K} {size} err / (3e-4 scale + 1e-7) = {err / (3e-4 * scale + 1e-7):.4f}")
            assert err <= 3e-4 * scale + 1e-7, (what, err, scale)
        else:
            a, b = got.astype(np.float64).ravel(), ref.ravel()
            cs = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))
            print(f"FIGURE {what} {prec} K{K} {size} cosine {cs:.6f}")
            assert cs >= 0.98, (what, cs)


def test_evaluation_mode_rounds_and_has_no_gradient_through_the_rounding(env):
    nic, dev = env
    model, _ = _model(nic, dev, "fp32", 1)
    _, _, _, tx, _, _ = _inputs(model.M, SIZES[1], dev)
    out, inp, phi = _forward_with_phi(model, tx, None, training=False)
    assert torch.equal(out["y_in"], torch.round(out["y"]))
    assert (_host(inp).view(np.int32) == CR.anchor(_host(out["y_in"])).view(np.int32)).all()
    (gy,) = torch.autograd.grad(phi.sum() + out["y_in"].sum(), out["y"], allow_unused=True)
    assert gy is None or float(gy.abs().max()) == 0.0


def test_the_residual_model_takes_the_checkerboard_context(env):
    """HierarchicalMixtureResidual shares the latent side: the same three statements about phi, and a finite backward"""
    nic, dev = env
    model = nic.HierarchicalMixtureResidual(16, 3, context="checkerboard")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _state(model, 81).items()})
    model = model.to(dev)
    _, _, _, tx, tuz, tuy = _inputs(16, SIZES[1], dev)
    out, inp, phi = _forward_with_phi(model, tx, (tuz, tuy))
    nic.rd_loss(out, tx, LAM)["loss"].backward()
    mc = model.context_model.masked
    y_in, phi, bias = _host(out["y_in"]), _host(phi), _host(mc.bias)
    assert (_host(inp).view(np.int32) == CR.anchor(y_in).view(np.int32)).all()
    ref = CR.phi(y_in, _host(mc.weight), bias)
    assert (np.abs(phi - ref) <= 1e-4 * np.abs(ref) + 1e-5).all()
    anc = CR.is_anchor(*phi.shape[2:])
    want = np.ascontiguousarray(np.broadcast_to(bias[None, :, None, None], phi.shape))
    assert (phi.view(np.int32)[:, :, anc] == want.view(np.int32)[:, :, anc]).all()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert float(mc.weight.grad[:, :, torch.from_numpy(CR.mask(5) == 0)].abs().max()) > 0


def test_step_plan_is_the_eager_step(env):
    """two optimizer steps from the same seed, eager and planned (fp32): every loss and parameter bit for bit"""
    nic, dev = env
    from neural_image_compression_amd.plan import StepPlan
    g = torch.Generator(device="cpu").manual_seed(11)
    xs = [torch.rand(2, 3, 64, 64, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for _ in range(2)]

    def build():
        torch.manual_seed(3)
        m = nic.JointAutoregressiveHierarchical(16, 1, context="checkerboard").to(dev)
        return m, nic.FusedAdam(m.parameters(), lr=1e-3)

    ma, oa = build()
    torch.cuda.manual_seed(5)
    losses_a = []
    for i in range(2):
        oa.zero_grad(set_to_none=True)
        res = nic.rd_loss(ma(xs[i]), xs[i], LAM, sync=False)
        res["loss"].backward()
        oa.step()
        losses_a.append(float(res["loss"].detach()))
    mb, ob = build()
    plan = StepPlan(mb, nic.rd_loss, LAM, xs[0], tune=False)
    torch.cuda.manual_seed(5)
    losses_b = []
    for i in range(2):
        _, res = plan.step(xs[i])
        ob.step()
        losses_b.append(float(res["loss"].detach()))
    plan.close()
    assert losses_a == losses_b, (losses_a, losses_b)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_raster_is_the_default_constructor_bit_for_bit(env, prec):
    nic, dev = env
    M = WIDTH[prec]
    a = nic.JointAutoregressiveHierarchical(M, 3)
    b = nic.JointAutoregressiveHierarchical(M, 3, context="raster")
    st = _state(a, 71)
    grads = []
    _, _, _, tx, tuz, tuy = _inputs(M, SIZES[1], dev)
    outs = []
    for m in (a, b):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        m.to(dev)
        if prec == "bf16":
            m.set_precision("bf16")
        out = m(tx, noise=(tuz, tuy))
        nic.rd_loss(out, tx, LAM)["loss"].backward()
        outs.append(out)
        grads.append({n: p.grad for n, p in m.named_parameters()})
    assert list(outs[0]) == list(outs[1])
    for k in outs[0]:
        if torch.is_tensor(outs[0][k]):
            assert torch.equal(outs[0][k], outs[1][k]), k
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
