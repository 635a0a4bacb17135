"""The rate-level model (`rate_levels=Q`) on the GPU.

  * tables at zero: every gain is exp(0) = 1 and v * 1 = v, so at any quality the out-dict and the gradients of all
    shared parameters are bit for bit those of the plain model with the same weights (fp32 and bf16, both contexts);
  * random tables, fixed noise: against a composition that scales with torch ops (the four stacks of a plain model
    wrapped: encoder(x) * g_y, hyper_encoder(.) * g_z, hyper_decoder(. * ig_z), decoder(. * ig_y)) and runs everything
    else through the existing modules -- forward tensors bit for bit, every gradient within 5e-4 of its tensor's maximum
    (the project's gradient band; the two sides differ in the order of a few fp32 sums);
  * quality as a float and as a constant [B] tensor: the same bits; a mixed [B] tensor: the per-image runs;
  * three Trainer steps over two rate points.

M = 16 in fp32 and 64 in bf16, the smallest widths of the existing model tests; x is 2 x 3 x 64 x 64.

Run on the MI355X box:  python -m pytest tests/test_gpu_rate_model.py -m gpu -q"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_recipe as R

pytestmark = pytest.mark.gpu

WIDTH = {"fp32": 16, "bf16": 64}
CASES = [(prec, ctx) for prec in ("fp32", "bf16") for ctx in ("raster", "checkerboard")]
TABLES = ("log_gain_y", "log_inv_gain_y", "log_gain_z", "log_inv_gain_z")
Q, LAM, SIZE = 3, 0.01, (2, 64, 64)
OUT_KEYS = ["x_hat", "y", "y_in", "z", "z_in", "p_z", "logp_z", "p_y", "logp_y", "training"]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, torch.device("cuda:0")


def _state(model, seed):
    """golden_recipe's state for the model's keys; the mask buffer stays the model's own"""
    own = model.state_dict()
    st = R.make_state([(k, tuple(v.shape)) for k, v in own.items() if k not in TABLES], seed)
    return {k: (own[k].numpy().copy() if k.endswith(".mask") else v) for k, v in st.items()}


def _tables(M, seed):
    """log gains within +-0.7: gains between 0.5 and 2"""
    r = np.random.RandomState(seed)
    return {k: r.uniform(-0.7, 0.7, (Q, M)).astype(np.float32) for k in TABLES}


def _build(nic, dev, prec, ctx, K=1, rate_levels=None, tables=None, seed=61):
    model = nic.JointAutoregressiveHierarchical(WIDTH[prec], K, context=ctx, rate_levels=rate_levels)
    st = _state(model, seed)
    if rate_levels is not None and tables is not None:
        st.update(tables)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=tables is not None or rate_levels is None)
    model = model.to(dev)
    if prec == "bf16":
        model.set_precision("bf16")
    return model


def _inputs(M, dev, size=SIZE):
    B, H, W = size
    cl = lambda a: torch.from_numpy(a).to(dev).contiguous(memory_format=torch.channels_last)
    return cl(R.make_image(B, H, W, 62)), (cl(R.make_noise((B, M, H // 64, W // 64), 63)),
                                           cl(R.make_noise((B, M, H // 16, W // 16), 64)))


def _step(nic, model, x, noise, **kw):
    out = model(x, noise=noise, **kw)
    nic.rd_loss(out, x, LAM)["loss"].backward()
    torch.cuda.synchronize()
    return out, {n: p.grad for n, p in model.named_parameters()}


def _same_tensors(a, b, keys):
    for k in keys:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _param_keys(out):
    return [k for k in ("mu", "sigma", "weights", "mus", "sigmas") if k in out]


@pytest.mark.parametrize("q", [0.0, 1.3])
@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_zero_tables_are_the_plain_model_bit_for_bit(env, prec, ctx, q):
    nic, dev = env
    plain = _build(nic, dev, prec, ctx, K=3)
    rated = _build(nic, dev, prec, ctx, K=3, rate_levels=Q)
    assert all(not getattr(rated, k).any() for k in TABLES)
    x, noise = _inputs(plain.M, dev)
    out_p, grads_p = _step(nic, plain, x, noise)
    out_r, grads_r = _step(nic, rated, x, noise, quality=q)
    assert len(out_p) == 13 and list(out_r) == list(out_p) + ["quality"] and out_r["quality"] == q
    _same_tensors(out_r, out_p, list(out_p))
    assert set(grads_r) == set(grads_p) | set(TABLES)
    worst = {n: float((grads_r[n] - grads_p[n]).abs().max() / grads_p[n].abs().max().clamp_min(1e-30))
             for n in grads_p if not torch.equal(grads_r[n], grads_p[n])}
    print(f"{prec} {ctx} q={q}: {len(worst)} of {len(grads_p)} gradients differ, worst relative {max(worst.values(), default=0):.3e}")
    assert not worst, worst
    for k in TABLES:
        assert grads_r[k] is not None and bool(torch.isfinite(grads_r[k]).all())


class _Scaled(nn.Module):
    """a stack of the plain model with a per-channel scale (rows [1 or B][M], torch ops) behind or in front of it;
    everything else of the stack -- `precision`, `out_f32`, `net` -- is the inner module's"""

    def __init__(self, inner, rows, behind):
        super().__init__()
        self.inner, self.rows_fn, self.behind = inner, rows, behind

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__("inner"), name)

    def forward(self, t, **kw):
        s = self.rows_fn()[:, :, None, None]
        return self.inner(t, **kw) * s if self.behind else self.inner(t * s, **kw)


def _composition(nic, dev, prec, ctx, rated, q):
    """the plain model with `rated`'s weights, its four stacks wrapped -> (model, {table name: its own copy})"""
    ref = _build(nic, dev, prec, ctx)
    ref.load_state_dict({k: v for k, v in rated.state_dict().items() if k not in TABLES})
    own = {k: nn.Parameter(getattr(rated, k).detach().clone()) for k in TABLES}
    qs = rated.check_quality(q, SIZE[0])
    row = lambda k: (lambda: rated.gain_rows(qs, own[k])[0])
    ref.encoder = _Scaled(ref.encoder, row("log_gain_y"), True)
    ref.hyper_encoder = _Scaled(ref.hyper_encoder, row("log_gain_z"), True)
    ref.hyper_decoder = _Scaled(ref.hyper_decoder, row("log_inv_gain_z"), False)
    ref.decoder = _Scaled(ref.decoder, row("log_inv_gain_y"), False)
    ref.use_step_prep = rated.use_step_prep
    return ref, own


@pytest.mark.parametrize("q", [0.5, torch.tensor([0.25, 2.0])], ids=["q0.5", "q[0.25,2]"])
@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_random_tables_against_the_torch_composition(env, prec, ctx, q):
    nic, dev = env
    rated = _build(nic, dev, prec, ctx, rate_levels=Q, tables=_tables(WIDTH[prec], 5))
    ref, own = _composition(nic, dev, prec, ctx, rated, q)
    x, noise = _inputs(rated.M, dev)
    out, grads = _step(nic, rated, x, noise, quality=q)
    out_ref, grads_ref = _step(nic, ref, x, noise)
    _same_tensors(out, out_ref, OUT_KEYS + _param_keys(out_ref))
    grads_ref = {n.replace(".inner.", "."): g for n, g in grads_ref.items()}
    grads_ref.update({k: p.grad for k, p in own.items()})
    assert set(grads) == set(grads_ref)
    for n, g in grads.items():
        scale = float(grads_ref[n].abs().max())
        err = float((g - grads_ref[n]).abs().max())
        if n in TABLES:
            print(f"{prec} {ctx} {n}: err / (5e-4 max) = {err / max(5e-4 * scale, 1e-300):.4f}")
            assert scale > 0, n
        assert err <= 5e-4 * scale, (n, err, scale)


@pytest.mark.parametrize("prec,ctx", CASES, ids=str)
def test_float_and_constant_tensor_quality_give_the_same_bits(env, prec, ctx):
    nic, dev = env
    rated = _build(nic, dev, prec, ctx, rate_levels=Q, tables=_tables(WIDTH[prec], 6))
    x, noise = _inputs(rated.M, dev)
    out_f, grads_f = _step(nic, rated, x, noise, quality=1.25)
    for p in rated.parameters():
        p.grad = None
    out_t, grads_t = _step(nic, rated, x, noise, quality=torch.tensor([1.25, 1.25]))
    _same_tensors(out_f, out_t, OUT_KEYS + _param_keys(out_f))
    for n in grads_f:
        if n not in TABLES:            # (the tables' own gradients: one row summed over the batch, or two rows added)
            assert torch.equal(grads_f[n], grads_t[n]), n


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("ctx", ["raster", "checkerboard"])
def test_mixed_qualities_are_the_per_image_runs(env, ctx, training):
    nic, dev = env
    rated = _build(nic, dev, "fp32", ctx, rate_levels=Q, tables=_tables(WIDTH["fp32"], 7))
    x, (uz, uy) = _inputs(rated.M, dev)
    qs = [0.5, 2.0]
    with torch.no_grad():
        both = rated(x, training=training, noise=(uz, uy), quality=torch.tensor(qs))
        for b, q in enumerate(qs):
            one = rated(x[b:b + 1], training=training, noise=(uz[b:b + 1], uy[b:b + 1]), quality=q)
            for k in OUT_KEYS + _param_keys(one):
                if torch.is_tensor(one[k]):
                    assert torch.equal(both[k][b:b + 1], one[k]), (k, b)
    if not training:
        assert torch.equal(both["y_in"], torch.round(both["y"])) and torch.equal(both["z_in"], torch.round(both["z"]))


def test_evaluation_mode_has_no_gradient_through_the_rounding_but_through_the_gain(env):
    nic, dev = env
    rated = _build(nic, dev, "fp32", "raster", rate_levels=Q, tables=_tables(16, 8))
    x, _ = _inputs(16, dev)
    out = rated(x, training=False, quality=1.0)
    (g_in,) = torch.autograd.grad(out["y_in"].sum(), rated.log_gain_y, allow_unused=True, retain_graph=True)
    assert g_in is None or float(g_in.abs().max()) == 0.0                   # rint: zero, as _QuantizeFn's
    (g_vg,) = torch.autograd.grad(out["y"].sum(), rated.log_gain_y)
    assert float(g_vg.abs().max()) > 0                                       # the gained latent itself: it flows


def test_padded_forward_takes_the_quality(env):
    nic, dev = env
    rated = _build(nic, dev, "fp32", "raster", rate_levels=Q, tables=_tables(16, 9))
    img = torch.from_numpy(R.make_image(1, 80, 120, 3)).to(dev)
    out = nic.padded_forward(rated, img, quality=0.5)
    assert out["x_hat"].shape == img.shape and out["quality"] == 0.5 and out["padded_hw"] == (128, 128)
    with pytest.raises(ValueError, match="needs `quality`"):
        nic.padded_forward(rated, img)
    with pytest.raises(ValueError, match="outside"):
        nic.padded_forward(rated, img, quality=2.5)


def test_trainer_steps_over_two_rate_points(env, tmp_path):
    nic, dev = env
    from neural_image_compression_amd.trainer import Trainer
    rated = _build(nic, dev, "fp32", "raster", rate_levels=Q, tables=_tables(16, 10))
    x, _ = _inputs(16, dev)
    points = [(0.0, 0.002), (2.0, 0.05)]
    kw = dict(rd_loss=nic.rd_loss, rate_points=points, rate_seed=1, max_steps=3, device="cuda:0", writer=None,
              log_dir=str(tmp_path / "log"), checkpoint_path=str(tmp_path / "ck.pth"), log_interval=100, val_interval=100)
    tr = Trainer(rated, nic.FusedAdam(rated.parameters(), lr=1e-4), [x.cpu()], **kw)
    before = {k: getattr(rated, k).detach().clone() for k in TABLES}
    drawn = []
    for _ in range(3):
        out, res = tr.train_step(tr._next_batch())
        drawn.append(tr.last_rate_point)
        assert out["quality"] == tr.last_rate_point[0] and np.isfinite(float(res["loss"].detach()))
        for k in TABLES:
            g = getattr(rated, k).grad
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert set(drawn) == set(points)                                         # this seed draws both within three steps
    assert all(not torch.equal(before[k], getattr(rated, k).detach()) for k in TABLES)
    tr.val_loader = [x.cpu()]
    assert np.isfinite(tr.validate())
    tr.save_checkpoint()
    state = torch.load(str(tmp_path / "ck.pth"), map_location="cpu")
    assert set(TABLES) <= set(state["model"]) and "rate_rng" in state
    want = [tr._rate_rng.choice(points) for _ in range(8)]
    again = Trainer(rated, nic.FusedAdam(rated.parameters(), lr=1e-4), [x.cpu()], resume=True, **dict(kw, rate_seed=77))
    assert [again._rate_rng.choice(points) for _ in range(8)] == want
