"""The kernels around the MFMA ones -- entropy-parameter activation, Gaussian / mixture and factorised likelihoods,
the rate-distortion reduction, column sums, the small elementwise kernels, Adam, the logging kernels -- each against
a float64 CPU reference of the same operation (tests/ref64.py, pinned to the reference's fixtures by
tests/test_ref64.py) at the sizes they train at: more lanes than one grid holds (`ew_grid` caps at 2048 x 256),
real M / K, several loop trips per workgroup, ragged ends, unaligned pointers.

Bands are the project's (tests/test_oracle_golden.py, tests/test_gpu_parity.py, tests/test_gpu_optim.py); the one
derived band (mixture-weight gradient) is ref64.dw_band.  Every figure is printed before it is asserted.
Run on the MI355X box:  python -m pytest tests/test_gpu_latent_ops.py -m gpu -q -s"""
import functools

import numpy as np
import pytest
import torch

import ref64
from ref64 import close, close_norm, wide

pytestmark = pytest.mark.gpu

BIG = 4 * 600_000                      # more 4-element groups than one grid of 2048 x 256 lanes covers
TAILS = [BIG, BIG + 1, BIG + 2, BIG + 3]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    L.load()  # must be the in-tree HIP extension; raises if missing
    return nic, F_, L, torch.device("cuda:0")


def place(t, dev, fmt, grad=False):
    t = t.to(dev)
    t = t.contiguous(memory_format=torch.channels_last) if fmt == "nhwc" else t.contiguous()
    return t.requires_grad_(grad)


def cpu(t):
    return None if t is None else t.detach().cpu().contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def offset_by_one(t, dev):
    """a device copy of the flat fp32 tensor `t` that starts one float after a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)
    v = buf[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------
# Gaussian / mixture likelihood and the entropy-parameter activation
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _gmm_ref(case):
    B, M, h, w, K, seed = case
    x, params, _, _ = ref64.gmm_inputs(*case)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    p, logp, p_raw, grads = ref64.gmm_reference(x, params, K, gp, glogp)
    return x, params, gp, glogp, (p, logp, grads, p_raw)


@pytest.mark.parametrize("fmt", ["nhwc", "nchw"])
@pytest.mark.parametrize("case", ref64.GMM_CASES, ids=ref64.gmm_id)
def test_gmm_likelihood_vs_float64(env, case, fmt):
    """p, logp, dx, dparams of functional.gmm_likelihood with cotangents on logp only, on p only and on both.
    Gradients (and logp) are compared where p > 2e-3, exact zeros are required where the float64 likelihood is below
    bound / 4; tests/test_ref64.py asserts that this leaves out at most 2 % of the elements (measured: 0.12 % for
    K = 1, 0.60 % for K = 3, plus the 0.5 % generated clamped elements) and that none is near the bound."""
    nic, F_, L, dev = env
    B, M, h, w, K, seed = case
    x, params, gp, glogp, ref = _gmm_ref(case)
    tx, tp = place(x, dev, fmt, True), place(params, dev, fmt, True)
    dgp, dgl = place(gp, dev, fmt), place(glogp, dev, fmt)
    p, logp = F_.gmm_likelihood(tx, tp, K)
    grads = {}
    for mode, outs, cots in (("logp", [logp], [dgl]), ("p", [p], [dgp]), ("both", [p, logp], [dgp, dgl])):
        dx, dpar = torch.autograd.grad(outs, [tx, tp], cots, retain_graph=True)
        grads[mode] = (cpu(dx), cpu(dpar))
    report = {}
    try:
        ref64.check_gmm((cpu(p), cpu(logp), grads), ref, K, M, 0.5, f"{ref64.gmm_id(case)}/{fmt}", report)
    finally:
        print(ref64.gmm_id(case), fmt, {k: round(v, 3) for k, v in report.items()})


@pytest.mark.parametrize("fmt", ["nhwc", "nchw"])
@pytest.mark.parametrize("case", ref64.GMM_CASES, ids=ref64.gmm_id)
def test_entropy_params_activation_vs_float64(env, case, fmt):
    """every output of functional.entropy_params_activation at the fixture band (1e-4 relative + 1e-6) and its input
    gradient by close_norm at 1e-4, with softplus on both sides of its v > 20 switch"""
    nic, F_, L, dev = env
    B, M, h, w, K, seed = case
    raw = ref64.entropy_raw(B, M, h, w, K, seed)
    cot = ref64.cotangents(raw.shape, seed + 51)[0]
    r64 = wide(raw).requires_grad_(True)
    out64 = ref64.entropy_params(r64, M, K)
    (draw64,) = torch.autograd.grad(out64, r64, wide(cot))
    traw = place(raw, dev, fmt, True)
    out = F_.entropy_params_activation(traw, M, K)
    (draw,) = torch.autograd.grad(out, traw, place(cot, dev, fmt))
    print(ref64.gmm_id(case), fmt, "out", ref64.band_ratio(cpu(out), out64, 1e-4, 1e-6), "of its band, draw",
          ref64.norm_err(cpu(draw), draw64), "of its maximum")
    close(cpu(out), out64, 1e-4, 1e-6, "activated parameters")
    close_norm(cpu(draw), draw64, 1e-4, "draw")


# ---------------------------------------------------------------------------------------------
# factorised bottleneck
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", ref64.FE_CASES, ids=["x".join(map(str, c[0])) for c in ref64.FE_CASES])
def test_factorized_likelihood_vs_float64(env, shape, seed):
    """functional.factorized_likelihood: p, logp, dx and the eleven parameter gradients, cotangent on logp only (the
    training step's) and on both outputs; P = 512 and 1024 run several trips of the backward kernel's pixel loop with
    all four waves, P = 585 a ragged last trip, the 3-D input the non-4-D branch"""
    nic, F_, L, dev = env
    state = ref64.fe_state(shape[1], seed)
    x = ref64.fe_inputs(shape, seed)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    fmt = "nhwc" if len(shape) == 4 else "nchw"
    tx = place(x, dev, fmt, True)
    groups = [[t.to(dev).requires_grad_(True) for t in grp] for grp in state]
    flat = [t for grp in groups for t in grp]
    p, logp = F_.factorized_likelihood(tx, *groups)
    names = [f"{n}.{i}" for n, grp in zip(("matrices", "biases", "factors"), groups) for i in range(len(grp))]
    for mode, outs, cots, rp, rl in (("logp", [logp], [glogp], None, glogp), ("both", [p, logp], [gp, glogp], gp, glogp)):
        p64, logp64, dx64, gr64 = ref64.fe_reference(x, state, rp, rl)
        got = torch.autograd.grad(outs, [tx] + flat, [place(c, dev, fmt) for c in cots], retain_graph=True)
        errs = {"dx": ref64.norm_err(cpu(got[0]), dx64)}
        errs.update({n: ref64.norm_err(cpu(g), r) for n, g, r in zip(names, got[1:], gr64)})
        print(shape, mode, "p", ref64.band_ratio(cpu(p), p64, 1e-4, 1.5e-7), "logp",
              ref64.band_ratio(cpu(logp), logp64, 1e-4, 1e-6), "of their bands; gradients, of their maxima:",
              {k: f"{v:.1e}" for k, v in errs.items()})
        close(cpu(p), p64, 1e-4, 1.5e-7, "p")
        close(cpu(logp), logp64, 1e-4, 1e-6, "logp")
        for k, v in errs.items():
            assert v <= 1e-4, (mode, k, v)


# ---------------------------------------------------------------------------------------------
# rate-distortion loss
# ---------------------------------------------------------------------------------------------
# (B, H, W, M, x_hat offset by one float)
RD_CASES = [(32, 256, 256, 192, False), (1, 512, 768, 192, False), (70, 16, 24, 8, False), (3, 15, 23, 8, False),
            (4, 64, 64, 16, True)]


@pytest.mark.parametrize("B,H,W,M,unaligned", RD_CASES)
def test_rd_loss_vs_float64(env, B, H, W, M, unaligned):
    """nic.rd_loss: the nine scalars and the per-image mse / psnr at 1e-5, the three gradients with an upstream
    gradient of 1.7 (dlogp at 1e-5, dx_hat at 1e-4 + 1e-9 as test_rd_loss_golden).  B = 70 loops the final kernel's
    image loop, 15 x 23 x 3 floats per image takes the scalar partial kernel and the three-launch backward, and so
    does the aligned-size case whose x_hat starts one float after a 16-byte boundary."""
    nic, F_, L, dev = env
    g = torch.Generator().manual_seed(300 + B)
    hy, wy, hz, wz = -(-H // 16), -(-W // 16), -(-H // 64), -(-W // 64)
    logp_y = torch.log(torch.rand((B, M, hy, wy), generator=g) * 0.999 + 1e-3)
    logp_z = torch.log(torch.rand((B, M, hz, wz), generator=g) * 0.999 + 1e-3)
    x = torch.rand((B, 3, H, W), generator=g)
    # per-image error levels a decade apart, so that the per-image values differ
    x_hat = x + 0.05 * torch.randn((B, 3, H, W), generator=g) * torch.logspace(-1, 0, B).reshape(B, 1, 1, 1)
    lam, up = 0.013, 1.7
    refs = [t.requires_grad_(True) for t in wide(logp_y, logp_z, x_hat)]
    r = ref64.rd_loss(*refs, wide(x), lam)
    (r["loss"] * up).backward()
    ty, tz = place(logp_y, dev, "nhwc", True), place(logp_z, dev, "nhwc", True)
    tx = place(x, dev, "nhwc")
    if unaligned:
        th = offset_by_one(x_hat.permute(0, 2, 3, 1).contiguous(), dev).view(B, H, W, 3).permute(0, 3, 1, 2)
        th.requires_grad_(True)
        assert F_._nhwc(th).data_ptr() % 16 == 4
    else:
        th = place(x_hat, dev, "nhwc", True)
    res = nic.rd_loss({"logp_y": ty, "logp_z": tz, "x_hat": th}, tx, lam)
    (res["loss"] * up).backward()
    for k in ref64.RD_KEYS:
        print(k, float(res[k]), float(r[k]))
    for k in ref64.RD_KEYS:
        close(float(res[k]), float(r[k]), 1e-5, 0, k)
    close(cpu(res["mse_per_image"]), r["mse_per_image"], 1e-5, 0, "mse_per_image")
    close(cpu(res["psnr_per_image"]), r["psnr_per_image"], 1e-5, 0, "psnr_per_image")
    close(cpu(ty.grad), refs[0].grad, 1e-5, 0, "dlogp_y")
    close(cpu(tz.grad), refs[1].grad, 1e-5, 0, "dlogp_z")
    close(cpu(th.grad), refs[2].grad, 1e-4, 1e-9, "dx_hat")


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Cc,ld", [(524_288, 192, 192), (32_768 + 5, 192, 192), (1000, 72, 72), (1000, 70, 70),
                                     (4097, 3, 3), (999, 3, 4), (777, 640, 1280)])
def test_colsum_vs_float64(env, P, Cc, ld):
    """lic_colsum against in.double().sum(0) * scale by close_norm at 1e-4, and bit for bit on a second call: the chunk
    cap (P >= 32 768), C not a multiple of 64 / of 4, the RGB kernel with a P % 4 tail, an RGB shape with padded rows
    (which must not take the RGB kernel) and rows twice as long as C"""
    nic, F_, L, dev = env
    lib = L.load()
    full = randn((P, ld), 400 + Cc) + 0.1
    scale = 0.37
    ref = full[:, :Cc].double().sum(0) * scale
    t = full.to(dev)
    nbytes = lib.lic_colsum_workspace_bytes(P, Cc)
    outs = []
    for _ in range(2):
        ws = torch.full(((nbytes + 3) // 4,), float("nan"), device=dev)
        out = torch.full((Cc,), float("nan"), device=dev)
        L.check(lib.lic_colsum(F_._ptr(t), ld, P, Cc, scale, F_._ptr(out), F_._ptr(ws), nbytes, F_._stream()), "lic_colsum")
        outs.append(cpu(out))
    print((P, Cc, ld), ref64.norm_err(outs[0], ref), "of the maximum")
    close_norm(outs[0], ref, 1e-4, "column sums")
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    if ld == Cc:   # the product's wrapper
        assert torch.equal(bits(F_._colsum(t, P, Cc, scale)), bits(outs[0]))


# ---------------------------------------------------------------------------------------------
# small elementwise kernels: every remainder mod 4 above the grid cap, unaligned views
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TAILS)
def test_leaky_bwd_exact(env, n):
    nic, F_, L, dev = env
    y, dy = randn(n, 500 + n % 4), randn(n, 510 + n % 4)
    y[::1001] = 0.0          # y == 0 takes the slope side
    y[1::1001] = -0.0
    slope = 0.01
    want = torch.where(y > 0, dy, dy * slope)
    dx = F_._leaky_bwd(y.to(dev), dy.to(dev), slope)
    assert torch.equal(bits(dx), bits(want)), int((bits(dx) != bits(want)).sum())
    # scalar path: every operand one float after a 16-byte boundary
    uy, udy, out = offset_by_one(y, dev), offset_by_one(dy, dev), offset_by_one(torch.full((n,), float("nan")), dev)
    L.check(L.load().lic_leaky_bwd(F_._ptr(uy), F_._ptr(udy), F_._ptr(out), n, slope, F_._stream()), "lic_leaky_bwd")
    assert torch.equal(bits(out), bits(want))


def _reparam_inputs(n, bound, seed):
    """parameters of a GDN re-parametrisation: most well above the bound, 15 % below it, 1 % exactly on it"""
    g = torch.Generator().manual_seed(seed)
    p = torch.sqrt(torch.rand(n, generator=g) * 1.5 + 1e-4)
    u = torch.rand(n, generator=g)
    p = torch.where(u < 0.15, torch.full_like(p, bound * 0.25), p)
    p = torch.where((u >= 0.15) & (u < 0.16), torch.full_like(p, bound), p)
    return p


PEDESTAL = float(2.0 ** -36)
BOUNDS = (float(np.float32((1e-6 + PEDESTAL) ** 0.5)), float(np.float32(PEDESTAL ** 0.5)))   # beta's, gamma's


@pytest.mark.parametrize("n", TAILS)
def test_gdn_reparam_one_ulp(env, n):
    """lic_gdn_reparam = max(p, bound)^2 - pedestal.  The compiler contracts v * v - pedestal into one fused
    multiply-add (one rounding), fp32 torch on the CPU rounds the product first: the two differ by at most one unit in
    the last place on these inputs (asserted here on the CPU, with the fused value from float64), so the device is
    compared with the fp32 torch expression at 1 ulp, not bit for bit."""
    nic, F_, L, dev = env
    for bound in BOUNDS:
        p = _reparam_inputs(n, bound, 520 + n % 4)
        v = torch.clamp_min(p, bound)
        want = v * v - PEDESTAL
        fused = (v.double() * v.double() - PEDESTAL).float()
        assert int((bits(want) - bits(fused)).abs().max()) <= 1
        tp, out = p.to(dev), torch.full((n,), float("nan"), device=dev)
        L.check(L.load().lic_gdn_reparam(F_._ptr(tp), F_._ptr(out), n, bound, PEDESTAL, F_._stream()), "lic_gdn_reparam")
        d = (bits(out) - bits(want)).abs()
        print(n, bound, "ulp difference: max", int(d.max()), "elements off", int((d != 0).sum()))
        assert int(d.max()) <= 1
        at_bound = p <= bound
        assert torch.equal(bits(out)[at_bound], bits(fused)[at_bound])   # (one value: the fused one, exactly)


@pytest.mark.parametrize("n", TAILS)
def test_gdn_reparam_bwd2_exact(env, n):
    """both halves of lic_gdn_reparam_bwd2 (beta's nb elements, then gamma's): dp = dout * 2 * max(p, bound) where
    p >= bound or the gradient is negative, else 0 -- p exactly on the bound with gradients of either sign included"""
    nic, F_, L, dev = env
    nb = 1001
    sizes = (nb, n - nb)
    ps = [_reparam_inputs(m, b, 530 + i) for i, (m, b) in enumerate(zip(sizes, BOUNDS))]
    ds = [randn(m, 540 + i) for i, m in enumerate(sizes)]
    for p, b, d in zip(ps, BOUNDS, ds):
        on = p == b
        assert bool((d[on] > 0).any()) and bool((d[on] < 0).any())
    want = []
    for p, b, d in zip(ps, BOUNDS, ds):
        gr = d * 2.0 * torch.clamp_min(p, b)
        want.append(torch.where((p >= b) | (gr < 0), gr, torch.zeros_like(gr)))
    dbeta, dgamma = F_._reparam_bwd2(ps[0].to(dev), ds[0].to(dev), BOUNDS[0], ps[1].to(dev), ds[1].to(dev), BOUNDS[1])
    assert torch.equal(bits(dbeta), bits(want[0]))
    assert torch.equal(bits(dgamma), bits(want[1])), int((bits(dgamma) != bits(want[1])).sum())


@pytest.mark.parametrize("late", [(1, 0), (0, 1), (1, 1)], ids=str)
def test_gdn_reparam_late_pass_through_exact(env, late):
    """the data-parallel split of the same backward: lic_gdn_reparam_bwd2_late leaves a late half as the product
    dout * 2 * max(p, bound), lic_gdn_pass_batch zeroes what the bound does not let through -- together the bits of
    lic_gdn_reparam_bwd2 (more elements than one grid covers in gamma's half, 1001 in beta's)"""
    import ctypes as C
    nic, F_, L, dev = env
    sizes = (1001, TAILS[1] - 1001)
    ps = [_reparam_inputs(m, b, 530 + i) for i, (m, b) in enumerate(zip(sizes, BOUNDS))]
    ds = [randn(m, 540 + i) for i, m in enumerate(sizes)]
    lin = [d * 2.0 * torch.clamp_min(p, b) for p, b, d in zip(ps, BOUNDS, ds)]
    want = [torch.where((p >= b) | (g < 0), g, torch.zeros_like(g)) for p, b, g in zip(ps, BOUNDS, lin)]
    tp, td = [p.to(dev) for p in ps], [d.to(dev) for d in ds]
    out = [torch.empty_like(p) for p in tp]
    L.check(L.load().lic_gdn_reparam_bwd2_late(F_._ptr(tp[0]), F_._ptr(td[0]), F_._ptr(out[0]), sizes[0], BOUNDS[0],
                                               F_._ptr(tp[1]), F_._ptr(td[1]), F_._ptr(out[1]), sizes[1], BOUNDS[1],
                                               late[0], late[1], F_._stream()), "lic_gdn_reparam_bwd2_late")
    for k in range(2):
        assert torch.equal(bits(out[k]), bits(lin[k] if late[k] else want[k])), k
    jobs = (L.PassJob * 2)()
    n = 0
    for k in range(2):
        if late[k]:
            jobs[n].p, jobs[n].g, jobs[n].n, jobs[n].bound = tp[k].data_ptr(), out[k].data_ptr(), sizes[k], BOUNDS[k]
            n += 1
    guard = [o.clone() for o in out]
    L.check(L.load().lic_gdn_pass_batch(jobs, n, F_._stream()), "lic_gdn_pass_batch")
    for k in range(2):
        assert torch.equal(bits(out[k]), bits(want[k])), k
        assert late[k] or torch.equal(bits(out[k]), bits(guard[k]))      # (a half that was not named is not touched)
    assert L.load().lic_gdn_pass_batch(None, 1, None) == -1 and L.load().lic_gdn_pass_batch(jobs, 0, None) == 0


@pytest.mark.parametrize("n", TAILS)
def test_mul_inplace_exact(env, n):
    nic, F_, L, dev = env
    w, mask = randn(n, 550 + n % 4), (randn(n, 560) > 0).float()
    tw = w.to(dev)
    F_.mask_weight_(tw, mask.to(dev))
    assert torch.equal(bits(tw), bits(w * mask))


@pytest.mark.parametrize("dims", [(600, 40, 100), (7, 331, 1037)])
def test_permute3_exact(env, dims):
    """lic_permute3 over more elements than one grid covers, every axis order, into a strided destination"""
    nic, F_, L, dev = env
    src = randn(dims, 570)
    tsrc = src.to(dev)
    for perm in ((2, 0, 1), (1, 2, 0), (0, 2, 1)):
        want = src.permute(perm).contiguous()
        dst = torch.full(want.shape, float("nan"), device=dev)
        sv = tsrc.permute(perm)
        F_._permute3(tsrc, dst, tuple(want.shape), sv.stride(), dst.stride())
        assert torch.equal(bits(dst), bits(want)), perm


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("n", TAILS)
def test_gdn_dnorm_vs_float64(env, n, inverse):
    """lic_gdn_dnorm: t = 0.5 g x / sqrt(norm) (inverse) or -0.5 g x norm^-1.5, at the project's 1e-4 (+ 1e-6), through
    the 16-byte path with its tail and through the scalar path (operands one float off alignment)"""
    nic, F_, L, dev = env
    g, x = randn(n, 580 + n % 4), randn(n, 590 + n % 4)
    norm = torch.rand(n, generator=torch.Generator().manual_seed(600)) * 4 + 0.05
    g64, x64, n64 = wide(g, x, norm)
    ref = 0.5 * g64 * x64 / n64.sqrt() if inverse else -0.5 * g64 * x64 * n64 ** -1.5
    lib = L.load()
    for name, mk in (("aligned", lambda t: t.to(dev)), ("offset", lambda t: offset_by_one(t, dev))):
        tg, tx, tn, out = mk(g), mk(x), mk(norm), mk(torch.full((n,), float("nan")))
        L.check(lib.lic_gdn_dnorm(F_._ptr(tg), F_._ptr(tx), F_._ptr(tn), F_._ptr(out), n, inverse, F_._stream()),
                "lic_gdn_dnorm")
        print(n, inverse, name, ref64.band_ratio(cpu(out), ref, 1e-4, 1e-6), "of the band")
        close(cpu(out), ref, 1e-4, 1e-6, name)


# ---------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------
ADAM_LENGTHS = (1, 3, 37, 4096, 4097, 8191, 12_290, 100_003)
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8


def _adam_lengths(ntensors, seed):
    r = np.random.RandomState(seed)
    lens = [int(v) for v in r.choice(ADAM_LENGTHS[:-1], size=ntensors)]
    for i in r.choice(ntensors, size=3, replace=False):    # a few long tensors: tens of blocks with a ragged last one
        lens[int(i)] = ADAM_LENGTHS[-1]
    lens[:len(ADAM_LENGTHS)] = ADAM_LENGTHS                # and every length at least once
    return lens


def _adam_against_float64(params, opt, wd, seed):
    """three optimizer steps of `opt` over the device `params` against ref64.adam_step on the CPU"""
    g = torch.Generator().manual_seed(seed)
    p64 = [wide(cpu(p)) for p in params]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    for step in (1, 2, 3):
        for i, p in enumerate(params):
            gr = torch.randn(p.shape, generator=g) * (0.1 + (i % 7))
            p.grad = gr.to(p.device)
            p64[i], m64[i], v64[i] = ref64.adam_step(p64[i], wide(gr), m64[i], v64[i], step, LR, BETAS, EPS, wd)
        opt.step()
    worst_p = worst_v = 0.0
    state = opt.state_dict()["state"]
    for i, p in enumerate(params):
        # tests/test_gpu_optim.py's bound per step count: 1e-5 of the three updates of ~lr each + 1e-6 of the parameter
        tol = 1e-6 * float(p64[i].abs().max()) + 1e-5 * 3 * LR
        err = float((wide(cpu(p)) - p64[i]).abs().max())
        worst_p = max(worst_p, err / tol)
        v = wide(cpu(state[i]["exp_avg_sq"]))
        worst_v = max(worst_v, float((v - v64[i]).abs().max()) / max(float(v64[i].abs().max()), 1e-30))
        assert float(state[i]["step"]) == 3.0
    print(len(params), "tensors, wd", wd, ": parameters at", worst_p, "of their bound, exp_avg_sq off by", worst_v,
          "of its maximum")
    assert worst_p <= 1.0
    assert worst_v <= 1e-6


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("ntensors", [60, 150, 448])
def test_fused_adam_vs_float64(env, ntensors, wd):
    """one kernel instantiation each (<= 96, <= 224, <= 448 gradient addresses), hundreds of jobs for the block ->
    job search, tensors longer than one 4096-element block whose length is not a multiple of 4"""
    nic, F_, L, dev = env
    from neural_image_compression_amd.optim import FusedAdam
    params = [torch.nn.Parameter(randn(n, 700 + i).to(dev)) for i, n in enumerate(_adam_lengths(ntensors, ntensors))]
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    _adam_against_float64(params, opt, wd, 710 + ntensors)
    assert opt.fused_steps == 3


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_unaligned_views_vs_float64(env, wd):
    """parameters that are views one float off a 16-byte boundary: the kernel's scalar branch"""
    nic, F_, L, dev = env
    from neural_image_compression_amd.optim import FusedAdam
    params = [torch.nn.Parameter(offset_by_one(randn(n, 720 + i), dev)) for i, n in enumerate(ADAM_LENGTHS)]
    assert all(p.data_ptr() % 16 == 4 for p in params)
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    _adam_against_float64(params, opt, wd, 730)
    assert opt.fused_steps == 3


def test_fused_adam_449_tensors_takes_torch_path(env):
    """more tensors than lic_adam_run's argument block holds: torch's own update for the whole call, with the
    parameters and step counts torch.optim.Adam gives"""
    nic, F_, L, dev = env
    from neural_image_compression_amd.optim import FusedAdam
    pa = [torch.nn.Parameter(randn(37 + i % 5, 740 + i).to(dev)) for i in range(449)]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = torch.optim.Adam(pa, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)
    ob = FusedAdam(pb, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)
    g = torch.Generator().manual_seed(750)
    for _ in range(3):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).to(dev)
            a.grad, b.grad = gr, gr.clone()
        oa.step()
        ob.step()
    assert ob.fused_steps == 0
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), i
        assert float(sa[i]["step"]) == float(sb[i]["step"]) == 3.0


# ---------------------------------------------------------------------------------------------
# logging kernels
# ---------------------------------------------------------------------------------------------
def test_tensor_stats_above_block_cap_vs_numpy(env):
    """3 000 001 elements: 256 blocks x 256 lanes take 46 trips each and a ragged last one, NaNs in the last trip;
    the assertions of tests/test_data_pipeline.py::test_tensor_stats_vs_numpy"""
    nic, F_, L, dev = env
    from neural_image_compression_amd.data import tensor_stats
    n = 3_000_001
    a = (np.random.RandomState(800).randn(n) * 3 + 1).astype(np.float32)
    last_trip = n - (n % (256 * 256))
    a[last_trip + 5] = a[n - 1] = a[n - 77] = np.nan
    a[17] = np.nan
    t = torch.from_numpy(a).to(dev)
    st = tensor_stats(t, nbins=32)
    v = a[~np.isnan(a)].astype(np.float64)
    print("mean", st["mean"], v.mean(), "std", st["std"], v.std())
    assert st["count"] == v.size and st["nan"] == 4
    assert abs(st["mean"] - v.mean()) < 1e-9 and abs(st["std"] - v.std()) < 1e-7
    assert st["min"] == v.min() and st["max"] == v.max()
    b = np.floor((v.astype(np.float32) - np.float32(st["lo"])) * (np.float32(32) / (np.float32(st["hi"]) - np.float32(st["lo"])))).astype(np.int64)
    ref = np.bincount(np.clip(b, 0, 31), minlength=32)
    assert sum(st["hist"]) == v.size and np.abs(np.array(st["hist"]) - ref).sum() <= 2   # fp32 bin edges
    assert tensor_stats(t, nbins=32) == st                                # reproducible
    st2 = tensor_stats(t, nbins=8, lo=-1.0, hi=1.0)
    assert st2["hist"][0] == int((v < -0.75).sum()) and sum(st2["hist"]) == v.size


@pytest.mark.parametrize("n", TAILS)
def test_u8_to_f32_exact(env, n):
    nic, F_, L, dev = env
    from neural_image_compression_amd.data import u8_to_f32
    t = torch.from_numpy(np.random.RandomState(810 + n % 4).randint(0, 256, size=n).astype(np.uint8))
    want = t.float() / 255
    tt, out = t.to(dev), torch.full((n,), float("nan"), device=dev)
    L.check(L.load().lic_u8_to_f32(F_._ptr(tt), F_._ptr(out), n, F_._stream()), "lic_u8_to_f32")
    assert torch.equal(bits(out), bits(want))
    if n == BIG:   # the loader's wrapper, [B, H, W, 3] -> [B, 3, H, W]
        img = t.reshape(1, -1, 100, 3)
        assert torch.equal(bits(u8_to_f32(img.to(dev))), bits((img.float() / 255).permute(0, 3, 1, 2)))
