"""Pins tests/ref64.py (the float64 references of tests/test_gpu_latent_ops.py) to the reference-generated fixtures
under tests/golden/, within the bands tests/test_oracle_golden.py uses for the C oracle on the same fixtures, and
asserts on the CPU the conditions the input generators must meet for every seed the GPU cases use.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import golden_recipe as R
import ref64
from ref64 import close, close_norm, wide


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


# ---------------------------------------------------------------------------------------------
# the references against reference-generated data
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_entropy_params_golden(golden_dir, K):
    """the fixture stores the input of the whole EntropyParameters module: the three 1x1 convolutions around the
    activation are the C oracle's (pinned against torch in tests/test_oracle_golden.py), the activation and its
    backward are ref64's"""
    from oracle import oracle as O
    fx = load(golden_dir, f"op_entropy_parameters_K{K}.npz")
    M, B, h, w = int(fx["M"]), int(fx["B"]), int(fx["h"]), int(fx["w"])
    ks = [(k, tuple(s)) for k, s in json.loads(str(fx["keys_shapes"]))]
    st = R.make_state(ks, int(fx["seed_state"]))
    comb = R.make_noise((B, 4 * M, h, w), int(fx["seed_in"])) * 4 - 2
    a0 = O.leaky_relu_fwd(O.conv2d_fwd(comb, st["net.0.weight"], st["net.0.bias"], 1, 0))
    a1 = O.leaky_relu_fwd(O.conv2d_fwd(a0, st["net.2.weight"], st["net.2.bias"], 1, 0))
    raw = t64(O.conv2d_fwd(a1, st["net.4.weight"], st["net.4.bias"], 1, 0), True)
    ep = ref64.entropy_params(raw, M, K)
    G = 2 if K == 1 else 3
    outs = [o if K == 1 else o.reshape(B, K, M, h, w) for o in ep.chunk(G, dim=1)]
    loss = 0
    for i, o in enumerate(outs):
        close(o, fx[f"out{i}"], 1e-4, 1e-6, f"out{i}")
        cot = R.make_noise(tuple(o.shape), int(fx["seed_cot"]) + i) - 0.5
        loss = loss + (o * torch.from_numpy(cot).double()).sum()
    loss.backward()
    draw = raw.grad.float().numpy()
    close_norm(draw.sum(axis=(0, 2, 3)), fx["grad.net.4.bias"], 1e-4, "net.4.bias")
    da1, _, _ = O.conv2d_bwd(a1, st["net.4.weight"], draw, 1, 0)
    da0, _, _ = O.conv2d_bwd(a0, st["net.2.weight"], O.leaky_relu_bwd(a1, da1), 1, 0)
    dx, _, _ = O.conv2d_bwd(comb, st["net.0.weight"], O.leaky_relu_bwd(a0, da0), 1, 0)
    close_norm(dx, fx["dx"], 1e-4, "dx")


def test_gaussian_golden(golden_dir):
    fx = load(golden_dir, "op_gaussian.npz")
    B, M, h, w = fx["x"].shape
    cot = torch.from_numpy(R.make_noise((B, M, h, w), int(fx["seed_cot"])) - 0.5).double()
    x = t64(fx["x"], True)
    params = t64(np.concatenate([fx["mu"], fx["sigma"]], axis=1), True)
    p, logp = ref64.gmm_likelihood(x, params, 1)
    close(p, fx["p1"], 1e-4, 1.5e-7, "p1")
    (logp * cot).sum().backward()
    sel = fx["p1"] > 2e-3
    close(x.grad.numpy()[sel], fx["dx1"][sel], 5e-4, 1e-5, "dx1")
    close(params.grad.numpy()[:, :M][sel], fx["dmu1"][sel], 5e-4, 1e-5, "dmu1")
    close(params.grad.numpy()[:, M:][sel], fx["dsigma1"][sel], 5e-4, 1e-5, "dsigma1")
    # clamp region: zero gradient.  (Where the fixture's fp32 p sits on the bound while the float64 value is within a
    # factor 4 of it, either side is legitimate: those elements are in neither comparison.)
    p_raw = ref64.gmm_mass(x.detach(), params.detach(), 1)[0].numpy()
    dead = (fx["p1"] <= 1e-9) & (p_raw < ref64.BOUND / 4)
    assert dead.any() and (x.grad.numpy()[dead] == 0).all() and (params.grad.numpy()[:, :M][dead] == 0).all()
    ws = fx["weights"]
    K = ws.shape[1]
    x = t64(fx["x"], True)
    params = t64(np.concatenate([fx[k].reshape(B, K * M, h, w) for k in ("weights", "mus", "sigmas")], axis=1), True)
    p, logp = ref64.gmm_likelihood(x, params, K)
    close(p, fx["p3"], 1e-4, 1.5e-7, "p3")
    (logp * cot).sum().backward()
    sel = fx["p3"] > 2e-3
    close(x.grad.numpy()[sel], fx["dx3"][sel], 5e-4, 1e-5, "dx3")
    sel5 = np.broadcast_to(sel[:, None], ws.shape)
    blocks = ref64.split_params(params.grad, K, M)
    for name, key in (("dw3", "w"), ("dmu3", "mu"), ("dsigma3", "sigma")):
        close(blocks[key].numpy()[sel5], fx[name][sel5], 5e-4, 1e-5, name)


def test_factorized_golden(golden_dir):
    fx = load(golden_dir, "op_factorized.npz")
    ks = [(k, tuple(s)) for k, s in json.loads(str(fx["keys_shapes"]))]
    st = R.make_state(ks, int(fx["seed_state"]))
    groups = [[t64(st[f"{n}.{i}"], True) for i in range(c)] for n, c in (("matrices", 4), ("biases", 4), ("factors", 3))]
    x = t64(fx["x"], True)
    p, logp = ref64.factorized(x, *groups)
    close(p, fx["p"], 1e-4, 1e-9, "p")
    assert float(p.detach()[1, 0, 0, 0]) == 1e-9 and float(p.detach()[1, 0, 0, 1]) == 1e-9      # the clamp engages on the tails
    close(ref64.factorized(x, *groups, bound=0.0)[0], fx["p_raw"], 1e-4, 1e-12, "p_raw")
    cot = torch.from_numpy(R.make_noise(tuple(p.shape), int(fx["seed_cot"])) - 0.5).double()
    (logp * cot).sum().backward()
    close_norm(x.grad, fx["dx"], 1e-4, "dx")
    for n, grp in zip(("matrices", "biases", "factors"), groups):
        for i, t in enumerate(grp):
            close_norm(t.grad, fx[f"grad.{n}.{i}"], 1e-4, f"{n}.{i}")


def test_rd_loss_golden(golden_dir):
    fx = load(golden_dir, "op_rd_loss.npz")
    ly, lz, xh = (t64(fx[k], True) for k in ("logp_y", "logp_z", "x_hat"))
    res = ref64.rd_loss(ly, lz, xh, t64(fx["x"]), float(fx["lambda_rd"]))
    for k in ref64.RD_KEYS:
        close(float(res[k]), float(fx[k]), 1e-5, 0, k)
    close(res["mse_per_image"], fx["mse_per_image"], 1e-5, 0, "mse_img")
    close(res["psnr_per_image"], fx["psnr_per_image"], 1e-5, 0, "psnr_img")
    res["loss"].backward()
    close(ly.grad, fx["dlogp_y"], 1e-5, 0, "dlogp_y")
    close(lz.grad, fx["dlogp_z"], 1e-5, 0, "dlogp_z")
    close(xh.grad, fx["dx_hat"], 1e-4, 1e-9, "dx_hat")


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_is_torch_adam(wd):
    """ref64.adam_step against torch.optim.Adam itself, both in float64 on the CPU, three steps"""
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(1000, generator=g, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        gr = torch.randn(1000, generator=g, dtype=torch.float64)
        q.grad = gr.clone()
        opt.step()
        p, m, v = ref64.adam_step(p, gr, m, v, step, 3e-3, (0.9, 0.999), 1e-8, wd)
    assert float((p - q.detach()).abs().max()) <= 1e-13
    assert float((v - opt.state[q]["exp_avg_sq"]).abs().max()) <= 1e-15 * float(v.abs().max()) + 1e-30


# ---------------------------------------------------------------------------------------------
# conditions on the generated inputs, for every seed the GPU cases use
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref64.GMM_CASES, ids=ref64.gmm_id)
def test_gmm_inputs_meet_their_conditions(case):
    B, M, h, w, K, seed = case
    x, params, dead_gen, floor_gen = ref64.gmm_inputs(*case)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    p, logp, p_raw, grads = ref64.gmm_reference(x, params, K, gp, glogp)
    dead, live, border = ref64.gmm_regions(p_raw)
    # no element where fp32 may land on either side of the bound; the overwritten elements are what they are meant to be
    assert not bool(border.any())
    assert bool(dead_gen.any()) and bool(floor_gen.any())
    assert bool((dead == dead_gen).all()), "dead elements other than the generated ones (or generated ones alive)"
    close(p[floor_gen], torch.ones_like(p[floor_gen]), *ref64.P_BAND, "p at the sigma floor")
    for mode in ref64.GMM_MODES:     # the reference itself: no gradient through the clamp
        assert bool((grads[mode][0][dead] == 0).all())
    # at most 2 % of the elements are outside the gradient comparison (the clamped ones, checked for exact zeros, included)
    skipped = float((~(live & (p > ref64.P_RESOLVED))).double().mean())
    unresolved = float((live & (p <= ref64.P_RESOLVED)).double().mean())
    print(f"{ref64.gmm_id(case)}: {100 * unresolved:.2f} % with bound < p <= 2e-3, {100 * skipped:.2f} % with the clamped ones")
    assert skipped <= ref64.MAX_SKIPPED
    # the fp32 restatement of the same formulas stays inside every band the device is held to, the derived
    # mixture-weight band included
    max_g = max(float(gp.abs().max()), float(glogp.abs().max()))
    p32, logp32, _, grads32 = ref64.gmm_reference(x, params, K, gp, glogp, torch.float32)
    worst = ref64.check_gmm((p32, logp32, grads32), (p, logp, grads, p_raw), K, M, max_g, "fp32 restatement")
    print({k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("case", ref64.GMM_CASES, ids=ref64.gmm_id)
def test_entropy_raw_reaches_both_softplus_branches(case):
    B, M, h, w, K, seed = case
    raw = ref64.entropy_raw(B, M, h, w, K, seed)
    sg = raw.chunk(2 if K == 1 else 3, dim=1)[-1]
    assert bool((sg > 20).any()) and bool((sg == 20).any()) and bool((sg < -20).any())
    out32, out64 = ref64.entropy_params(raw, M, K), ref64.entropy_params(wide(raw), M, K)
    close(out32, out64, 1e-4, 1e-6, "fp32 restatement")


@pytest.mark.parametrize("shape,seed", ref64.FE_CASES, ids=[str(c[1]) for c in ref64.FE_CASES])
def test_factorized_inputs_leave_the_project_band_room(shape, seed):
    """close_norm at 1e-4 is met by the fp32 restatement with room to spare on every case: the device is held to the
    project's band as it stands"""
    st, x = ref64.fe_state(shape[1], seed), ref64.fe_inputs(shape, seed)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    p, logp, dx, gr = ref64.fe_reference(x, st, gp, glogp)
    p32, logp32, dx32, gr32 = ref64.fe_reference(x, st, gp, glogp, torch.float32)
    close(p32, p, 1e-4, 1.5e-7, "p")
    close(logp32, logp, 1e-4, 1e-6, "logp")
    worst = max([ref64.norm_err(dx32, dx)] + [ref64.norm_err(a, b) for a, b in zip(gr32, gr)])
    print(f"{shape}: fp32 restatement at {worst:.2e} of the maximum")
    assert worst <= 0.5e-4
