"""Plain-torch references for the latent-side operations, written from the reference's formulas with torch ops only
and differentiated by torch.autograd.  Every function computes in the dtype of its inputs: the tests call them
with float64 tensors widened from the fp32 inputs the device sees (`wide`), and with the fp32 tensors themselves
when they need the "fp32 restatement" -- what fp32 arithmetic of the same formula gives on the host.

Also the input generators of tests/test_gpu_latent_ops.py, so that tests/test_ref64.py can assert their
conditions (share of elements left out of a gradient comparison, no element near the likelihood bound) on the
CPU for every seed the GPU cases use.

tests/test_ref64.py pins these functions to the reference-generated fixtures under tests/golden/.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

BOUND = 1e-9          # likelihood lower bound (EntropyModels.py:29-31)
P_RESOLVED = 2e-3     # gradients that divide by p are compared where p exceeds this (tests/test_oracle_golden.py)
MAX_SKIPPED = 0.02    # at most this share of a case's elements may be left out of a gradient comparison


def wide(*ts):
    out = tuple(None if t is None else t.detach().double() for t in ts)
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------
def entropy_params(raw, M, K):
    """ParametersModels.py:43-64 on the flat [B, G*K*M, h, w] tensor: K == 1 -> (mu, softplus(.) + 1e-6);
    else (softmax over K, identity, softplus(.) + 1e-6), each block k-major.  Returns the flat activated tensor."""
    B, CH, h, w = raw.shape
    if K == 1:
        mu, sg = raw.chunk(2, dim=1)
        return torch.cat([mu, F.softplus(sg) + 1e-6], dim=1)
    wt, mus, sgs = (t.reshape(B, K, M, h, w) for t in raw.chunk(3, dim=1))
    wt = F.softmax(wt, dim=1)
    sgs = F.softplus(sgs) + 1e-6
    return torch.cat([t.reshape(B, K * M, h, w) for t in (wt, mus, sgs)], dim=1)


def _gcdf(t):
    return 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))


def gmm_mass(x, params, K):
    """unclamped likelihood and the per-component bin masses [B, K, M, h, w]"""
    B, M, h, w = x.shape
    if K == 1:
        mu, sg = (t.reshape(B, 1, M, h, w) for t in params.chunk(2, dim=1))
        wt = None
    else:
        wt, mu, sg = (t.reshape(B, K, M, h, w) for t in params.chunk(3, dim=1))
    xe = x.unsqueeze(1)
    mass = _gcdf((xe + 0.5 - mu) / sg) - _gcdf((xe - 0.5 - mu) / sg)
    return (mass if wt is None else wt * mass).sum(dim=1), mass


def gmm_likelihood(x, params, K, bound=BOUND):
    """EntropyModels.py:188-233 with the clamp (:29-31) and the log (Models.py:86-87): (p, logp)"""
    p = gmm_mass(x, params, K)[0].clamp_min(bound)
    return p, torch.log(p)


def factorized(x, matrices, biases, factors, bound=BOUND):
    """EntropyModels.py:88-151: the 4-layer cumulative, the sign trick (sign detached), clamp, log.  x: [B, C, ...]"""
    C = x.shape[1]
    flat = x.transpose(0, 1).reshape(C, 1, -1)

    def logits(v):
        for i in range(4):
            v = torch.matmul(F.softplus(matrices[i]), v) + biases[i]
            if i < 3:
                v = v + torch.tanh(factors[i]) * torch.tanh(v)
        return v
    lower, upper = logits(flat - 0.5), logits(flat + 0.5)
    s = -torch.sign(lower + upper).detach()
    pmf = torch.abs(torch.sigmoid(s * upper) - torch.sigmoid(s * lower))
    p = pmf.reshape(C, x.shape[0], *x.shape[2:]).transpose(0, 1).clamp_min(bound)
    return p, torch.log(p)


RD_KEYS = ("loss", "bpp_y", "bpp_z", "bpp_total", "mse", "psnr", "bits_y", "bits_z", "bits_total")


def rd_loss(logp_y, logp_z, x_hat, x, lambda_rd):
    """RateDistortionLoss.py:5-49: the nine scalars (0-d tensors) and the per-image mse / psnr"""
    npix = x.shape[2] * x.shape[3]
    bits_y = -logp_y.sum(dim=(1, 2, 3)) / math.log(2.0)
    bits_z = -logp_z.sum(dim=(1, 2, 3)) / math.log(2.0)
    bpp_y, bpp_z = (bits_y / npix).mean(), (bits_z / npix).mean()
    mse_img = ((x_hat - x) ** 2).mean(dim=(1, 2, 3))
    mse = mse_img.mean()
    return {"loss": bpp_y + bpp_z + lambda_rd * 255 ** 2 * mse, "bpp_y": bpp_y, "bpp_z": bpp_z,
            "bpp_total": bpp_y + bpp_z, "mse": mse, "psnr": -10 * torch.log10(mse + 1e-8),
            "bits_y": bits_y.mean(), "bits_z": bits_z.mean(), "bits_total": (bits_y + bits_z).mean(),
            "mse_per_image": mse_img, "psnr_per_image": -10 * torch.log10(mse_img + 1e-8)}


def adam_step(p, g, m, v, step, lr, betas, eps, wd):
    """torch.optim.Adam (no amsgrad, L2 weight decay), update number `step` (1-based): new (p, m, v)"""
    b1, b2 = betas
    if wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


# ---------------------------------------------------------------------------------------------
# comparison helpers (the project's bands: tests/test_oracle_golden.py, tests/test_gpu_parity.py)
# ---------------------------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)


def band_ratio(a, b, rtol, atol):
    """worst |a - b| / (atol + rtol |b|); 0 for an empty selection"""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    r = np.abs(a - b) / (atol + rtol * np.abs(b))
    return float(np.nan_to_num(r, nan=np.inf).max())


def close(a, b, rtol, atol, what=""):
    r = band_ratio(a, b, rtol, atol)
    assert r <= 1.0, f"{what}: {r:.3g} x the band {rtol:g} * |ref| + {atol:g}"


def norm_err(a, b):
    """max |a - b| over max |b| (tensor-level relative error, for sums over many terms)"""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.nan_to_num(np.abs(a - b), nan=np.inf).max() / max(np.abs(b).max(), 1e-30))


def close_norm(a, b, rtol=1e-4, what=""):
    e = norm_err(a, b)
    assert e <= rtol, f"{what}: {e:.3e} of the tensor's maximum (allowed {rtol:.3e})"


# ---------------------------------------------------------------------------------------------
# inputs of the likelihood / entropy-parameter cases
# ---------------------------------------------------------------------------------------------
# (B, M, h, w, K, seed): configs 2 and 3k, one Kodak frame, and a shape where nothing divides anything
GMM_CASES = [(32, 192, 16, 16, 1, 101), (32, 128, 16, 16, 3, 102), (1, 192, 32, 48, 3, 103), (3, 20, 5, 7, 2, 104)]


def gmm_id(c):
    return "B%d-M%d-%dx%d-K%d" % c[:5]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(shape, lo, hi, g):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@functools.lru_cache(maxsize=2)
def gmm_inputs(B, M, h, w, K, seed):
    """fp32 (x [B,M,h,w], params [B,G*K*M,h,w] activated, dead mask, floor mask).

    mu ~ U(-4, 4), sigma = softplus(U(-3, 3)) + 1e-6, weights = softmax(U(-2, 2)) over K, x = round(mu_k + sigma_k *
    N(0, 1)) for a random component k.  Then 1 % of the elements are overwritten with edge values:
      dead:  x an integer at least 8 sigma_k (+ half a bin) beyond every component, either side, so the float64
             likelihood is far below bound / 4 and the fp32 one is exactly 0 before the clamp;
      floor: every sigma_k at its floor 1e-6 and every mu_k = x (an integer): p = sum of the weights = 1."""
    g = _gen(seed)
    sh = (B, K, M, h, w)
    mu = _uniform(sh, -4.0, 4.0, g)
    sg = F.softplus(_uniform(sh, -3.0, 3.0, g)) + 1e-6
    wt = F.softmax(_uniform(sh, -2.0, 2.0, g), dim=1)
    k = torch.randint(0, K, (B, 1, M, h, w), generator=g)
    z = torch.randn((B, M, h, w), generator=g)
    x = torch.round(mu.gather(1, k)[:, 0] + sg.gather(1, k)[:, 0] * z)
    u = torch.rand((B, M, h, w), generator=g)
    dead, floor = u < 0.005, (u >= 0.005) & (u < 0.01)
    side = torch.rand((B, M, h, w), generator=g) < 0.5
    extra = torch.randint(0, 4, (B, M, h, w), generator=g).float()
    hi = torch.ceil((mu + 8.0 * sg).amax(dim=1) + 0.5) + extra
    lo = torch.floor((mu - 8.0 * sg).amin(dim=1) - 0.5) - extra
    x = torch.where(dead, torch.where(side, hi, lo), x)
    fl = floor.unsqueeze(1).expand(sh)
    sg = torch.where(fl, torch.full_like(sg, 1e-6), sg)
    mu = torch.where(fl, x.unsqueeze(1).expand(sh), mu)
    blocks = (mu, sg) if K == 1 else (wt, mu, sg)
    params = torch.cat([t.reshape(B, K * M, h, w) for t in blocks], dim=1).contiguous()
    return x.contiguous(), params, dead, floor


def cotangents(shape, seed):
    """(cotangent on p, cotangent on logp), U(-0.5, 0.5)"""
    g = _gen(seed)
    return _uniform(shape, -0.5, 0.5, g), _uniform(shape, -0.5, 0.5, g)


GMM_MODES = ("logp", "p", "both")


def gmm_reference(x, params, K, gp, glogp, dtype=torch.float64):
    """p, logp, the unclamped likelihood, and for each cotangent mode (dx, dparams), in `dtype` on the CPU"""
    xr = x.detach().to(dtype).requires_grad_(True)
    pr = params.detach().to(dtype).requires_grad_(True)
    p, logp = gmm_likelihood(xr, pr, K)
    with torch.no_grad():
        p_raw = gmm_mass(xr, pr, K)[0]
    grads = {}
    for mode in GMM_MODES:
        loss = 0
        if mode in ("logp", "both"):
            loss = loss + (logp * glogp.to(dtype)).sum()
        if mode in ("p", "both"):
            loss = loss + (p * gp.to(dtype)).sum()
        grads[mode] = torch.autograd.grad(loss, (xr, pr), retain_graph=True)
    return p.detach(), logp.detach(), p_raw, grads


def gmm_regions(p_raw64, bound=BOUND):
    """(dead, live, borderline) by the float64 unclamped likelihood: below bound / 4 the fp32 result is clamped for
    certain, above 4 * bound it is not; in between fp32 may land on either side"""
    dead = p_raw64 < bound / 4
    live = p_raw64 > 4 * bound
    return dead, live, ~(dead | live)


def split_params(t, K, M):
    """flat [B, G*K*M, h, w] -> dict of [B, K, M, h, w] blocks"""
    B, _, h, w = t.shape
    names = ("mu", "sigma") if K == 1 else ("w", "mu", "sigma")
    return {n: b.reshape(B, K, M, h, w) for n, b in zip(names, t.chunk(len(names), dim=1))}


# the project's bands for the likelihood (tests/test_oracle_golden.py::test_gaussian_golden)
P_BAND = (1e-4, 1.5e-7)
LOGP_BAND = (1e-4, 1e-6)
GRAD_BAND = (5e-4, 1e-5)


def dw_band(max_g):
    """mixture-weight gradient dw_k = g * mass_k / p: a bin mass carries the 1.5e-7 absolute floor of P_BAND, the
    smallest compared p is P_RESOLVED, the largest cotangent is max_g: 1.5e-7 / 2e-3 * max_g = 7.5e-5 * max_g"""
    return (5e-4, P_BAND[1] / P_RESOLVED * max_g)


def check_gmm(got, ref, K, M, max_g, what, report=None):
    """got / ref: (p, logp, {mode: (dx, dparams)}); ref also carries p_raw at index 3.  Asserts the bands on
    the live elements, exact zeros and p == bound on the dead ones."""
    p64, logp64, grads64, p_raw = ref
    dead, live, border = gmm_regions(p_raw)
    assert not bool(border.any()), f"{what}: {int(border.sum())} elements near the bound"
    sel = live & (p64 > P_RESOLVED)
    worst = {}
    worst["p"] = band_ratio(got[0], p64, *P_BAND)
    # log p = log(p (1 + d)) moves by d = 1.5e-7 / p: like the gradients it is compared where p is resolved; below that
    # the device's logp must be the logarithm of the device's own p (which the band above holds), to fp32 rounding
    # of a value of magnitude up to |log bound| = 20.7 (one ulp there is 1.9e-6)
    worst["logp"] = band_ratio(got[1][sel], logp64[sel], *LOGP_BAND)
    worst["logp_of_p"] = band_ratio(got[1], torch.log(got[0].double()), 1e-6, 1e-6)
    assert bool((got[0][dead].double() == float(np.float32(BOUND))).all()), f"{what}: clamped p != bound"
    for mode in GMM_MODES:
        dx, dpar = got[2][mode]
        dx64, dpar64 = grads64[mode]
        assert bool((dx[dead] == 0).all()), f"{what}/{mode}: dx not zero in the clamped region"
        worst[f"{mode}.dx"] = band_ratio(dx[sel], dx64[sel], *GRAD_BAND)
        g_blocks, r_blocks = split_params(dpar, K, M), split_params(dpar64, K, M)
        for n in g_blocks:
            sel5, dead5 = (m.unsqueeze(1).expand(g_blocks[n].shape) for m in (sel, dead))
            assert bool((g_blocks[n][dead5] == 0).all()), f"{what}/{mode}: d{n} not zero in the clamped region"
            band = dw_band(max_g) if n == "w" else GRAD_BAND
            worst[f"{mode}.d{n}"] = band_ratio(g_blocks[n][sel5], r_blocks[n][sel5], *band)
    if report is not None:
        report.update(worst)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the band (multiples of it): {bad}"
    return worst


# ---------------------------------------------------------------------------------------------
# inputs of the entropy-parameter activation cases (same shapes and seeds + 50)
# ---------------------------------------------------------------------------------------------
def entropy_raw(B, M, h, w, K, seed):
    """raw [B, G*K*M, h, w] fp32: U(-6, 6), with 2 % of the elements spread over [-40, 40] so that softplus runs
    on both sides of its v > 20 switch and the softmax sees dominant logits, and a few exactly at 20"""
    g = _gen(seed + 50)
    G = 2 if K == 1 else 3
    sh = (B, G * K * M, h, w)
    raw = _uniform(sh, -6.0, 6.0, g)
    u = torch.rand(sh, generator=g)
    raw = torch.where(u < 0.02, _uniform(sh, -40.0, 40.0, g), raw)
    raw = torch.where((u >= 0.02) & (u < 0.021), torch.full_like(raw, 20.0), raw)
    return raw.contiguous()


# ---------------------------------------------------------------------------------------------
# inputs of the factorised cases
# ---------------------------------------------------------------------------------------------
FE_CASES = [((32, 192, 4, 4), 201), ((16, 192, 8, 8), 202), ((1, 192, 8, 12), 203), ((5, 7, 9, 13), 204),
            ((6, 24, 50), 205)]


def fe_state(C, seed):
    """the eleven parameter tensors from golden_recipe.make_state, as (matrices, biases, factors) of fp32 tensors"""
    import golden_recipe as R
    shapes = [(C, 3, 1), (C, 3, 3), (C, 3, 3), (C, 1, 3)], [(C, 3, 1)] * 3 + [(C, 1, 1)], [(C, 3, 1)] * 3
    ks = [(f"{n}.{i}", s) for n, ss in zip(("matrices", "biases", "factors"), shapes) for i, s in enumerate(ss)]
    st = R.make_state(ks, seed)
    return tuple([torch.from_numpy(st[f"{n}.{i}"]) for i in range(len(ss))]
                 for n, ss in zip(("matrices", "biases", "factors"), shapes))


def fe_inputs(shape, seed):
    """z as the hyper-encoder hands it over in training: integers of a few units plus U(-0.5, 0.5) noise, fp32"""
    g = _gen(seed)
    return (torch.round(2.0 * torch.randn(shape, generator=g)) + _uniform(shape, -0.5, 0.5, g)).contiguous()


def fe_reference(x, state, gp, glogp, dtype=torch.float64):
    """p, logp, dx and the eleven parameter gradients for the cotangents (gp on p, glogp on logp; either None)"""
    xr = x.detach().to(dtype).requires_grad_(True)
    ps = [[t.detach().to(dtype).requires_grad_(True) for t in grp] for grp in state]
    p, logp = factorized(xr, *ps)
    loss = 0
    if gp is not None:
        loss = loss + (p * gp.to(dtype)).sum()
    if glogp is not None:
        loss = loss + (logp * glogp.to(dtype)).sum()
    flat = [t for grp in ps for t in grp]
    grads = torch.autograd.grad(loss, [xr] + flat)
    return p.detach(), logp.detach(), grads[0], list(grads[1:])
