"""The case table of tests/test_gpu_fences.py: for every entry of the latent, loss, metric, window, table and Adam
kernels the smallest sizes at which it can still go wrong, the shift (elements off the 16-byte alignment) of every
operand, the inputs and the reference.  Not a test module: tests/test_fence_cases.py states the table's coverage and
runs every reference on the CPU; tests/test_gpu_fences.py launches every case between canary fences (guarded.py).

A case's inputs come from the generators the value tests already use (ref64.py, msssim_ref64.py, the recipes of
test_gpu_latent_ops.py, test_gpu_checker_kernels.py, test_gpu_window.py and test_gpu_resample.py, restated here where
they live in a GPU test module) at the case's own size.  `band` names the statement and the band of the entry's
existing value test; no band is defined here.

make(case) -> (inputs, want): two dicts of CPU tensors / numpy arrays in the layout the entry takes.  References are
cached per (entry, sizes, seed): shifts never change them."""
from __future__ import annotations

import functools
import itertools
import math

import numpy as np
import torch

import checker_ref as CR
import msssim_ref64 as M
import rate_device_ref as RD
import ref64
import resample_ref as RR
import window_ref as WR
from ref64 import wide

N_LIST = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 1027)
U8_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)
PEDESTAL = float(2.0 ** -36)
BOUNDS = (float(np.float32((1e-6 + PEDESTAL) ** 0.5)), float(np.float32(PEDESTAL ** 0.5)))   # beta's, gamma's
SLOPE = 0.01
BOUND = ref64.BOUND
PASS_MAX_JOBS = 32           # LIC_PASS_MAX_JOBS
AD_ITEMS = 4096              # elements per block of the lic_adam_plan partition
GMM_WAVE_MAX = 32768         # lic_gmm_cdf_tables: P * M <= 32768 takes the wave-per-element kernel, above it the
#                              thread-per-element loop (lic_elementwise.hip, `if (P * M <= 32768)`)
LR, BETAS, EPS, WD = 3e-3, (0.9, 0.999), 1e-8, 0.01
ADAM_STEP = 3                # the 1-based update number the Adam case performs (bias corrections of step 3)

# group -> entries, as the issue lists them
GROUPS = {
    "a": ("lic_leaky_bwd", "lic_gdn_dnorm", "lic_anchor_add", "lic_rd_loss_bwd", "lic_rd_loss_bwd_lam"),
    "b": ("lic_mul_inplace", "lic_quantize", "lic_quantize_anchor", "lic_permute3", "lic_gdn_reparam",
          "lic_gdn_reparam_bwd", "lic_gdn_reparam_bwd2", "lic_gdn_reparam_bwd2_late", "lic_gdn_pass_batch",
          "lic_entropy_params_fwd", "lic_entropy_params_bwd", "lic_gmm_likelihood_fwd", "lic_gmm_likelihood_bwd",
          "lic_factorized_fwd", "lic_factorized_bwd", "lic_factorized_channel_logits", "lic_fe_pack", "lic_fe_unpack",
          "lic_colsum"),
    "c": ("lic_quantize_bf16", "lic_quantize_anchor_bf16", "lic_leaky_bwd_bf16", "lic_gdn_dnorm_bf16"),
    "d": ("lic_u8_to_f32", "lic_tensor_stats", "lic_window_u8_to_f32", "lic_window_f32", "lic_resample_u8_to_f32"),
    "e": ("lic_msssim", "lic_msssim_bwd"),
    "f": ("lic_factorized_cdf_tables", "lic_gmm_cdf_tables"),
    "g": ("lic_adam_run", "lic_swap_run"),
}
ENTRIES = tuple(e for g in GROUPS.values() for e in g)
GROUP_OF = {e: g for g, es in GROUPS.items() for e in es}

# the operands whose alignment decides (or could decide) the path an entry takes, in the order of Case.shifts
OPERANDS = {
    "lic_leaky_bwd": ("y", "dy", "dx"),
    "lic_gdn_dnorm": ("g", "x", "norm", "t"),
    "lic_anchor_add": ("g", "g_anchor", "out"),
    "lic_rd_loss_bwd": ("x_hat", "x", "dx_hat", "dlogp_y", "dlogp_z"),
    "lic_rd_loss_bwd_lam": ("x_hat", "x", "dx_hat", "dlogp_y", "dlogp_z"),
    "lic_adam_run": ("p", "g", "m", "v"),
    "lic_swap_run": ("p", "e"),
}

# group c: what the bf16 entries' own tests already hold between fences.  Neither runs the n list below 8 or the
# sizes the entries must refuse, so the cases here are not repeated ones.
ALREADY_FENCED = {
    "lic_quantize_anchor_bf16": "test_gpu_checker_kernels.py::test_quantize_anchor_bf16_casts_exactly (n = 4, 120, 224; "
                                "fp32 and bf16 outputs between fences)",
    "lic_leaky_bwd_bf16": "test_gpu_bf16_reductions.py::test_leaky_bwd_bf16_exact (n = 8, 16, 2040, 2048, 2056; 8 "
                          "sentinels on either side)",
    "lic_gdn_dnorm_bf16": "test_gpu_bf16_reductions.py::test_gdn_dnorm_bf16_vs_float64 (the same n and sentinels)",
    "lic_quantize_bf16": None,
}


class Case:
    """entry, sizes (dict), shifts (one per OPERANDS[entry]; a single number: every operand), seed, band (the statement
    and band of the entry's value test)"""

    def __init__(self, entry, sizes, shifts, seed, band):
        self.entry, self.sizes, self.shifts, self.seed, self.band = entry, dict(sizes), shifts, seed, band

    @property
    def key(self):
        return (self.entry, tuple(sorted((k, _hashable(v)) for k, v in self.sizes.items())), self.seed)

    @property
    def id(self):
        s = ",".join(f"{k}={v}" for k, v in self.sizes.items())
        return f"{self.entry}[{s};shift={self.shifts}]"

    def shift(self, name):
        if isinstance(self.shifts, int):
            return self.shifts
        return self.shifts[OPERANDS[self.entry].index(name)] if name in OPERANDS.get(self.entry, ()) else 0

    def __repr__(self):
        return self.id


def _hashable(v):
    return tuple(_hashable(u) for u in v) if isinstance(v, (list, tuple)) else v


def shift_combos(k):
    """every operand independently at 0 or 1, then all at 2 and all at 3"""
    return [tuple(c) for c in itertools.product((0, 1), repeat=k)] + [(2,) * k, (3,) * k]


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def randn(shape, seed):
    """test_gpu_latent_ops.py's"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def reparam_inputs(n, bound, seed):
    """test_gpu_latent_ops.py's parameters of a GDN re-parametrisation: most well above the bound, 15 % below it, 1 %
    exactly on it; here element 0 is below it and element n - 1 exactly on it whatever n is"""
    g = torch.Generator().manual_seed(seed)
    p = torch.sqrt(torch.rand(n, generator=g) * 1.5 + 1e-4)
    u = torch.rand(n, generator=g)
    p = torch.where(u < 0.15, torch.full_like(p, bound * 0.25), p)
    p = torch.where((u >= 0.15) & (u < 0.16), torch.full_like(p, bound), p)
    p[0] = bound * 0.25
    p[n - 1] = bound
    return p


def quantize_inputs(shape, seed):
    """test_gpu_checker_kernels.py's: exact ties, signed zeros and small negatives (rint gives -0.0) among random
    values"""
    r = np.random.RandomState(seed)
    n = int(np.prod(shape))
    v = (r.randn(n) * 4).astype(np.float32)
    special = np.array([0.5, -0.5, 1.5, 2.5, -0.0, 0.0, -0.3, 0.49999997], np.float32)
    at = r.permutation(n)[:min(n, special.size)]
    v[at] = special[:at.size]
    return v.reshape(shape), r.rand(*shape).astype(np.float32)


def quantize_want(v, u, training):
    return (v + (u - np.float32(0.5))).astype(np.float32) if training else np.rint(v).astype(np.float32)


def image_u8(h, w, seed, c=3):
    """test_gpu_window.py's"""
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def factor3(n):
    """n = n0 * n1 * n2, the prime factors dealt out in turn"""
    d, f, m = [1, 1, 1], 2, n
    k = 0
    while m > 1:
        while m % f:
            f += 1
        d[k % 3] *= f
        m //= f
        k += 1
    return tuple(sorted(d))


def nhwc_shape(n):
    """(B, h, w, C) with B * h * w * C == n: the first C of 3, 4, 2, 1 that divides n, then a near-square image"""
    C = next(c for c in (3, 4, 2, 1) if n % c == 0)
    p = n // C
    h = max(d for d in range(1, int(math.isqrt(p)) + 1) if p % d == 0)
    return (1, h, p // h, C)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------------------
# a. 16-byte path with scalar tail
# ---------------------------------------------------------------------------------------------------------------------
def _cases_leaky():
    return [Case("lic_leaky_bwd", {"n": n}, s, 500 + n, "exact: test_gpu_latent_ops.py::test_leaky_bwd_exact")
            for n in N_LIST for s in shift_combos(3)]


def _make_leaky(c):
    n = c.sizes["n"]
    y, dy = randn(n, c.seed), randn(n, c.seed + 1)
    y[::5] = 0.0             # y == 0 takes the slope side
    y[1::5] = -0.0
    return {"y": y, "dy": dy}, {"dx": torch.where(y > 0, dy, dy * SLOPE)}


def _cases_dnorm():
    return [Case("lic_gdn_dnorm", {"n": n, "inverse": inv}, s, 580 + n,
                 "close(1e-4, 1e-6) to float64: test_gpu_latent_ops.py::test_gdn_dnorm_vs_float64")
            for inv in (0, 1) for n in N_LIST for s in shift_combos(4)]


def _make_dnorm(c):
    n, inverse = c.sizes["n"], c.sizes["inverse"]
    g, x = randn(n, c.seed), randn(n, c.seed + 1)
    norm = torch.rand(n, generator=torch.Generator().manual_seed(c.seed + 2)) * 4 + 0.05
    g64, x64, n64 = wide(g, x, norm)
    ref = 0.5 * g64 * x64 / n64.sqrt() if inverse else -0.5 * g64 * x64 * n64 ** -1.5
    return {"g": g, "x": x, "norm": norm}, {"t": ref}


# pixel count -> (B, h, w): odd and even sides, more than one image
PIXEL_SHAPES = {1: [(1, 1, 1)], 2: [(1, 1, 2), (2, 1, 1)], 3: [(1, 1, 3), (1, 3, 1)], 85: [(1, 5, 17)],
                341: [(1, 11, 31)], 64: [(1, 8, 8), (2, 4, 8)], 256: [(1, 16, 16), (4, 8, 8)], 32: [(1, 4, 8), (2, 4, 4)],
                128: [(2, 8, 8), (1, 8, 16)]}


def anchor_add_shapes():
    """every (B, h, w, C), C in {3, 4, 8}, whose element count is one of N_LIST"""
    return [(B, h, w, C) for C in (3, 4, 8) for n in N_LIST if n % C == 0 for B, h, w in PIXEL_SHAPES[n // C]]


def _cases_anchor_add():
    band = "exact: test_gpu_checker_kernels.py::test_anchor_add_is_the_backward_of_both_outputs"
    return [Case("lic_anchor_add", {"B": B, "h": h, "w": w, "C": C}, s, 5 + B * h * w * C, band)
            for B, h, w, C in anchor_add_shapes() for s in shift_combos(3)]


def _make_anchor_add(c):
    shape = tuple(c.sizes[k] for k in "BhwC")
    r = np.random.RandomState(c.seed)
    g, ga = r.randn(*shape).astype(np.float32), r.randn(*shape).astype(np.float32)
    g.ravel()[:2] = (-0.0, 0.0)[:min(2, g.size)]
    return {"g": _t(g), "g_anchor": _t(ga)}, {"out": _t((g + CR.anchor_nhwc(ga)).astype(np.float32))}


RD_SIZES = [(B, nx, ny, nz) for B in (1, 3) for nx in (3, 4, 12, 1035) for ny in (1, 5) for nz in (1, 5)]
RD_LAMBDA, RD_UP = 0.013, 1.7
RD_LAMBDAS = np.array([0.013, 0.0, 0.05], np.float32)


def _cases_rd(entry):
    band = ("dlogp close(1e-5, 0), dx_hat close(1e-4, 1e-9) to float64: test_gpu_latent_ops.py::test_rd_loss_vs_float64"
            if entry == "lic_rd_loss_bwd" else
            "dlogp as lic_rd_loss_bwd's; dx_hat exact, (x_hat - x) * fl32(gl * kx_b): "
            "test_gpu_rate_device_kernels.py::test_per_image_loss_backward")
    return [Case(entry, {"B": B, "nx": nx, "ny": ny, "nz": nz}, s, 300 + B + nx, band)
            for B, nx, ny, nz in RD_SIZES for s in shift_combos(5)]


@functools.lru_cache(maxsize=None)
def _rd_reference(B, nx, ny, nz, seed, per_image):
    g = torch.Generator().manual_seed(seed)
    logp_y = torch.log(torch.rand((B, ny, 1, 1), generator=g) * 0.999 + 1e-3)
    logp_z = torch.log(torch.rand((B, nz, 1, 1), generator=g) * 0.999 + 1e-3)
    x = torch.rand((B, 1, 1, nx), generator=g)            # (one row of nx "pixels": num_pixels = nx)
    x_hat = x + 0.05 * torch.randn((B, 1, 1, nx), generator=g)
    refs = [t.requires_grad_(True) for t in wide(logp_y, logp_z, x_hat)]
    lam = RD_LAMBDAS[:B].copy()
    if per_image:
        r = ref64.rd_loss(*refs, wide(x), 0.0)
        loss = r["loss"] + (_t(lam).double() * 255.0 ** 2 * r["mse_per_image"]).mean()
    else:
        loss = ref64.rd_loss(*refs, wide(x), RD_LAMBDA)["loss"]
    (loss * RD_UP).backward()
    inputs = {"x_hat": x_hat.reshape(-1), "x": x.reshape(-1), "gl": torch.tensor([RD_UP])}
    want = {"dlogp_y": refs[0].grad.reshape(-1), "dlogp_z": refs[1].grad.reshape(-1), "dx_hat": refs[2].grad.reshape(-1)}
    if per_image:
        inputs["lambda_img"] = _t(lam)
        xh, xx = x_hat.reshape(B, nx).numpy(), x.reshape(B, nx).numpy()
        k = [np.float32(np.float32(RD_UP) * RD.kx32(float(v), nx, B)) for v in lam]
        want["dx_hat_exact"] = _t(np.stack([(xh[b] - xx[b]).astype(np.float32) * k[b] for b in range(B)]).reshape(-1))
    return inputs, want


def _make_rd(c):
    s = c.sizes
    return _rd_reference(s["B"], s["nx"], s["ny"], s["nz"], c.seed, c.entry == "lic_rd_loss_bwd_lam")


# ---------------------------------------------------------------------------------------------------------------------
# b. one element per lane
# ---------------------------------------------------------------------------------------------------------------------
def _flat(entry, band, seed0, extra=({},)):
    return [Case(entry, {"n": n, **e}, s, seed0 + n, band) for e in extra for n in N_LIST for s in (0, 1)]


def _make_mul(c):
    n = c.sizes["n"]
    w, mask = randn(n, c.seed), (randn(n, c.seed + 1) > 0).float()
    return {"w": w, "mask": mask}, {"w": w * mask}


def _make_quantize(c):
    n, training = c.sizes["n"], c.sizes["training"]
    v, u = quantize_inputs((n,), c.seed)
    return {"v": _t(v), "u": _t(u)}, {"out": _t(quantize_want(v, u, training))}


def _make_quantize_anchor(c):
    shape, training = nhwc_shape(c.sizes["n"]), c.sizes["training"]
    v, u = quantize_inputs(shape, c.seed)
    out = quantize_want(v, u, training)
    return {"v": _t(v), "u": _t(u)}, {"out": _t(out), "out_anchor": _t(CR.anchor_nhwc(out))}


PERMS = ((2, 0, 1), (1, 2, 0), (0, 2, 1))


def _make_permute3(c):
    src = randn(factor3(c.sizes["n"]), c.seed)
    return {"src": src}, {f"dst{p}": src.permute(p).contiguous() for p in PERMS}


def _make_reparam(c):
    n, bound = c.sizes["n"], BOUNDS[c.sizes["which"]]
    p = reparam_inputs(n, bound, c.seed)
    v = torch.clamp_min(p, bound)
    want = v * v - PEDESTAL
    fused = (v.double() * v.double() - PEDESTAL).float()
    return {"p": p}, {"out": want, "fused": fused, "at_bound": p <= bound}


def _reparam_bwd_want(p, d, bound):
    gr = d * 2.0 * torch.clamp_min(p, bound)
    return gr, torch.where((p >= bound) | (gr < 0), gr, torch.zeros_like(gr))


def _reparam_pair(n, bound, seed):
    """parameters and gradients; where the parameter sits on or below the bound both signs of the gradient occur"""
    p, d = reparam_inputs(n, bound, seed), randn(n, seed + 1)
    if n >= 2:
        d[0], d[n - 1] = abs(d[0]) + 0.1, -abs(d[n - 1]) - 0.1
    return p, d


def _make_reparam_bwd(c):
    p, d = _reparam_pair(c.sizes["n"], BOUNDS[c.sizes["which"]], c.seed)
    return {"p": p, "dout": d}, {"dp": _reparam_bwd_want(p, d, BOUNDS[c.sizes["which"]])[1]}


def next_n(n):
    return N_LIST[(N_LIST.index(n) + 4) % len(N_LIST)]


def _make_reparam_bwd2(c):
    nb, ng = c.sizes["n"], c.sizes["ng"]
    late = c.sizes.get("late", (0, 0))
    inputs, want = {}, {}
    for k, (name, m) in enumerate((("b", nb), ("g", ng))):
        p, d = _reparam_pair(m, BOUNDS[k], c.seed + 10 * k)
        lin, passed = _reparam_bwd_want(p, d, BOUNDS[k])
        inputs["p" + name], inputs["do" + name] = p, d
        want["dp" + name] = lin if late[k] else passed
    return inputs, want


PASS_LENGTHS = (1, 255, 257)


def _cases_pass_batch():
    band = "exact: test_gpu_latent_ops.py::test_gdn_reparam_late_pass_through_exact"
    return [Case("lic_gdn_pass_batch", {"njobs": j}, s, 545 + j, band) for j in (1, 2, PASS_MAX_JOBS) for s in (0, 1)]


def _make_pass_batch(c):
    inputs, want = {"bounds": []}, {}
    for j in range(c.sizes["njobs"]):
        n, bound = PASS_LENGTHS[j % 3], BOUNDS[j % 2]
        p, d = _reparam_pair(n, bound, c.seed + 7 * j)
        lin, passed = _reparam_bwd_want(p, d, bound)
        inputs[f"p{j}"], inputs[f"g{j}"] = p, lin
        inputs["bounds"].append(bound)
        want[f"g{j}"] = passed
    return inputs, want


PIXEL_CASES = [(P, Mm, K) for P in (1, 3, 257) for Mm in (1, 3, 5, 8) for K in (1, 2, 3, 8)]


def rows(t):
    """NCHW [1, CH, P, 1] -> the NHWC rows [P][CH] the entries take"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[2], t.shape[1]).contiguous()


def unrows(t, P):
    """[P][CH] -> NCHW [1, CH, P, 1]"""
    return t.reshape(1, P, 1, -1).permute(0, 3, 1, 2).contiguous()


def _cases_pixel(entry, band, seed0):
    return [Case(entry, {"P": P, "M": Mm, "K": K}, s, seed0 + 100 * P + 10 * Mm + K, band)
            for P, Mm, K in PIXEL_CASES for s in (0, 1)]


@functools.lru_cache(maxsize=None)
def _entropy_reference(P, Mm, K, seed):
    raw = ref64.entropy_raw(1, Mm, P, 1, K, seed)
    cot = ref64.cotangents(raw.shape, seed + 51)[0]
    r64 = wide(raw).requires_grad_(True)
    out64 = ref64.entropy_params(r64, Mm, K)
    (draw64,) = torch.autograd.grad(out64, r64, wide(cot))
    out32 = ref64.entropy_params(raw, Mm, K)          # the fp32 restatement: the backward entry's `out` operand
    return ({"raw": rows(raw), "out": rows(out32), "dout": rows(cot)},
            {"out": rows(out64.detach()), "draw": rows(draw64)})


def _make_entropy(c):
    s = c.sizes
    return _entropy_reference(s["P"], s["M"], s["K"], c.seed)


@functools.lru_cache(maxsize=None)
def _gmm_reference(P, Mm, K, seed):
    x, params, _, _ = ref64.gmm_inputs(1, Mm, P, 1, K, seed)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    p, logp, p_raw, grads = ref64.gmm_reference(x, params, K, gp, glogp)
    return ({"x": rows(x), "params": rows(params), "dp": rows(gp), "dlogp": rows(glogp)},
            {"ref": (p, logp, grads, p_raw)})


def _make_gmm(c):
    s = c.sizes
    return _gmm_reference(s["P"], s["M"], s["K"], c.seed)


FE_SIZES = [(C, P) for C in (1, 3, 5) for P in (1, 255, 256, 257, 513)]
FE_TENSORS = [("matrices", 4), ("biases", 4), ("factors", 3)]


def fe_packed(state):
    """the eleven tensors [C][out][in] -> the [C][43] operand: matrices (3, 9, 9, 3) | biases (3, 3, 3, 1) | factors
    (3, 3, 3), each in its own row-major order"""
    C = state[0][0].shape[0]
    return torch.cat([t.reshape(C, -1) for grp in state for t in grp], dim=1).contiguous()


# The parameter gradients are held to 1e-4 of each tensor's own maximum.  With one channel the last bias's gradient is
# ONE number, a sum over the pixels whose terms cancel: at the seeds 200 + 10 C + P of (C, P) = (1, 1) and (1, 257) it
# is 1e-4 and 1e-2 where its terms are of order 1, and fp32 cannot hold the band there -- torch's fp32 autograd on the
# host is 1.2e-3 of the maximum off at both, the kernel 1.9e-3 at (1, 1).  A case says something about the kernel only
# where fp32 arithmetic can hold the band at all, so tests/test_fence_cases.py requires the fp32 host restatement of
# every case to hold it, and these two sizes have seeds at which it does (3.5e-6 and 1.6e-5 of the maximum).
FE_SEEDS = {(1, 1): 1211, (1, 257): 1468}


def _cases_fe(entry, band):
    return [Case(entry, {"C": C, "P": P}, s, FE_SEEDS.get((C, P), 200 + 10 * C + P), band)
            for C, P in FE_SIZES for s in (0, 1)]


@functools.lru_cache(maxsize=None)
def _fe_reference(C, P, seed):
    state = ref64.fe_state(C, seed)
    x = ref64.fe_inputs((1, C, P, 1), seed)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    want = {}
    for mode, rp in (("logp", None), ("both", gp)):
        p64, logp64, dx64, gr64 = ref64.fe_reference(x, state, rp, glogp)
        want[mode] = {"p": rows(p64), "logp": rows(logp64), "dx": rows(dx64), "grads": gr64}
    return {"x": rows(x), "fe_params": fe_packed(state), "dp": rows(gp), "dlogp": rows(glogp)}, want


def fe_fp32_restatement_error(C, P, seed):
    """worst error, of its tensor's maximum, of a parameter gradient that torch's fp32 autograd forms on the host"""
    state = ref64.fe_state(C, seed)
    x = ref64.fe_inputs((1, C, P, 1), seed)
    gp, glogp = ref64.cotangents(x.shape, seed + 1)
    worst = 0.0
    for rp in (None, gp):
        r64 = ref64.fe_reference(x, state, rp, glogp)
        r32 = ref64.fe_reference(x, state, rp, glogp, dtype=torch.float32)
        worst = max([worst] + [ref64.norm_err(a, b) for a, b in zip(r32[3], r64[3])])
    return worst


def _make_fe(c):
    return _fe_reference(c.sizes["C"], c.sizes["P"], c.seed)


def fe_logits64(state, ch, xs):
    """channel_logits_cumulative of channel `ch` in float64 (ref64.factorized's inner function on one channel)"""
    import torch.nn.functional as F
    mats, bs, fs = ([t[ch:ch + 1].double() for t in grp] for grp in state)
    v = xs.double().reshape(1, 1, -1)
    for i in range(4):
        v = torch.matmul(F.softplus(mats[i]), v) + bs[i]
        if i < 3:
            v = v + torch.tanh(fs[i]) * torch.tanh(v)
    return v.reshape(-1)


def _make_channel_logits(c):
    n = c.sizes["n"]
    state = ref64.fe_state(3, c.seed)
    xs = ref64.fe_inputs((n,), c.seed)
    return {"fe_params": fe_packed(state), "xs": xs, "ch": n % 3}, {"cdf": torch.sigmoid(fe_logits64(state, n % 3, xs))}


FE_PACK_C = (1, 3, 5, 6)     # 43, 129, 215 and 258 floats: one block of 256 lanes and one float more


def _make_fe_pack(c):
    state = ref64.fe_state(c.sizes["C"], c.seed)
    inputs = {f"t{k}": t.reshape(-1).contiguous() for k, t in enumerate(t for grp in state for t in grp)}
    return inputs, {"packed": fe_packed(state).reshape(-1)}


def _make_fe_unpack(c):
    C = c.sizes["C"]
    dpacked = randn((C, 43), c.seed)
    widths, at, blocks = [3, 9, 9, 3, 3, 3, 3, 1, 3, 3, 3], 0, []
    for wd in widths:           # parameter k's [C][n_k] block at C * prefix_k
        blocks.append(dpacked[:, at:at + wd].reshape(-1))
        at += wd
    return {"dpacked": dpacked.reshape(-1)}, {"flat": torch.cat(blocks)}


# (ld - C, col0): packed rows; pitched rows that keep the 16-byte path where C % 4 == 0; pitched rows that do not
COLSUM_PITCH = ((0, 0), (8, 4), (3, 1))
COLSUM_SIZES = [(P, C) for C in (1, 3, 4, 64, 70) for P in (1, 15, 16, 17, 4099)]
COLSUM_SCALE = 0.37


def _cases_colsum():
    band = "close_norm(1e-4) to float64: test_gpu_latent_ops.py::test_colsum_vs_float64"
    out = []
    for P, C in COLSUM_SIZES:
        for pad, col0 in COLSUM_PITCH:
            for s in ((0, 1) if pad == 0 else (0,)):
                out.append(Case("lic_colsum", {"P": P, "C": C, "ld": C + pad, "col0": col0}, s, 400 + C + P, band))
    return out


def _make_colsum(c):
    P, C = c.sizes["P"], c.sizes["C"]
    src = randn((P, C), c.seed) + 0.1
    return {"in": src}, {"out": src.double().sum(0) * COLSUM_SCALE}


# ---------------------------------------------------------------------------------------------------------------------
# c. bf16 elementwise.  n % 8 (leaky, dnorm) or n % 4 (quantize) must be 0: every other n of the list is a refusal,
# LIC_ERR_UNSUPPORTED, that must leave the guarded outputs untouched.
# ---------------------------------------------------------------------------------------------------------------------
BF = torch.bfloat16


def bf16_legal(entry, n):
    return n % (4 if "quantize" in entry else 8) == 0


def _cases_bf16():
    out = []
    for n in N_LIST:
        for tr in (0, 1):
            out.append(Case("lic_quantize_bf16", {"n": n, "training": tr}, 0, 17 + n,
                            "exact, bf16 copies round-to-nearest-even: test_gpu_checker_kernels.py::"
                            "test_quantize_anchor_bf16_casts_exactly"))
            out.append(Case("lic_quantize_anchor_bf16", {"n": n, "training": tr}, 0, 17 + n,
                            "exact, bf16 copies round-to-nearest-even: test_gpu_checker_kernels.py::"
                            "test_quantize_anchor_bf16_casts_exactly"))
        out.append(Case("lic_leaky_bwd_bf16", {"n": n}, 0, n,
                        "exact: test_gpu_bf16_reductions.py::test_leaky_bwd_bf16_exact"))
        for inv in (0, 1):
            out.append(Case("lic_gdn_dnorm_bf16", {"n": n, "inverse": inv}, 0, n + inv,
                            "bf16_close (2^-8 relative + its scale floor) to float64: test_gpu_bf16_reductions.py::"
                            "test_gdn_dnorm_bf16_vs_float64"))
    return out


def rne_bf16(a):
    return _t(np.ascontiguousarray(a)).to(BF)


def _make_quantize_bf16(c):
    n, training = c.sizes["n"], c.sizes["training"]
    shape = nhwc_shape(n) if "anchor" in c.entry else (n,)
    v, u = quantize_inputs(shape, c.seed)
    out = quantize_want(v, u, training)
    want = {"out": _t(out), "v_bf16": rne_bf16(v), "out_bf16": rne_bf16(out)}
    if "anchor" in c.entry:
        anc = CR.anchor_nhwc(out)
        want.update(out_anchor=_t(anc), anchor_bf16=rne_bf16(anc))
    return {"v": _t(v), "u": _t(u)}, want


def _make_leaky_bf16(c):
    n = c.sizes["n"]
    gen = torch.Generator().manual_seed(c.seed)
    y = torch.randn(n, generator=gen).to(BF)
    special = torch.tensor([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -127, -2.0 ** -127, 1.0, -1.0]).to(BF)
    y[:min(n, 8)] = special[:min(n, 8)]
    dy = torch.randn(n, generator=gen).to(BF)
    low = (dy.float() * torch.tensor(SLOPE, dtype=torch.float32)).to(BF)
    return {"y": y, "dy": dy}, {"dx": torch.where(y.float() > 0, dy, low)}


def _make_dnorm_bf16(c):
    n, inverse = c.sizes["n"], c.sizes["inverse"]
    gen = torch.Generator().manual_seed(c.seed)
    g, x = torch.randn(n, generator=gen).to(BF), torch.randn(n, generator=gen).to(BF)
    norm = (torch.rand(n, generator=gen) * 4 + 0.05).to(BF)
    g64, x64, n64 = g.double(), x.double(), norm.double()
    want = 0.5 * g64 * x64 / n64.sqrt() if inverse else -0.5 * g64 * x64 * n64 ** -1.5
    return {"g": g, "x": x, "norm": norm}, {"t": want}


# ---------------------------------------------------------------------------------------------------------------------
# d. input pipeline and statistics
# ---------------------------------------------------------------------------------------------------------------------
def _cases_u8():
    band = "exact, float(v) / 255: test_gpu_latent_ops.py::test_u8_to_f32_exact"
    ok = [Case("lic_u8_to_f32", {"n": n, "refuse": ""}, 0, 810 + n, band) for n in U8_N]
    bad = [Case("lic_u8_to_f32", {"n": n, "refuse": r}, 0, 810 + n, "LIC_ERR_INVALID, nothing written: include/lic.h")
           for n in (5, 1024) for r in ("out+1", "out+2", "out+3", "in+1", "in+2", "in+3")]
    return ok + bad


def _make_u8(c):
    t = _t(np.random.RandomState(c.seed).randint(0, 256, size=c.sizes["n"]).astype(np.uint8))
    return {"in": t}, {"out": t.float() / 255}


STATS_SIZES = [(n, nbins) for n in (1, 255, 2048, 2049) for nbins in (1, 64, 4096)]


def _cases_stats():
    band = ("count, NaN count, min, max exact; mean within 1e-9, std within 1e-7; histogram total exact and within 2 "
            "counts of the fp32 bins: test_data_pipeline.py::test_tensor_stats_vs_numpy")
    return [Case("lic_tensor_stats", {"n": n, "nbins": nb}, s, 800 + n, band) for n, nb in STATS_SIZES for s in (0, 1)]


STATS_LO, STATS_HI = -8.0, 10.0


def _make_stats(c):
    n, nbins = c.sizes["n"], c.sizes["nbins"]
    a = (np.random.RandomState(c.seed).randn(n) * 3 + 1).astype(np.float32)
    if n > 1:                       # NaNs in the first, the last and one middle element
        a[0] = a[n - 1] = a[n // 2] = np.nan
    v = a[~np.isnan(a)].astype(np.float64)
    lo, hi = np.float32(STATS_LO), np.float32(STATS_HI)
    b = np.floor((v.astype(np.float32) - lo) * (np.float32(nbins) / (hi - lo))).astype(np.int64)
    want = {"count": v.size, "nan": int(np.isnan(a).sum()), "mean": v.mean(), "std": v.std(), "min": v.min(),
            "max": v.max(), "hist": np.bincount(np.clip(b, 0, nbins - 1), minlength=nbins)}
    return {"x": _t(a)}, want


WINDOWS = [(5, 7), (8, 8)]
WINDOW_IMAGES = [(20, 31), (33, 17), (9, 40)]
# (image, y0, x0): inside, over the top / left, over the bottom / right, over all four sides of the smallest image
WINDOW_ROWS = [(0, 3, 5), (1, -4, 2), (2, 1, -3), (0, 14, 26), (1, -2, -2), (2, 2, 33), (0, 0, 0)]


def _cases_window(entry):
    band = {"lic_window_u8_to_f32": "exact: test_gpu_window.py::test_overhanging_flipped_and_ragged_tail_windows",
            "lic_window_f32": "exact: test_gpu_window.py::test_window_f32_matches_torch_pad_for_every_layout",
            "lic_resample_u8_to_f32": "exact: test_gpu_resample.py (resample_ref.resample_window_f32)"}[entry]
    out = []
    for (h, w), C, flip in itertools.product(WINDOWS, (1, 3), (0, 1)):
        borders = (None,) if entry == "lic_resample_u8_to_f32" else (WR.ZERO, WR.REPLICATE, WR.REFLECT)
        if entry == "lic_window_f32" and flip:
            continue                 # (lic_window_f32 has no flip)
        for border in borders:
            sizes = {"h": h, "w": w, "C": C, "flip": flip}
            if border is not None:
                sizes["border"] = border
            if entry == "lic_window_f32":
                for layout in ("nchw", "nhwc", "view"):
                    out.append(Case(entry, {**sizes, "layout": layout}, 0, 21 + h + C, band))
            else:
                out.append(Case(entry, sizes, 0, 21 + h + C, band))
    return out


def _make_window_u8(c):
    s = c.sizes
    images = [image_u8(H, W, c.seed + i, s["C"]) for i, (H, W) in enumerate(WINDOW_IMAGES)]
    rows_ = [(i, y, x, s["flip"]) for i, y, x in WINDOW_ROWS]
    ref = np.stack([WR.window_ref(images[i], y, x, s["h"], s["w"], s["border"], bool(f)) for i, y, x, f in rows_])
    return {"images": images, "rows": rows_, "prefix": 5}, {"out": ref.astype(np.float32) / np.float32(255)}


WINDOW_F32_SRC = (2, 12, 15)          # B, Hs, Ws
WINDOW_F32_AT = [(-3, -4), (5, 6), (0, 0), (9, 11), (-2, 10)]     # (y0, x0): overhanging every side in turn


def _make_window_f32(c):
    s = c.sizes
    B, Hs, Ws = WINDOW_F32_SRC
    src = randn((B, s["C"], Hs, Ws), c.seed)
    a = src.permute(0, 2, 3, 1).numpy()
    want = {(y0, x0): np.stack([WR.window_ref(a[b], y0, x0, s["h"], s["w"], s["border"]) for b in range(B)])
            for y0, x0 in WINDOW_F32_AT}
    return {"src": src}, want


# (Hs, Ws) -> (Hn, Wn): a copy, the largest downscale (by 2), odd sizes in between
RESAMPLE_IMAGES = [((20, 31), (20, 31)), ((33, 40), (17, 20)), ((29, 23), (21, 16))]


def _make_resample(c):
    s = c.sizes
    h, w = s["h"], s["w"]
    images = [image_u8(H, W, c.seed + i, s["C"]) for i, ((H, W), _) in enumerate(RESAMPLE_IMAGES)]
    jobs = []
    for i, (_, (Hn, Wn)) in enumerate(RESAMPLE_IMAGES):
        for y0, x0 in ((0, 0), (Hn - h, Wn - w), ((Hn - h) // 2, 1)):      # first and last rows / columns, the middle
            jobs.append((i, Hn, Wn, y0, x0, s["flip"]))
    ref = np.stack([RR.resample_window_f32(images[i], Hn, Wn, y0, x0, h, w, bool(f)) for i, Hn, Wn, y0, x0, f in jobs])
    return {"images": images, "jobs": jobs, "prefix": 3}, {"out": ref}


# ---------------------------------------------------------------------------------------------------------------------
# e. MS-SSIM: the smallest legal sides, odd and even at every scale
# ---------------------------------------------------------------------------------------------------------------------
MS_SHAPES = [(1, 1, 161, 161), (2, 3, 162, 165), (1, 2, 193, 161)]
MS_LAYOUTS = ("nchw", "nhwc", "view")


def _cases_ms(entry):
    band = ("value within VALUE_BAND = 2e-5 of float64: test_msssim.py" if entry == "lic_msssim" else
            "dx within GRAD_BAND = 5e-4 of max |gradient| of float64 autograd: test_gpu_msssim_grad.py")
    return [Case(entry, {"B": B, "C": C, "H": H, "W": W, "layout": lay}, 0, 40 + H, band)
            for B, C, H, W in MS_SHAPES for lay in MS_LAYOUTS]


@functools.lru_cache(maxsize=None)
def _ms_reference(B, C, H, W, seed):
    x, y = M.pair(B, C, H, W, seed, 0.05)
    up = ref64.cotangents((B, C), seed + 1)[0] + 1.0               # gout, U(0.5, 1.5)
    X = wide(x).requires_grad_(True)
    per = M.ms_ssim_per_channel(X, wide(y), 1.0)
    (per * wide(up)).sum().backward()
    tmin = float(M.scale_terms(wide(x), wide(y), 1.0).min())
    return {"x": x, "y": y, "gout": up.reshape(-1)}, {"out": per.detach().reshape(-1), "dx": X.grad, "min_term": tmin}


def _make_ms(c):
    s = c.sizes
    return _ms_reference(s["B"], s["C"], s["H"], s["W"], c.seed)


# ---------------------------------------------------------------------------------------------------------------------
# f. coder tables
# ---------------------------------------------------------------------------------------------------------------------
FE_TABLE_SIZES = [(C, S) for C in (1, 5) for S in (2, 64, 65, 66, 129)]


def quantize_cdf64(F, S):
    """cum[i] = max_{j <= i} floor(clip(F_j, 0, 1) (65536 - S)) + i with cum[0] = 0, cum[S] = 65536 (include/lic.h)"""
    c = np.floor(np.clip(F, 0.0, 1.0) * (65536 - S)).astype(np.int64)
    c[:, 0] = 0
    c = np.maximum.accumulate(np.minimum(c, 65536 - S), axis=1)
    c[:, S] = 65536 - S
    return c + np.arange(S + 1)


def _cases_fe_tables():
    band = "within 1 count of the float64 table: test_gpu_codec_windows.py::test_factorized_tables_beyond_one_trip"
    return [Case("lic_factorized_cdf_tables", {"C": C, "S": S}, s, 31 + C, band) for C, S in FE_TABLE_SIZES for s in (0, 1)]


def _make_fe_tables(c):
    C, S = c.sizes["C"], c.sizes["S"]
    lo = -(S // 2)
    state = ref64.fe_state(C, c.seed)
    xs = torch.arange(lo, lo + S + 1, dtype=torch.float32) - 0.5
    F = np.stack([torch.sigmoid(fe_logits64(state, ch, xs)).numpy() for ch in range(C)])
    F[:, 0], F[:, S] = 0.0, 1.0
    return {"fe_params": fe_packed(state), "lo": lo}, {"out": quantize_cdf64(F, S)}


# the last: the smallest case above GMM_WAVE_MAX elements (P * M = 32769 with M = 1)
GMM_TABLE_SIZES = [(1, 1, 1, 1), (3, 5, 3, 8), (2, 4, 1, 32), (1, 3, 2, 33), (1, 2, 1, 64), (GMM_WAVE_MAX + 1, 1, 1, 1)]
GMM_TABLE_BAND = 2     # counts: FLOAT64_BAND of test_gpu_codec_windows.py


def _cases_gmm_tables():
    band = ("within 2 counts of the float64 table on the device's centre: test_gpu_codec_windows.py::"
            "test_gmm_tables_beyond_one_chunk")
    return [Case("lic_gmm_cdf_tables", {"P": P, "M": Mm, "K": K, "W": W}, s, 190 + 10 * K + W, band)
            for P, Mm, K, W in GMM_TABLE_SIZES for s in (0, 1)]


def gmm_blocks(params_rows, K, Mm):
    """[P][G*K*M] rows -> (weights, mus, sigmas) [K, P*M] in the table kernels' element order"""
    P = params_rows.shape[0]
    a = params_rows.numpy().reshape(P, -1, K, Mm)                     # [P][G][K][M]
    blk = [a[:, g].transpose(1, 0, 2).reshape(K, P * Mm) for g in range(a.shape[1])]
    return (np.ones_like(blk[0]), blk[0], blk[1]) if K == 1 else tuple(blk)


def gmm_tables64(w_, mu_, sg_, center, W):
    """test_gpu_codec_windows.py's float64 restatement, the window placed on the given centre"""
    S = 2 * W + 1
    x = center.astype(np.float64)[:, None] - W + np.arange(S + 1, dtype=np.float64)[None, :] - 0.5
    F = np.zeros_like(x)
    for k in range(mu_.shape[0]):
        t = (x - mu_[k].astype(np.float64)[:, None]) / sg_[k].astype(np.float64)[:, None]
        F += w_[k].astype(np.float64)[:, None] * (0.5 * (1.0 + torch.erf(_t(t / math.sqrt(2.0))).numpy()))
    return quantize_cdf64(F, S)


@functools.lru_cache(maxsize=None)
def _gmm_table_inputs(P, Mm, K, seed):
    _, params, _, _ = ref64.gmm_inputs(1, Mm, P, 1, K, seed)
    return rows(params)


def _make_gmm_tables(c):
    s = c.sizes
    pr = _gmm_table_inputs(s["P"], s["M"], s["K"], c.seed)
    w_, mu_, sg_ = gmm_blocks(pr, s["K"], s["M"])
    mean = np.zeros(mu_.shape[1], np.float32)
    for k in range(s["K"]):
        mean = mean + w_[k] * mu_[k]
    center = np.rint(mean).astype(np.int64)           # the host's centre; the GPU test places the window on the device's
    return {"params": pr, "blocks": (w_, mu_, sg_)}, {"center": center, "out": gmm_tables64(w_, mu_, sg_, center, s["W"])}


# ---------------------------------------------------------------------------------------------------------------------
# g. Adam
# ---------------------------------------------------------------------------------------------------------------------
ADAM_LENGTHS = (1, 3, 4, 5, 4095, 4096, 4097, 8193)


def _cases_adam():
    band = ("p within 1e-6 max|p| + 1e-5 lr per update, exp_avg_sq within 1e-6 of its maximum, of float64: "
            "test_gpu_latent_ops.py::test_fused_adam_vs_float64")
    out = []
    for i, s in enumerate(shift_combos(4)):
        lens = tuple(ADAM_LENGTHS[(3 * i + j) % len(ADAM_LENGTHS)] for j in (0, 3, 6))
        out.append(Case("lic_adam_run", {"lengths": lens}, s, 700 + i, band))
    # the 16-byte path is taken only where p, g, m and v are all aligned, and the element-by-element one has its own
    # loop: both run every length (the tail of 3 at 4095, none at 4 and 4096, two blocks and one element at 8193)
    for s in ((0, 0, 0, 0), (1, 1, 1, 1)):
        for i, lens in enumerate(((3, 4095, 8193), (4, 4096, 5), (1, 4097, 4095))):
            out.append(Case("lic_adam_run", {"lengths": lens}, s, 730 + 3 * s[0] + i, band))
    return out


def _make_adam(c):
    inputs, want = {}, {}
    bc = ADAM_STEP
    for j, n in enumerate(c.sizes["lengths"]):
        p, g = randn(n, c.seed + 10 * j), randn(n, c.seed + 10 * j + 1) * (0.1 + j)
        m, v = randn(n, c.seed + 10 * j + 2) * 0.1, randn(n, c.seed + 10 * j + 3) ** 2 * 0.01
        inputs.update({f"p{j}": p, f"g{j}": g, f"m{j}": m, f"v{j}": v})
        p64, m64, v64 = ref64.adam_step(wide(p), wide(g), wide(m), wide(v), bc, LR, BETAS, EPS, WD)
        want.update({f"p{j}": p64, f"m{j}": m64, f"v{j}": v64})
    return inputs, want


def _cases_swap():
    return [Case("lic_swap_run", {"lengths": (5, 4097, 8193)}, s, 760, "exact (loads and stores only): include/lic.h; "
                 "test_gpu_ema.py") for s in ((0, 1), (1, 0), (0, 0), (2, 3))]


def _make_swap(c):
    inputs, want = {}, {}
    for j, n in enumerate(c.sizes["lengths"]):
        inputs[f"p{j}"], inputs[f"e{j}"] = randn(n, c.seed + 2 * j), randn(n, c.seed + 2 * j + 1)
        want[f"p{j}"], want[f"e{j}"] = inputs[f"e{j}"], inputs[f"p{j}"]
    return inputs, want


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
_EXACT = "exact: "
CASES = {
    "lic_leaky_bwd": _cases_leaky(),
    "lic_gdn_dnorm": _cases_dnorm(),
    "lic_anchor_add": _cases_anchor_add(),
    "lic_rd_loss_bwd": _cases_rd("lic_rd_loss_bwd"),
    "lic_rd_loss_bwd_lam": _cases_rd("lic_rd_loss_bwd_lam"),
    "lic_mul_inplace": _flat("lic_mul_inplace", _EXACT + "test_gpu_latent_ops.py::test_mul_inplace_exact", 550),
    "lic_quantize": _flat("lic_quantize", _EXACT + "test_gpu_checker_kernels.py::"
                          "test_quantize_anchor_is_quantize_and_its_anchors", 7, ({"training": 0}, {"training": 1})),
    "lic_quantize_anchor": _flat("lic_quantize_anchor", _EXACT + "test_gpu_checker_kernels.py::"
                                 "test_quantize_anchor_is_quantize_and_its_anchors", 7, ({"training": 0}, {"training": 1})),
    "lic_permute3": _flat("lic_permute3", _EXACT + "test_gpu_latent_ops.py::test_permute3_exact", 570),
    "lic_gdn_reparam": _flat("lic_gdn_reparam", "within 1 ulp of the fp32 statement, the fused value on the bound: "
                             "test_gpu_latent_ops.py::test_gdn_reparam_one_ulp", 520, ({"which": 0}, {"which": 1})),
    "lic_gdn_reparam_bwd": _flat("lic_gdn_reparam_bwd", _EXACT + "the statement of test_gpu_latent_ops.py::"
                                 "test_gdn_reparam_bwd2_exact on one parameter", 530, ({"which": 0}, {"which": 1})),
    "lic_gdn_reparam_bwd2": [Case("lic_gdn_reparam_bwd2", {"n": n, "ng": next_n(n)}, s, 530 + n, _EXACT +
                                  "test_gpu_latent_ops.py::test_gdn_reparam_bwd2_exact") for n in N_LIST for s in (0, 1)],
    "lic_gdn_reparam_bwd2_late": [Case("lic_gdn_reparam_bwd2_late", {"n": n, "ng": next_n(n), "late": late}, s, 530 + n,
                                       _EXACT + "test_gpu_latent_ops.py::test_gdn_reparam_late_pass_through_exact")
                                  for n in N_LIST for late in ((1, 0), (0, 1), (1, 1)) for s in (0, 1)],
    "lic_gdn_pass_batch": _cases_pass_batch(),
    "lic_entropy_params_fwd": _cases_pixel("lic_entropy_params_fwd", "close(1e-4, 1e-6) to float64: "
                                           "test_gpu_latent_ops.py::test_entropy_params_activation_vs_float64", 1000),
    "lic_entropy_params_bwd": _cases_pixel("lic_entropy_params_bwd", "close_norm(1e-4) to float64 autograd: "
                                           "test_gpu_latent_ops.py::test_entropy_params_activation_vs_float64", 1000),
    "lic_gmm_likelihood_fwd": _cases_pixel("lic_gmm_likelihood_fwd", "ref64.check_gmm (P_BAND, LOGP_BAND): "
                                           "test_gpu_latent_ops.py::test_gmm_likelihood_vs_float64", 2000),
    "lic_gmm_likelihood_bwd": _cases_pixel("lic_gmm_likelihood_bwd", "ref64.check_gmm (GRAD_BAND, dw_band; exact zeros "
                                           "where clamped): test_gpu_latent_ops.py::test_gmm_likelihood_vs_float64", 2000),
    "lic_factorized_fwd": _cases_fe("lic_factorized_fwd", "p close(1e-4, 1.5e-7), logp close(1e-4, 1e-6) to float64: "
                                    "test_gpu_latent_ops.py::test_factorized_likelihood_vs_float64"),
    "lic_factorized_bwd": _cases_fe("lic_factorized_bwd", "dx and the eleven parameter gradients within 1e-4 of their "
                                    "maxima: test_gpu_latent_ops.py::test_factorized_likelihood_vs_float64"),
    "lic_factorized_channel_logits": _flat("lic_factorized_channel_logits", "sigmoid(logits) close(1e-5, 1e-7): "
                                           "test_gpu_parity.py::test_factorized_golden (cdf_ch2)", 210),
    "lic_fe_pack": [Case("lic_fe_pack", {"C": C}, s, 220 + C, _EXACT + "a gather; test_oracle_golden.py's fe_pack layout")
                    for C in FE_PACK_C for s in (0, 1)],
    "lic_fe_unpack": [Case("lic_fe_unpack", {"C": C}, s, 230 + C, _EXACT + "a scatter; test_oracle_golden.py's fe_unpack "
                           "layout") for C in FE_PACK_C for s in (0, 1)],
    "lic_colsum": _cases_colsum(),
    "lic_u8_to_f32": _cases_u8(),
    "lic_tensor_stats": _cases_stats(),
    "lic_window_u8_to_f32": _cases_window("lic_window_u8_to_f32"),
    "lic_window_f32": _cases_window("lic_window_f32"),
    "lic_resample_u8_to_f32": _cases_window("lic_resample_u8_to_f32"),
    "lic_msssim": _cases_ms("lic_msssim"),
    "lic_msssim_bwd": _cases_ms("lic_msssim_bwd"),
    "lic_factorized_cdf_tables": _cases_fe_tables(),
    "lic_gmm_cdf_tables": _cases_gmm_tables(),
    "lic_adam_run": _cases_adam(),
    "lic_swap_run": _cases_swap(),
}
for _c in _cases_bf16():
    CASES.setdefault(_c.entry, []).append(_c)

MAKERS = {
    "lic_leaky_bwd": _make_leaky, "lic_gdn_dnorm": _make_dnorm, "lic_anchor_add": _make_anchor_add,
    "lic_rd_loss_bwd": _make_rd, "lic_rd_loss_bwd_lam": _make_rd, "lic_mul_inplace": _make_mul,
    "lic_quantize": _make_quantize, "lic_quantize_anchor": _make_quantize_anchor, "lic_permute3": _make_permute3,
    "lic_gdn_reparam": _make_reparam, "lic_gdn_reparam_bwd": _make_reparam_bwd, "lic_gdn_reparam_bwd2": _make_reparam_bwd2,
    "lic_gdn_reparam_bwd2_late": _make_reparam_bwd2, "lic_gdn_pass_batch": _make_pass_batch,
    "lic_entropy_params_fwd": _make_entropy, "lic_entropy_params_bwd": _make_entropy,
    "lic_gmm_likelihood_fwd": _make_gmm, "lic_gmm_likelihood_bwd": _make_gmm,
    "lic_factorized_fwd": _make_fe, "lic_factorized_bwd": _make_fe,
    "lic_factorized_channel_logits": _make_channel_logits, "lic_fe_pack": _make_fe_pack, "lic_fe_unpack": _make_fe_unpack,
    "lic_colsum": _make_colsum, "lic_quantize_bf16": _make_quantize_bf16, "lic_quantize_anchor_bf16": _make_quantize_bf16,
    "lic_leaky_bwd_bf16": _make_leaky_bf16, "lic_gdn_dnorm_bf16": _make_dnorm_bf16, "lic_u8_to_f32": _make_u8,
    "lic_tensor_stats": _make_stats, "lic_window_u8_to_f32": _make_window_u8, "lic_window_f32": _make_window_f32,
    "lic_resample_u8_to_f32": _make_resample, "lic_msssim": _make_ms, "lic_msssim_bwd": _make_ms,
    "lic_factorized_cdf_tables": _make_fe_tables, "lic_gmm_cdf_tables": _make_gmm_tables, "lic_adam_run": _make_adam,
    "lic_swap_run": _make_swap,
}

_MADE = {}


def make(case):
    """(inputs, want) of a case, made once per (entry, sizes, seed)"""
    if case.key not in _MADE:
        _MADE[case.key] = MAKERS[case.entry](case)
    return _MADE[case.key]


def forget(entry):
    """drops the cached inputs and references of an entry (the GPU test frees them entry by entry)"""
    for k in [k for k in _MADE if k[0] == entry]:
        del _MADE[k]
