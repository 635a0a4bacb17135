"""Canary fences around every output, workspace and input of the latent, loss, metric, window, table and Adam entries,
called through the C ABI at the smallest sizes at which they can still go wrong (tests/fence_cases.py; its coverage is
stated on the CPU by tests/test_fence_cases.py).

For every case: the return code is LIC_OK; no output's fence, pitch column or (for a strided view) gap was written;
no element of an output the header calls fully written still holds the pattern; every input, fences included, is
bit for bit what was put there; and the values hold the statement and the band of the entry's own value test, which
the case table cites.  Inputs live inside the quiet-NaN pattern too, so a read past an operand's end does not hide in
allocator slack: it turns a value, a sum or a NaN count.

One line per entry is printed before anything is asserted.
Run on the MI355X box:  python -m pytest tests/test_gpu_fences.py -m gpu -q -s

One run on an MI355X: 39 passed in 5.78 s.  pytest --durations, the entries above 0.05 s (the rest 0.01 - 0.05 s):
  0.81 s lic_entropy_params_fwd (with the float64 references the _bwd entry shares)   0.65 s lic_rd_loss_bwd_lam
  0.57 s lic_rd_loss_bwd   0.35 s lic_leaky_bwd   0.19 s lic_gdn_dnorm   0.19 s lic_gmm_likelihood_bwd
  0.09 s lic_gmm_likelihood_fwd   0.08 s lic_factorized_fwd   0.07 s lic_msssim

  group  entries  cases  calls of the C ABI  worst ratio to its band
  a       5       3036     3036    0.0084  (lic_rd_loss_bwd dx_hat; leaky_bwd, anchor_add and the _lam dx_hat are exact)
  b      19       1016     1394    0.28    (lic_factorized_bwd; lic_gmm_likelihood 0.275; lic_gdn_reparam differs from the
                                            fp32 statement by its one allowed ulp; ten entries are exact)
  c       4        105      105    0.91    (lic_gdn_dnorm_bf16 against one bf16 rounding; the other three are exact)
  d       5        113      257    4e-9    (lic_tensor_stats mean / std; the other four are exact)
  e       2         18       27    0.091   (lic_msssim_bwd; lic_msssim 0.038)
  f       2         32       32    1.0     (lic_factorized_cdf_tables: its 1 count; lic_gmm_cdf_tables 1 count of its 2)
  g       2         28       28    0.21    (lic_adam_run p, exp_avg and exp_avg_sq; lic_swap_run is exact)

No fence tripped on any entry.  One finding, in a band and not in a kernel: lic_factorized_bwd at C = 1 holds the last
bias's gradient, ONE number per channel, to 1e-4 of itself; where that sum cancels to 1e-4 of its terms fp32 misses the
band on the host as on the device (fence_cases.FE_SEEDS has the sizes, the figures and the condition that
tests/test_fence_cases.py asserts on every case).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fence_cases as FC
import ref64
from guarded import Guarded, Guarded4D, GuardedBytes, words, workspace

pytestmark = pytest.mark.gpu

LIC_OK, LIC_ERR_INVALID, LIC_ERR_UNSUPPORTED = 0, -1, -2
WORST = {}         # entry -> worst ratio of a compared value to its band (0 where the statement is exact)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import data as D
    from neural_image_compression_amd import functional as F_
    return L, L.load(), F_, D, torch.device("cuda:0")   # L.load(): the in-tree HIP extension; raises if missing


def _ibits(t):
    """a CPU tensor's bits as integers of its element size"""
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(got, want, what):
    got, want = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a for a in (got, want))
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _ibits(got) != _ibits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {int(bad.nonzero()[0])}"


class Kit:
    """the operands of one case: inputs inside the pattern, outputs between fences; finish() is everything that holds
    for every entry"""

    def __init__(self, env, case):
        self.L, self.lib, self.F_, self.D, self.dev = env
        self.case, self.ins, self.outs, self.calls, self.buffers = case, [], [], 0, 0

    def word(self, inplace=False):
        """the pattern of the next buffer of this case: each its own (guarded.words)"""
        self.buffers += 1
        return words(self.buffers - 1, inplace)

    def inp(self, name, t, shift=None):
        """a flat operand of any type inside the pattern, `shift` elements off its alignment"""
        shift = self.case.shift(name) if shift is None else shift
        if t.dtype == torch.float32:
            g = Guarded.holding(t.reshape(1, -1), self.dev, shift=shift, word=self.word())
        else:
            g = GuardedBytes.holding(t, self.dev, shift=shift, word=self.word())
        self.ins.append((name, g, t))
        return g

    def keep(self, name, g, t):
        """an operand placed by the caller (pitched rows, a strided view)"""
        self.ins.append((name, g, t))
        return g

    def out(self, name, n, shift=None, dtype=torch.float32, full=True, g=None, start=None):
        """an output of n elements; full: the header calls every element written.  start: the operand an in-place
        entry finds there (its fences then hold finite floats, which the update of a lane too many changes)"""
        shift = self.case.shift(name) if shift is None else shift
        if g is None:
            word = self.word(inplace=start is not None)
            g = Guarded(1, n, self.dev, shift=shift, word=word) if dtype == torch.float32 else \
                GuardedBytes(n, dtype, self.dev, shift, word)
        if start is not None:
            g.t.copy_(start.reshape(1, -1))
            full = False
        self.outs.append((name, g, full))
        return g

    def call(self, fn, *args, rc=LIC_OK):
        got = fn(*args, self.F_._stream())
        self.calls += 1
        assert got == rc, f"{self.case.id}: {fn.__name__} returned {got}, not {rc}"

    def finish(self):
        torch.cuda.synchronize()
        for name, g, full in self.outs:
            g.check(f"{self.case.id} {name}")
            if full:
                assert g.unwritten() == 0, f"{self.case.id} {name}: {g.unwritten()} elements were left unwritten"
        self.inputs_intact()

    def inputs_intact(self):
        for name, g, t in self.ins:
            g.check(f"{self.case.id} input {name}")
            same(g.cpu(), t, f"{self.case.id} input {name} changed")

    def untouched(self):
        """after a call that must refuse: nothing written, no operand changed"""
        torch.cuda.synchronize()
        for name, g, _ in self.outs:
            assert g.untouched(), f"{self.case.id} {name}: written by a call that was refused"
        self.inputs_intact()


def f32(g):
    return g.cpu().reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# a. 16-byte path with scalar tail
# ---------------------------------------------------------------------------------------------------------------------
def run_leaky(k, c, i, w):
    n = c.sizes["n"]
    y, dy, dx = k.inp("y", i["y"]), k.inp("dy", i["dy"]), k.out("dx", n)
    k.call(k.lib.lic_leaky_bwd, y.ptr(), dy.ptr(), dx.ptr(), n, FC.SLOPE)
    k.finish()
    same(f32(dx), w["dx"], c.id)
    return 0.0


def run_dnorm(k, c, i, w):
    n = c.sizes["n"]
    g, x, nm, t = k.inp("g", i["g"]), k.inp("x", i["x"]), k.inp("norm", i["norm"]), k.out("t", n)
    k.call(k.lib.lic_gdn_dnorm, g.ptr(), x.ptr(), nm.ptr(), t.ptr(), n, c.sizes["inverse"])
    k.finish()
    r = ref64.band_ratio(f32(t), w["t"], 1e-4, 1e-6)
    assert r <= 1.0, (c.id, r)
    return r


def run_anchor_add(k, c, i, w):
    B, h, wd, Cc = (c.sizes[q] for q in "BhwC")
    g, ga, out = k.inp("g", i["g"]), k.inp("g_anchor", i["g_anchor"]), k.out("out", B * h * wd * Cc)
    k.call(k.lib.lic_anchor_add, g.ptr(), ga.ptr(), out.ptr(), B, h, wd, Cc)
    k.finish()
    same(f32(out), w["out"], c.id)
    return 0.0


def run_rd(k, c, i, w):
    B, nx, ny, nz = (c.sizes[q] for q in ("B", "nx", "ny", "nz"))
    xh, x, gl = k.inp("x_hat", i["x_hat"]), k.inp("x", i["x"]), k.inp("gl", i["gl"], 0)
    dy, dz, dx = k.out("dlogp_y", B * ny), k.out("dlogp_z", B * nz), k.out("dx_hat", B * nx)
    if c.entry == "lic_rd_loss_bwd":
        k.call(k.lib.lic_rd_loss_bwd, xh.ptr(), x.ptr(), ny, nz, nx, B, nx, FC.RD_LAMBDA, gl.ptr(), dy.ptr(), dz.ptr(),
               dx.ptr())
    else:
        lam = k.inp("lambda_img", i["lambda_img"], 0)
        k.call(k.lib.lic_rd_loss_bwd_lam, xh.ptr(), x.ptr(), ny, nz, nx, B, nx, lam.ptr(), gl.ptr(), dy.ptr(), dz.ptr(),
               dx.ptr())
    k.finish()
    r = max(ref64.band_ratio(f32(dy), w["dlogp_y"], 1e-5, 0), ref64.band_ratio(f32(dz), w["dlogp_z"], 1e-5, 0),
            ref64.band_ratio(f32(dx), w["dx_hat"], 1e-4, 1e-9))
    assert r <= 1.0, (c.id, r)
    if "dx_hat_exact" in w:
        same(f32(dx), w["dx_hat_exact"], c.id + " dx_hat")
    return r


# ---------------------------------------------------------------------------------------------------------------------
# b. one element per lane
# ---------------------------------------------------------------------------------------------------------------------
def run_mul(k, c, i, w):
    n = c.sizes["n"]
    wt = k.out("w", n, start=i["w"])
    mask = k.inp("mask", i["mask"])
    k.call(k.lib.lic_mul_inplace, wt.ptr(), mask.ptr(), n)
    k.finish()
    same(f32(wt), w["w"], c.id)
    return 0.0


def run_quantize(k, c, i, w):
    n, tr = c.sizes["n"], c.sizes["training"]
    v, u, out = k.inp("v", i["v"]), k.inp("u", i["u"]), k.out("out", n)
    k.call(k.lib.lic_quantize, v.ptr(), u.ptr() if tr else None, out.ptr(), n, tr)
    k.finish()
    same(f32(out), w["out"], c.id)
    return 0.0


def run_quantize_anchor(k, c, i, w):
    n, tr = c.sizes["n"], c.sizes["training"]
    B, h, wd, Cc = FC.nhwc_shape(n)
    v, u, out, anc = k.inp("v", i["v"]), k.inp("u", i["u"]), k.out("out", n), k.out("out_anchor", n)
    k.call(k.lib.lic_quantize_anchor, v.ptr(), u.ptr() if tr else None, out.ptr(), anc.ptr(), B, h, wd, Cc, tr)
    k.finish()
    same(f32(out), w["out"], c.id + " out")
    same(f32(anc), w["out_anchor"], c.id + " out_anchor")
    return 0.0


def run_permute3(k, c, i, w):
    src = i["src"]
    s = k.inp("src", src)
    for perm in FC.PERMS:
        want = w[f"dst{perm}"]
        A, Bd, Cd = want.shape
        ld = Cd + 3            # rows pitched inside canaries: the destination is a strided one
        dst = k.out(f"dst{perm}", 0, g=Guarded(A * Bd, Cd, k.dev, ld=ld, col0=1, shift=c.shifts, word=k.word()))
        sv = src.permute(perm).stride()
        k.call(k.lib.lic_permute3, s.ptr(), dst.ptr(), A, Bd, Cd, sv[0], sv[1], sv[2], Bd * ld, ld, 1)
    k.finish()
    for perm in FC.PERMS:
        same(k.outs[FC.PERMS.index(perm)][1].cpu(), w[f"dst{perm}"], f"{c.id} {perm}")
    return 0.0


def run_reparam(k, c, i, w):
    n, bound = c.sizes["n"], FC.BOUNDS[c.sizes["which"]]
    p, out = k.inp("p", i["p"]), k.out("out", n)
    k.call(k.lib.lic_gdn_reparam, p.ptr(), out.ptr(), n, bound, FC.PEDESTAL)
    k.finish()
    got = f32(out)
    d = (got.view(torch.int32) - w["out"].view(torch.int32)).abs()
    assert int(d.max()) <= 1, (c.id, int(d.max()))
    same(got[w["at_bound"]], w["fused"][w["at_bound"]], c.id + " on the bound")
    return float(d.max())


def run_reparam_bwd(k, c, i, w):
    n, bound = c.sizes["n"], FC.BOUNDS[c.sizes["which"]]
    p, d, dp = k.inp("p", i["p"]), k.inp("dout", i["dout"]), k.out("dp", n)
    k.call(k.lib.lic_gdn_reparam_bwd, p.ptr(), d.ptr(), dp.ptr(), n, bound)
    k.finish()
    same(f32(dp), w["dp"], c.id)
    return 0.0


def run_reparam_bwd2(k, c, i, w):
    nb, ng = c.sizes["n"], c.sizes["ng"]
    pb, dob, pg, dog = (k.inp(q, i[q]) for q in ("pb", "dob", "pg", "dog"))
    dpb, dpg = k.out("dpb", nb), k.out("dpg", ng)
    args = (pb.ptr(), dob.ptr(), dpb.ptr(), nb, FC.BOUNDS[0], pg.ptr(), dog.ptr(), dpg.ptr(), ng, FC.BOUNDS[1])
    if c.entry == "lic_gdn_reparam_bwd2":
        k.call(k.lib.lic_gdn_reparam_bwd2, *args)
    else:
        k.call(k.lib.lic_gdn_reparam_bwd2_late, *args, *c.sizes["late"])
    k.finish()
    same(f32(dpb), w["dpb"], c.id + " beta")
    same(f32(dpg), w["dpg"], c.id + " gamma")
    return 0.0


def run_pass_batch(k, c, i, w):
    nj = c.sizes["njobs"]
    jobs = (k.L.PassJob * nj)()
    gs = []
    for j in range(nj):
        p = k.inp(f"p{j}", i[f"p{j}"])
        g = k.out(f"g{j}", i[f"g{j}"].numel(), start=i[f"g{j}"])
        jobs[j].p, jobs[j].g, jobs[j].n, jobs[j].bound = p.ptr(), g.ptr(), i[f"g{j}"].numel(), i["bounds"][j]
        gs.append(g)
    k.call(k.lib.lic_gdn_pass_batch, jobs, nj)
    k.finish()
    for j, g in enumerate(gs):
        same(f32(g), w[f"g{j}"], f"{c.id} job {j}")
    return 0.0


def run_entropy_fwd(k, c, i, w):
    P, Mm, K = (c.sizes[q] for q in "PMK")
    raw, out = k.inp("raw", i["raw"].reshape(-1)), k.out("out", i["raw"].numel())
    k.call(k.lib.lic_entropy_params_fwd, raw.ptr(), out.ptr(), P, Mm, K)
    k.finish()
    r = ref64.band_ratio(f32(out), w["out"].reshape(-1), 1e-4, 1e-6)
    assert r <= 1.0, (c.id, r)
    return r


def run_entropy_bwd(k, c, i, w):
    P, Mm, K = (c.sizes[q] for q in "PMK")
    raw, o, do = (k.inp(q, i[q].reshape(-1)) for q in ("raw", "out", "dout"))
    draw = k.out("draw", i["raw"].numel())
    k.call(k.lib.lic_entropy_params_bwd, raw.ptr(), o.ptr(), do.ptr(), draw.ptr(), P, Mm, K)
    k.finish()
    e = ref64.norm_err(f32(draw), w["draw"].reshape(-1))
    assert e <= 1e-4, (c.id, e)
    return e / 1e-4


def _gmm_fwd(k, c, i):
    P, Mm, K = (c.sizes[q] for q in "PMK")
    x, par = k.inp("x", i["x"].reshape(-1)), k.inp("params", i["params"].reshape(-1))
    p, logp = k.out("p", P * Mm), k.out("logp", P * Mm)
    k.call(k.lib.lic_gmm_likelihood_fwd, x.ptr(), par.ptr(), p.ptr(), logp.ptr(), P, Mm, K, FC.BOUND)
    return x, par, p, logp


def run_gmm_fwd(k, c, i, w):
    P, Mm, K = (c.sizes[q] for q in "PMK")
    _, _, p, logp = _gmm_fwd(k, c, i)
    k.finish()
    p64, logp64, _, p_raw = w["ref"]
    gp, gl = FC.unrows(f32(p), P), FC.unrows(f32(logp), P)
    dead, live, border = ref64.gmm_regions(p_raw)
    sel = live & (p64 > ref64.P_RESOLVED)
    worst = {"p": ref64.band_ratio(gp, p64, *ref64.P_BAND), "logp": ref64.band_ratio(gl[sel], logp64[sel], *ref64.LOGP_BAND),
             "logp_of_p": ref64.band_ratio(gl, torch.log(gp.double()), 1e-6, 1e-6)}
    assert bool((gp[dead].double() == float(np.float32(FC.BOUND))).all()), c.id
    assert max(worst.values()) <= 1.0, (c.id, worst)
    return max(worst.values())


def run_gmm_bwd(k, c, i, w):
    P, Mm, K = (c.sizes[q] for q in "PMK")
    x, par, p, logp = _gmm_fwd(k, c, i)
    dp, dl = k.inp("dp", i["dp"].reshape(-1)), k.inp("dlogp", i["dlogp"].reshape(-1))
    grads = {}
    for mode, a, b in (("logp", None, dl), ("p", dp, None), ("both", dp, dl)):
        dx, dpar = k.out(f"dx/{mode}", P * Mm), k.out(f"dparams/{mode}", i["params"].numel())
        k.call(k.lib.lic_gmm_likelihood_bwd, x.ptr(), par.ptr(), a.ptr() if a else None, b.ptr() if b else None, dx.ptr(),
               dpar.ptr(), P, Mm, K, FC.BOUND)
        grads[mode] = (dx, dpar)
    k.finish()
    got = (FC.unrows(f32(p), P), FC.unrows(f32(logp), P),
           {m: (FC.unrows(f32(dx), P), FC.unrows(f32(dpar), P)) for m, (dx, dpar) in grads.items()})
    worst = ref64.check_gmm(got, w["ref"], K, Mm, 0.5, c.id)
    return max(worst.values())


def _fe_split(flat, Cc):
    """[C][43] -> the eleven [C][n_k] blocks"""
    a, out, at = flat.reshape(Cc, 43), [], 0
    for wd in (3, 9, 9, 3, 3, 3, 3, 1, 3, 3, 3):
        out.append(a[:, at:at + wd])
        at += wd
    return out


def run_fe_fwd(k, c, i, w):
    Cc, P = c.sizes["C"], c.sizes["P"]
    x, par = k.inp("x", i["x"].reshape(-1)), k.inp("fe_params", i["fe_params"].reshape(-1))
    p, logp = k.out("p", P * Cc), k.out("logp", P * Cc)
    k.call(k.lib.lic_factorized_fwd, x.ptr(), par.ptr(), p.ptr(), logp.ptr(), P, Cc, FC.BOUND)
    k.finish()
    r = max(ref64.band_ratio(f32(p), w["both"]["p"].reshape(-1), 1e-4, 1.5e-7),
            ref64.band_ratio(f32(logp), w["both"]["logp"].reshape(-1), 1e-4, 1e-6))
    assert r <= 1.0, (c.id, r)
    return r


def run_fe_bwd(k, c, i, w):
    Cc, P = c.sizes["C"], c.sizes["P"]
    x, par = k.inp("x", i["x"].reshape(-1)), k.inp("fe_params", i["fe_params"].reshape(-1))
    dp, dl = k.inp("dp", i["dp"].reshape(-1)), k.inp("dlogp", i["dlogp"].reshape(-1))
    outs = {}
    for mode, a in (("logp", None), ("both", dp)):
        dx, dpar = k.out(f"dx/{mode}", P * Cc), k.out(f"dparams/{mode}", Cc * 43)
        k.call(k.lib.lic_factorized_bwd, x.ptr(), par.ptr(), a.ptr() if a else None, dl.ptr(), dx.ptr(), dpar.ptr(), P, Cc,
               FC.BOUND)
        outs[mode] = (dx, dpar)
    k.finish()
    errs = {}
    for mode, (dx, dpar) in outs.items():
        errs[f"{mode}.dx"] = ref64.norm_err(f32(dx), w[mode]["dx"].reshape(-1))
        for j, (got, ref) in enumerate(zip(_fe_split(f32(dpar), Cc), w[mode]["grads"])):
            errs[f"{mode}.{j}"] = ref64.norm_err(got, ref.reshape(Cc, -1))
    bad = {q: v for q, v in errs.items() if not v <= 1e-4}
    assert not bad, (c.id, bad)
    return max(errs.values()) / 1e-4


def run_channel_logits(k, c, i, w):
    n = c.sizes["n"]
    par, xs, out = k.inp("fe_params", i["fe_params"].reshape(-1)), k.inp("xs", i["xs"]), k.out("out", n)
    k.call(k.lib.lic_factorized_channel_logits, par.ptr(), i["ch"], xs.ptr(), out.ptr(), n)
    k.finish()
    r = ref64.band_ratio(torch.sigmoid(f32(out)), w["cdf"], 1e-5, 1e-7)
    assert r <= 1.0, (c.id, r)
    return r


def run_fe_pack(k, c, i, w):
    Cc = c.sizes["C"]
    gs = [k.inp(f"t{j}", i[f"t{j}"]) for j in range(11)]
    packed = k.out("packed", Cc * 43)
    k.call(k.lib.lic_fe_pack, (C.c_void_p * 11)(*[g.ptr() for g in gs]), packed.ptr(), Cc)
    k.finish()
    same(f32(packed), w["packed"], c.id)
    return 0.0


def run_fe_unpack(k, c, i, w):
    Cc = c.sizes["C"]
    dpk, flat = k.inp("dpacked", i["dpacked"]), k.out("flat", Cc * 43)
    k.call(k.lib.lic_fe_unpack, dpk.ptr(), flat.ptr(), Cc)
    k.finish()
    same(f32(flat), w["flat"], c.id)
    return 0.0


def run_colsum(k, c, i, w):
    P, Cc, ld, col0 = (c.sizes[q] for q in ("P", "C", "ld", "col0"))
    src = k.keep("in", Guarded.holding(i["in"], k.dev, ld=ld, col0=col0, shift=c.shifts, word=k.word()), i["in"])
    nbytes = k.lib.lic_colsum_workspace_bytes(P, Cc)
    ws, out = k.out("workspace", 0, g=workspace(nbytes, k.dev, k.word()), full=False), k.out("out", Cc)
    k.call(k.lib.lic_colsum, src.ptr(), ld, P, Cc, FC.COLSUM_SCALE, out.ptr(), ws.ptr(), nbytes)
    k.finish()
    e = ref64.norm_err(f32(out), w["out"])
    assert e <= 1e-4, (c.id, e)
    return e / 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# c. bf16 elementwise
# ---------------------------------------------------------------------------------------------------------------------
def run_quantize_bf16(k, c, i, w):
    n, tr = c.sizes["n"], c.sizes["training"]
    anchor = "anchor" in c.entry
    v, u = k.inp("v", i["v"].reshape(-1)), k.inp("u", i["u"].reshape(-1))
    names = ("out", "out_anchor") if anchor else ("out",)
    names16 = ("v_bf16", "out_bf16", "anchor_bf16") if anchor else ("v_bf16", "out_bf16")
    o32 = [k.out(q, n) for q in names]
    o16 = [k.out(q, n, dtype=FC.BF) for q in names16]
    legal = FC.bf16_legal(c.entry, n)
    args = [v.ptr(), u.ptr() if tr else None] + [g.ptr() for g in o32 + o16]
    if anchor:
        k.call(k.lib.lic_quantize_anchor_bf16, *args, *FC.nhwc_shape(n), tr, rc=LIC_OK if legal else LIC_ERR_UNSUPPORTED)
    else:
        k.call(k.lib.lic_quantize_bf16, *args, n, tr, rc=LIC_OK if legal else LIC_ERR_UNSUPPORTED)
    if not legal:
        k.untouched()
        return 0.0
    k.finish()
    for q, g in zip(names + names16, o32 + o16):
        same(g.cpu().reshape(-1), w[q], f"{c.id} {q}")
    return 0.0


def run_leaky_bf16(k, c, i, w):
    n = c.sizes["n"]
    y, dy, dx = k.inp("y", i["y"]), k.inp("dy", i["dy"]), k.out("dx", n, dtype=FC.BF)
    legal = FC.bf16_legal(c.entry, n)
    k.call(k.lib.lic_leaky_bwd_bf16, y.ptr(), dy.ptr(), dx.ptr(), n, FC.SLOPE, rc=LIC_OK if legal else LIC_ERR_UNSUPPORTED)
    if not legal:
        k.untouched()
        return 0.0
    k.finish()
    same(dx.cpu(), w["dx"], c.id)
    return 0.0


def run_dnorm_bf16(k, c, i, w):
    n = c.sizes["n"]
    g, x, nm, t = k.inp("g", i["g"]), k.inp("x", i["x"]), k.inp("norm", i["norm"]), k.out("t", n, dtype=FC.BF)
    legal = FC.bf16_legal(c.entry, n)
    k.call(k.lib.lic_gdn_dnorm_bf16, g.ptr(), x.ptr(), nm.ptr(), t.ptr(), n, c.sizes["inverse"],
           rc=LIC_OK if legal else LIC_ERR_UNSUPPORTED)
    if not legal:
        k.untouched()
        return 0.0
    k.finish()
    a, b = t.cpu().double().numpy(), w["t"].numpy()
    s = max(np.abs(b).max(), 1e-30)                   # bf16_close of tests/test_gpu_bf16.py
    r = float((np.abs(a - b) / (2.0 ** -8 * np.abs(b) + 2.0 ** -8 * 1e-2 * s + 1e-30)).max())
    assert r <= 1.0, (c.id, r)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# d. input pipeline and statistics
# ---------------------------------------------------------------------------------------------------------------------
def run_u8(k, c, i, w):
    n, refuse = c.sizes["n"], c.sizes["refuse"]
    off_in = int(refuse[3:]) if refuse.startswith("in") else 0
    off_out = int(refuse[4:]) if refuse.startswith("out") else 0
    src, out = k.inp("in", i["in"], off_in), k.out("out", n, off_out)
    k.call(k.lib.lic_u8_to_f32, src.ptr(), out.ptr(), n, rc=LIC_ERR_INVALID if refuse else LIC_OK)
    if refuse:
        k.untouched()
        return 0.0
    k.finish()
    same(f32(out), w["out"], c.id)
    return 0.0


def run_stats(k, c, i, w):
    n, nbins = c.sizes["n"], c.sizes["nbins"]
    x = k.inp("x", i["x"])
    stats, hist = k.out("stats", 6, dtype=torch.float64), k.out("hist", nbins, dtype=torch.int64)
    nbytes = k.lib.lic_tensor_stats_workspace_bytes()
    ws = k.out("workspace", 0, g=workspace(nbytes, k.dev, k.word()), full=False)
    k.call(k.lib.lic_tensor_stats, x.ptr(), n, nbins, FC.STATS_LO, FC.STATS_HI, stats.ptr(), hist.ptr(), ws.ptr(), nbytes)
    k.finish()
    s, h = stats.cpu().numpy(), hist.cpu().numpy()
    assert s[5] == w["nan"], f"{c.id}: {s[5]} NaNs counted, {w['nan']} placed (a canary read past the end counts as one)"
    assert s[0] == w["count"] and s[3] == w["min"] and s[4] == w["max"], (c.id, s, w)
    mean = s[1] / max(s[0], 1.0)
    std = max(s[2] / max(s[0], 1.0) - mean * mean, 0.0) ** 0.5
    r = max(abs(mean - w["mean"]) / 1e-9, abs(std - w["std"]) / 1e-7)
    assert r < 1.0, (c.id, mean, w["mean"], std, w["std"])
    assert h.sum() == w["count"] and np.abs(h - w["hist"]).sum() <= 2, (c.id, int(np.abs(h - w["hist"]).sum()))
    return r


def _pool(images, prefix):
    sizes = np.array([a.size for a in images])
    offsets = prefix + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return np.concatenate([np.full(prefix, 0xAB, np.uint8)] + [a.reshape(-1) for a in images]), offsets


def _table(k, jobs):
    """a job table (numpy records) on the device, 8-byte aligned, inside the pattern"""
    return k.inp("jobs", torch.from_numpy(jobs.view(np.uint8).copy()), 0)


def run_window_u8(k, c, i, w):
    s = c.sizes
    images, rows = i["images"], np.asarray(i["rows"], np.int64)
    pool, offsets = _pool(images, i["prefix"])
    sizes = np.array([images[j].shape[:2] for j in rows[:, 0]])
    jobs = k.D.window_jobs(offsets[rows[:, 0]], sizes, rows[:, 1], rows[:, 2], rows[:, 3], s["h"], s["w"], s["border"],
                           C=s["C"], pool_bytes=pool.size)
    pl, tab = k.inp("pool", torch.from_numpy(pool), 0), _table(k, jobs)
    out = k.out("out", w["out"].size)
    k.call(k.lib.lic_window_u8_to_f32, pl.ptr(), tab.ptr(), len(rows), s["h"], s["w"], s["C"], s["border"], out.ptr())
    k.finish()
    same(f32(out), torch.from_numpy(w["out"]), c.id)
    return 0.0


def run_window_f32(k, c, i, w):
    s = c.sizes
    src = i["src"]
    B, Cc, Hs, Ws = src.shape
    st = Guarded4D.layout(src.shape, s["layout"])
    g = k.keep("src", Guarded4D.holding(src, st, k.dev, word=k.word()), src)
    outs = {}
    for y0, x0 in FC.WINDOW_F32_AT:
        outs[(y0, x0)] = k.out(f"out@{y0},{x0}", B * s["h"] * s["w"] * Cc)
        k.call(k.lib.lic_window_f32, g.ptr(), *st, B, Cc, Hs, Ws, y0, x0, s["h"], s["w"], s["border"], outs[(y0, x0)].ptr())
    k.finish()
    for at, o in outs.items():
        same(f32(o), torch.from_numpy(np.ascontiguousarray(w[at])), f"{c.id} at {at}")
    return 0.0


def run_resample(k, c, i, w):
    s = c.sizes
    images, jobs_ = i["images"], np.asarray(i["jobs"], np.int64)
    pool, offsets = _pool(images, i["prefix"])
    sizes = np.array([images[j].shape[:2] for j in jobs_[:, 0]])
    jobs = k.D.resample_jobs(offsets[jobs_[:, 0]], sizes, jobs_[:, 1:3], jobs_[:, 3], jobs_[:, 4], jobs_[:, 5], s["h"],
                             s["w"], C=s["C"], pool_bytes=pool.size)
    pl, tab = k.inp("pool", torch.from_numpy(pool), 0), _table(k, jobs)
    out = k.out("out", w["out"].size)
    k.call(k.lib.lic_resample_u8_to_f32, pl.ptr(), tab.ptr(), len(jobs_), s["h"], s["w"], s["C"], out.ptr())
    k.finish()
    same(f32(out), torch.from_numpy(w["out"]), c.id)
    return 0.0


# ---------------------------------------------------------------------------------------------------------------------
# e. MS-SSIM
# ---------------------------------------------------------------------------------------------------------------------
def _ms_forward(k, c, i):
    s = c.sizes
    shape = (s["B"], s["C"], s["H"], s["W"])
    st = Guarded4D.layout(shape, s["layout"])
    x = k.keep("x", Guarded4D.holding(i["x"], st, k.dev, word=k.word()), i["x"])
    y = k.keep("y", Guarded4D.holding(i["y"], st, k.dev, word=k.word()), i["y"])
    BC = s["B"] * s["C"]
    out, lev = k.out("out", BC), k.out("level_out", 5 * BC * 2)
    nbytes = k.lib.lic_msssim_workspace_bytes(*shape)
    assert nbytes > 0
    ws = k.out("workspace", 0, g=workspace(nbytes, k.dev, k.word()), full=False)
    k.call(k.lib.lic_msssim, x.ptr(), y.ptr(), *shape, *st, 1.0, out.ptr(), lev.ptr(), ws.ptr(), nbytes)
    return shape, st, x, y, out, lev, ws, nbytes


def run_msssim(k, c, i, w):
    _, _, _, _, out, _, _, _ = _ms_forward(k, c, i)
    k.finish()
    err = float((f32(out).double() - w["out"]).abs().max())
    assert err <= FC.M.VALUE_BAND, (c.id, err)
    return err / FC.M.VALUE_BAND


def run_msssim_bwd(k, c, i, w):
    shape, st, x, y, out, lev, ws, nbytes = _ms_forward(k, c, i)
    torch.cuda.synchronize()
    lev0, ws0 = lev.buf.cpu().clone(), ws.buf.cpu().clone()
    gout = k.inp("gout", i["gout"], 0)
    dx = k.out("dx", 0, g=Guarded4D(shape, st, k.dev, word=k.word()))
    nb = k.lib.lic_msssim_bwd_workspace_bytes(*shape)
    assert nb > 0
    bws = k.out("bwd workspace", 0, g=workspace(nb, k.dev, k.word()), full=False)
    k.call(k.lib.lic_msssim_bwd, x.ptr(), y.ptr(), *shape, *st, 1.0, lev.ptr(), ws.ptr(), nbytes, gout.ptr(), dx.ptr(),
           bws.ptr(), nb)
    k.finish()
    assert torch.equal(lev.buf.cpu(), lev0) and torch.equal(ws.buf.cpu(), ws0), f"{c.id}: the backward wrote a forward result"
    g64 = w["dx"]
    err = float((dx.cpu().double() - g64).abs().max() / g64.abs().max())
    assert err <= FC.M.GRAD_BAND, (c.id, err)
    return err / FC.M.GRAD_BAND


# ---------------------------------------------------------------------------------------------------------------------
# f. coder tables
# ---------------------------------------------------------------------------------------------------------------------
def _table_invariants(t, S, what):
    assert (t[:, 0] == 0).all() and (t[:, S] == 65536).all() and (np.diff(t, axis=1) >= 1).all(), what


def run_fe_tables(k, c, i, w):
    Cc, S = c.sizes["C"], c.sizes["S"]
    par = k.inp("fe_params", i["fe_params"].reshape(-1))
    out = k.out("out", Cc * (S + 1), dtype=torch.int32)
    k.call(k.lib.lic_factorized_cdf_tables, par.ptr(), Cc, i["lo"], S, out.ptr())
    k.finish()
    t = out.cpu().numpy().view(np.uint32).astype(np.int64).reshape(Cc, S + 1)
    _table_invariants(t, S, c.id)
    d = int(np.abs(t - w["out"]).max())
    assert d <= 1, (c.id, d)
    return float(d)


def run_gmm_tables(k, c, i, w):
    P, Mm, K, W = (c.sizes[q] for q in "PMKW")
    S, n = 2 * W + 1, P * Mm
    par = k.inp("params", i["params"].reshape(-1))
    cen, out = k.out("center", n, dtype=torch.int32), k.out("out", n * (S + 1), dtype=torch.int32)
    k.call(k.lib.lic_gmm_cdf_tables, par.ptr(), P, Mm, K, W, cen.ptr(), out.ptr())
    k.finish()
    cdev = cen.cpu().numpy().astype(np.int64)
    t = out.cpu().numpy().view(np.uint32).astype(np.int64).reshape(n, S + 1)
    _table_invariants(t, S, c.id)
    assert (np.abs(cdev - w["center"]) <= 1).all(), c.id      # (the device forms the mean with fused multiply-adds)
    want = w["out"] if (cdev == w["center"]).all() else FC.gmm_tables64(*i["blocks"], cdev, W)
    d = int(np.abs(t - want).max())
    assert d <= FC.GMM_TABLE_BAND, (c.id, d)
    return d / FC.GMM_TABLE_BAND


# ---------------------------------------------------------------------------------------------------------------------
# g. Adam
# ---------------------------------------------------------------------------------------------------------------------
def _job_table(k, rows):
    """(p, m, v, n) address tuples -> the lic_adam_job array on the device, partitioned by lic_adam_plan; its blocks"""
    arr = (k.L.AdamJob * len(rows))()
    for j, row in zip(arr, rows):
        j.p, j.m, j.v, j.n = row
    blocks = k.lib.lic_adam_plan(arr, len(rows))
    assert blocks > 0
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(k.dev), int(blocks)


def run_adam(k, c, i, w):
    lens = c.sizes["lengths"]
    g, outs, rows = [], [], []
    for j, n in enumerate(lens):
        g.append(k.inp(f"g{j}", i[f"g{j}"], c.shift("g")))
        trio = []
        for q in "pmv":
            o = k.out(f"{q}{j}", n, c.shift(q), start=i[f"{q}{j}"])     # in place: they start as the operands
            trio.append(o)
        outs.append(trio)
        rows.append((trio[0].ptr(), trio[1].ptr(), trio[2].ptr(), n))
    tab, blocks = _job_table(k, rows)
    assert blocks == sum(-(-n // FC.AD_ITEMS) for n in lens)
    gptrs = (C.c_void_p * len(lens))(*[x.ptr() for x in g])
    b1, b2 = FC.BETAS
    k.call(k.lib.lic_adam_run, C.c_void_p(tab.data_ptr()), len(lens), blocks, gptrs, FC.LR, b1, b2, FC.EPS, FC.WD,
           1.0 - b1 ** FC.ADAM_STEP, 1.0 - b2 ** FC.ADAM_STEP)
    k.finish()
    worst = 0.0
    for j, (p, m, v) in enumerate(outs):
        p64, m64, v64 = w[f"p{j}"], w[f"m{j}"], w[f"v{j}"]
        tol = 1e-6 * float(p64.abs().max()) + 1e-5 * 1 * FC.LR          # one update
        rp = float((f32(p).double() - p64).abs().max()) / tol
        rv = float((f32(v).double() - v64).abs().max()) / max(float(v64.abs().max()), 1e-30) / 1e-6
        rm = float((f32(m).double() - m64).abs().max()) / max(float(m64.abs().max()), 1e-30) / 1e-6   # (as exp_avg_sq)
        assert rp <= 1.0 and rv <= 1.0 and rm <= 1.0, (c.id, j, rp, rv, rm)
        worst = max(worst, rp, rv, rm)
    return worst


def run_swap(k, c, i, w):
    lens = c.sizes["lengths"]
    ps, es = [], []
    for j, n in enumerate(lens):
        for q, lst in (("p", ps), ("e", es)):
            o = k.out(f"{q}{j}", n, c.shift(q), start=i[f"{q}{j}"])
            lst.append(o)
    tab, blocks = _job_table(k, [(p.ptr(), p.ptr(), p.ptr(), n) for p, n in zip(ps, lens)])   # (only p and n are read)
    ema = torch.tensor([e.ptr() for e in es], dtype=torch.int64, device=k.dev)
    k.call(k.lib.lic_swap_run, C.c_void_p(tab.data_ptr()), len(lens), blocks, C.c_void_p(ema.data_ptr()))
    k.finish()
    for j in range(len(lens)):
        same(f32(ps[j]), w[f"p{j}"], f"{c.id} p{j}")
        same(f32(es[j]), w[f"e{j}"], f"{c.id} e{j}")
    return 0.0


RUNNERS = {
    "lic_leaky_bwd": run_leaky, "lic_gdn_dnorm": run_dnorm, "lic_anchor_add": run_anchor_add, "lic_rd_loss_bwd": run_rd,
    "lic_rd_loss_bwd_lam": run_rd, "lic_mul_inplace": run_mul, "lic_quantize": run_quantize,
    "lic_quantize_anchor": run_quantize_anchor, "lic_permute3": run_permute3, "lic_gdn_reparam": run_reparam,
    "lic_gdn_reparam_bwd": run_reparam_bwd, "lic_gdn_reparam_bwd2": run_reparam_bwd2,
    "lic_gdn_reparam_bwd2_late": run_reparam_bwd2, "lic_gdn_pass_batch": run_pass_batch,
    "lic_entropy_params_fwd": run_entropy_fwd, "lic_entropy_params_bwd": run_entropy_bwd,
    "lic_gmm_likelihood_fwd": run_gmm_fwd, "lic_gmm_likelihood_bwd": run_gmm_bwd, "lic_factorized_fwd": run_fe_fwd,
    "lic_factorized_bwd": run_fe_bwd, "lic_factorized_channel_logits": run_channel_logits, "lic_fe_pack": run_fe_pack,
    "lic_fe_unpack": run_fe_unpack, "lic_colsum": run_colsum, "lic_quantize_bf16": run_quantize_bf16,
    "lic_quantize_anchor_bf16": run_quantize_bf16, "lic_leaky_bwd_bf16": run_leaky_bf16,
    "lic_gdn_dnorm_bf16": run_dnorm_bf16, "lic_u8_to_f32": run_u8, "lic_tensor_stats": run_stats,
    "lic_window_u8_to_f32": run_window_u8, "lic_window_f32": run_window_f32, "lic_resample_u8_to_f32": run_resample,
    "lic_msssim": run_msssim, "lic_msssim_bwd": run_msssim_bwd, "lic_factorized_cdf_tables": run_fe_tables,
    "lic_gmm_cdf_tables": run_gmm_tables, "lic_adam_run": run_adam, "lic_swap_run": run_swap,
}


@pytest.mark.parametrize("entry", FC.ENTRIES)
def test_fences(env, entry):
    """every case of one entry; the first failure is reported with its case after the entry's line is printed"""
    assert set(RUNNERS) == set(FC.ENTRIES)
    cases = FC.CASES[entry]
    calls, worst, failure = 0, 0.0, None
    for c in cases:
        inputs, want = FC.make(c)
        k = Kit(env, c)
        try:
            worst = max(worst, RUNNERS[entry](k, c, inputs, want))
        except AssertionError as e:
            print(f"\n  {c.id}: {str(e)[:400]}")
            failure = failure or e
        calls += k.calls
        if failure is not None and torch.cuda.is_available():
            torch.cuda.synchronize()
    FC.forget(entry)
    WORST[entry] = worst
    print(f"\n{entry} (group {FC.GROUP_OF[entry]}): {len(cases)} cases, {calls} calls of the C ABI, worst {worst:.3g} of its band"
          + ("" if failure is None else "  -- FAILED"))
    if failure is not None:
        raise failure
