"""CPU checks of tests/gdn_ref64.py, the float64 statement of GDN / IGDN that tests/test_gpu_gdn_fp32.py holds the fp32
kernels to: it agrees with the oracle within the oracle's fp32 rounding and with torch.autograd of its own forward; its
exact-input cases give the same fp32 bits whichever way a sum is ordered; its banded inputs leave no element out."""
import numpy as np
import pytest
import torch

import gdn_ref64 as G

U = 2.0 ** -24   # fp32 unit roundoff
LO = float(np.float32(1e-6))   # the smallest beta_eff, as fp32 holds it


def _nchw(a):
    """[P][C] -> the oracle's [1][C][P][1]"""
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a.T.reshape(1, a.shape[1], a.shape[0], 1)).astype(np.float32)


def _pc(a):
    return torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[1], a.shape[2]).T))


def _within(got, ref, bound, what):
    err = (G.f64(got) - G.f64(ref)).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: {worst:.3f} of the rounding bound")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("C", G.WIDTHS)
def test_reference_agrees_with_the_oracle(C, inverse):
    """the oracle sums one fp32 term at a time: a sum of n terms is within (n - 1) u of the sum of their magnitudes
    (first order), the factors add a few u more.  Bounds used: (C + 8) u of norm, of |y|, of dx's magnitude sum `mag`, and of
    sum |t| for d beta_eff (t is rounded to fp32, the sum itself runs in double)."""
    from oracle import oracle as O
    P = 37
    inp = G.banded_inputs(C, inverse, P)
    x, g, gamma_e, beta_e = inp["x"], inp["g"], inp["gamma_e"], inp["beta_e"]
    y64, n64 = G.fwd(x, beta_e, gamma_e, inverse)
    y, nrm = O.gdn_fwd(_nchw(x), beta_e.numpy(), gamma_e.numpy(), inverse)
    k = (C + 8) * U
    _within(_pc(nrm), n64, k * n64, "norm")
    _within(_pc(y), y64, k * y64.abs(), "y")
    nrm32 = _pc(nrm)                       # the backward of both reads the same fp32 pool
    t64, dx64, mag = G.bwd(g, x, nrm32, gamma_e, inverse)
    dx, dbe, _ = O.gdn_bwd(_nchw(x), nrm, gamma_e.numpy(), _nchw(g), inverse)
    _within(_pc(dx), dx64, k * mag, "dx")
    _within(torch.from_numpy(dbe), t64.sum(0), k * t64.abs().sum(0), "d beta_eff")


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("inverse", [0, 1])
def test_reference_backward_is_autograd_of_its_forward(inverse, with_res):
    C, P = 64, 21
    inp = G.banded_inputs(C, inverse, P)
    x = inp["x"].double().requires_grad_(True)
    beta_e = inp["beta_e"].double().requires_grad_(True)
    res = inp["res"].double().requires_grad_(True) if with_res else None
    g = inp["g"].double()
    y, norm = G.fwd(x, beta_e, inp["gamma_e"], inverse, res)
    y0, _ = G.fwd(inp["x"], inp["beta_e"], inp["gamma_e"], inverse)
    if with_res:
        assert torch.equal(y.detach(), y0 + inp["res"].double())
    grads = torch.autograd.grad([y], [x, beta_e] + ([res] if with_res else []), [g])
    t, dx, mag = G.bwd(g, inp["x"], norm.detach(), inp["gamma_e"], inverse)
    assert bool(((grads[0] - dx).abs() <= 1e-12 * mag).all()), float(((grads[0] - dx).abs() / mag.clamp_min(1e-300)).max())
    assert bool(((grads[1] - t.sum(0)).abs() <= 1e-12 * t.abs().sum(0)).all())
    if with_res:
        assert torch.equal(grads[2], g)
    # mag bounds |dx| and is the sum of the magnitudes of its terms
    assert bool((dx.abs() <= mag * (1 + 1e-12)).all())


def test_block_colsums():
    a = torch.arange(130 * 3, dtype=torch.float64).reshape(130, 3)
    cs = G.block_colsums(a, 64)
    assert cs.shape == (3, 3)
    for b, (lo, hi) in enumerate(((0, 64), (64, 128), (128, 130))):
        assert torch.equal(cs[b], a[lo:hi].sum(0))
    assert G.block_colsums(a[:64], 64).shape == (1, 3) and G.block_colsums(a[:65], 64).shape == (2, 3)


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("C", G.WIDTHS)
def test_exact_cases_do_not_depend_on_summation_order(C, inverse, kind):
    """norm (forward), t, dx and the 64-pixel block sums of t and dx (backward) in fp32 arithmetic, every sum ascending
    and descending: both equal the float64 result bit for bit"""
    for P in (1, 65, 357):
        inp = (G.exact_fwd_inputs if kind == "fwd" else G.exact_bwd_inputs)(C, inverse, P)
        ref = G.exact_reference(kind, inp, inverse)
        for descending in (False, True):
            got = G.fp32_ordered(kind, inp, inverse, descending)
            assert set(got) == set(ref)
            for name in ref:
                assert got[name].dtype == np.float32
                assert G.same_bits(got[name], ref[name]), (P, name, descending)
        if kind == "bwd":   # the case is not degenerate: most of t and dx is non-zero, both norms occur
            assert float((ref["t"] != 0).double().mean()) > 0.5 and float((ref["dx"] != 0).double().mean()) > 0.5
            assert P == 1 or set(inp["norm"].unique().tolist()) == {1.0, 4.0}


def test_same_bits_tells_values_apart():
    a = torch.tensor([1.0, 0.0, -0.0, 3.5], dtype=torch.float32)
    assert G.same_bits(a, a.double()) and G.same_bits(a, torch.tensor([1.0, -0.0, 0.0, 3.5]))
    assert not G.same_bits(a, torch.tensor([1.0, 0.0, 0.0, 3.5000002], dtype=torch.float32))
    assert not G.same_bits(torch.tensor([float("nan")]), torch.tensor([1.0]))
    with pytest.raises(AssertionError):
        G.same_bits(a, torch.tensor([1.0, 0.0, 0.0, 3.5 + 2.0 ** -30], dtype=torch.float64))


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_banded_inputs_leave_nothing_out(case):
    """norm > 0 everywhere (the float64 pool and the generated one), x has its zero pixels and four decades of pixel
    magnitudes, gamma_e is non-negative and far from symmetric: no comparison of the GPU cases needs to skip an element"""
    C, inverse, P = case
    inp = G.banded_inputs(C, inverse, P)
    _, norm = G.fwd(inp["x"], inp["beta_e"], inp["gamma_e"], inverse)
    assert float(norm.min()) >= LO and bool(torch.isfinite(norm).all())
    assert float(inp["norm"].min()) >= 0.25 and float(inp["norm"].max()) <= 3.25
    assert float(inp["beta_e"].min()) >= LO and float(inp["beta_e"].max()) <= 1.0
    gam = inp["gamma_e"]
    assert float(gam.min()) >= 0 and float((gam - gam.t()).abs().mean()) > 0.5 * float(gam.mean())
    for p in G.zero_pixels(P):
        assert not bool(inp["x"][p].any())
    if P >= 357:
        amp = inp["x"].abs().amax(1)
        amp = amp[amp > 0]
        assert float(amp.max() / amp.min()) > 1e3
    t, dx, mag = G.bwd(inp["g"], inp["x"], inp["norm"], gam, inverse)
    assert bool(torch.isfinite(dx).all()) and bool((mag >= dx.abs() * (1 - 1e-12)).all())


def test_case_table():
    assert len(G.CASES) == len(set(G.CASES)) == 34
    assert {c[2] for c in G.CASES} == {1, 63, 64, 65, 357, 65_537}
    assert {c[0] for c in G.CASES if c[2] == G.BIG} == {192, 64}
    assert set(G.OWN_NORM_CASES) <= set(G.CASES)
