"""The case table of the fence tests (tests/fence_cases.py) on the CPU: which entries it holds, that every case the
issue of the fence tests names is in it (a case dropped later fails here), and that every case's reference runs on
the host and is finite -- so a NaN the GPU test sees is a canary, never the reference's."""
import itertools

import numpy as np
import pytest
import torch

import fence_cases as FC
import ref64

# the entries the fence tests are to cover, group by group
WANTED = {
    "a": {"lic_leaky_bwd", "lic_gdn_dnorm", "lic_anchor_add", "lic_rd_loss_bwd", "lic_rd_loss_bwd_lam"},
    "b": {"lic_mul_inplace", "lic_quantize", "lic_quantize_anchor", "lic_permute3", "lic_gdn_reparam",
          "lic_gdn_reparam_bwd", "lic_gdn_reparam_bwd2", "lic_gdn_reparam_bwd2_late", "lic_gdn_pass_batch",
          "lic_entropy_params_fwd", "lic_entropy_params_bwd", "lic_gmm_likelihood_fwd", "lic_gmm_likelihood_bwd",
          "lic_factorized_fwd", "lic_factorized_bwd", "lic_factorized_channel_logits", "lic_fe_pack", "lic_fe_unpack",
          "lic_colsum"},
    "c": {"lic_quantize_bf16", "lic_quantize_anchor_bf16", "lic_leaky_bwd_bf16", "lic_gdn_dnorm_bf16"},
    "d": {"lic_u8_to_f32", "lic_tensor_stats", "lic_window_u8_to_f32", "lic_window_f32", "lic_resample_u8_to_f32"},
    "e": {"lic_msssim", "lic_msssim_bwd"},
    "f": {"lic_factorized_cdf_tables", "lic_gmm_cdf_tables"},
    "g": {"lic_adam_run", "lic_swap_run"},
}
N_LIST = {1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 1027}


def _sizes(entry, *keys):
    return {tuple(c.sizes[k] for k in keys) for c in FC.CASES[entry]}


def test_the_table_holds_exactly_the_listed_entries_and_each_is_bound():
    from neural_image_compression_amd import _lib as L
    assert {g: set(es) for g, es in FC.GROUPS.items()} == WANTED
    assert set(FC.CASES) == set(FC.ENTRIES) == set().union(*WANTED.values()) == set(FC.MAKERS)
    for entry in FC.ENTRIES:
        assert entry in L.SIGNATURES, entry
        assert FC.CASES[entry], entry
        for c in FC.CASES[entry]:
            assert c.entry == entry and c.band and ("test_" in c.band or "include/lic.h" in c.band), c
    for entry in ("lic_colsum", "lic_msssim", "lic_msssim_bwd", "lic_tensor_stats"):
        name = {"lic_msssim_bwd": "lic_msssim_bwd_workspace_bytes"}.get(entry, entry + "_workspace_bytes")
        assert name in L.SIGNATURES
    assert set(FC.ALREADY_FENCED) == WANTED["c"]
    assert FC.PASS_MAX_JOBS == 32 and FC.AD_ITEMS == 4096


def _combos(k):
    return set(itertools.product((0, 1), repeat=k)) | {(2,) * k, (3,) * k}


def test_vectorised_entries_have_every_size_and_every_shift_combination():
    for entry, k in (("lic_leaky_bwd", 3), ("lic_gdn_dnorm", 4)):
        assert FC.N_LIST == tuple(sorted(N_LIST)) and len(FC.OPERANDS[entry]) == k
        keys = ("n", "inverse") if entry == "lic_gdn_dnorm" else ("n",)
        by_size = {}
        for c in FC.CASES[entry]:
            by_size.setdefault(tuple(c.sizes[q] for q in keys), set()).add(c.shifts)
        want = {(n,) for n in N_LIST} if len(keys) == 1 else {(n, i) for n in N_LIST for i in (0, 1)}
        assert set(by_size) == want, entry
        assert all(s == _combos(k) for s in by_size.values()), entry
    # lic_anchor_add: C in {3, 4, 8}, every n of the list that C divides, odd and even sides, every combination
    by_shape = {}
    for c in FC.CASES["lic_anchor_add"]:
        by_shape.setdefault(tuple(c.sizes[q] for q in "BhwC"), set()).add(c.shifts)
    assert all(s == _combos(3) for s in by_shape.values())
    for Cc in (3, 4, 8):
        assert {B * h * w * C for B, h, w, C in by_shape if C == Cc} == {n for n in N_LIST if n % Cc == 0}, Cc
    assert any(h % 2 and w % 2 for _, h, w, _ in by_shape) and any(h % 2 == 0 and w % 2 == 0 for _, h, w, _ in by_shape)
    assert any(h % 2 != w % 2 for _, h, w, _ in by_shape) and any(B > 1 for B, _, _, _ in by_shape)
    # the two rd_loss backward entries: the whole product of sizes, every combination of the five pointers
    for entry in ("lic_rd_loss_bwd", "lic_rd_loss_bwd_lam"):
        by_size = {}
        for c in FC.CASES[entry]:
            by_size.setdefault(tuple(c.sizes[q] for q in ("B", "nx", "ny", "nz")), set()).add(c.shifts)
        assert set(by_size) == set(itertools.product((1, 3), (3, 4, 12, 1035), (1, 5), (1, 5))), entry
        assert all(s == _combos(5) for s in by_size.values()), entry
    # Adam: lengths around AD_ITEMS, three jobs, p / g / m / v independently
    adam = FC.CASES["lic_adam_run"]
    assert {c.shifts for c in adam} == _combos(4) and all(len(c.sizes["lengths"]) == 3 for c in adam)
    # the 16-byte path needs p, g, m and v all aligned: every length runs it, at shift 0 and at a common shift too
    for s in ((0, 0, 0, 0), (1, 1, 1, 1)):
        assert {n for c in adam if c.shifts == s for n in c.sizes["lengths"]} == {1, 3, 4, 5, 4095, 4096, 4097, 8193}, s
    assert {n for c in adam for n in c.sizes["lengths"]} == {1, 3, 4, 5, 4095, 4096, 4097, 8193}
    assert any(c.shifts[0] != c.shifts[1] for c in FC.CASES["lic_swap_run"])


def test_one_element_per_lane_entries_have_their_sizes():
    flat = ("lic_mul_inplace", "lic_quantize", "lic_quantize_anchor", "lic_permute3", "lic_gdn_reparam",
            "lic_gdn_reparam_bwd", "lic_gdn_reparam_bwd2", "lic_gdn_reparam_bwd2_late", "lic_factorized_channel_logits")
    for entry in flat:
        for s in (0, 1):
            assert {c.sizes["n"] for c in FC.CASES[entry] if c.shifts == s} == N_LIST, (entry, s)
    for entry in ("lic_quantize", "lic_quantize_anchor"):
        assert _sizes(entry, "training") == {(0,), (1,)}
    assert _sizes("lic_gdn_reparam_bwd2_late", "late") == {((1, 0),), ((0, 1),), ((1, 1),)}
    assert _sizes("lic_gdn_pass_batch", "njobs") == {(1,), (2,), (32,)} and set(FC.PASS_LENGTHS) == {1, 255, 257}
    pixel = set(itertools.product((1, 3, 257), (1, 3, 5, 8), (1, 2, 3, 8)))
    for entry in ("lic_entropy_params_fwd", "lic_entropy_params_bwd", "lic_gmm_likelihood_fwd", "lic_gmm_likelihood_bwd"):
        assert _sizes(entry, "P", "M", "K") == pixel, entry
    for entry in ("lic_factorized_fwd", "lic_factorized_bwd"):
        assert _sizes(entry, "C", "P") == set(itertools.product((1, 3, 5), (1, 255, 256, 257, 513))), entry
    cs = FC.CASES["lic_colsum"]
    assert _sizes("lic_colsum", "P", "C") == set(itertools.product((1, 15, 16, 17, 4099), (1, 3, 4, 64, 70)))
    for P, Cc in _sizes("lic_colsum", "P", "C"):
        mine = [c for c in cs if (c.sizes["P"], c.sizes["C"]) == (P, Cc)]
        assert any(c.sizes["ld"] == Cc for c in mine) and any(c.sizes["ld"] > Cc and c.sizes["col0"] > 0 for c in mine)
    assert any(c.sizes["C"] == 3 and c.sizes["ld"] == 3 and c.shifts == 0 for c in cs)      # the colsum3 kernel


def test_the_other_groups_have_their_sizes():
    for entry in WANTED["c"]:
        assert {c.sizes["n"] for c in FC.CASES[entry]} == N_LIST, entry
        assert any(FC.bf16_legal(entry, n) for n in N_LIST) and not all(FC.bf16_legal(entry, n) for n in N_LIST)
    u8 = FC.CASES["lic_u8_to_f32"]
    assert {c.sizes["n"] for c in u8 if not c.sizes["refuse"]} == {1, 2, 3, 4, 5, 7, 1023, 1024, 1025}
    assert {c.sizes["refuse"][:2] for c in u8 if c.sizes["refuse"]} == {"ou", "in"}
    assert _sizes("lic_tensor_stats", "n", "nbins") == set(itertools.product((1, 255, 2048, 2049), (1, 64, 4096)))
    for entry in ("lic_window_u8_to_f32", "lic_window_f32"):
        assert _sizes(entry, "h", "w", "C", "border") == set(itertools.product((5, 8), (7, 8), (1, 3), (0, 1, 2))) - \
            {(5, 8, c, b) for c in (1, 3) for b in (0, 1, 2)} - {(8, 7, c, b) for c in (1, 3) for b in (0, 1, 2)}
    assert _sizes("lic_window_u8_to_f32", "flip") == _sizes("lic_resample_u8_to_f32", "flip") == {(0,), (1,)}
    assert _sizes("lic_resample_u8_to_f32", "h", "w", "C") == {(5, 7, 1), (5, 7, 3), (8, 8, 1), (8, 8, 3)}
    assert _sizes("lic_window_f32", "layout") == {("nchw",), ("nhwc",), ("view",)}
    shapes = {(1, 1, 161, 161), (2, 3, 162, 165), (1, 2, 193, 161)}
    for entry in WANTED["e"]:
        assert _sizes(entry, "B", "C", "H", "W", "layout") == {s + (lay,) for s in shapes for lay in ("nchw", "nhwc", "view")}
    assert _sizes("lic_factorized_cdf_tables", "C", "S") == set(itertools.product((1, 5), (2, 64, 65, 66, 129)))
    gm = _sizes("lic_gmm_cdf_tables", "P", "M", "K", "W")
    assert {(1, 1, 1, 1), (3, 5, 3, 8), (2, 4, 1, 32), (1, 3, 2, 33), (1, 2, 1, 64)} <= gm
    above = [s for s in gm if s[0] * s[1] > FC.GMM_WAVE_MAX]
    assert above and min(s[0] * s[1] for s in above) == FC.GMM_WAVE_MAX + 1


def _finite(v, what):
    if isinstance(v, dict):
        for k, u in v.items():
            _finite(u, f"{what}.{k}")
    elif isinstance(v, (list, tuple)):
        for i, u in enumerate(v):
            _finite(u, f"{what}[{i}]")
    elif isinstance(v, torch.Tensor):
        if v.is_floating_point():
            assert bool(torch.isfinite(v.float() if v.dtype == torch.bfloat16 else v).all()), what
    elif isinstance(v, np.ndarray):
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), what
    elif isinstance(v, float):
        assert np.isfinite(v), what


@pytest.mark.parametrize("entry", FC.ENTRIES)
def test_every_reference_runs_on_the_host_and_is_finite(entry):
    made = 0
    for c in FC.CASES[entry]:
        inputs, want = FC.make(c)
        _finite(want, c.id)
        if entry != "lic_tensor_stats":            # (its input holds the NaNs the entry is to count)
            _finite(inputs, c.id + " inputs")
        made += 1
        if entry.startswith("lic_gmm_likelihood"):
            # the conditions ref64.check_gmm asserts on the reference itself: nothing near the bound
            p64, logp64, grads, p_raw = want["ref"]
            dead, live, border = ref64.gmm_regions(p_raw)
            assert not bool(border.any()), c.id
        if entry in ("lic_msssim", "lic_msssim_bwd"):
            assert want["min_term"] > FC.M.MIN_TERM, (c.id, want["min_term"])
        if entry == "lic_gdn_reparam":
            assert int((want["out"].view(torch.int32) - want["fused"].view(torch.int32)).abs().max()) <= 1
    FC.forget(entry)
    assert made == len(FC.CASES[entry]) > 0


def test_fp32_can_hold_the_parameter_gradient_band_at_every_factorised_case():
    """1e-4 of a tensor's own maximum presumes that the maximum is of the order of the terms summed into it.  At C = 1
    a parameter tensor is a few numbers, the last bias one, and where that sum cancels fp32 arithmetic of any order
    misses the band (fence_cases.FE_SEEDS names the two sizes and the figures).  The GPU test
    holds the kernel to the band, so every case must be one where an fp32 host restatement holds it."""
    for Cc, P, seed in sorted({(c.sizes["C"], c.sizes["P"], c.seed) for c in FC.CASES["lic_factorized_bwd"]}):
        e = FC.fe_fp32_restatement_error(Cc, P, seed)
        print(Cc, P, seed, f"{e:.2e}")
        assert e <= 1e-4, (Cc, P, seed, e)
