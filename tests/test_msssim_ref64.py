"""tests/msssim_ref64.py pinned to oracle/torch_ref.ms_ssim on the CPU: same value, same gradient (fp32 autograd
through the oracle), and the condition on the inputs of tests/test_gpu_msssim_grad.py -- every per-scale term of
every image-channel above MIN_TERM, so that no compared gradient sits near the relu's kink."""
import pytest
import torch

import msssim_ref64 as M
from oracle import torch_ref as TR


def _oracle_value_and_grad(x, y, data_range, size_average=True, upstream=None):
    X = x.clone().requires_grad_(True)
    val = TR.ms_ssim(X, y, data_range=data_range, size_average=size_average)
    up = torch.ones_like(val) if upstream is None else upstream
    (val * up).sum().backward()
    return val.detach(), X.grad


@pytest.mark.parametrize("name", list(M.CASES))
def test_float64_restatement_matches_the_oracle(name):
    x, y, data_range, _ = M.case_inputs(name)
    v64, g64, tmin = M.value_and_grad(x, y, data_range)
    assert tmin > M.MIN_TERM, tmin
    v32, g32 = _oracle_value_and_grad(x, y, data_range)
    assert abs(float(v64) - float(v32)) <= M.VALUE_BAND, (float(v64), float(v32))
    scale = float(g64.abs().max())
    err = float((g32.double() - g64).abs().max()) / scale
    print(f"{name}: value {float(v64):.6f}, smallest term {tmin:.3f}, fp32 oracle gradient {err:.2e} of max|g| "
          f"({err / M.GRAD_BAND:.2f} of the band)")
    assert err <= M.GRAD_BAND, err
    # the same formula in fp32 is the oracle's, operation for operation
    v32r, g32r, _ = M.value_and_grad(x, y, data_range, dtype=torch.float32)
    assert abs(float(v32r) - float(v32)) <= 1e-6
    assert float((g32r - g32).abs().max()) <= 1e-4 * scale


def test_per_image_values_and_a_non_uniform_upstream_gradient():
    x, y, data_range, _ = M.case_inputs("crop_nchw")
    up = torch.tensor([0.25, -1.5])
    v64, g64, _ = M.value_and_grad(x, y, data_range, size_average=False, upstream=up)
    v32, g32 = _oracle_value_and_grad(x, y, data_range, size_average=False, upstream=up)
    assert v64.shape == (2,) and float((v64 - v32.double()).abs().max()) <= M.VALUE_BAND
    assert float((g32.double() - g64).abs().max()) <= M.GRAD_BAND * float(g64.abs().max())
    # image 1's gradient is -6 times what a unit upstream gradient of 0.25 would give image 0's formula: sign and scale
    _, g1, _ = M.value_and_grad(x[1:], y[1:], data_range, size_average=False)
    assert torch.allclose(g64[1:], -1.5 * g1, rtol=1e-9, atol=1e-15)


def test_the_undefined_point_case_has_a_non_positive_term():
    x, y = M.undefined_pair()
    terms = M.scale_terms(x.double(), y.double(), 1.0)          # [5, B, C]
    assert float(terms[:, 0].min()) <= 0.0, terms[:, 0]          # image 0: value 0, derivative undefined
    assert float(terms[:, 1].min()) > M.MIN_TERM, terms[:, 1]    # image 1: a regular pair
    val = M.ms_ssim(x.double(), y.double(), 1.0, size_average=False)
    assert float(val[0]) == 0.0 and float(val[1]) > 0.5
