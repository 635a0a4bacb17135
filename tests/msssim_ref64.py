"""Plain-torch reference for MS-SSIM and its gradient: `oracle/torch_ref.ms_ssim` restated so that it computes in
the dtype of its inputs.  The tests call it with float64 tensors widened from the fp32 inputs the device sees and
let torch.autograd differentiate it on the CPU; tests/test_msssim_ref64.py pins it to `TR.ms_ssim` (value and fp32
autograd gradient).

Also the input generators and the shared bands of tests/test_gpu_msssim_grad.py, so that the CPU test can assert
the condition on the inputs (every per-scale term of every image-channel above MIN_TERM) for the very cases the
GPU test compares.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
GRAD_BAND = 5e-4      # of the tensor's max |gradient|: the project's gradient band (tests/test_gpu_variants.py)
VALUE_BAND = 2e-5     # values: the band of tests/test_msssim.py
MIN_TERM = 0.05       # every per-scale term of a parity case must exceed this (far from the relu's kink)


def window(dtype, size=11, sigma=1.5):
    """the package builds its window in fp32; a wider computation uses those fp32 values"""
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).to(dtype)


def _filter(x, g):
    C, k = x.shape[1], g.numel()
    if x.shape[2] >= k:
        x = F.conv2d(x, g.view(1, 1, k, 1).repeat(C, 1, 1, 1), groups=C)
    if x.shape[3] >= k:
        x = F.conv2d(x, g.view(1, 1, 1, k).repeat(C, 1, 1, 1), groups=C)
    return x


def _terms(X, Y, data_range, g, K=(0.01, 0.03)):
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _filter(X, g), _filter(Y, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _filter(X * X, g) - mu1_sq
    s2 = _filter(Y * Y, g) - mu2_sq
    s12 = _filter(X * Y, g) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def scale_terms(X, Y, data_range):
    """[5, B, C]: mean cs of scales 0..3, mean ssim of scale 4 (before the relu), in X's dtype"""
    if min(X.shape[-2:]) <= (11 - 1) * 2 ** 4:
        raise ValueError("Image size should be larger than 160 due to the 4 downsamplings in ms-ssim")
    g = window(X.dtype)
    terms = []
    for i in range(5):
        ssim_c, cs = _terms(X, Y, data_range, g)
        if i < 4:
            terms.append(cs)
            pad = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(terms + [ssim_c], dim=0)


def ms_ssim_per_channel(X, Y, data_range=255.0):
    """[B, C]: prod_l relu(term_l)^w_l"""
    w = torch.tensor(WEIGHTS, dtype=X.dtype).view(-1, 1, 1)
    return torch.prod(torch.relu(scale_terms(X, Y, data_range)) ** w, dim=0)


def ms_ssim(X, Y, data_range=255.0, size_average=True):
    val = ms_ssim_per_channel(X, Y, data_range)
    return val.mean() if size_average else val.mean(1)


def value_and_grad(x, y, data_range=1.0, size_average=True, upstream=None, dtype=torch.float64):
    """x, y: fp32 CPU tensors.  Returns (value, d sum(value * upstream) / d x, smallest per-scale term), computed
    in `dtype`; `upstream` (shape of the value) defaults to ones."""
    X = x.detach().to(dtype).requires_grad_(True)
    Y = y.detach().to(dtype)
    terms = scale_terms(X, Y, data_range)
    w = torch.tensor(WEIGHTS, dtype=dtype).view(-1, 1, 1)
    per = torch.prod(torch.relu(terms) ** w, dim=0)
    val = per.mean() if size_average else per.mean(1)
    up = torch.ones_like(val) if upstream is None else upstream.to(dtype)
    (val * up).sum().backward()
    return val.detach(), X.grad.detach(), float(terms.detach().min())


# ---------------------------------------------------------------------------------------------
# inputs: a smooth image plus Gaussian noise (tests/test_msssim.py's recipe, without the clamp of y: a clamp
# would put a kink of its own into the compared function's input, not into the function)
# ---------------------------------------------------------------------------------------------
def pair(B, C, H, W, seed, noise=0.05, scale=1.0):
    r = np.random.RandomState(seed)
    base = torch.from_numpy(r.rand(B, C, (H + 15) // 16, (W + 15) // 16).astype(np.float32))
    y = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    y = (y + 0.1 * torch.from_numpy(r.rand(B, C, H, W).astype(np.float32))).clamp(0, 1)
    x = y + noise * torch.from_numpy(r.randn(B, C, H, W).astype(np.float32))
    return (scale * x).contiguous(), (scale * y).contiguous()   # x: the distorted image (differentiated), y: the original


# name: (B, C, H, W, seed, noise sigma, data_range, layout)
CASES = {
    "crop_nchw": (2, 3, 256, 256, 1, 0.05, 1.0, "nchw"),
    "crop_nhwc": (2, 3, 256, 256, 2, 0.10, 1.0, "nhwc"),
    "odd_sides": (1, 3, 200, 161, 3, 0.05, 1.0, "nchw"),      # a pad at several scales; one map column at the last
    "kodak_luma": (1, 1, 512, 768, 4, 0.02, 1.0, "nchw"),
    "view": (2, 3, 200, 176, 5, 0.20, 1.0, "view"),           # a window of a larger tensor
    "range255": (1, 3, 256, 192, 6, 0.05, 255.0, "nhwc"),
}


def case_inputs(name):
    B, C, H, W, seed, noise, data_range, layout = CASES[name]
    x, y = pair(B, C, H, W, seed, noise, scale=data_range)
    return x, y, data_range, layout


def undefined_pair(seed=7):
    """a batch of two: image 0 is (1 - y, y) on a textured y (negative structure terms), image 1 a regular pair"""
    r = np.random.RandomState(seed)
    y0 = torch.from_numpy(r.rand(1, 3, 192, 208).astype(np.float32))
    x1, y1 = pair(1, 3, 192, 208, seed + 1, 0.05)
    return torch.cat([1.0 - y0, x1]).contiguous(), torch.cat([y0, y1]).contiguous()
