"""Bit pins for the transposed-tile epilogue of the bf16 direct and fused kernels (csrc/lic_epilogue_bf16.h): the
halo-resident kernels (strided and transposed, plain and with the fused GDN / IGDN pool), igemm_bf16_kernel's FUSE
variant at every instantiated tile, the RGB stem (with the pool, and its PLAIN instantiation through the head's data
gradient) and the one-sweep GDN backward.  Every tensor a launch writes is hashed (CRC-32 of its bytes) and compared
with tests/golden/bf16_epilogue_bits.json; every case asserts through KERNEL_TRACE that the intended kernel ran.

The tolerance tests in test_gpu_bf16.py say the kernels are RIGHT to within an ulp; this one says a change that was
meant to leave the arithmetic alone DID: the rounding points (x and x^2 to bf16, fp32 norm, bf16 norm) and the
summation orders are what the fused and two-launch paths, lic_gdn_bwd_bf16_recompute and every declared bf16
tolerance rest on.

Regenerating the fixture: a DELIBERATE change of a rounding point or of a summation order in one of these kernels is
the only reason to.  Build the tree whose bits are to be pinned and run, on the GPU,

    python tests/test_gpu_bf16_epilogue_bits.py [output.json]        (default: the fixture itself)

then commit the file with the change and say in the commit which digests moved and why.  The module uses only the
functional layer, FORCE_IGEMM and KERNEL_TRACE (and, for the backward sweep, the C entry points the existing tests
call), so it runs unchanged on older trees: a refactor generates the fixture on its parent's build."""
import json
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_recipe as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_epilogue_bits.json")


def rb(a):
    """round a numpy fp32 array to bf16-representable values"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).float().numpy()


def crc(t):
    t = t.detach().contiguous()
    raw = t.view(torch.int16) if t.dtype == BF else t
    return zlib.crc32(raw.cpu().numpy().tobytes())


def nhwc(a, d, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(d).contiguous(memory_format=torch.channels_last)
    return t if dtype is None else t.to(dtype)


# ---- conv -> GDN / IGDN in one launch: (k, s, p, ci, co, H, W, B, transposed, output_padding, inverse, force_bm)
FUSED = {
    "halo_gdn_64_128_37x45":    (5, 2, 2, 64, 128, 37, 45, 2, False, 0, False, 512),   # partial tiles both ways
    "halo_igdn_192_128_16x20":  (5, 2, 2, 192, 128, 16, 20, 2, False, 0, True, 512),   # six chunks, IGDN
    "halot_igdn_64_128_19x21":  (5, 2, 2, 64, 128, 19, 21, 2, True, 1, True, 512),
    "igemm_tn1_64_64_11x9":     (5, 2, 2, 64, 64, 11, 9, 2, False, 0, False, 64),
    "igemm_tn2_64_128_16x16":   (5, 2, 2, 64, 128, 16, 16, 2, False, 0, False, 128),
    "igemm_tn3_72_192_8x8":     (3, 1, 1, 72, 192, 8, 8, 2, False, 0, False, 128),      # stores the norm (192 channels)
    "igemm_bm256_64_128_40x36": (5, 2, 2, 64, 128, 40, 36, 2, False, 0, False, 256),
    "igemm_t4_igdn_128_192_7x5": (5, 2, 2, 128, 192, 7, 5, 2, True, 1, True, 64),       # transposed, 4 phases
    "stem_64_21x19":            (5, 2, 2, 3, 64, 21, 19, 3, False, 0, False, 64),
    "stem_128_20x18":           (5, 2, 2, 3, 128, 20, 18, 2, False, 0, False, 128),
    "stem_192_12x12_gdn":       (5, 2, 2, 3, 192, 12, 12, 1, False, 0, False, 64),
    "stem_192_12x12_igdn":      (5, 2, 2, 3, 192, 12, 12, 1, False, 0, True, 64),
}
NO_BIAS = [k for k in FUSED if k.startswith("igemm_")]   # the FUSE variant loads its bias under a condition

# ---- plain epilogue of the halo kernels: (ci, co, H, W, B, transposed)
PLAIN = {
    "halo_plain_64_128_37x45":    (64, 128, 37, 45, 2, False),
    "halot_plain_128_128_19x37":  (128, 128, 19, 37, 2, True),
}
PLAIN_MODES = {"bf16": dict(), "f32": dict(out_f32=True), "leaky": dict(leaky=True, slope=0.01)}

# ---- one-sweep GDN backward: (C, P, inverse)
SWEEP = {"sweep_64_37_gdn": (64, 37, False), "sweep_64_37_igdn": (64, 37, True),
         "sweep_128_131_gdn": (128, 131, False), "sweep_128_131_igdn": (128, 131, True)}


def _env():
    import neural_image_compression_amd as nic  # noqa: F401
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd import functional_bf16 as FB
    return F_, FB, torch.device("cuda:0")


def run_fused(key, bias=True):
    F_, FB, d = _env()
    from neural_image_compression_amd.layers import GDN
    k, s, p, ci, co, H, W, B, tr, op, inverse, bm = FUSED[key]
    r = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    stem = ci < 4
    x = rb(r.randn(B, ci, H, W).astype(np.float32))
    wshape = (ci, co, k, k) if tr else (co, ci, k, k)
    w = torch.from_numpy(rb(r.randn(*wshape).astype(np.float32) / math.sqrt(ci * k * k))).to(d).requires_grad_(True)
    b = torch.from_numpy(rb(0.1 * r.randn(co).astype(np.float32))).to(d).requires_grad_(True) if bias else None
    g = GDN(co, inverse=inverse).to(d)
    with torch.no_grad():
        g.beta.copy_(torch.from_numpy(R.make_param("g.beta", (co,), 3)))
        g.gamma.copy_(torch.from_numpy(R.make_param("g.gamma", (co, co), 3)))
    bb, gb, pd = g.beta_reparam.bound_value, g.gamma_reparam.bound_value, g.beta_reparam.pedestal_value
    tx = nhwc(x, d, None if stem else BF)
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = (bm, 0, 0), names
    try:
        y = FB.conv_gdn_bf16(tx, w, b, g.beta, g.gamma, s, p, inverse, bb, gb, pd, transposed=tr, output_padding=op)
        _, _, conv_out, norm, _, _ = y.grad_fn.saved_tensors      # what the training forward wrote beside y
        with torch.no_grad():
            y_inf = FB.conv_gdn_bf16(tx, w, b, g.beta, g.gamma, s, p, inverse, bb, gb, pd, transposed=tr, output_padding=op)
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    if stem:
        assert f"stem_gdn_bf16_kernel<{co // 32}, {8 if co == 192 else 4}>" in names, names
    elif bm == 512:
        assert ("halo_convt_bf16_kernel<2, true>" if tr else "halo_conv_bf16_kernel<2, true, 0>") in names, names
    else:
        assert any(n.startswith(f"igemm_bf16_kernel<{256 if bm == 256 else 128}, {co // 64}, false, true") for n in names), names
    assert conv_out is not None and (norm is not None) == (co == 192)
    out = {"y": crc(y), "conv": crc(conv_out), "y_no_grad": crc(y_inf)}
    if norm is not None:
        out["norm"] = crc(norm)
    return out


def run_plain(key, mode):
    F_, FB, d = _env()
    ci, co, H, W, B, tr = PLAIN[key]
    r = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    x = rb(r.randn(B, ci, H, W).astype(np.float32))
    wshape = (ci, co, 5, 5) if tr else (co, ci, 5, 5)
    w = torch.from_numpy(rb(r.randn(*wshape).astype(np.float32) / math.sqrt(ci * 25))).to(d)
    b = torch.from_numpy(rb(0.1 * r.randn(co).astype(np.float32))).to(d)
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = (512, 0, 1), names
    try:
        with torch.no_grad():
            if tr:
                y = FB.conv_transpose2d_bf16(nhwc(x, d, BF), w, b, 2, 2, 1, **PLAIN_MODES[mode])
            else:
                y = FB.conv2d_bf16(nhwc(x, d, BF), w, b, 2, 2, **PLAIN_MODES[mode])
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    assert ("halo_convt_bf16_kernel<2, false>" if tr else "halo_conv_bf16_kernel<2, false, 0>") in names, names
    assert y.dtype == (torch.float32 if mode == "f32" else BF)
    return {"y": crc(y)}


def run_head_dgrad():
    """the stem kernel's PLAIN instantiation: the data gradient of the RGB head (test_head_direct_bf16's 128-channel
    9 x 40 shape)"""
    F_, FB, d = _env()
    C, B, Hi, Wi = 128, 2, 9, 40
    r = np.random.RandomState(C + Hi + Wi)
    xh = rb(r.randn(B, C, Hi, Wi).astype(np.float32))
    wt = torch.from_numpy(rb((r.randn(C, 3, 5, 5) / math.sqrt(C * 25)).astype(np.float32))).to(d).requires_grad_(True)
    bt = torch.from_numpy(rb(r.randn(3).astype(np.float32))).to(d).requires_grad_(True)
    g = rb(r.randn(B, 3, 2 * Hi, 2 * Wi).astype(np.float32))
    txh = nhwc(xh, d, BF).requires_grad_(True)
    names = set()
    F_.KERNEL_TRACE = names
    try:
        out = FB.image_conv_transpose2d_bf16(txh, wt, bt, 2, 2, 1)
        out.backward(nhwc(g, d))
        torch.cuda.synchronize()
    finally:
        F_.KERNEL_TRACE = None
    assert any("plain" in n for n in names), names
    return {"dx": crc(txh.grad)}


def run_sweep(key):
    F_, FB, d = _env()
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd.functional import _ptr, _stream
    C, P, inverse = SWEEP[key]
    lib = L.load()
    r = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    x = torch.from_numpy(rb(r.randn(P, C).astype(np.float32))).to(BF).to(d)
    g = torch.from_numpy(rb(r.randn(P, C).astype(np.float32))).to(BF).to(d)
    nrm = torch.from_numpy(rb((r.rand(P, C) * 3.0 + 0.25).astype(np.float32))).to(BF).to(d)
    gamma_e = torch.from_numpy(rb(np.abs(r.randn(C, C)).astype(np.float32) * 0.05)).to(d)
    beta_e = torch.from_numpy((r.rand(C) * 0.5 + 0.1).astype(np.float32)).to(d)
    gp = FB._pack_bf16(gamma_e, 1, C, C, 0, C, 1, kperm=True)
    gpT = FB._pack_bf16(gamma_e, 1, C, C, 0, 1, C, kperm=True)
    rows = lib.lic_gdn_bwd_bf16_partial_rows(P)
    out = {}
    for what in ("stored", "recomputed"):          # gdn_bwd_bf16_kernel<C / 32, CS = true, RN = false | true>
        dx, t = torch.empty_like(x), torch.empty_like(x)
        pt = torch.full((rows, C), float("nan"), device=d)
        pdx = torch.full((rows, C), float("nan"), device=d)
        if what == "stored":
            L.check(lib.lic_gdn_bwd_bf16(_ptr(g), _ptr(x), _ptr(nrm), _ptr(gp), _ptr(dx), _ptr(t), _ptr(pt), _ptr(pdx), P, C,
                                         int(inverse), _stream()), "lic_gdn_bwd_bf16")
        else:
            L.check(lib.lic_gdn_bwd_bf16_recompute(_ptr(g), _ptr(x), _ptr(gp), _ptr(gpT), _ptr(beta_e), _ptr(dx), _ptr(t),
                                                   _ptr(pt), _ptr(pdx), P, C, int(inverse), _stream()),
                    "lic_gdn_bwd_bf16_recompute")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pt).all()) and bool(torch.isfinite(pdx).all())
        out.update({f"{what}.t": crc(t), f"{what}.dx": crc(dx), f"{what}.colsum_t": crc(pt), f"{what}.colsum_dx": crc(pdx)})
    return out


CASES = {}
for _k in FUSED:
    CASES[_k] = (run_fused, (_k,))
for _k in NO_BIAS:
    CASES[_k + "_nobias"] = (run_fused, (_k, False))
for _k in PLAIN:
    for _m in PLAIN_MODES:
        CASES[f"{_k}_{_m}"] = (run_plain, (_k, _m))
CASES["stem_plain_head_dgrad_128_9x40"] = (run_head_dgrad, ())
for _k in SWEEP:
    CASES[_k] = (run_sweep, (_k,))


@pytest.fixture(scope="module")
def pinned():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bf16_epilogue_bits(pinned, case):
    fn, args = CASES[case]
    got = fn(*args)
    assert case in pinned, f"{case} is not in the fixture"
    assert got == pinned[case], {k: (got.get(k), pinned[case].get(k)) for k in set(got) | set(pinned[case])
                                 if got.get(k) != pinned[case].get(k)}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    res = {}
    for case in sorted(CASES):
        fn, args = CASES[case]
        res[case] = fn(*args)
        print(case, res[case], flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(res)} cases to {path}")
