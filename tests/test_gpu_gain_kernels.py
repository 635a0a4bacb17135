"""lic_gain_quantize and lic_gain_bwd (the gain units of the variable-rate model) against the plain statements
of tests/gain_ref.py, every output between canaries (guarded.py).

Shapes (B, h, w, C): one element; C = 5 (no 16-byte pieces) with an odd w, so the anchor parity flips from row to row;
C = 8 over several images; the model's C = 192 (48 16-byte pieces a pixel, or three passes of lic_gain_bwd's 64 lanes on
the single-float path); and h * w = 2 * LIC_GAIN_SLAB_PIXELS + 5, so that stage two of the backward adds three partial
rows, the last one of a ragged slab.  Each with one scale row for the batch
(s_stride = 0) and one per image (s_stride = C).

Forward: every output bit for bit the float32 statement; bf16 copies bit for bit torch's round-to-nearest-even cast.
Backward: on small integers, where every product and sum is exact in fp32, dv and ds ARE the float64 statement; on random
data dv is fl32(t * s) bit for bit and ds lies within (hw + 2) * 2^-24 * sum |t_i v_i| of float64 -- the standard bound of
an fp32 sum of hw rounded products in any order ((hw - 1) additions and one product, each within 2^-24 relative, and two
more roundings inside t), first order; two runs agree in every bit, and so do the 16-byte and the single-float path.

Run on the MI355X box:  python -m pytest tests/test_gpu_gain_kernels.py -m gpu -q"""
import numpy as np
import pytest
import torch

import gain_ref as G
from guarded import Guarded

pytestmark = pytest.mark.gpu

SLAB = 32                                              # LIC_GAIN_SLAB_PIXELS (asserted against the binding below)
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 5), (3, 7, 9, 8), (1, 4, 4, 192), (2, 3, 23, 12)]
CANARY16 = 0x7FC1                                      # a bf16 quiet NaN no conversion of these inputs produces, as int16
GRADS = ["g", "o", "a", "go", "oa", "goa"]             # which of d_vg, d_out, d_anchor a backward call is given


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    L.load()  # must be the in-tree HIP extension; raises if missing
    assert L.GAIN_SLAB_PIXELS == SLAB and SHAPES[-1][1] * SHAPES[-1][2] == 2 * SLAB + 5
    return L, F_, torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _rne_bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()


class Guarded16:
    """n bf16 values between two fences of 64, everything pre-filled with CANARY16; `shift`: off its 8-byte alignment"""

    def __init__(self, n, dev, shift=0):
        self.n, self.lo = n, 64 + shift
        self.buf = torch.full((n + 128 + shift,), CANARY16, dtype=torch.int16, device=dev)

    def ptr(self):
        return self.buf.data_ptr() + 2 * self.lo

    def values(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def check(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == CANARY16).all() and (b[self.lo + self.n:] == CANARY16).all(), f"{what}: a fence was written"


def _forward_inputs(shape, rows, seed):
    """values whose gained product has exact ties, signed zeros and a product an FMA would round differently"""
    r = np.random.RandomState(seed)
    B, h, w, C = shape
    n = B * h * w * C
    v = (r.randn(n) * 4).astype(np.float32)
    s = r.uniform(0.25, 4.0, (rows, C)).astype(np.float32)
    s[:, 0] = 0.5                                       # channel 0: exact products, so the ties below are ties of vg
    u = r.rand(n).astype(np.float32)
    special = np.array([5.0, -5.0, 3.0, 1.0, -0.0, 0.0, -0.5, 7.0], np.float32)   # * 0.5: 2.5, -2.5, 1.5, .5, -0, 0, -.25, 3.5
    at = (r.permutation(n // C)[:special.size]) * C
    v[at] = special[:at.size]
    if C > 1:                                           # channel 1 of pixel 0: (1 + 2^-23)^2 + 2^-24, the FMA-sensitive tie
        v[1], u[1] = np.float32(1.0 + 2.0 ** -23), np.float32(0.5 + 2.0 ** -24)
        s[:, 1] = np.float32(1.0 + 2.0 ** -23)
    return v.reshape(shape), u.reshape(shape), s


def _run_forward(env, v, u, s, mode, extras, shift=0):
    """-> dict of what the launch wrote (numpy), after the canary checks.  `shift`: vg off its 16-byte alignment."""
    L, F_, dev = env
    B, h, w, C = v.shape
    n = v.size
    dv, ds = torch.from_numpy(v).to(dev), torch.from_numpy(s).to(dev)
    du = torch.from_numpy(u).to(dev) if mode == G.NOISE else None
    quant = mode != G.SCALE
    vg = Guarded(1, n, dev, shift=shift)
    out = Guarded.flat(n, dev) if quant else None
    anc = Guarded.flat(n, dev) if (quant and extras) else None
    g16 = Guarded16(n, dev) if extras else None
    o16 = Guarded16(n, dev) if (quant and extras) else None
    a16 = Guarded16(n, dev) if (quant and extras) else None
    ptr = lambda g: None if g is None else g.ptr()
    L.check(L.load().lic_gain_quantize(F_._ptr(dv), F_._ptr(du), F_._ptr(ds), 0 if s.shape[0] == 1 else C, vg.ptr(),
                                       ptr(out), ptr(anc), ptr(g16), ptr(o16), ptr(a16), B, h, w, C, mode, F_._stream()),
            "lic_gain_quantize")
    torch.cuda.synchronize()
    got = {}
    for name, g in (("vg", vg), ("out", out), ("anchor", anc)):
        if g is not None:
            assert g.unwritten() == 0, name
            g.check(name)
            got[name] = g.cpu().numpy().reshape(v.shape)
    for name, g in (("vg16", g16), ("out16", o16), ("anchor16", a16)):
        if g is not None:
            g.check(name)
            got[name] = g.values().reshape(v.shape)
    return got


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "anchor+bf16"])
@pytest.mark.parametrize("mode", [G.SCALE, G.NOISE, G.ROUND], ids=["scale", "noise", "round"])
@pytest.mark.parametrize("per_image", [False, True], ids=["stride0", "strideC"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_is_the_float32_statement(env, shape, per_image, mode, extras):
    v, u, s = _forward_inputs(shape, shape[0] if per_image else 1, 11 + mode)
    got = _run_forward(env, v, u, s, mode, extras)
    vg, out, anc = G.forward(v, u, s, mode)
    want = {"vg": vg, "out": out, "anchor": anc}
    for name in ("vg", "out", "anchor"):
        assert (name in got) == (want[name] is not None and (name != "anchor" or extras)), name
        if name in got:
            assert (_bits(got[name]) == _bits(want[name])).all(), name
            if name + "16" in got:
                assert (got[name + "16"] == _rne_bf16_bits(got[name])).all(), name + " bf16"
    assert ("vg16" in got) == extras


@pytest.mark.parametrize("mode", [G.SCALE, G.NOISE, G.ROUND], ids=["scale", "noise", "round"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] % 4 == 0], ids=str)
def test_forward_paths_write_the_same_bytes(env, shape, mode):
    """vg one float off its 16-byte alignment sends the launch down the single-float path"""
    v, u, s = _forward_inputs(shape, shape[0], 21)
    a, b = _run_forward(env, v, u, s, mode, True), _run_forward(env, v, u, s, mode, True, shift=1)
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def _given(grads, arrays):
    return [arr if key in grads else None for key, arr in zip("goa", arrays)]


def _run_backward(env, v, s, d_vg, d_out, d_anchor, shift=0):
    """-> (dv, ds) as numpy after the canary checks; the workspace is exactly lic_gain_bwd_workspace_bytes, fenced too"""
    L, F_, dev = env
    lib = L.load()
    B, h, w, C = v.shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    tv, ts, tg, to, ta = up(v), up(s), up(d_vg), up(d_out), up(d_anchor)
    dv, ds = Guarded(1, v.size, dev, shift=shift), Guarded(B, C, dev)
    nbytes = lib.lic_gain_bwd_workspace_bytes(B, h * w, C)
    assert nbytes == G.bwd_workspace_bytes(B, h * w, C, SLAB)
    ws = Guarded.flat(nbytes // 4, dev)
    L.check(lib.lic_gain_bwd(F_._ptr(tv), F_._ptr(ts), 0 if s.shape[0] == 1 else C, F_._ptr(tg), F_._ptr(to), F_._ptr(ta),
                             dv.ptr(), ds.ptr(), B, h, w, C, ws.ptr(), nbytes, F_._stream()), "lic_gain_bwd")
    torch.cuda.synchronize()
    assert dv.unwritten() == 0 and ds.unwritten() == 0
    dv.check("dv"), ds.check("ds"), ws.check("workspace")
    return dv.cpu().numpy().reshape(v.shape), ds.cpu().numpy()


@pytest.mark.parametrize("grads", GRADS)
@pytest.mark.parametrize("per_image", [False, True], ids=["stride0", "strideC"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_exact_on_small_integers(env, shape, per_image, grads):
    """|v|, |d| <= 4, s in {1, 2, 4, 0.5}: |t| <= 12, |t v| <= 48, sums below 2^24 -- nothing rounds"""
    r = np.random.RandomState(31)
    B, h, w, C = shape
    v = r.randint(-4, 5, shape).astype(np.float32)
    s = r.choice([1.0, 2.0, 4.0, 0.5], (B if per_image else 1, C)).astype(np.float32)
    d = _given(grads, [r.randint(-4, 5, shape).astype(np.float32) for _ in range(3)])
    dv, ds = _run_backward(env, v, s, *d)
    dv64, ds64, _ = G.backward64(v, s, *d)
    assert (_bits(dv) == _bits(dv64.astype(np.float32))).all() and np.array_equal(dv.astype(np.float64), dv64)
    assert np.array_equal(ds.astype(np.float64), ds64)


@pytest.mark.parametrize("grads", GRADS)
@pytest.mark.parametrize("per_image", [False, True], ids=["stride0", "strideC"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_on_random_data(env, shape, per_image, grads):
    r = np.random.RandomState(41)
    B, h, w, C = shape
    v = (r.randn(*shape) * 3).astype(np.float32)
    s = r.uniform(0.25, 4.0, (B if per_image else 1, C)).astype(np.float32)
    d = _given(grads, [r.randn(*shape).astype(np.float32) for _ in range(3)])
    dv, ds = _run_backward(env, v, s, *d)
    want_dv, _ = G.dv32(s, *d)
    assert (_bits(dv) == _bits(want_dv)).all()
    _, ds64, mag = G.backward64(v, s, *d)
    err, bound = np.abs(ds.astype(np.float64) - ds64), (h * w + 2) * 2.0 ** -24 * mag
    print(f"ds: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    dv2, ds2 = _run_backward(env, v, s, *d)
    assert dv.tobytes() == dv2.tobytes() and ds.tobytes() == ds2.tobytes()           # the same bits on every run
    if C % 4 == 0:                                                                      # and on either path
        dv1, ds1 = _run_backward(env, v, s, *d, shift=1)
        assert dv.tobytes() == dv1.tobytes() and ds.tobytes() == ds1.tobytes()
