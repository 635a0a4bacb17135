"""lic_quantize_anchor, lic_quantize_anchor_bf16 and lic_anchor_add (the checkerboard context's elementwise kernels)
bit for bit against numpy (checker_ref.py), every output between canaries (guarded.py).  The shapes are the smallest at
which the kernels can go wrong: an odd w, so the parity flips from row to row; one pixel; C = 6, where the four floats
of a 16-byte piece straddle two pixels; more than one image.

Run on the MI355X box:  python -m pytest tests/test_gpu_checker_kernels.py -m gpu -q"""
import numpy as np
import pytest
import torch

import checker_ref as CR
from guarded import Guarded

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 5, 4), (1, 1, 1, 4), (1, 4, 4, 6), (2, 2, 7, 8)]
SHAPES_BF16 = [s for s in SHAPES if s != (1, 4, 4, 6)]
CANARY16 = 0x7FC1                  # a bf16 quiet NaN no conversion of these inputs produces, as int16


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd import functional as F_
    L.load()  # must be the in-tree HIP extension; raises if missing
    return L, F_, torch.device("cuda:0")


def _inputs(shape, seed):
    """values with exact ties, signed zeros and small negatives (rint gives -0.0) among random ones"""
    r = np.random.RandomState(seed)
    n = int(np.prod(shape))
    v = (r.randn(n) * 4).astype(np.float32)
    special = np.array([0.5, -0.5, 1.5, 2.5, -0.0, 0.0, -0.3, 0.49999997], np.float32)
    at = r.permutation(n)[:min(n, special.size)]
    v[at] = special[:at.size]
    return v.reshape(shape), r.rand(*shape).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _want(v, u, training):
    out = (v + (u - np.float32(0.5))).astype(np.float32) if training else np.rint(v).astype(np.float32)
    return out, CR.anchor_nhwc(out)


def _rne_bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()


class Guarded16:
    """n bf16 values between two fences of 64, everything pre-filled with CANARY16"""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 128,), CANARY16, dtype=torch.int16, device=dev)

    def ptr(self):
        return self.buf.data_ptr() + 128

    def values(self):
        return self.buf[64:64 + self.n].cpu().numpy()

    def check(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:64] == CANARY16).all() and (b[64 + self.n:] == CANARY16).all(), f"{what}: a fence was written"

    def untouched(self):
        return bool((self.buf.cpu().numpy() == CANARY16).all())


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_quantize_anchor_is_quantize_and_its_anchors(env, shape, training):
    L, F_, dev = env
    lib = L.load()
    B, h, w, C = shape
    v, u = _inputs(shape, 7 + training)
    n = v.size
    dv, du = torch.from_numpy(v).to(dev), torch.from_numpy(u).to(dev)
    out, anc = Guarded.flat(n, dev), Guarded.flat(n, dev)
    L.check(lib.lic_quantize_anchor(F_._ptr(dv), F_._ptr(du) if training else None, out.ptr(), anc.ptr(), B, h, w, C,
                                    training, F_._stream()), "lic_quantize_anchor")
    want, want_anchor = _want(v, u, training)
    assert out.unwritten() == 0 and anc.unwritten() == 0
    assert (_bits(out.cpu().numpy().reshape(shape)) == _bits(want)).all()
    assert (_bits(anc.cpu().numpy().reshape(shape)) == _bits(want_anchor)).all()
    out.check("out")
    anc.check("out_anchor")
    # the main output is lic_quantize's
    plain = torch.empty(n, device=dev)
    L.check(lib.lic_quantize(F_._ptr(dv), F_._ptr(du), F_._ptr(plain), n, training, F_._stream()), "lic_quantize")
    assert (_bits(plain.cpu().numpy()) == _bits(out.cpu().numpy()).ravel()).all()
    # +0.0 off the anchors, whatever the sign of the value; the value itself, sign of zero included, on them
    off = ~np.broadcast_to(CR.is_anchor(h, w)[None, :, :, None], shape)
    assert (_bits(anc.cpu().numpy().reshape(shape))[off] == 0).all()


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("shape", SHAPES_BF16, ids=str)
@pytest.mark.parametrize("copies", [(1, 1, 1), (0, 0, 1), (1, 0, 0), (0, 0, 0)], ids=str)
def test_quantize_anchor_bf16_casts_exactly(env, shape, training, copies):
    L, F_, dev = env
    lib = L.load()
    B, h, w, C = shape
    v, u = _inputs(shape, 17 + training)
    n = v.size
    dv, du = torch.from_numpy(v).to(dev), torch.from_numpy(u).to(dev)
    out, anc = Guarded.flat(n, dev), Guarded.flat(n, dev)
    g16 = [Guarded16(n, dev) for _ in range(3)]
    ptrs = [g.ptr() if on else None for g, on in zip(g16, copies)]
    L.check(lib.lic_quantize_anchor_bf16(F_._ptr(dv), F_._ptr(du) if training else None, out.ptr(), anc.ptr(), *ptrs, B, h,
                                         w, C, training, F_._stream()), "lic_quantize_anchor_bf16")
    want, want_anchor = _want(v, u, training)
    got, got_anchor = out.cpu().numpy().reshape(shape), anc.cpu().numpy().reshape(shape)
    assert (_bits(got) == _bits(want)).all() and (_bits(got_anchor) == _bits(want_anchor)).all()
    out.check("out")
    anc.check("out_anchor")
    for g, on, src, what in zip(g16, copies, (v, got, got_anchor), ("v_bf16", "out_bf16", "anchor_bf16")):
        g.check(what)
        if on:      # round-to-nearest-even of the fp32 result, bit for bit
            assert (g.values() == _rne_bf16_bits(src).ravel()).all(), what
        else:
            assert g.untouched(), what


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_anchor_add_is_the_backward_of_both_outputs(env, shape):
    L, F_, dev = env
    B, h, w, C = shape
    r = np.random.RandomState(5)
    g, ga = r.randn(*shape).astype(np.float32), r.randn(*shape).astype(np.float32)
    g.ravel()[:2] = (-0.0, 0.0)
    out = Guarded.flat(g.size, dev)
    dg, dga = torch.from_numpy(g).to(dev), torch.from_numpy(ga).to(dev)
    L.check(L.load().lic_anchor_add(F_._ptr(dg), F_._ptr(dga), out.ptr(), B, h, w, C, F_._stream()), "lic_anchor_add")
    want = (g + CR.anchor_nhwc(ga)).astype(np.float32)
    assert out.unwritten() == 0 and (_bits(out.cpu().numpy().reshape(shape)) == _bits(want)).all()
    out.check("out")
    # off its 16-byte alignment the element-by-element path writes the same bits
    off = Guarded(1, g.size, dev, shift=1)
    L.check(L.load().lic_anchor_add(F_._ptr(dg), F_._ptr(dga), off.ptr(), B, h, w, C, F_._stream()), "lic_anchor_add")
    assert (_bits(off.cpu().numpy().reshape(shape)) == _bits(want)).all()
    off.check("out, shifted")


def test_refusals_launch_nothing(env):
    L, F_, dev = env
    lib = L.load()
    B, h, w, C = 2, 3, 5, 4
    n = B * h * w * C
    src = torch.zeros(n + 4, device=dev)
    out, anc, o16 = Guarded.flat(n, dev), Guarded.flat(n, dev), Guarded16(n, dev)
    p, s = src.data_ptr(), F_._stream()
    invalid = [                                       # LIC_ERR_INVALID = -1, LIC_ERR_UNSUPPORTED = -2 (lic.h)
        lib.lic_quantize_anchor(None, None, out.ptr(), anc.ptr(), B, h, w, C, 0, s),
        lib.lic_quantize_anchor(p, None, None, anc.ptr(), B, h, w, C, 0, s),
        lib.lic_quantize_anchor(p, None, out.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor(p, None, out.ptr(), anc.ptr(), B, h, w, C, 1, s),          # training without noise
        lib.lic_quantize_anchor(p, None, out.ptr(), anc.ptr(), 0, h, w, C, 0, s),
        lib.lic_quantize_anchor(p, None, out.ptr(), anc.ptr(), B, -1, w, C, 0, s),
        lib.lic_quantize_anchor(p, None, out.ptr(), anc.ptr(), B, h, 0, C, 0, s),
        lib.lic_quantize_anchor(p, None, out.ptr(), anc.ptr(), B, h, w, 0, 0, s),
        lib.lic_quantize_anchor_bf16(None, None, out.ptr(), anc.ptr(), None, o16.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), None, None, o16.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr(), None, o16.ptr(), None, B, h, w, C, 1, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr(), None, o16.ptr(), None, B, h, w, -4, 0, s),
        lib.lic_anchor_add(None, p, out.ptr(), B, h, w, C, s),
        lib.lic_anchor_add(p, None, out.ptr(), B, h, w, C, s),
        lib.lic_anchor_add(p, p, None, B, h, w, C, s),
        lib.lic_anchor_add(p, p, out.ptr(), B, h, w, 0, s),
    ]
    assert invalid == [-1] * len(invalid), invalid
    unsupported = [
        # exactly where lic_quantize_bf16 refuses: a count that is no multiple of 4, an fp32 pointer off 16 bytes, a
        # bf16 pointer off 8
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr(), None, o16.ptr(), None, 1, 1, 1, 6, 0, s),
        lib.lic_quantize_anchor_bf16(p + 4, None, out.ptr(), anc.ptr(), None, o16.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr() + 4, anc.ptr(), None, o16.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr() + 8, None, o16.ptr(), None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, p + 4, out.ptr(), anc.ptr(), None, o16.ptr(), None, B, h, w, C, 1, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr(), None, o16.ptr() + 2, None, B, h, w, C, 0, s),
        lib.lic_quantize_anchor_bf16(p, None, out.ptr(), anc.ptr(), None, None, o16.ptr() + 4, B, h, w, C, 0, s),
        lib.lic_quantize_bf16(p, None, out.ptr(), None, o16.ptr(), 6, 0, s),
        lib.lic_quantize_bf16(p + 4, None, out.ptr(), None, o16.ptr(), n, 0, s),
        lib.lic_quantize_bf16(p, None, out.ptr(), None, o16.ptr() + 2, n, 0, s),
    ]
    assert unsupported == [-2] * len(unsupported), unsupported
    torch.cuda.synchronize()
    assert out.untouched() and anc.untouched() and o16.untouched()
