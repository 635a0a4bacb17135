"""The checkerboard context restated in numpy / float64, independent of the package: `anchor`, the
mask, phi = masked_conv(anchor(y)) and a brute-force decode schedule.  NCHW arrays unless said otherwise."""
import numpy as np


def is_anchor(h, w):
    """[h, w] bool: pixel (i, j) is an anchor when i + j is even"""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (i + j) % 2 == 0


def anchor(v):
    """v [..., h, w] (NCHW) -> v at the anchors, +0.0 elsewhere"""
    v = np.asarray(v)
    return np.where(is_anchor(v.shape[-2], v.shape[-1]), v, np.zeros((), v.dtype))


def anchor_nhwc(v):
    """the same for an NHWC [B, h, w, C] array"""
    v = np.asarray(v)
    return np.where(is_anchor(v.shape[1], v.shape[2])[None, :, :, None], v, np.zeros((), v.dtype))


def live_taps(k=5):
    """[(r, s)]: tap (r, s) of a k x k kernel is live exactly when (r - k//2) + (s - k//2) is odd"""
    assert k % 2 == 1
    return [(r, s) for r in range(k) for s in range(k) if ((r - k // 2) + (s - k // 2)) % 2 != 0]


def mask(k=5):
    m = np.zeros((k, k), np.float64)
    for r, s in live_taps(k):
        m[r, s] = 1.0
    return m


def tap_mask(k=5):
    """the bit layout of MaskedConv2d._tap_mask: bit r * k + s"""
    return sum(1 << (r * k + s) for r, s in live_taps(k))


def phi(y_in, weight, bias):
    """masked_conv(anchor(y_in)) in float64: y_in [B, C, h, w], weight [O, C, k, k] (masked here), bias [O]"""
    y = anchor(np.asarray(y_in, np.float64))
    wt = np.asarray(weight, np.float64)
    k = wt.shape[2]
    p = k // 2
    B, C, h, w = y.shape
    yp = np.zeros((B, C, h + 2 * p, w + 2 * p))
    yp[:, :, p:p + h, p:p + w] = y
    out = np.broadcast_to(np.asarray(bias, np.float64)[None, :, None, None], (B, wt.shape[0], h, w)).copy()
    for r, s in live_taps(k):
        out += np.einsum("bchw,oc->bohw", yp[:, :, r:r + h, s:s + w], wt[:, :, r, s])
    return out


def brute_force_schedule(h, w, k=5):
    """[[(i, j)]] per step, raster order inside a step.  A pixel's context is masked_conv(anchor(y)): it depends on
    the in-plane pixels its live taps land on that `anchor` does not zero.  A pixel goes to the earliest step in which
    all of those are already decoded."""
    p = k // 2
    anc = is_anchor(h, w)
    deps = {}
    for i in range(h):
        for j in range(w):
            deps[i, j] = [(i + r - p, j + s - p) for r, s in live_taps(k)
                          if 0 <= i + r - p < h and 0 <= j + s - p < w and anc[i + r - p, j + s - p]]
    done, steps = set(), []
    while len(done) < h * w:
        now = [q for q in sorted(deps) if q not in done and all(d in done for d in deps[q])]
        assert now, "the dependencies have a cycle"
        steps.append(now)
        done.update(now)
    return steps
