"""numpy restatement of the 8-bit bicubic resize that lic_resample_u8_to_f32 implements (include/lic.h holds
the definition): Python float coefficients, integer accumulation.  Not a test module."""
import numpy as np

PRECISION_BITS = 22


def _bicubic(t: float) -> float:
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def axis_coefficients(n_in: int, n_out: int, first: int = 0, count=None):
    """[(xmin, int32 k[...])] for output indices first .. first + count - 1 of an axis resized n_in -> n_out"""
    count = n_out - first if count is None else count
    if n_out == n_in:
        return [(xx, np.array([1 << PRECISION_BITS], np.int64)) for xx in range(first, first + count)]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5)) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww = ww + v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5)) for v in w]
        out.append((xmin, np.array(k, np.int64)))
    return out


def _pass(src: np.ndarray, coefs) -> np.ndarray:
    """resample axis 0 of uint8 src [n_in, ...] -> uint8 [len(coefs), ...]"""
    out = np.empty((len(coefs),) + src.shape[1:], np.uint8)
    for i, (xmin, k) in enumerate(coefs):
        taps = src[xmin:xmin + len(k)].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, taps, axes=(0, 0))
        assert np.all(np.abs(acc) < 2 ** 31)                            # the definition is 32-bit arithmetic
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_window(src: np.ndarray, Hn: int, Wn: int, y0: int = 0, x0: int = 0, h=None, w=None, flip: bool = False):
    """uint8 [Hs, Ws, C] -> uint8 [h, w, C]: rows y0 .. y0+h-1, columns x0 .. x0+w-1 of src resized to Hn x Wn,
    computed from those rows and columns only; `flip` mirrors the window"""
    Hs, Ws, _ = src.shape
    h = Hn - y0 if h is None else h
    w = Wn - x0 if w is None else w
    assert Hs <= 2 * Hn and Hn <= Hs and Ws <= 2 * Wn and Wn <= Ws
    assert 0 <= y0 and y0 + h <= Hn and 0 <= x0 and x0 + w <= Wn
    rows = axis_coefficients(Hs, Hn, y0, h)
    cols = axis_coefficients(Ws, Wn, x0, w)
    r0 = rows[0][0]
    r1 = rows[-1][0] + len(rows[-1][1])
    mid = _pass(np.ascontiguousarray(src[r0:r1].transpose(1, 0, 2)), cols).transpose(1, 0, 2)   # [r1-r0, w, C]
    out = _pass(mid, [(xmin - r0, k) for xmin, k in rows])
    return out[:, ::-1].copy() if flip else out


def resample_window_f32(src, Hn, Wn, y0, x0, h, w, flip=False) -> np.ndarray:
    """the kernel's output for one job: fp32 [h, w, C], float(v) / 255 in one division"""
    return resample_window(src, Hn, Wn, y0, x0, h, w, flip).astype(np.float32) / np.float32(255)
