"""Numpy statement of the window rule of lic_window_u8_to_f32 / lic_window_f32 (include/lic.h):
out[oy, ox, c] = src(border(y0 + oy), border(x0 + ox'), c), ox' = w - 1 - ox when flipped.
Written from the rule, with index arithmetic only; tests compare it with np.pad on the CPU and the
kernels with it on the GPU."""
import numpy as np

ZERO, REPLICATE, REFLECT = 0, 1, 2


def resolve(v: np.ndarray, n: int, border: int):
    """coordinates v of a side of n samples -> (in-range indices, keep mask)"""
    v = np.asarray(v, np.int64)
    inside = (v >= 0) & (v < n)
    if border == ZERO:
        return np.clip(v, 0, n - 1), inside
    if border == REPLICATE:
        return np.clip(v, 0, n - 1), np.ones_like(inside)
    if border == REFLECT:
        if (-v.min() >= n) or (v.max() - (n - 1) >= n):
            raise ValueError("reflect overhang reaches the source side")
        r = np.where(v < 0, -v, np.where(v >= n, 2 * (n - 1) - v, v))
        return r, np.ones_like(inside)
    raise ValueError(f"border {border}")


def window_ref(img: np.ndarray, y0: int, x0: int, h: int, w: int, border: int, flip: bool = False) -> np.ndarray:
    """img [Hs, Ws, C] -> [h, w, C] of img's dtype"""
    Hs, Ws = img.shape[:2]
    ox = np.arange(w)
    if flip:
        ox = w - 1 - ox
    sy, ky = resolve(y0 + np.arange(h), Hs, border)
    sx, kx = resolve(x0 + ox, Ws, border)
    out = img[sy[:, None], sx[None, :]]
    keep = ky[:, None] & kx[None, :]
    return np.where(keep[:, :, None], out, np.zeros((), img.dtype))


def batch_ref(images, rows, crop: int) -> np.ndarray:
    """rows [n, 4] = (image, y0, x0, flip) -> float32 [n, crop, crop, C] of v / 255 (float32 division)"""
    out = [window_ref(images[int(i)], int(y), int(x), crop, crop, ZERO, bool(f)) for i, y, x, f in rows]
    return np.stack(out).astype(np.float32) / np.float32(255)
