"""numpy restatement of the codec's slice rule, its decode schedule and the rows lic_ctx_gather
builds, written from the rule's text and not from codec.py or lic_ctx.hip: pixel by pixel, tap by tap, no vector
tricks.  Shared by test_ctx_slices_host.py, test_gpu_ctx_gather.py and test_gpu_codec_slices.py."""
import numpy as np

PAD = 2
# the 12 live taps of the type-A 5x5 mask as (dr, ds), in the order of ContextCodec.taps (row-major over the kernel)
TAPS = [(r - PAD, s - PAD) for r in range(5) for s in range(5) if r < PAD or (r == PAD and s < PAD)]


def tap_live(i, j, dr, ds, h, w, R):
    """does tap (dr, ds) of pixel (i, j) contribute y_hat[i + dr, j + ds]?  Inside the image, and, for a tap of a row
    above, inside the pixel's slice of R rows"""
    if not (0 <= i + dr < h and 0 <= j + ds < w):
        return False
    return dr >= 0 or (i % R) + dr >= 0


def step_of(i, j, R, pad=PAD):
    return j + (pad + 1) * (i % R)


def n_steps(h, w, R, pad=PAD):
    return w + (pad + 1) * (min(R, h) - 1)


def schedule(h, w, R, pad=PAD):
    """[(rows, cols)] per step, rows ascending; steps that hold no pixel (w < pad + 1 only) are left out"""
    by_step = {}
    for i in range(h):
        for j in range(w):
            by_step.setdefault(step_of(i, j, R, pad), []).append((i, j))
    return [(np.array([p[0] for p in by_step[t]], np.int64), np.array([p[1] for p in by_step[t]], np.int64))
            for t in sorted(by_step)]


def unsliced_schedule(h, w, pad=PAD):
    """the schedule of the codec before slices existed, as it stood in ContextCodec._wavefront"""
    k = pad + 1
    steps = []
    for t in range(w + k * (h - 1)):
        ii = np.array([i for i in range(h) if 0 <= t - k * i < w], dtype=np.int64)
        if ii.size:
            steps.append((ii, t - k * ii))
    return steps


def same_schedule(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def gather(y, R, pix, taps=TAPS, psi=None):
    """y [B, h, w, M], pix: raster indices (any out of range gives a zero row), psi [B, h*w, C] or None
    -> (win [B*n, len(taps)*M], psi rows [B*n, C] or None), row b * n + k for entry k of pix"""
    B, h, w, M = y.shape
    n = len(pix)
    win = np.zeros((B * n, len(taps) * M), y.dtype)
    rows = None if psi is None else np.zeros((B * n, psi.shape[2]), psi.dtype)
    for b in range(B):
        for k, px in enumerate(pix):
            if not 0 <= px < h * w:
                continue
            i, j = divmod(int(px), w)
            for t, (dr, ds) in enumerate(taps):
                if tap_live(i, j, dr, ds, h, w, R):
                    win[b * n + k, t * M:(t + 1) * M] = y[b, i + dr, j + ds]
            if psi is not None:
                rows[b * n + k] = psi[b, px]
    return win, rows
