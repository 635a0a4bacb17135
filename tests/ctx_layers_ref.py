"""numpy restatement of the rows lic_ctx_gather_layers builds, written from its contract in include/lic.h and not from
lic_ctx.hip: pixel by pixel, tap by tap, layer by layer.  The latent plane has `y_pix` channels per pixel; layer l
owns channels [c0, c0 + M_l) and gets rows of its own, as if it were the only layer of a plane that starts at channel
c0.  The tap rule is ctx_slices_ref.tap_live's.  Shared by test_ctx_layers_ref.py and test_gpu_ctx_gather_layers.py."""
import numpy as np

import ctx_slices_ref as SR


def gather_layers(y, R, pix, layers, taps=SR.TAPS, psi=None):
    """y [B, h, w, y_pix]; layers [(c0, M_l)]; pix: raster indices (any out of range gives zero rows); psi
    [B, h*w, C] or None -> [(win [B*n, len(taps)*M_l], psi rows [B*n, C] or None) per layer], row b * n + k for
    entry k of pix"""
    B, h, w, y_pix = y.shape
    n = len(pix)
    out = []
    for c0, M in layers:
        assert 0 <= c0 and M > 0 and c0 + M <= y_pix
        win = np.zeros((B * n, len(taps) * M), y.dtype)
        rows = None if psi is None else np.zeros((B * n, psi.shape[2]), psi.dtype)
        for b in range(B):
            for k, px in enumerate(pix):
                if not 0 <= px < h * w:
                    continue
                i, j = divmod(int(px), w)
                for t, (dr, ds) in enumerate(taps):
                    if SR.tap_live(i, j, dr, ds, h, w, R):
                        win[b * n + k, t * M:(t + 1) * M] = y[b, i + dr, j + ds, c0:c0 + M]
                if psi is not None:
                    rows[b * n + k] = psi[b, px]
        out.append((win, rows))
    return out
