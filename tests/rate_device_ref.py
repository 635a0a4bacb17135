"""Plain statements of the device-quality entries: lic_gain_rows_fwd / lic_gain_rows_bwd and the per-image
lambda of lic_rd_loss_fwd_lam / lic_rd_loss_bwd_lam.  numpy only.

Levels: qc = min(max(q, 0), Q-1) with a NaN counting as 0, i = min(floor(qc), Q-2), l = fl32(qc - i) (exact: qc - i has
no more bits than qc).  Rows: exp((1 - l) * T[i] + l * T[i+1]).  Table gradient: for b = 0, 1, ..., B-1 in that order,
d_tables[t][i_b] += ((1 - l_b) * rows[t][b]) * d_rows[t][b], then d_tables[t][i_b + 1] += (l_b * rows[t][b]) * d_rows[t][b];
in float32 every operation is rounded on its own, which is what the kernel writes bit for bit."""
import numpy as np

F = np.float32


def levels(q, Q):
    """q [B] float32 -> (i int32 [B], l float32 [B])"""
    q = np.asarray(q, F)
    qc = np.where(np.isnan(q), F(0), np.minimum(np.maximum(q, F(0)), F(Q - 1))).astype(F)
    i = np.minimum(np.floor(qc).astype(np.int32), Q - 2).astype(np.int32)
    return i, (qc - i.astype(F)).astype(F)


def rows64(q, tables):
    """tables [k][Q][M] -> rows [k][B][M], float64 arithmetic on the float32 operands"""
    T = np.asarray(tables, np.float64)
    i, l = levels(q, T.shape[1])
    l = l.astype(np.float64)[None, :, None]
    return np.exp((1.0 - l) * T[:, i] + l * T[:, i + 1])


def table_grad(i, l, rows, d_rows, Q, dtype):
    """-> (d_tables [k][Q][M], sum of |terms| [k][Q][M]) in `dtype`, the images in rising order; d_rows: a list of k
    arrays [B][M] or None (no gradient: a zero slice)"""
    rows = np.asarray(rows, dtype)
    k, B, M = rows.shape
    out, mag = np.zeros((k, Q, M), dtype), np.zeros((k, Q, M), dtype)
    one = dtype(1)
    for t in range(k):
        if d_rows[t] is None:
            continue
        g = np.asarray(d_rows[t], dtype)
        for b in range(B):
            lb = dtype(l[b])
            first = (((one - lb).astype(dtype) * rows[t, b]).astype(dtype) * g[b]).astype(dtype)
            second = ((lb * rows[t, b]).astype(dtype) * g[b]).astype(dtype)
            out[t, i[b]] = (out[t, i[b]] + first).astype(dtype)
            out[t, i[b] + 1] = (out[t, i[b] + 1] + second).astype(dtype)
            mag[t, i[b]] += np.abs(first)
            mag[t, i[b] + 1] += np.abs(second)
    return out, mag


def distortion_term64(lams, mse_img):
    """slot 9 of lic_rd_loss_fwd_lam in float64: sum_b lambda_b * 65025 * mse_b / B"""
    lams, mse_img = np.asarray(lams, np.float64), np.asarray(mse_img, np.float64)
    return float((lams * 65025.0 * mse_img).sum() / len(lams))


def loss_slot0(bpp_total, distortion):
    """slot 0: fl32(out[3] + out[9])"""
    return F(F(bpp_total) + F(distortion))


def kx32(lam, nx, B):
    """lic_rd_loss_bwd's kx for one lambda: fl32(fl32(fl32(lam * 65025) * 2) / fl32(fl32(nx) * fl32(B)))"""
    a = F(F(lam) * F(65025.0))
    b = F(a * F(2.0))
    return F(b / F(F(nx) * F(B)))
