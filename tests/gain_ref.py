"""Plain statements of the gain units, for the tests of lic_gain_quantize / lic_gain_bwd, of the rate-level
model and of the LICRATE1 envelope.  numpy only.

Forward, float32 throughout, every operation rounded on its own (numpy never contracts a multiply with an add):
  vg = fl32(v * s);  NOISE: out = fl32(vg + fl32(u - 0.5));  ROUND: out = rint(vg) (ties to even);
  anchor(out) = out where pixel (i, j) has i + j even, +0 elsewhere.
Backward, float64: t = d_vg + d_out + anchor(d_anchor) (absent terms left out), dv = t * s, ds[b][c] = sum_pixels t * v.
Tensors are NHWC [B][h][w][C]; the scale s is [1 or B][C]."""
import struct
import zlib

import numpy as np

SCALE, NOISE, ROUND = 0, 1, 2


def anchor_mask(h, w):
    """[h][w] bool: i + j even"""
    return (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0


def anchor(t):
    """t [B][h][w][C] -> t at the anchors, +0 elsewhere"""
    return np.where(anchor_mask(t.shape[1], t.shape[2])[None, :, :, None], t, t.dtype.type(0))


def rows_of(s, B):
    """the scale [1 or B][C] as [B][1][1][C]"""
    s = np.asarray(s)
    assert s.ndim == 2 and s.shape[0] in (1, B)
    return np.broadcast_to(s, (B, s.shape[1]))[:, None, None, :]


def forward(v, u, s, mode):
    """-> (vg, out, anchor(out)); out and its anchors are None for SCALE.  float32 in, float32 out."""
    v = np.asarray(v, np.float32)
    vg = (v * rows_of(np.asarray(s, np.float32), v.shape[0])).astype(np.float32)
    if mode == SCALE:
        return vg, None, None
    if mode == NOISE:
        half = (np.asarray(u, np.float32) - np.float32(0.5)).astype(np.float32)
        out = (vg + half).astype(np.float32)
    else:
        out = np.rint(vg).astype(np.float32)
    return vg, out, anchor(out)


def grad_sum(d_vg, d_out, d_anchor, dtype):
    """t = d_vg + d_out + anchor(d_anchor), in that order, absent terms left out, every sum rounded to `dtype`"""
    terms = [None if d_vg is None else np.asarray(d_vg, dtype), None if d_out is None else np.asarray(d_out, dtype),
             None if d_anchor is None else anchor(np.asarray(d_anchor, dtype))]
    terms = [t for t in terms if t is not None]
    assert terms
    t = terms[0]
    for more in terms[1:]:
        t = (t + more).astype(dtype)
    return t


def backward64(v, s, d_vg=None, d_out=None, d_anchor=None):
    """-> (dv [B][h][w][C], ds [B][C], sum_pixels |t * v| [B][C]) in float64"""
    v = np.asarray(v, np.float64)
    t = grad_sum(d_vg, d_out, d_anchor, np.float64)
    dv = t * rows_of(np.asarray(s, np.float64), v.shape[0])
    return dv, (t * v).sum(axis=(1, 2)), np.abs(t * v).sum(axis=(1, 2))


def dv32(s, d_vg=None, d_out=None, d_anchor=None):
    """fl32(t * s) with t summed in float32 in the stated order: what lic_gain_bwd writes bit for bit"""
    t = grad_sum(d_vg, d_out, d_anchor, np.float32)
    return (t * rows_of(np.asarray(s, np.float32), t.shape[0])).astype(np.float32), t


def interpolate(log_g, q):
    """the gain row of quality q from a table of log gains [Q][M]: exp((1 - l) * log_g[i] + l * log_g[i + 1]) with
    i = floor(q) clamped to Q - 2, l = q - i.  float64."""
    log_g = np.asarray(log_g, np.float64)
    Q = log_g.shape[0]
    assert Q >= 2 and 0 <= q <= Q - 1
    i = min(int(np.floor(q)), Q - 2)
    lf = q - i
    return np.exp((1.0 - lf) * log_g[i] + lf * log_g[i + 1])


def bwd_workspace_bytes(B, hw, C, slab):
    return 4 * B * (-(-hw // slab)) * C


# ---- the LICRATE1 envelope, read with struct alone ------------------------------------------------------------------
ENVELOPE_MAGIC = b"LICRATE1"


def make_envelope(inner, q, Q, pad=0, length=None, magic=ENVELOPE_MAGIC, crc=None):
    """an envelope with any field set freely (and, unless `crc` is given, a CRC-32 that is right for it)"""
    body = struct.pack("<8sfHHI", magic, q, Q, pad, len(inner) if length is None else length) + bytes(inner)
    return body + struct.pack("<I", (zlib.crc32(body) & 0xFFFFFFFF) if crc is None else crc)


def read_envelope(blob):
    """-> (q, Q, pad, inner length, inner, crc_ok); no checks but the sizes it needs"""
    magic, q, Q, pad, n = struct.unpack_from("<8sfHHI", blob, 0)
    assert magic == ENVELOPE_MAGIC
    inner = bytes(blob[20:20 + n])
    crc_ok = struct.unpack_from("<I", blob, len(blob) - 4)[0] == (zlib.crc32(bytes(blob[:-4])) & 0xFFFFFFFF)
    return q, Q, pad, n, inner, crc_ok
