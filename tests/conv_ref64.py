"""The fp32 convolution family (include/lic.h: lic_igemm, lic_wgrad, lic_im2col, lic_col2im) stated in float64 from fp32
operands, and the cases and inputs of tests/test_gpu_conv_fp32.py.  Imports no product code and nothing of the GPU.

    lic_igemm    out[b,oh,ow,n] = bias[n] + sum_{r,s,k} in[b, oh*stride-pad+r, ow*stride-pad+s, k] W[r*kw+s][k][n]
      transposed out[b,oy,ox,n] = bias[n] + sum_{r,s,k : oy = ih*stride-pad+r, ox = iw*stride-pad+s} in[b,ih,iw,k] W[r*kw+s][k][n]
                 taps outside `tap_mask` drop out, prologue 1 squares `in`, then the epilogue (NONE, LEAKY with res ->
                 out2, MUL_LEAKY_MASK)
    lic_wgrad    R[tap][m][n] = sum_{b,hs,ws} row[b,hs,ws,m] col[b,hs,ws,n], the gathered operand G read at
                 (hs*stride-pad+r, ws*stride-pad+s), 0 outside; dst[m*dst_sm + n*dst_sn + tap*dst_stap] = scale R
    lic_im2col   col[(b,oh,ow)][(r*kw+s)*C + c] = x[b, oh*stride-pad+r, ow*stride-pad+s, c], columns [kh*kw*C, Kpad) zero
    lic_col2im   out[b,oy,ox,c] = bias[c] + sum_{r,s : oy = ih*stride-pad+r, ...} col[(b,ih,iw)][(r*kw+s)*C + c]

They are written as torch double convolutions, slices and einsums of the logical operands W[tap][k][n]; nothing of the
kernels' tiles, chunks, phases or splits appears.  With every result comes S, the float64 sum of the magnitudes of that
element's own terms (|bias| included): the rounding error of an fp32 sum of those terms, in any order, is a multiple of
2^-24 S, so the banded tests hold every element to |err| <= A S with that element's own S, and an exact case is one whose
S stays below 2^24 on integer data (`exact_ok`): then every partial sum is an integer below 2^24 and fp32 forms it without
rounding in any order, tile or split.  tests/test_conv_ref64.py pins these statements to oracle/oracle.py.

The bands.  A is the smallest power of two at least 4 x the worst err / S measured on the MI355X over the banded cases
of its family (the worst of a few thousand rounding errors moves by that much between seeds); none may exceed 2^-19, the
loosest band the project gives a route that accumulates in fp32 (A32 of conv_image_bf16_ref.py).  Measured:

    family                                  worst err / S     A
    lic_igemm, one K slice  (y, dx)         2^-21.51 (3.34e-7)   2^-19
    lic_igemm, K split + finish kernel      2^-22.07 (2.27e-7)   2^-20
    lic_wgrad + slab reduction, lic_colsum  2^-21.35 (3.74e-7)   2^-19
    RGB column route (im2col / col2im)      2^-22.31 (1.92e-7)   2^-20
"""
from __future__ import annotations

import zlib

import numpy as np
import torch
import torch.nn.functional as TF

A_IGEMM = 2.0 ** -19
A_SPLIT = 2.0 ** -20
A_WGRAD = 2.0 ** -19
A_RGB = 2.0 ** -20
A_CEILING = 2.0 ** -19
EXACT_LIMIT = 2.0 ** 24
SLOPE = 0.25          # LeakyReLU slope of the cases: a power of two, so the exact cases stay exact
SCALE = 0.5           # lic_wgrad's `scale` where a case sets one
IG_BK = 16            # channels per K chunk of lic_igemm (csrc/lic_gemm.hip); pixels per K chunk of lic_wgrad
MAX_TAPS = 28         # conv_desc_check: the kernels' per-phase tap list has 28 slots
PGROUP_TILES = 128    # phase_order: a four-phase launch is phase-sorted from 128 M tiles per phase on


def f64(a):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double()
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def conv_out_size(H, W, k, stride, pad, transposed, out_pad=0):
    if transposed:
        return (H - 1) * stride - 2 * pad + k + out_pad, (W - 1) * stride - 2 * pad + k + out_pad
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def mask_a_bits(k):
    """tap_mask of mask A: the taps strictly before the centre in raster order"""
    live = 0
    for r in range(k):
        for s in range(k):
            if r < k // 2 or (r == k // 2 and s < k // 2):
                live |= 1 << (r * k + s)
    return live


def live_taps(kh, kw, tap_mask):
    return torch.tensor([1.0 if (tap_mask == 0 or (tap_mask >> t) & 1) else 0.0 for t in range(kh * kw)], dtype=torch.float64)


# ---------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------
def igemm(x, Wl, g, bias=None, tap_mask=0, sq=False):
    """(acc + bias, S) of one lic_igemm launch before its epilogue: x [B,Hi,Wi,K], Wl [taps,K,N] the logical weight,
    g the descriptor's geometry (B Hi Wi Cin Ho Wo Cout kh kw stride pad transposed) -> two [B,Ho,Wo,N] doubles"""
    x, Wl, bias = f64(x), f64(Wl), f64(bias)
    kh, kw, st, pad = g["kh"], g["kw"], g["stride"], g["pad"]
    taps, K, N = Wl.shape
    assert taps == kh * kw and tuple(x.shape) == (g["B"], g["Hi"], g["Wi"], K) and K == g["Cin"] and N == g["Cout"]
    if sq:
        x = x * x
    Wl = Wl * live_taps(kh, kw, tap_mask)[:, None, None]

    def run(xx, ww, bb):
        xn = xx.permute(0, 3, 1, 2)
        w4 = ww.reshape(kh, kw, K, N)
        if not g["transposed"]:
            y = TF.conv2d(xn, w4.permute(3, 2, 0, 1), None, st, pad)
        else:
            oph = g["Ho"] - ((g["Hi"] - 1) * st - 2 * pad + kh)
            opw = g["Wo"] - ((g["Wi"] - 1) * st - 2 * pad + kw)
            y = TF.conv_transpose2d(xn, w4.permute(2, 3, 0, 1), None, st, pad, output_padding=(oph, opw))
        assert tuple(y.shape[2:]) == (g["Ho"], g["Wo"]), (y.shape, g)
        y = y.permute(0, 2, 3, 1).contiguous()
        return y if bb is None else y + bb
    return run(x, Wl, bias), run(x.abs(), Wl.abs(), None if bias is None else bias.abs())


def leaky(v, slope=SLOPE):
    return torch.where(v > 0, v, v * slope)


def epilogue(v, epi, slope=SLOPE, aux=None, res=None):
    """(out, out2) of lic_igemm's epilogue on v = acc + bias.  LIC_EPI_NONE: v (+ res); LIC_EPI_LEAKY: out = leaky(v),
    out2 = out + res; LIC_EPI_MUL_LEAKY_MASK: v (aux > 0 ? 1 : slope) (+ res)"""
    res, aux = f64(res), f64(aux)
    if epi == "leaky":
        out = leaky(v, slope)
        return out, (None if res is None else out + res)
    if epi == "mulmask":
        v = torch.where(aux > 0, v, v * slope)
    return (v if res is None else v + res), None


def wgrad(P, G, g, drop_pixel=None):
    """(scale R, S) of one lic_wgrad launch: P [B,Hs,Ws,Cp], G [B,Hl,Wl,Cg], g the descriptor's fields -> two
    [taps,Cm,Cn] doubles.  drop_pixel: a mutant's small-grid pixel (flat index) left out of the sum"""
    P, G = f64(P), f64(G)
    B, Hs, Ws, kh, kw, st, pad = g["B"], g["Hs"], g["Ws"], g["kh"], g["kw"], g["stride"], g["pad"]
    assert tuple(P.shape) == (B, Hs, Ws, g["Cp"]) and tuple(G.shape) == (B, g["Hl"], g["Wl"], g["Cg"])
    if g.get("sq_p"):
        P = P * P
    if g.get("sq_g"):
        G = G * G
    if drop_pixel is not None:
        P = P.clone()
        P.view(-1, P.shape[3])[drop_pixel] = 0.0
    below = max(0, (Hs - 1) * st - pad + kh - g["Hl"])
    right = max(0, (Ws - 1) * st - pad + kw - g["Wl"])
    Gp = TF.pad(G, (0, 0, pad, right, pad, below))
    scale = float(g.get("scale", 1.0))
    R, S = [], []
    for r in range(kh):
        for s in range(kw):
            Gt = Gp[:, r:r + (Hs - 1) * st + 1:st, s:s + (Ws - 1) * st + 1:st, :]
            rows, cols = (Gt, P) if g["g_is_row"] else (P, Gt)
            R.append(scale * torch.einsum("bhwm,bhwn->mn", rows, cols))
            S.append(abs(scale) * torch.einsum("bhwm,bhwn->mn", rows.abs(), cols.abs()))
    return torch.stack(R), torch.stack(S)


def colsum(a):
    """(sum over pixels, S): the bias gradient of a [.., C] output gradient"""
    a = f64(a).reshape(-1, a.shape[-1])
    return a.sum(0), a.abs().sum(0)


def im2col(x, Ho, Wo, kh, kw, stride, pad, Kpad):
    """x [B,H,W,C] -> col [B*Ho*Wo, Kpad] (a copy: exact in every format)"""
    x = f64(x)
    B, H, W, C = x.shape
    below = max(0, (Ho - 1) * stride - pad + kh - H)
    right = max(0, (Wo - 1) * stride - pad + kw - W)
    xp = TF.pad(x, (0, 0, pad, right, pad, below))
    col = torch.zeros((B, Ho, Wo, Kpad), dtype=torch.float64)
    for r in range(kh):
        for s in range(kw):
            t = r * kw + s
            col[..., t * C:(t + 1) * C] = xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride, :]
    return col.reshape(B * Ho * Wo, Kpad)


def col2im(col, bias, B, Hi, Wi, C, Ho, Wo, kh, kw, stride, pad, drop_last_row=False):
    """(out, S): col [B*Hi*Wi, Kpad] -> out [B,Ho,Wo,C].  drop_last_row: a mutant without input row Hi - 1"""
    col, bias = f64(col), f64(bias)
    c4 = col.reshape(B, Hi, Wi, -1)
    if drop_last_row:
        c4 = c4.clone()
        c4[:, Hi - 1] = 0.0

    def run(cc, bb):
        # a canvas large enough for every scatter target, cropped to the output window afterwards
        Hc, Wc = (Hi - 1) * stride + kh + max(0, Ho), (Wi - 1) * stride + kw + max(0, Wo)
        out = torch.zeros((B, Hc, Wc, C), dtype=torch.float64)
        for r in range(kh):
            for s in range(kw):
                t = r * kw + s
                out[:, r:r + (Hi - 1) * stride + 1:stride, s:s + (Wi - 1) * stride + 1:stride, :] += cc[..., t * C:(t + 1) * C]
        out = out[:, pad:pad + Ho, pad:pad + Wo, :].contiguous()      # oy = ih*stride - pad + r
        return out if bb is None else out + bb
    return run(c4, bias), run(c4.abs(), None if bias is None else bias.abs())


# ---------------------------------------------------------------------------------------------
# layers: which launches a conv / transposed conv layer is, as functional.py runs it
# ---------------------------------------------------------------------------------------------
def logical_weight(w, kind, dgrad):
    """layer weight (conv [Cout,Cin,kh,kw], convT [Cin,Cout,kh,kw]) -> W[tap][k][n] of the forward launch (k over the
    layer's input channels) or of the data-gradient launch (k over its output channels)"""
    d0, d1 = w.shape[0], w.shape[1]
    w3 = w.reshape(d0, d1, -1)
    if kind == "conv":
        return w3.permute(2, 0, 1) if dgrad else w3.permute(2, 1, 0)
    return w3.permute(2, 1, 0) if dgrad else w3.permute(2, 0, 1)


def pack_strides(kind, dgrad, cin, cout, taps):
    """(taps, K, N, s_tap, s_k, s_n) that read logical_weight(w, kind, dgrad) from the contiguous layer weight"""
    if kind == "conv":
        s_co, s_ci = cin * taps, taps
    else:
        s_ci, s_co = cout * taps, taps
    return (taps, cout, cin, 1, s_co, s_ci) if dgrad else (taps, cin, cout, 1, s_ci, s_co)


class ICase:
    """one convolution layer and the lic_igemm launches of it that the tests run"""

    def __init__(self, name, kind, k, s, p, op, B, H, W, cin, cout, *, mask=False, bias=True, epi="none", in_extra=0,
                 in_off=0, out_ld=None, out_col0=0, aux_extra=0, sq=False, tiles=None, splits=(0,), dgrad=False):
        self.name, self.kind, self.k, self.s, self.p, self.op = name, kind, k, s, p, op
        self.B, self.H, self.W, self.cin, self.cout = B, H, W, cin, cout
        self.Ho, self.Wo = conv_out_size(H, W, k, s, p, kind == "convT", op)
        self.tap_mask = mask_a_bits(k) if mask else 0
        self.bias, self.epi, self.sq = bias, epi, sq
        self.in_extra, self.in_off = in_extra, in_off              # in_ld = Cin + in_extra; `in` moved by in_off floats
        self.out_ld, self.out_col0 = (cout if out_ld is None else out_ld), out_col0   # out = columns [col0, col0 + Cout)
        self.aux_extra = aux_extra
        self.tiles, self.splits, self.dgrad = tiles, tuple(splits), dgrad

    def __repr__(self):
        return self.name

    def geom(self, which="fwd"):
        t = self.kind == "convT"
        if which == "fwd":
            return dict(B=self.B, Hi=self.H, Wi=self.W, Cin=self.cin, Ho=self.Ho, Wo=self.Wo, Cout=self.cout, kh=self.k,
                        kw=self.k, stride=self.s, pad=self.p, transposed=int(t))
        return dict(B=self.B, Hi=self.Ho, Wi=self.Wo, Cin=self.cout, Ho=self.H, Wo=self.W, Cout=self.cin, kh=self.k,
                    kw=self.k, stride=self.s, pad=self.p, transposed=int(not t))

    def vec(self, which="fwd"):
        """float4 loads of the A operand legal (igemm_fill's p.vec)"""
        if which == "dgrad":
            return self.cout % 4 == 0
        return self.cin % 4 == 0 and self.in_extra % 4 == 0 and self.in_off % 4 == 0

    def tile_list(self, which="fwd"):
        """the forced tiles the planner accepts for this launch, (0, 0) = the automatic one"""
        n = self.cin if which == "dgrad" else self.cout
        npad = 32 if n <= 32 else (n + 63) // 64 * 64
        if isinstance(self.tiles, list) and which == "fwd":
            return list(self.tiles)
        if self.tiles != "all" or not self.vec(which):
            return [(0, 0)]
        return [(bm, tn) for bm in (64, 128) for tn in (1, 2, 3) if npad % (64 * tn) == 0]

    def launches(self):
        """(which, (bm, tn), split): split 0 = automatic without workspace, "ws" = automatic with one, n = forced"""
        out = [("fwd", t, sp) for t in self.tile_list("fwd") for sp in self.splits]
        if self.dgrad:
            out += [("dgrad", t, 0) for t in self.tile_list("dgrad")]
        return out

    def max_chunks(self, which="fwd"):
        """K chunks of the phase with the most live taps: (live taps) x ceil(K / 16)"""
        g = self.geom(which)
        cpt = (g["Cin"] + IG_BK - 1) // IG_BK
        live = [t for t in range(self.k * self.k) if self.tap_mask == 0 or (self.tap_mask >> t) & 1]
        if not (g["transposed"] and self.s > 1):
            return len(live) * cpt, cpt
        best = 0
        for py in range(self.s):
            for px in range(self.s):
                n = sum(1 for t in live if (py + self.p - t // self.k) % self.s == 0 and (px + self.p - t % self.k) % self.s == 0)
                best = max(best, n)
        return best * cpt, cpt

    def chunks_per_split(self, split):
        """lic.h's force_split: min(split, chunks) slices of ceil(chunks / slices) chunks -> (chunks per slice, slices)"""
        mc, _ = self.max_chunks()
        cps = -(-mc // min(split, mc))
        return cps, -(-mc // cps)


def _ic(*a, **k):
    return ICase(*a, **k)


M_SPLITS = (0, 2, 4, 7)    # of 27 chunks, three per tap: slices of 14, 7 and 4 chunks all begin inside a tap
IGEMM_CASES = [
    # every forced tile on the LDS-DMA kernels, forward and mirrored; chunks per phase 72 | 100; 108 72 72 48 | 72 48 48 32; 200
    _ic("c3-128", "conv", 3, 1, 1, 0, 2, 9, 7, 128, 128, tiles="all", dgrad=True),
    _ic("c5s2-64-192", "conv", 5, 2, 2, 0, 3, 18, 10, 64, 192, tiles="all", dgrad=True),
    _ic("t5s2-128", "convT", 5, 2, 2, 1, 3, 7, 5, 128, 128, tiles="all", dgrad=True),        # even output sides 14 x 10
    _ic("t5s2-odd-32-64", "convT", 5, 2, 2, 0, 2, 7, 5, 32, 64, tiles="all", dgrad=True),    # odd output sides 13 x 9: 18 12 12 8
    _ic("t3s2-48-64", "convT", 3, 2, 1, 1, 2, 6, 5, 48, 64, tiles="all", bias=False),        # 12 6 6 3 chunks
    _ic("m5-64-128", "conv", 5, 1, 2, 0, 2, 12, 7, 64, 128, mask=True, tiles="all", dgrad=True),   # 12 live taps: 48 chunks
    _ic("c1-192", "conv", 1, 1, 0, 0, 1, 13, 11, 192, 192, tiles="all", dgrad=True),         # 12 chunks
    _ic("c1-16-64", "conv", 1, 1, 0, 0, 1, 9, 7, 16, 64, tiles="all"),                       # one chunk: the ring's shortest tail
    _ic("c1-32-64", "conv", 1, 1, 0, 0, 1, 9, 7, 32, 64, tiles="all"),                       # two chunks
    # the 1x1 stride-2 padding-0 skip of ResidualBlockWithStride (odd sides: 9 x 7 -> 5 x 4; its data gradient reaches every
    # input pixel of even row and column and must leave the others exactly zero); Cin = 20: a ragged K
    _ic("c1s2-128", "conv", 1, 2, 0, 0, 2, 9, 7, 128, 128, tiles="all", dgrad=True),
    _ic("c1s2-64-192", "conv", 1, 2, 0, 0, 2, 9, 7, 64, 192, tiles="all", dgrad=True),
    _ic("c1s2-k20-64", "conv", 1, 2, 0, 0, 2, 9, 7, 20, 64, tiles="all", dgrad=True),
    # prologue 1 (the operand squared on load) keeps the register-staged kernels: every tile of those
    _ic("sq1-128", "conv", 1, 1, 0, 0, 1, 13, 11, 128, 128, sq=True, tiles="all", bias=False),
    _ic("sq1-192", "conv", 1, 1, 0, 0, 1, 13, 11, 192, 192, sq=True, tiles="all"),
    # ragged K: a partial last chunk, behind a pitch whose padding holds NaNs
    _ic("k20-64", "conv", 5, 2, 2, 0, 2, 11, 9, 20, 64, tiles="all", in_extra=4),
    _ic("k36-60", "conv", 3, 1, 1, 0, 2, 9, 7, 36, 60, tiles="all", out_ld=64),              # Npad 64 > Cout, % 4 == 0
    _ic("t-k20-64", "convT", 5, 2, 2, 1, 2, 6, 5, 20, 64, tiles="all", in_extra=12),
    # scalar loads of A: Cin % 4 != 0; an operand 4 bytes off 16-byte alignment
    _ic("k18-30", "conv", 3, 1, 1, 0, 2, 9, 7, 18, 30),                                      # and Cout % 4 != 0, Npad 32
    _ic("k3-64", "conv", 5, 2, 2, 0, 2, 11, 9, 3, 64),
    _ic("unaligned-32-64", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 64, in_off=1),
    _ic("t-k18-66", "convT", 3, 2, 1, 1, 2, 6, 5, 18, 66),                                   # two N tiles, the second ragged
    # Npad = 32: the ragged-N kernels (the 128-row one only by the automatic plan, from 512 tiles of 128 pixels on)
    _ic("n32-32-24", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 24),
    _ic("n32-big-20-24", "conv", 3, 1, 1, 0, 1, 256, 256, 20, 24),
    # the output as a channel slice of a wider tensor
    _ic("slice-vec", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 64, tiles="all", out_ld=200, out_col0=68, in_extra=8),
    _ic("slice-scalar", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 64, out_ld=131, out_col0=67),
    _ic("slice-convT", "convT", 5, 2, 2, 1, 2, 6, 5, 32, 60, out_ld=100, out_col0=20),
    # one phase-sorted launch: 2 * 72 * 72 / 64 = 162 M tiles per phase
    _ic("pgroup-16-64", "convT", 5, 2, 2, 1, 2, 72, 72, 16, 64, tiles=[(64, 1)]),
    # K splits that begin inside a tap (27 chunks, 3 per tap), bias and LeakyReLU applied once by the finish kernels
    _ic("split-48-64", "conv", 3, 1, 1, 0, 2, 9, 7, 48, 64, epi="leaky", tiles="all", splits=M_SPLITS),
    _ic("split-48-30", "conv", 3, 1, 1, 0, 2, 9, 7, 48, 30, epi="leaky", splits=M_SPLITS),           # the scalar finish kernel
    _ic("split-pitched", "conv", 3, 1, 1, 0, 2, 9, 7, 48, 64, splits=M_SPLITS, out_ld=77, out_col0=5),   # scalar finish, pitch
    _ic("split-convT", "convT", 3, 2, 1, 1, 2, 6, 5, 40, 128, epi="leaky", tiles="all", splits=(0, 2, 8)),   # 3 6 6 12 chunks, 3 per tap
    _ic("split-128-192", "conv", 3, 1, 1, 0, 1, 9, 7, 72, 192, tiles="all", splits=(0, 2, 6, 32)),   # 45 chunks, 5 per tap
    # the automatic plan with and without a workspace: 27 chunks of one 64-pixel tile -> three slices
    _ic("auto-ws", "conv", 3, 1, 1, 0, 1, 8, 8, 48, 64, epi="leaky", splits=(0, "ws")),
    # epilogues
    _ic("leaky-res", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 64, epi="leaky_res", tiles="all"),
    _ic("leaky-res-scalar", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 30, epi="leaky_res"),
    _ic("mulmask", "convT", 3, 2, 1, 1, 2, 6, 5, 64, 64, epi="mulmask", bias=False, aux_extra=12, tiles="all"),
    _ic("mulmask-scalar", "conv", 3, 1, 1, 0, 2, 9, 7, 32, 64, epi="mulmask", bias=False, aux_extra=3),
]
ICASE = {c.name: c for c in IGEMM_CASES}
MID_TAP = [("split-48-64", 2), ("split-48-64", 4), ("split-48-64", 7), ("split-48-30", 4), ("split-pitched", 7),
           ("split-convT", 8),("split-128-192", 6), ("split-128-192", 32)]
PGROUP_CASE = "pgroup-16-64"


class WCase:
    """one lic_wgrad launch family: the descriptor's geometry, the destination layout and the forced plans"""

    def __init__(self, name, B, Hs, Ws, Cp, Hl, Wl, Cg, k, s, p, g_is_row, *, sq_p=0, sq_g=0, scale=1.0, layout="dense",
                 tile=(0, 0), splits=(1, 2, 3, 99), p_extra=0, g_extra=0, p_off=0):
        self.name, self.tile, self.splits, self.layout = name, tile, tuple(splits), layout
        self.g = dict(B=B, Hs=Hs, Ws=Ws, Cp=Cp, Hl=Hl, Wl=Wl, Cg=Cg, kh=k, kw=k, stride=s, pad=p, g_is_row=int(g_is_row),
                      sq_p=sq_p, sq_g=sq_g, scale=scale)
        self.p_extra, self.g_extra, self.p_off = p_extra, g_extra, p_off
        self.Cm, self.Cn = (Cg, Cp) if g_is_row else (Cp, Cg)
        self.taps = k * k
        self.pixels = B * Hs * Ws
        self.nchunks = -(-self.pixels // IG_BK)

    def __repr__(self):
        return self.name

    def vec(self):
        return self.g["Cp"] % 4 == 0 and self.g["Cg"] % 4 == 0 and self.p_extra % 4 == 0 and self.g_extra % 4 == 0 and self.p_off % 4 == 0

    def dst_strides(self):
        """(dst_sm, dst_sn, dst_stap, floats spanned): conv = [Cn][Cm][taps], convT = [Cm][Cn][taps] (the weight layouts of
        functional._conv_backward), *-gap = the same inside a larger tensor, dense = [tap][m][n] with a row pitch"""
        t, Cm, Cn = self.taps, self.Cm, self.Cn
        sm, sn, st = {"conv": (t, Cm * t, 1), "convT": (Cn * t, t, 1), "conv-gap": (t + 1, Cm * (t + 1) + 2, 1),
                      "convT-gap": (Cn * (t + 2) + 3, t + 2, 1), "dense": (Cn + 3, 1, Cm * (Cn + 3) + 5)}[self.layout]
        return sm, sn, st, (Cm - 1) * sm + (Cn - 1) * sn + (t - 1) * st + 1

    def split_plan(self, split):
        """wg_plan's force_split: min(split, chunks) slices of ceil(chunks / slices) 16-pixel chunks"""
        cps = -(-self.nchunks // min(split, self.nchunks))
        return cps, -(-self.nchunks // cps)


def _w_layer(name, kind, k, s, p, op, B, H, W, cin, cout, **kw):
    """the weight gradient of a conv / convT layer as functional._conv_backward launches it"""
    Ho, Wo = conv_out_size(H, W, k, s, p, kind == "convT", op)
    if kind == "conv":      # small grid = the output gradient, gathered = the input; rows = input channels
        return WCase(name, B, Ho, Wo, cout, H, W, cin, k, s, p, 1, layout=kw.pop("layout", "conv"), **kw)
    return WCase(name, B, H, W, cin, Ho, Wo, cout, k, s, p, 0, layout=kw.pop("layout", "convT"), **kw)


def _w_dense(name, pixels, Cp, Cg, g_is_row, **kw):
    return WCase(name, 1, 1, pixels, Cp, 1, pixels, Cg, 1, 1, 0, g_is_row, **kw)


def _wgrad_cases():
    out = []
    for tm, tn in ((1, 1), (1, 3), (2, 1), (2, 2), (2, 3)):
        for full in (True, False):
            cm, cn = (64 * tm, 64 * tn) if full else (64 * tm - 12, 64 * tn - 20)
            tag = f"{tm}{tn}{'f' if full else 'r'}"
            # 70 small-grid pixels: five chunks, the last of 6 pixels
            if tm == 1:
                out.append(_w_layer(f"conv5-{tag}", "conv", 5, 2, 2, 0, 2, 10, 13, cm, cn, tile=(tm, tn),
                                    layout="conv" if full else "conv-gap", scale=1.0 if full else SCALE))
                out.append(_w_layer(f"convT3-{tag}", "convT", 3, 2, 1, 0, 2, 5, 7, cm, cn, tile=(tm, tn), splits=(2,),
                                    layout="convT-gap" if full else "convT"))
            else:
                out.append(_w_layer(f"convT5-{tag}", "convT", 5, 2, 2, 1, 2, 5, 7, cm, cn, tile=(tm, tn),
                                    layout="convT" if full else "convT-gap", scale=1.0 if full else SCALE))
                out.append(_w_layer(f"conv3-{tag}", "conv", 3, 2, 1, 0, 2, 10, 13, cm, cn, tile=(tm, tn), splits=(2,),
                                    layout="conv-gap" if full else "conv"))
            # the squared operands of the GDN gradients: on the column side (LDS-DMA kernel), on the row side (register-staged)
            out.append(_w_dense(f"sqcol-{tag}", 70, cm, cn, 0, sq_g=1, tile=(tm, tn), scale=SCALE))
            out.append(_w_dense(f"sqrow-{tag}", 70, cn, cm, 1, sq_g=1, tile=(tm, tn), splits=(1, 3)))
            out.append(_w_dense(f"sqrow-p-{tag}", 70, cm, cn, 0, sq_p=1, tile=(tm, tn), splits=(2,)))
    out += [
        _w_layer("conv5-33", "conv", 5, 2, 2, 0, 2, 10, 13, 192, 192, tile=(3, 3)),
        _w_layer("convT3-33-384", "convT", 3, 2, 1, 1, 2, 5, 7, 384, 192, tile=(3, 3), splits=(1, 3), layout="convT-gap"),
        _w_dense("sqcol-33", 70, 192, 192, 0, sq_g=1, tile=(3, 3), splits=(2, 99)),
        # scalar loads: channel counts that are no multiple of 4; an operand 4 bytes off 16-byte alignment
        _w_layer("conv3-odd", "conv", 3, 2, 1, 0, 2, 10, 13, 22, 41, layout="conv-gap"),
        _w_dense("dense-off", 70, 24, 40, 0, p_off=1, splits=(1, 3)),
        # pitched operands; the automatic plan (force_split 0); a pixel count of whole chunks and of one pixel more
        _w_dense("dense-pitched", 70, 64, 64, 1, p_extra=8, g_extra=4, tile=(1, 1)),
        _w_dense("dense-auto", 1000, 76, 128, 0, splits=(0,)),
        _w_dense("dense-64px", 64, 64, 64, 0, tile=(1, 1), splits=(1, 2, 4, 99)),
        _w_dense("dense-65px", 65, 64, 64, 0, tile=(1, 1), splits=(1, 2, 4, 99)),
        _w_layer("c1-rgbstem", "conv", 1, 1, 0, 0, 1, 1, 300, 76, 64, splits=(0, 2)),
    ]
    return out


layer_wcase = _w_layer
WGRAD_CASES = _wgrad_cases()
WCASE = {c.name: c for c in WGRAD_CASES}

# lic_im2col / lic_col2im: (name, B, H, W, C, k, stride, pad, out_pad, Kpad - k*k*C) of the layer x [B,H,W,C] -> conv -> [B,Ho,Wo,.]
# (im2col runs forward on it; col2im runs its transposed twin, Ho x Wo columns scattered to H x W)
COL_CASES = [
    ("k5-even-pad1", 2, 12, 10, 3, 5, 2, 2, 1, 1),     # Kpad 76 > 75; the transposed twin has output_padding 1
    ("k5-odd-pad1", 2, 11, 9, 3, 5, 2, 2, 0, 1),       # odd sides, output_padding 0
    ("k3-even-tight", 2, 12, 10, 3, 3, 2, 1, 1, 0),    # Kpad 27 = kh*kw*C (not a multiple of 4: the scalar kernel)
    ("k3-odd-pad", 1, 11, 9, 3, 3, 2, 1, 0, 5),        # Kpad 32
    ("k5-c4-tight", 1, 9, 11, 4, 5, 2, 2, 0, 0),       # Kpad 100 = kh*kw*C, a multiple of 4
    ("k1-s2-rgb", 2, 12, 10, 3, 1, 2, 0, 1, 1),        # the RGB skip of the 3x3 model: Kpad 4 = functional._kpad(1, 1, 3), one
                                                       # 16-byte store per pixel (im2col_vec_kernel<float, 4>, col2im_fast_kernel)
]


def col_geom(c):
    name, B, H, W, C, k, s, p, op, extra = c
    Ho, Wo = conv_out_size(H, W, k, s, p, False)
    assert conv_out_size(Ho, Wo, k, s, p, True, op) == (H, W), name
    return dict(B=B, H=H, W=W, C=C, k=k, s=s, p=p, op=op, Ho=Ho, Wo=Wo, Kpad=k * k * C + extra)


# ---------------------------------------------------------------------------------------------
# inputs (fp32 torch tensors on the CPU)
# ---------------------------------------------------------------------------------------------
def _gen(name, salt):
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) * 16 + salt) % (2 ** 63))


def _ints(lo, hi, shape, g_):
    return torch.randint(lo, hi + 1, shape, generator=g_).float()


def igemm_inputs(c, exact):
    """x [B,H,W,Cin], the layer weight w, bias [Cout], dy / res / aux [B,Ho,Wo,Cout].  exact: integers, x in [-3, 3],
    w in [-2, 2] (drawn independently for every tap and channel pair), bias in [-4, 4]; banded: normal, w scaled by
    1 / sqrt(fan-in) as the existing tests do"""
    g_ = _gen(c.name, 1 if exact else 2)
    wshape = (c.cout, c.cin, c.k, c.k) if c.kind == "conv" else (c.cin, c.cout, c.k, c.k)
    xs, ys = (c.B, c.H, c.W, c.cin), (c.B, c.Ho, c.Wo, c.cout)
    if exact:
        d = dict(x=_ints(-3, 3, xs, g_), w=_ints(-2, 2, wshape, g_), b=_ints(-4, 4, (c.cout,), g_), dy=_ints(-3, 3, ys, g_),
                 res=_ints(-3, 3, ys, g_), aux=_ints(-2, 2, ys, g_))
    else:
        fan = c.cin * c.k * c.k / (c.s * c.s if c.kind == "convT" else 1)
        d = dict(x=torch.randn(xs, generator=g_), w=torch.randn(wshape, generator=g_) / fan ** 0.5,
                 b=torch.randn((c.cout,), generator=g_), dy=torch.randn(ys, generator=g_), res=torch.randn(ys, generator=g_),
                 aux=torch.randn(ys, generator=g_))
    if not c.bias:
        d["b"] = None
    return d


def igemm_reference(c, inp, which="fwd", **mut):
    """dict(out, S[, out2]) of the launch `which` of the layer: float64.  mut: the mutants of `igemm_mutant`"""
    g = c.geom(which)
    if which == "fwd":
        Wl = logical_weight(inp["w"], c.kind, False)
        v, S = igemm(inp["x"], Wl, g, inp["b"], c.tap_mask, c.sq)
        epi = "leaky" if c.epi == "leaky_res" else c.epi
        out, out2 = epilogue(v, epi, SLOPE, inp["aux"] if c.epi == "mulmask" else None, inp["res"] if c.epi == "leaky_res" else None)
        return dict(out=out, S=S, out2=out2, pre=v)
    v, S = igemm(inp["dy"], logical_weight(inp["w"], c.kind, True), g, None, c.tap_mask, False)
    return dict(out=v, S=S, out2=None, pre=v)


def wgrad_inputs(c, exact):
    g, g_ = c.g, _gen(c.name, 3 if exact else 4)
    ps, gs = (g["B"], g["Hs"], g["Ws"], g["Cp"]), (g["B"], g["Hl"], g["Wl"], g["Cg"])
    if exact:
        return dict(P=_ints(-3, 3, ps, g_), G=_ints(-3, 3, gs, g_))
    return dict(P=torch.randn(ps, generator=g_), G=torch.randn(gs, generator=g_))


def wgrad_reference(c, inp, **mut):
    R, S = wgrad(inp["P"], inp["G"], c.g, **mut)
    return dict(R=R, S=S)


def scatter_dst(c, R, fill):
    """the flat destination of `c`: R[tap][m][n] at m*sm + n*sn + tap*stap, `fill` everywhere else"""
    sm, sn, st, span = c.dst_strides()
    flat = torch.full((span,), fill, dtype=R.dtype)
    t, m, n = torch.meshgrid(torch.arange(c.taps), torch.arange(c.Cm), torch.arange(c.Cn), indexing="ij")
    idx = (m * sm + n * sn + t * st).reshape(-1)
    assert len(torch.unique(idx)) == idx.numel(), "the destination layout maps two elements to one address"
    flat[idx] = R.reshape(-1)
    return flat, idx


def col_inputs(c, exact):
    """x [B,H,W,C]; the column matrix of the transposed twin [B*Ho*Wo, Kpad] (its padding columns hold values too: col2im
    must not read them); bias [C]"""
    q, g_ = col_geom(c), _gen(c[0], 5 if exact else 6)
    xs, cs = (q["B"], q["H"], q["W"], q["C"]), (q["B"] * q["Ho"] * q["Wo"], q["Kpad"])
    if exact:
        return dict(x=_ints(-3, 3, xs, g_), col=_ints(-3, 3, cs, g_), b=_ints(-4, 4, (q["C"],), g_))
    return dict(x=torch.randn(xs, generator=g_), col=torch.randn(cs, generator=g_), b=torch.randn((q["C"],), generator=g_))


def exact_ok(S):
    """every element's sum of magnitudes is below 2^24: with integer terms every partial sum, in any order, is an integer
    fp32 holds"""
    return bool((f64(S) < EXACT_LIMIT).all())


# ---------------------------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------------------------
def err_over_S(got, ref, S):
    """worst |got - ref| / S over EVERY element (NaN counts as infinite; an element with S = 0 must be exact)"""
    got, ref, S = f64(got), f64(ref), f64(S)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    err = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    r = torch.where(err == 0, torch.zeros_like(err), err / S)
    return float(r.max()) if r.numel() else 0.0


def old_output_band_passes(got, ref):
    """the whole-tensor band the fp32 outputs had: 1e-5 + 1e-4 |ref| (tests/test_gpu_variants.py `close`)"""
    got, ref = f64(got), f64(ref)
    return bool(((got - ref).abs() <= 1e-5 + 1e-4 * ref.abs()).all())


def old_gradient_band_passes(got, ref):
    """the band the gradients had: 1e-4 of the tensor's maximum (`close_norm`)"""
    got, ref = f64(got), f64(ref)
    return bool((got - ref).abs().max() <= 1e-4 * max(float(ref.abs().max()), 1e-30))


def canon_bits(a):
    """int32 patterns of `a` as fp32 with -0 folded into +0 (an exact sum of zeros has either sign)"""
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    a32 = a.to(torch.float32)
    assert torch.equal(a32.double(), a.double()) or bool(torch.isnan(a32).any()), "not representable in fp32"
    return (a32 + 0.0).contiguous().view(torch.int32)


def same_bits(got, ref):
    got, ref = canon_bits(got), canon_bits(ref)
    return got.shape == ref.shape and bool(torch.equal(got, ref))


# ---------------------------------------------------------------------------------------------
# mutants of the float64 statements: each is the statement with one defect of the kind a kernel can have
# ---------------------------------------------------------------------------------------------
def _mut_drop_tap_channel(exact):
    c = ICASE["c5s2-64-192"]
    inp = igemm_inputs(c, exact)
    ref = igemm_reference(c, inp)
    bad = dict(inp)
    bad["w"] = inp["w"].clone()
    bad["w"][:, 17, 3, 1] = 0.0                     # tap (3, 1) of input channel 17
    return "output", ref["out"], igemm_reference(c, bad)["out"], ref["S"], A_IGEMM


def _mut_dead_tap_live(exact):
    c = ICASE["m5-64-128"]
    inp = igemm_inputs(c, exact)
    ref = igemm_reference(c, inp)
    g = c.geom()
    v, _ = igemm(inp["x"], logical_weight(inp["w"], c.kind, False), g, inp["b"], c.tap_mask | (1 << 12), False)   # the centre tap
    return "output", ref["out"], v, ref["S"], A_IGEMM


def _mut_swap_phase_parities(exact):
    """output pixels of row parity a, column parity b take the taps of parity (b, a)"""
    c = ICASE["t5s2-128"]
    inp = igemm_inputs(c, exact)
    ref = igemm_reference(c, inp)
    bad = dict(inp)
    bad["w"] = inp["w"].transpose(2, 3).contiguous()
    alt = igemm_reference(c, bad)["out"]
    mut = ref["out"].clone()
    mut[:, 0::2, 1::2] = alt[:, 0::2, 1::2]
    mut[:, 1::2, 0::2] = alt[:, 1::2, 0::2]
    return "output", ref["out"], mut, ref["S"], A_IGEMM


def _mut_bias_per_slab(exact):
    c = ICASE["split-pitched"]
    inp = igemm_inputs(c, exact)
    ref = igemm_reference(c, inp)
    _, slabs = c.chunks_per_split(4)
    return "output", ref["out"], ref["out"] + (slabs - 1) * inp["b"].double(), ref["S"], A_SPLIT


def _mut_partial_chunk_reads_on(exact):
    """the last chunk of every tap (channels 20 .. 31 of Cin = 20) reads what lies behind the pixel's channels -- the
    next pixel's first channels -- against the weights of the channels it should have read as zero"""
    c = ICASE["k20-64"]
    inp = igemm_inputs(c, exact)
    ref = igemm_reference(c, inp)
    over = IG_BK * (-(-c.cin // IG_BK)) - c.cin
    xs = torch.zeros_like(inp["x"])
    xs[:, :, :-1, :over] = inp["x"][:, :, 1:, :over]
    Wl = logical_weight(inp["w"], c.kind, False).clone()
    Wl[:, over:, :] = 0.0
    extra, _ = igemm(xs, Wl, c.geom(), None, 0, False)
    return "output", ref["out"], ref["out"] + extra, ref["S"], A_IGEMM


def _mut_drop_seam_pixel(exact):
    c = WCASE["convT5-22f"]
    inp = wgrad_inputs(c, exact)
    ref = wgrad_reference(c, inp)
    cps, _ = c.split_plan(2)
    return "gradient", ref["R"], wgrad_reference(c, inp, drop_pixel=cps * IG_BK)["R"], ref["S"], A_WGRAD


def _masked_dw(exact):
    c = ICASE["m5-64-128"]
    inp = igemm_inputs(c, exact)
    g = dict(B=c.B, Hs=c.Ho, Ws=c.Wo, Cp=c.cout, Hl=c.H, Wl=c.W, Cg=c.cin, kh=c.k, kw=c.k, stride=c.s, pad=c.p, g_is_row=1)
    R, S = wgrad(inp["dy"], inp["x"], g)
    return c, R, S


def _mut_dw_masked(exact):
    c, R, S = _masked_dw(exact)
    return "gradient", R, R * live_taps(c.k, c.k, c.tap_mask)[:, None, None], S, A_WGRAD


def _mut_dst_strides_exchanged(exact):
    c = WCASE["conv5-11f"]                       # 64 x 64: a square layer
    assert c.Cm == c.Cn
    inp = wgrad_inputs(c, exact)
    ref = wgrad_reference(c, inp)
    return "gradient", ref["R"], ref["R"].transpose(1, 2).contiguous(), ref["S"], A_WGRAD


def _mut_col2im_last_row(exact):
    c = COL_CASES[0]
    q, inp = col_geom(c), col_inputs(c, exact)
    args = (q["B"], q["Ho"], q["Wo"], q["C"], q["H"], q["W"], q["k"], q["k"], q["s"], q["p"])
    out, S = col2im(inp["col"], inp["b"], *args)
    return "output", out, col2im(inp["col"], inp["b"], *args, drop_last_row=True)[0], S, A_RGB


MUTANTS = {
    "one tap dropped at one input channel": _mut_drop_tap_channel,
    "one dead tap of mask A live": _mut_dead_tap_live,
    "phase parities of the transposed convolution swapped": _mut_swap_phase_parities,
    "bias added once per K slab": _mut_bias_per_slab,
    "partial last chunk reads on instead of zeros": _mut_partial_chunk_reads_on,
    "one pixel dropped at a lic_wgrad split seam": _mut_drop_seam_pixel,
    "dw of the masked convolution masked": _mut_dw_masked,
    "dst_sm / dst_sn exchanged on a square layer": _mut_dst_strides_exchanged,
    "col2im without the last input row": _mut_col2im_last_row,
}


# ---------------------------------------------------------------------------------------------
# descriptors: the fields of lic_igemm_desc / lic_wgrad_desc of a launch, written into any object with those attributes
# (the ctypes mirrors of _lib.py); addresses are plain integers
# ---------------------------------------------------------------------------------------------
EPI_CODE = {"none": 0, "leaky": 1, "leaky_res": 1, "mulmask": 2}


def fill_igemm_desc(d, c, which, tile, split, addr):
    """addr: in, w, out and, where the case has them, bias, out2, res, aux, workspace (+ workspace_bytes)"""
    g = c.geom(which)
    fwd = which == "fwd"
    d.in_, d.w, d.out = addr["in"], addr["w"], addr["out"]
    d.bias = addr.get("bias") if (fwd and c.bias) else None
    d.in_ld = g["Cin"] + (c.in_extra if fwd else 0)
    d.out_ld = c.out_ld if fwd else g["Cout"]
    d.out2_ld = d.res_ld = d.aux2_ld = d.aux3_ld = d.out3_ld = g["Cout"]
    d.aux_ld = g["Cout"] + (c.aux_extra if fwd else 0)
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = g["B"], g["Hi"], g["Wi"], g["Cin"], g["Ho"], g["Wo"], g["Cout"]
    d.kh, d.kw, d.stride, d.pad, d.transposed = g["kh"], g["kw"], g["stride"], g["pad"], g["transposed"]
    d.prologue = 1 if (fwd and c.sq) else 0
    d.epilogue = EPI_CODE[c.epi] if fwd else 0
    d.tap_mask, d.slope = c.tap_mask, SLOPE
    if fwd and c.epi == "leaky_res":
        d.res, d.out2 = addr["res"], addr["out2"]
    if fwd and c.epi == "mulmask":
        d.aux = addr["aux"]
    d.force_bm, d.force_tn = tile
    d.force_split = split if isinstance(split, int) else 0
    if split not in (0, 1):     # (1 = never split: needs no workspace)
        d.workspace, d.workspace_bytes = addr["workspace"], addr["workspace_bytes"]
    return d


def fill_wgrad_desc(d, c, split, addr):
    g = c.g
    d.p, d.g, d.dst = addr["p"], addr["g"], addr["dst"]
    d.p_ld, d.g_ld = g["Cp"] + c.p_extra, g["Cg"] + c.g_extra
    d.dst_sm, d.dst_sn, d.dst_stap, _ = c.dst_strides()
    d.B, d.Hs, d.Ws, d.Cp, d.Hl, d.Wl, d.Cg = g["B"], g["Hs"], g["Ws"], g["Cp"], g["Hl"], g["Wl"], g["Cg"]
    d.kh, d.kw, d.stride, d.pad = g["kh"], g["kw"], g["stride"], g["pad"]
    d.g_is_row, d.sq_p, d.sq_g, d.scale = g["g_is_row"], g["sq_p"], g["sq_g"], g["scale"]
    d.force_tm, d.force_tn = c.tile
    d.force_split = split
    return d
