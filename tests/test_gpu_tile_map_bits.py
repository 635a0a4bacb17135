"""Bit pins for the tile-to-pixel map of the MFMA GEMM kernels (csrc/lic_tile_map.h): the XCD-contiguous workgroup
remap, the implicit-GEMM tile decode (rotated and phase-sorted 4-phase launches, K splits), the row -> gather origin
and row -> output pixel maps, the weight-gradient workgroup decode and its small-grid -> gathered pixel map, and the
elementwise epilogue of igemm_kernel on both of its value types.  Covered: every row of the fp32 igemm and wgrad
variant tables and every non-FUSE row of the bf16 igemm table (test_gpu_bf16_epilogue_bits.py pins the FUSE rows,
test_gpu_bf16_reductions.py holds lic_wgrad_bf16 to an exact reference).  Every tensor a launch writes is hashed
(CRC-32 of its bytes) and compared with tests/golden/tile_map_bits.json; every case asserts through KERNEL_TRACE that
the intended variant ran, and test_every_table_row_ran that no row of those tables was left out.

A misplaced pixel does not fail to build and need not leave a tolerance: inputs are real-valued, so two swapped
pixels change a digest.  The tolerance tests say the kernels are RIGHT; this one says that a change meant to leave
index arithmetic, summation order and rounding alone DID.

Regenerating the fixture: only for a DELIBERATE change of a summation order or rounding point in these kernels.  Build
the tree whose bits are to be pinned and run, on the GPU,

    python tests/test_gpu_tile_map_bits.py [output.json]        (default: the fixture itself)

then commit the file with the change and say in the commit which digests moved and why.  The module uses only
functional._igemm / _wgrad / _pack_conv_weight / _pack_dense, functional_bf16._igemm_bf16 / _pack_conv_weight_bf16,
FORCE_IGEMM, FORCE_WGRAD and KERNEL_TRACE, so it runs unchanged on older trees: a refactor generates the fixture on its
parent's build."""
import json
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_map_bits.json")
(EPI_NONE, EPI_LEAKY, EPI_MUL_LEAKY_MASK, EPI_GDN, EPI_IGDN, EPI_GDN_BWD, EPI_IGDN_BWD, EPI_CONV_GDN,
 EPI_CONV_IGDN) = range(9)
RAN = {}     # case -> kernel names it traced (test_every_table_row_ran)


def crc(t):
    t = t.detach().contiguous()
    raw = t.view(torch.int16) if t.dtype == BF else t
    return zlib.crc32(raw.cpu().numpy().tobytes())


def _env():
    import neural_image_compression_amd as nic  # noqa: F401
    from neural_image_compression_amd import functional as F_
    from neural_image_compression_amd import functional_bf16 as FB
    return F_, FB, torch.device("cuda:0")


def _rng(key):
    return np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)


def _out_size(H, W, k, s, p, tr, op):
    if tr:
        return (H - 1) * s - 2 * p + k + op, (W - 1) * s - 2 * p + k + op
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def igemm_name(bm, tn, vec=True, full=True, fuse=False, glds=True):
    return "igemm_kernel<%d, %d, %s>" % (bm, tn, ", ".join(str(bool(v)).lower() for v in (vec, full, fuse, glds)))


# ---- fp32 implicit GEMM ------------------------------------------------------------------------------------------
# k, s, p: kernel, stride, pad; tr / op: transposed, output_padding; H, W, B: input; ci, co; force: FORCE_IGEMM;
# epi / pro: epilogue / prologue; res, out2: pass those operands; pitch: row pitch of the output view (0 = co);
# kern: the variant that must run
def conv(k, s, p, ci, co, H, W, B, kern, tr=False, op=0, force=None, epi=EPI_NONE, pro=0, res=False, out2=False,
         out3=False, pitch=0):
    return dict(k=k, s=s, p=p, ci=ci, co=co, H=H, W=W, B=B, kern=kern, tr=tr, op=op, force=force, epi=epi, pro=pro,
                res=res, out2=out2, out3=out3, pitch=pitch)


IGEMM = {}
# 1. 4-phase transposed launches below 128 M tiles: phases rotate tile by tile; even and odd Ho / Wo; a partial last
#    M tile in every phase
for _H, _W in ((7, 5), (19, 21)):
    for _op in (1, 0):
        for _bm in (64, 128):
            IGEMM[f"t4_rot_{_H}x{_W}_op{_op}_bm{_bm}"] = conv(5, 2, 2, 16, 64, _H, _W, 2, igemm_name(_bm, 1), tr=True,
                                                             op=_op, force=(_bm, 1, 0))
# 2. phase-sorted groups: 8192 rows per phase = 128 tiles of 64; 10240 rows = 160 tiles, padded to 192 (the padding
#    tiles exit at once)
IGEMM["t4_sorted_128x128"] = conv(3, 2, 1, 16, 64, 64, 64, 2, igemm_name(64, 1), tr=True, op=1, force=(64, 1, 0))
IGEMM["t4_sorted_128x160_padded"] = conv(3, 2, 1, 16, 64, 64, 80, 2, igemm_name(64, 1), tr=True, op=1, force=(64, 1, 0))
# 3. single phase, P no multiple of 64, Cin = 20 (ragged last K chunk); every tile of the LDS-DMA loop
for _bm, _tn in ((64, 1), (128, 1), (64, 2), (128, 2), (64, 3), (128, 3)):
    IGEMM[f"s1_3x3_9x7_bm{_bm}_tn{_tn}"] = conv(3, 1, 1, 20, 64 * _tn, 9, 7, 2, igemm_name(_bm, _tn), force=(_bm, _tn, 0))
    IGEMM[f"s2_5x5_11x9_bm{_bm}_tn{_tn}"] = conv(5, 2, 2, 20, 64 * _tn, 11, 9, 3, igemm_name(_bm, _tn),
                                                force=(_bm, _tn, 0))
# 4. split K on a 5x5 layer with 16x16 output: 50 chunks in 3 x 17 and 7 x 8, so splits start inside a tap;
#    igemm_finish4_kernel (Cout % 4 == 0) and igemm_finish_kernel (Cout = 5)
IGEMM["split3_192_tn3"] = conv(5, 1, 2, 20, 192, 16, 16, 2, igemm_name(64, 3), force=(64, 3, 3))
IGEMM["split7_192_tn3_leaky"] = conv(5, 1, 2, 20, 192, 16, 16, 2, igemm_name(64, 3), force=(64, 3, 7), epi=EPI_LEAKY)
IGEMM["split3_64_tn1"] = conv(5, 1, 2, 20, 64, 16, 16, 2, igemm_name(64, 1), force=(64, 1, 3))
IGEMM["split7_64_tn1"] = conv(5, 1, 2, 20, 64, 16, 16, 2, igemm_name(64, 1), force=(64, 1, 7))
IGEMM["split3_3_5_scalar"] = conv(5, 1, 2, 3, 5, 16, 16, 2, igemm_name(64, 1, False, False, False, False), force=(0, 0, 3))
IGEMM["split7_3_5_scalar_leaky"] = conv(5, 1, 2, 3, 5, 16, 16, 2, igemm_name(64, 1, False, False, False, False),
                                        force=(0, 0, 7), epi=EPI_LEAKY)
# 5. scalar A gathers with the scalar epilogue; ragged N with the vector epilogue, at both M tiles (the 128-row one is
#    taken from 512 tiles on: 2 x 192 x 176 = 67584 output pixels)
IGEMM["scalar_3_5_21x19"] = conv(5, 2, 2, 3, 5, 21, 19, 2, igemm_name(64, 1, False, False, False, False))
IGEMM["ragged_8_24_21x19"] = conv(5, 2, 2, 8, 24, 21, 19, 2, igemm_name(64, 1, True, False, False, False))
IGEMM["ragged_16_24_192x176_bm128"] = conv(5, 1, 2, 16, 24, 192, 176, 2, igemm_name(128, 1, True, False, False, False))
# 6. every elementwise epilogue on f32x4 (Cout = 64) and on float (Cout = 6 into a view of row pitch 7), 1x1 and 3x3,
#    LEAKY + residual also on a 4-phase transposed launch
_OPS = {"none": dict(), "leaky": dict(epi=EPI_LEAKY), "leaky_res": dict(epi=EPI_LEAKY, res=True, out2=True),
        "mask": dict(epi=EPI_MUL_LEAKY_MASK), "gdn": dict(epi=EPI_GDN, out2=True), "igdn": dict(epi=EPI_IGDN, out2=True),
        "gdn_bwd": dict(epi=EPI_GDN_BWD), "igdn_bwd": dict(epi=EPI_IGDN_BWD), "none_res": dict(res=True)}
for _i, (_o, _kw) in enumerate(sorted(_OPS.items())):
    _k = (1, 3)[_i & 1]
    IGEMM[f"epi_{_o}_v4_{_k}x{_k}"] = conv(_k, 1, _k // 2, 16, 64, 9, 7, 2, igemm_name(64, 1), force=(64, 1, 0), **_kw)
    IGEMM[f"epi_{_o}_f1_{_k}x{_k}"] = conv(_k, 1, _k // 2, 16, 6, 9, 7, 2, igemm_name(64, 1, True, False, False, False),
                                          pitch=7, **_kw)
IGEMM["epi_leaky_res_v4_t4"] = conv(3, 2, 1, 16, 64, 9, 7, 2, igemm_name(64, 1), tr=True, op=1, force=(64, 1, 0),
                                    **_OPS["leaky_res"])
IGEMM["epi_leaky_res_f1_t4"] = conv(3, 2, 1, 16, 6, 9, 7, 2, igemm_name(64, 1, True, False, False, False), tr=True, op=1,
                                    pitch=7, **_OPS["leaky_res"])
#    prologues 1 (x^2), 2 and 3 (dL/dnorm of a GDN / IGDN, written to out2) on the 1x1 shape: the register-staged loop
for _bm, _tn in ((64, 1), (128, 1), (64, 2), (128, 2), (64, 3), (128, 3)):
    IGEMM[f"pro1_gdn_bm{_bm}_tn{_tn}"] = conv(1, 1, 0, 64 * _tn, 64 * _tn, 9, 7, 2, igemm_name(_bm, _tn, glds=False),
                                             force=(_bm, _tn, 0), epi=EPI_GDN, pro=1, out2=True)
for _bm in (64, 128):
    IGEMM[f"pro2_gdn_bwd_bm{_bm}"] = conv(1, 1, 0, 64, 64, 9, 7, 2, igemm_name(_bm, 1, glds=False), force=(_bm, 1, 0),
                                         epi=EPI_GDN_BWD, pro=2, out2=True)
    IGEMM[f"pro3_igdn_bwd_bm{_bm}"] = conv(1, 1, 0, 64, 64, 9, 7, 2, igemm_name(_bm, 1, glds=False), force=(_bm, 1, 0),
                                          epi=EPI_IGDN_BWD, pro=3, out2=True)
# 7. conv -> GDN / IGDN in one launch, with and without the stored conv output and norm
for _tn in (1, 2, 3):
    for _e, _n in ((EPI_CONV_GDN, "gdn"), (EPI_CONV_IGDN, "igdn")):
        IGEMM[f"fused_{_n}_{64 * _tn}"] = conv(3, 1, 1, 16, 64 * _tn, 9, 7, 2, igemm_name(64, _tn, fuse=True), epi=_e,
                                              out2=True, out3=True)
    IGEMM[f"fused_gdn_{64 * _tn}_infer"] = conv(3, 1, 1, 16, 64 * _tn, 9, 7, 2, igemm_name(64, _tn, fuse=True),
                                               epi=EPI_CONV_GDN)
IGEMM["fused_igdn_128_t4"] = conv(5, 2, 2, 16, 128, 7, 5, 2, igemm_name(64, 2, fuse=True), tr=True, op=1,
                                  epi=EPI_CONV_IGDN, out2=True, out3=True)


def _conv_operands(key, c, d, positive):
    """input [B,H,W,ci], weight in nn layout, bias; `positive`: operands of an rsqrt / sqrt epilogue"""
    r = _rng(key)
    x = r.randn(c["B"], c["H"], c["W"], c["ci"]).astype(np.float32)
    wshape = (c["ci"], c["co"], c["k"], c["k"]) if c["tr"] else (c["co"], c["ci"], c["k"], c["k"])
    w = (r.randn(*wshape) / math.sqrt(c["ci"] * c["k"] * c["k"])).astype(np.float32)
    b = (0.1 * r.randn(c["co"])).astype(np.float32)
    if positive:
        x, w, b = np.abs(x) + 0.25, np.abs(w) + 0.01, np.abs(b) + 0.1
    return r, torch.from_numpy(x).to(d), torch.from_numpy(w).to(d), torch.from_numpy(b).to(d)


def run_igemm(key):
    F_, FB, d = _env()
    c = IGEMM[key]
    epi, pro, co, ci, B = c["epi"], c["pro"], c["co"], c["ci"], c["B"]
    fused = epi in (EPI_CONV_GDN, EPI_CONV_IGDN)
    positive = epi in (EPI_GDN, EPI_IGDN) or pro in (2, 3)
    r, x, w, b = _conv_operands(key, c, d, positive)
    Ho, Wo = _out_size(c["H"], c["W"], c["k"], c["s"], c["p"], c["tr"], c["op"])
    P = B * Ho * Wo

    def act(pos=False, ch=co):     # an activation-shaped operand [P][ch]
        a = r.randn(P, ch).astype(np.float32)
        return torch.from_numpy(np.abs(a) + 0.25 if pos else a).to(d)

    pitch = c["pitch"] or co
    buf = torch.full((P, pitch), -7.0, device=d)     # the columns past Cout of a pitched view must stay untouched
    out = buf[:, :co]
    kw = dict(bias=b, prologue=pro, epilogue=epi, slope=0.125)
    wrote = {"out": buf}
    if c["res"]:
        kw["res"] = act()
    if c["out2"]:
        kw["out2"] = wrote["out2"] = torch.full((P, ci if pro in (2, 3) else co), -7.0, device=d)
    if c["out3"]:
        kw["out3"] = wrote["out3"] = torch.full((P, co), -7.0, device=d)
    if fused:
        gamma_t = torch.from_numpy((np.abs(r.randn(co, co)) * 0.05 + 0.001).astype(np.float32)).to(d)
        kw["aux"] = F_._pack_dense(gamma_t)
        kw["aux2"] = torch.from_numpy((r.rand(co) * 0.5 + 0.1).astype(np.float32)).to(d)
    elif epi in (EPI_MUL_LEAKY_MASK, EPI_GDN, EPI_IGDN):
        kw["aux"] = act()
    elif epi in (EPI_GDN_BWD, EPI_IGDN_BWD):
        kw["aux"], kw["aux2"], kw["aux3"] = (x.reshape(P, ci) if pro in (2, 3) else act()), act(), act(pos=True)
    wp = F_._pack_conv_weight(w, c["tr"], for_dgrad=False)
    names = set()
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = c["force"], names
    try:
        F_._igemm(x, wp, out, B=B, Hi=c["H"], Wi=c["W"], Cin=ci, Ho=Ho, Wo=Wo, Cout=co, kh=c["k"], kw=c["k"],
                  stride=c["s"], pad=c["p"], transposed=c["tr"], out_ld=pitch if c["pitch"] else None, **kw)
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
    assert names == {c["kern"]}, (names, c["kern"])
    RAN[key] = names
    assert bool(torch.isfinite(out).all())
    return {k: crc(v) for k, v in wrote.items()}


# ---- fp32 weight gradient ----------------------------------------------------------------------------------------
# (kernel, TM, TN, third template argument, FULL): every row of g_wgrad_variants
WGRAD_ROWS = [("wgrad_kernel", 1, 1, False, False)]
for _tm, _tn in ((1, 1), (1, 3), (2, 1), (2, 2), (2, 3)):
    for _full in (False, True):
        WGRAD_ROWS.append(("wgrad_kernel", _tm, _tn, True, _full))
        for _sqb in (False, True):
            WGRAD_ROWS.append(("wgrad_glds_kernel", _tm, _tn, _sqb, _full))
WGRAD_ROWS += [("wgrad_glds_kernel", 3, 3, False, True), ("wgrad_glds_kernel", 3, 3, True, True)]
# small grid / large grid: gathered 5x5 stride 2 (Ps = 3 * 6 * 5 = 90: no multiple of the 16-pixel chunk, padding taps
# dead) and ungathered 1x1
WGRAD_GEO = {"g5": (3, 6, 5, 11, 9, 5, 2, 2), "u1": (3, 9, 7, 9, 7, 1, 1, 0)}
WGRAD = {}
for _i, (_kn, _tm, _tn, _flag, _full) in enumerate(WGRAD_ROWS):
    for _j, _geo in enumerate(sorted(WGRAD_GEO)):
        _nm = "%s<%d, %d, %s, %s>" % (_kn, _tm, _tn, str(_flag).lower(), str(_full).lower())
        WGRAD[f"wg_{_kn[6:-7] or 'reg'}_{_tm}{_tn}_{int(_flag)}{int(_full)}_{_geo}"] = dict(
            kern=_nm, tm=_tm, tn=_tn, geo=_geo, full=_full, scalar=(_kn == "wgrad_kernel" and not _flag),
            sq_row=(_kn == "wgrad_kernel" and _flag), sq_col=(_kn == "wgrad_glds_kernel" and _flag),
            g_is_row=bool((_i + _j) & 1), split=(1, 2, 5)[(_i + 2 * _j) % 3])


def run_wgrad(key):
    F_, FB, d = _env()
    c = WGRAD[key]
    B, Hs, Ws, Hl, Wl, k, s, pad = WGRAD_GEO[c["geo"]]
    tm, tn = c["tm"], c["tn"]
    if c["scalar"]:
        cm, cn = 3, 5
    elif c["full"]:
        cm, cn = (128 if tm == 1 else 64 * tm), (128 if tn == 1 else 64 * tn)
    else:
        cm, cn = 64 * tm + 8, 64 * tn - 20     # a second, mostly dead tile in M; a ragged one in N
    g_is_row = c["g_is_row"]
    cg, cp = (cm, cn) if g_is_row else (cn, cm)
    r = _rng(key)
    p = torch.from_numpy(r.randn(B * Hs * Ws, cp).astype(np.float32)).to(d)
    g = torch.from_numpy(r.randn(B * Hl * Wl, cg).astype(np.float32)).to(d)
    taps = k * k
    dst = torch.full((cm, cn, taps), float("nan"), device=d)
    sq_g, sq_p = (c["sq_row"], c["sq_col"]) if g_is_row else (c["sq_col"], c["sq_row"])
    names = set()
    F_.FORCE_WGRAD, F_.KERNEL_TRACE = (0 if c["scalar"] else tm, 0 if c["scalar"] else tn, c["split"]), names
    try:
        F_._wgrad(p, g, dst, B=B, Hs=Hs, Ws=Ws, Cp=cp, Hl=Hl, Wl=Wl, Cg=cg, kh=k, kw=k, stride=s, pad=pad,
                  g_is_row=g_is_row, dst_sm=cn * taps, dst_sn=taps, dst_stap=1, sq_p=int(sq_p), sq_g=int(sq_g), scale=0.5)
        torch.cuda.synchronize()
    finally:
        F_.FORCE_WGRAD, F_.KERNEL_TRACE = None, None
    assert names == {c["kern"]}, (names, c["kern"])
    RAN[key] = names
    assert bool(torch.isfinite(dst).all())
    return {"dw": crc(dst)}


# ---- plain igemm_bf16_kernel and the plain halo kernels ----------------------------------------------------------
def bf16_name(bm, tn, sq=False, ring=None):
    ring = ring or (4 if bm == 256 or (bm == 128 and tn <= 2 and not sq) else 3)
    return "igemm_bf16_kernel<%d, %d, %s, false, %d, %d>" % (bm, tn, str(sq).lower(), ring, 8 if bm == 256 else 4)


def hconv(k, s, p, ci, co, H, W, B, kern, force, tr=False, op=0, epi=EPI_NONE, pro=0, out2=False, f32=False, ring3=False):
    return dict(k=k, s=s, p=p, ci=ci, co=co, H=H, W=W, B=B, kern=kern, tr=tr, op=op, force=force, epi=epi, pro=pro,
                out2=out2, f32=f32, ring3=ring3)


IGEMMH = {}
for _tn in (1, 2, 3):
    for _bm in (64, 128, 256):
        # 4-phase transposed, odd output (19 x 17 -> 37 x 33)
        IGEMMH[f"h_t4_bm{_bm}_tn{_tn}"] = hconv(5, 2, 2, 64, 64 * _tn, 19, 17, 2, bf16_name(_bm, _tn), (_bm, 0, 0), tr=True)
    for _bm in (64, 128):
        IGEMMH[f"h_sq_gdn_bm{_bm}_tn{_tn}"] = hconv(1, 1, 0, 64 * _tn, 64 * _tn, 9, 7, 2, bf16_name(_bm, _tn, sq=True),
                                                   (_bm, 0, 0), epi=EPI_GDN, pro=1, out2=True)
for _tn in (1, 2):    # the three-buffer ring of the 128-row tile (tuning aid)
    IGEMMH[f"h_ring3_bm128_tn{_tn}"] = hconv(3, 1, 1, 72, 64 * _tn, 9, 7, 2, bf16_name(128, _tn, ring=3), (128, 0, 0),
                                             ring3=True)
IGEMMH["h_leaky_bm128_tn1"] = hconv(3, 1, 1, 72, 64, 9, 7, 2, bf16_name(128, 1), (128, 0, 0), epi=EPI_LEAKY)
IGEMMH["h_gdn_bwd_bm256_tn2"] = hconv(1, 1, 0, 128, 128, 20, 13, 2, bf16_name(256, 2), (256, 0, 0), epi=EPI_GDN_BWD)
IGEMMH["h_split3_bf16_out"] = hconv(5, 2, 2, 64, 192, 16, 16, 2, bf16_name(128, 3), (128, 0, 3))
IGEMMH["h_split3_f32_out"] = hconv(5, 2, 2, 64, 192, 16, 16, 2, bf16_name(128, 3), (128, 0, 3), f32=True)
IGEMMH["h_halo_plain"] = hconv(5, 2, 2, 64, 128, 19, 21, 2, "halo_conv_bf16_kernel<2, false, 0>", (512, 0, 1))
IGEMMH["h_halot_plain"] = hconv(5, 2, 2, 64, 128, 9, 11, 2, "halo_convt_bf16_kernel<2, false>", (512, 0, 1), tr=True, op=1)


def rb(a):
    """round a numpy fp32 array to bf16-representable values"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).float().numpy()


def run_igemm_bf16(key):
    F_, FB, d = _env()
    c = IGEMMH[key]
    epi, pro, co, ci, B = c["epi"], c["pro"], c["co"], c["ci"], c["B"]
    r = _rng(key)
    positive = epi in (EPI_GDN, EPI_IGDN)
    x = r.randn(B, c["H"], c["W"], ci).astype(np.float32)
    wshape = (ci, co, c["k"], c["k"]) if c["tr"] else (co, ci, c["k"], c["k"])
    w = (r.randn(*wshape) / math.sqrt(ci * c["k"] * c["k"])).astype(np.float32)
    b = (0.1 * r.randn(co)).astype(np.float32)
    if positive:
        x, w, b = np.abs(x) + 0.25, np.abs(w) + 0.01, np.abs(b) + 0.1
    xt = torch.from_numpy(rb(x)).to(d).to(BF)
    wt, bt = torch.from_numpy(rb(w)).to(d), torch.from_numpy(rb(b)).to(d)
    Ho, Wo = _out_size(c["H"], c["W"], c["k"], c["s"], c["p"], c["tr"], c["op"])
    P = B * Ho * Wo

    def act(pos=False):
        a = r.randn(P, co).astype(np.float32)
        return torch.from_numpy(rb(np.abs(a) + 0.25 if pos else a)).to(d).to(BF)

    out = torch.full((P, co), -7.0, device=d, dtype=torch.float32 if c["f32"] else BF)
    kw = dict(bias=bt, prologue=pro, epilogue=epi, slope=0.125)
    wrote = {"out": out}
    if c["out2"]:
        kw["out2"] = wrote["out2"] = torch.full((P, co), -7.0, device=d, dtype=BF)
    if epi in (EPI_GDN, EPI_IGDN):
        kw["aux"] = act()
    elif epi in (EPI_GDN_BWD, EPI_IGDN_BWD):
        kw["aux"], kw["aux2"], kw["aux3"] = act(), act(), act(pos=True)
    wp = FB._pack_conv_weight_bf16(wt, c["tr"], False)
    names = set()
    old = os.environ.get("LIC_BF16_RING")
    if c["ring3"]:
        os.environ["LIC_BF16_RING"] = "3"
    F_.FORCE_IGEMM, F_.KERNEL_TRACE = c["force"], names
    try:
        FB._igemm_bf16(xt, wp, out, B=B, Hi=c["H"], Wi=c["W"], Cin=ci, Ho=Ho, Wo=Wo, Cout=co, kh=c["k"], kw=c["k"],
                       stride=c["s"], pad=c["p"], transposed=c["tr"], **kw)
        torch.cuda.synchronize()
    finally:
        F_.FORCE_IGEMM, F_.KERNEL_TRACE = None, None
        if c["ring3"]:
            if old is None:
                del os.environ["LIC_BF16_RING"]
            else:
                os.environ["LIC_BF16_RING"] = old
    assert names == {c["kern"]}, (names, c["kern"])
    RAN[key] = names
    assert bool(torch.isfinite(out.float()).all())
    return {k: crc(v) for k, v in wrote.items()}


CASES = {}
for _k in IGEMM:
    CASES[_k] = (run_igemm, (_k,))
for _k in WGRAD:
    CASES[_k] = (run_wgrad, (_k,))
for _k in IGEMMH:
    CASES[_k] = (run_igemm_bf16, (_k,))


@pytest.fixture(scope="module")
def pinned():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tile_map_bits(pinned, case):
    fn, args = CASES[case]
    got = fn(*args)
    assert case in pinned, f"{case} is not in the fixture"
    assert got == pinned[case], {k: (got.get(k), pinned[case].get(k)) for k in set(got) | set(pinned[case])
                                 if got.get(k) != pinned[case].get(k)}


def test_every_table_row_ran(pinned, tmp_path):
    """the cases above (run here when this test is selected alone) launch every row of g_igemm_variants and
    g_wgrad_variants and every non-FUSE row of g_igemmh_variants; the rows are read off the library's kernel symbols,
    which tests/test_variant_tables.py holds equal to the tables"""
    import test_variant_tables as V
    from neural_image_compression_amd import _lib
    for case in sorted(CASES):
        if case not in RAN:
            fn, args = CASES[case]
            fn(*args)
    rows = set()
    for nm in V.library_kernels(_lib.LIB_PATH, str(tmp_path)):
        if nm.startswith(("igemm_kernel<", "wgrad_kernel<", "wgrad_glds_kernel<")):
            rows.add(nm)
        elif nm.startswith("igemm_bf16_kernel<") and nm.split(", ")[3] == "false":
            rows.add(nm)
        elif nm in ("halo_conv_bf16_kernel<2, false, 0>", "halo_convt_bf16_kernel<2, false>"):
            rows.add(nm)
    assert len(rows) >= 18 + 33 + 17 + 2, sorted(rows)   # fp32 igemm, fp32 wgrad, plain bf16 igemm, plain halo
    ran = set().union(*RAN.values())
    assert not rows - ran, "table rows no case launches:\n  " + "\n  ".join(sorted(rows - ran))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    res = {}
    for case in sorted(CASES):
        fn, args = CASES[case]
        res[case] = fn(*args)
        print(case, res[case], flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(res)} cases to {path}")
