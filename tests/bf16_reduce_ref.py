"""Numpy statements of the bf16 backward contraction and reduction side (include/lic.h): the weight-gradient
contraction of lic_wgrad_bf16, the host planner behind it (wgh_plan / lic_pick_splits), and the two reductions of
lic_reduce_batch in the association order their kernels document.  Written from the header's formulas with index
arithmetic only -- no GPU, no HIP, no torch.

Also the case lists of tests/test_gpu_bf16_reductions.py, so that tests/test_bf16_reduce_ref.py can assert on the
CPU what they cover (every row of the kernel table, every ring tail, every last-split residue) and that their
integer data stays exact: operands from {-3..3} are exact in bf16, every product and every partial sum is an integer
below 2^24, fp32 accumulation is then exact in ANY order, and the comparison with the kernel is `==`."""
from __future__ import annotations

import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

SLABS, COLUMNS = 0, 1
EPI_NONE, EPI_REPARAM = 0, 1
MAX_JOBS = 32
WH_BK = 32                      # pixels per chunk of wgrad_bf16_kernel
INT_LIMIT = 2 ** 24
SCALES = (1.0, 0.5, -2.0)


def bf16_round(a):
    """fp32 -> nearest-even bf16-representable fp32 (finite values)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


# ---------------------------------------------------------------------------------------------
# the weight-gradient contraction
# ---------------------------------------------------------------------------------------------
def gather(G, d, r, s):
    """G [B, Hl, Wl, Cg] sampled at (hs*stride - pad + r, ws*stride - pad + s) -> [B, Hs, Ws, Cg], zero outside"""
    B, Hl, Wl, Cg = G.shape
    hl = np.arange(d.Hs) * d.stride - d.pad + r
    wl = np.arange(d.Ws) * d.stride - d.pad + s
    okh, okw = (hl >= 0) & (hl < Hl), (wl >= 0) & (wl < Wl)
    out = G[:, np.clip(hl, 0, Hl - 1)][:, :, np.clip(wl, 0, Wl - 1)]
    return out * (okh[:, None] & okw[None, :])[None, :, :, None]


def wgrad_ref(P, G, d, square=None, absolute=False):
    """scale * R[tap][m][n], R = sum_{b,hs,ws} row[..m] * col[..n] in float64 (exact for integer operands).
    P [B, Hs, Ws, Cp], G [B, Hl, Wl, Cg]; `d` carries the scalar fields of lic_wgrad_desc.  `square` is how sq_g
    squares (default x * x; the bf16 kernels round the square to bf16 once, which is the identity on small integers).
    absolute: |scale| * sum |row| * |col| over the same terms (the summation bound's weight)."""
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    assert P.shape == (d.B, d.Hs, d.Ws, d.Cp) and G.shape == (d.B, d.Hl, d.Wl, d.Cg)
    if d.sq_g:
        G = G * G if square is None else np.asarray(square(G), np.float64)
    if absolute:
        P, G = np.abs(P), np.abs(G)
    Ps = d.B * d.Hs * d.Ws
    Cm, Cn = (d.Cg, d.Cp) if d.g_is_row else (d.Cp, d.Cg)
    R = np.empty((d.kh * d.kw, Cm, Cn), np.float64)
    p2 = P.reshape(Ps, d.Cp)
    for r in range(d.kh):
        for s in range(d.kw):
            g2 = gather(G, d, r, s).reshape(Ps, d.Cg)
            R[r * d.kw + s] = g2.T @ p2 if d.g_is_row else p2.T @ g2
    return R * (abs(d.scale) if absolute else d.scale)


def scatter_offsets(ntaps, Cm, Cn, sm, sn, stap):
    """offsets[tap][m][n] = m * sm + n * sn + tap * stap"""
    return (np.arange(ntaps)[:, None, None] * stap + np.arange(Cm)[None, :, None] * sm +
            np.arange(Cn)[None, None, :] * sn)


# ---------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------
def pick(C):
    """widest tile (64-channel units, at most 3) that divides the channel count's 64-padding"""
    u = (C + 63) // 64
    return 3 if u % 3 == 0 else (2 if u % 2 == 0 else (1 if u == 1 else (3 if u > 4 else 2)))


def pick_splits(base, slots, max_sk):
    """fewest whole rounds of the machine whose last one is >= 90 % full"""
    best, best_eff = 1, 0.0
    max_sk = max(1, min(max_sk, 512))
    for r in range(1, 5):
        sk = (r * slots) // base
        if sk < 1:
            continue
        sk = min(sk, max_sk)
        wgs = base * sk
        eff = wgs / float(((wgs + slots - 1) // slots) * slots)
        if eff > best_eff + 0.03:
            best, best_eff = sk, eff
        if eff >= 0.9 or sk == max_sk:
            break
    return best


def plan_ref(d, detail=False):
    """(TM, TN, splitk, cps, [chunks of each split]) of lic_wgrad_bf16 for `d`"""
    Cm, Cn = (d.Cg, d.Cp) if d.g_is_row else (d.Cp, d.Cg)
    TM, TN = pick(Cm), pick(Cn)
    MTt, NTt = -(-Cm // (64 * TM)), -(-Cn // (64 * TN))
    nchunks = -(-(d.B * d.Hs * d.Ws) // WH_BK)
    base = MTt * NTt * d.kh * d.kw
    max_sk = (nchunks + 15) // 16
    slots = 256 * (2 if TM + TN >= 5 else 3)
    sk = pick_splits(base, slots, max_sk)
    cps = -(-nchunks // sk)
    splitk = -(-nchunks // cps)
    nloc = [min(nchunks, (i + 1) * cps) - i * cps for i in range(splitk)]
    if detail:
        return SimpleNamespace(TM=TM, TN=TN, splitk=splitk, cps=cps, nloc=nloc, base=base, slots=slots, max_sk=max_sk,
                               picked=sk, nchunks=nchunks)
    return TM, TN, splitk, cps, nloc


def kernel_name_ref(d):
    TM, TN = plan_ref(d)[:2]
    return f"wgrad_bf16_kernel<{TM}, {TN}, {'true' if d.sq_g else 'false'}>"


# ---------------------------------------------------------------------------------------------
# lic_reduce_batch
# ---------------------------------------------------------------------------------------------
def _reparam(v, pv, bound):
    """lic_gdn_reparam_bwd in fp32: g = v * 2 * max(p, bound), kept when p >= bound or g < 0"""
    v, pv, bound = np.asarray(v, np.float32), np.asarray(pv, np.float32), np.float32(bound)
    g = (v * np.float32(2.0)) * np.maximum(pv, bound)
    return np.where((pv >= bound) | (g < 0), g, np.float32(0.0)).astype(np.float32)


def reduce_slabs_ref(job, slabs, param=None):
    """LIC_REDUCE_SLABS in the kernels' association order, in fp32: slab z into partial sum z % 8 while full groups of
    eight remain, the rest into sum 0, then ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), times scale, epilogue.
    slabs [splitk][ntaps][Cm][Cn]; param: flat array indexed like dst.  -> (offsets, fp32 values) of the kept
    locations (m < Mvalid, n < Nvalid)."""
    slabs = np.asarray(slabs, np.float32).reshape(job.splitk, job.ntaps, job.Cm, job.Cn)
    a8 = [np.zeros(slabs.shape[1:], np.float32) for _ in range(8)]
    z = 0
    while z + 8 <= job.splitk:
        for k in range(8):
            a8[k] = a8[k] + slabs[z + k]
        z += 8
    while z < job.splitk:
        a8[0] = a8[0] + slabs[z]
        z += 1
    acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]))
    v = (acc * np.float32(job.scale)).astype(np.float32)
    Mv = job.Mvalid if 0 < job.Mvalid <= job.Cm else job.Cm
    Nv = job.Nvalid if 0 < job.Nvalid <= job.Cn else job.Cn
    m, n = np.arange(job.Cm), np.arange(job.Cn)
    mo = (m // job.mdiv) * job.sm + (m % job.mdiv) * job.smr if job.mdiv else m * job.sm
    no = (n // job.ndiv) * job.sn + (n % job.ndiv) * job.snr if job.ndiv else n * job.sn
    off = np.arange(job.ntaps)[:, None, None] * job.stap + mo[None, :, None] + no[None, None, :]
    off, v = off[:, :Mv, :Nv].reshape(-1), v[:, :Mv, :Nv].reshape(-1)
    if job.epilogue == EPI_REPARAM:
        v = _reparam(v, np.asarray(param, np.float32)[off], job.bound)
    return off.astype(np.int64), v


def reduce_columns_ref(job, parts, param=None):
    """LIC_REDUCE_COLUMNS: rows ly, ly + 16, ... summed in double per lane, the 16 lanes in order, (float)(t * scale),
    epilogue.  parts [splitk][Cn] -> (offsets = column indices, fp32 values)"""
    parts = np.asarray(parts, np.float32).reshape(job.splitk, job.Cn).astype(np.float64)
    t = np.zeros(job.Cn, np.float64)
    for ly in range(16):
        acc = np.zeros(job.Cn, np.float64)
        for y in range(ly, job.splitk, 16):
            acc = acc + parts[y]
        t = t + acc
    v = (t * np.float64(np.float32(job.scale))).astype(np.float32)
    if job.epilogue == EPI_REPARAM:
        v = _reparam(v, np.asarray(param, np.float32)[:job.Cn], job.bound)
    return np.arange(job.Cn, dtype=np.int64), v


# ---------------------------------------------------------------------------------------------
# the weight-gradient cases
# ---------------------------------------------------------------------------------------------
_WFIELDS = ("name B Hs Ws Hl Wl kh kw stride pad Cp Cg g_is_row sq_g scale p_pad g_pad offset layout data")
WgradCase = namedtuple("WgradCase", _WFIELDS)


def g1x1(B, Hs, Ws):
    return dict(B=B, Hs=Hs, Ws=Ws, Hl=Hs, Wl=Ws, k=1, stride=1, pad=0)


def px(Ps):
    """1x1 geometry of Ps pixels (B * Hs * Ws = Ps, one image row)"""
    return g1x1(1, 1, Ps)


def conv5(B, Hs, Ws, odd=False):
    """5x5 stride 2 pad 2: the large grid 2 Hs (or 2 Hs - 1: the last taps fall outside as well)"""
    return dict(B=B, Hs=Hs, Ws=Ws, Hl=2 * Hs - odd, Wl=2 * Ws - odd, k=5, stride=2, pad=2)


def conv5s1(B, Hs, Ws):
    return dict(B=B, Hs=Hs, Ws=Ws, Hl=Hs, Wl=Ws, k=5, stride=1, pad=2)


def conv3(B, Hs, Ws):
    return dict(B=B, Hs=Hs, Ws=Ws, Hl=Hs, Wl=Ws, k=3, stride=1, pad=1)


def sub2(B, Hs, Ws):
    """1x1 stride 2 pad 0: gathered without taps"""
    return dict(B=B, Hs=Hs, Ws=Ws, Hl=2 * Hs, Wl=2 * Ws, k=1, stride=2, pad=0)


def _build_wgrad_cases():
    cases = []

    def add(tag, geo, Cp, Cg, g_is_row=0, sq_g=0, p_pad=0, g_pad=0, offset=0, layout="weight", data="int"):
        odd = "o" if geo["stride"] == 2 and geo["Hl"] != 2 * geo["Hs"] else ""
        name = (f"{tag}-{geo['B']}x{geo['Hs']}x{geo['Ws']}-k{geo['k']}s{geo['stride']}{odd}-{Cp}x{Cg}"
                f"{'-grow' if g_is_row else ''}{'-sq' if sq_g else ''}-{layout}-{data}")
        assert all(c.name != name for c in cases), name
        cases.append(WgradCase(name, geo["B"], geo["Hs"], geo["Ws"], geo["Hl"], geo["Wl"], geo["k"], geo["k"],
                               geo["stride"], geo["pad"], Cp, Cg, g_is_row, sq_g, SCALES[len(cases) % 3], p_pad, g_pad,
                               offset, layout, data))

    lay = ("weight", "transpose", "gaps")
    # every row of the table through channel counts alone; 3 x 5 x 7 pixels, nothing a power of two
    full = [(cm, cn) for cm in (64, 128, 192) for cn in (64, 128, 192)]
    for i, (cm, cn) in enumerate(full):
        add("table", g1x1(3, 5, 7), cm, cn, layout=lay[i % 3], p_pad=8 * (i % 2), g_pad=16 * (i % 2), offset=i % 2)
    for c in (64, 128, 192, 72, 136):       # the squared rows (GDN d-gamma: C x C), and a ragged count each
        add("table", g1x1(3, 5, 7), c, c, sq_g=1, layout="transpose" if c == 128 else "weight",
            p_pad=8 if c == 72 else 0, g_pad=16 if c == 72 else 0)
    # channel tails: one live slot; a nearly empty second sub-tile; pick -> 2 and 3 with a ragged second tile row
    for i, (cp, cg) in enumerate(((8, 192), (72, 136), (200, 64), (320, 72), (136, 200), (8, 8), (64, 320))):
        add("tails", g1x1(3, 5, 7), cp, cg, layout=lay[i % 3], p_pad=8, g_pad=16, offset=1)
    # ring tails: unsplit launches of 1 .. 7 chunks, ragged last chunk
    for Ps in (1, 31, 32, 33, 64, 65, 97, 128, 129, 161, 193):
        add("ring", px(Ps), 64, 64)
        add("ring", px(Ps), 192, 128, layout="transpose")
    # split launches whose last split is shorter, lengths in every residue mod 3.  The planner splits only when the
    # launch then fills 3 % of the machine (lic_pick_splits): 25 taps, or 25 tiles of a 1x1 product
    for Ps in (520, 600, 1090, 2100):
        add("split", conv5s1(1, 2, Ps // 2), 64, 64)
        add("split", conv5s1(1, 2, Ps // 2), 72, 136, p_pad=8, g_pad=16, offset=1, layout="gaps")
    add("split", conv5s1(1, 2, 545), 192, 192, layout="transpose")
    add("split", px(520), 640, 640)
    add("split", px(1090), 640, 640, sq_g=1)
    # 25 taps x 4 tiles: a round of the machine holds 5 splits, fewer than the 16-chunk rule allows
    add("split", conv5(1, 52, 50), 320, 320)
    # pixel decoding (gathered operand): division by 1; one column; nothing a power of two
    for geo in (conv3(5, 1, 1), conv3(1, 7, 1), conv3(3, 5, 7)):
        for g_is_row in (0, 1):
            add("pixels", geo, 64, 128, g_is_row=g_is_row, layout=lay[g_is_row])
    # gathered operand with borders on both sides, either role
    for geo in (conv5(2, 4, 6), conv5(2, 4, 6, odd=True), conv3(2, 6, 5), sub2(2, 5, 3)):
        for g_is_row in (0, 1):
            add("gather", geo, 64, 64, g_is_row=g_is_row, layout=lay[g_is_row])
            add("gather", geo, 72, 192, g_is_row=g_is_row, p_pad=8, g_pad=16, offset=1, layout=lay[2 - g_is_row])
    add("gather", conv5(3, 9, 8, odd=True), 128, 200, g_is_row=1, g_pad=16)     # 216 pixels: 7 chunks, ragged
    # real-valued data (bf16-rounded normal deviates): one geometry per tile family, one split launch
    for cm, cn in full:
        add("real", conv3(3, 5, 7), cm, cn, data="real", g_is_row=(cm + cn) // 64 % 2)
    for c in (64, 128, 192):
        add("real", g1x1(3, 5, 7), c, c, sq_g=1, data="real")
    add("real", conv5s1(1, 2, 545), 64, 64, data="real")
    add("real", conv5(2, 9, 9, odd=True), 192, 72, data="real", p_pad=8, g_pad=16, offset=1, layout="gaps")
    return cases


WGRAD_CASES = _build_wgrad_cases()
TABLE_ROWS = tuple(f"wgrad_bf16_kernel<{tm}, {tn}, false>" for tm in (1, 2, 3) for tn in (1, 2, 3)) + \
    tuple(f"wgrad_bf16_kernel<{t}, {t}, true>" for t in (1, 2, 3))


def wgrad_layout(c):
    """(dst_sm, dst_sn, dst_stap, floats of dst) of a case: a real [Cm][Cn][kh][kw] weight, its transpose
    [Cn][Cm][kh][kw], or the weight with gaps between taps, columns and rows"""
    Cm, Cn = (c.Cg, c.Cp) if c.g_is_row else (c.Cp, c.Cg)
    kk = c.kh * c.kw
    if c.layout == "weight":
        return Cn * kk, kk, 1, Cm * Cn * kk
    if c.layout == "transpose":
        return kk, Cm * kk, 1, Cm * Cn * kk
    assert c.layout == "gaps"
    sn = 2 * kk + 1
    sm = Cn * sn + 5
    return sm, sn, 2, Cm * sm


def wgrad_fields(c):
    """the scalar fields of the lic_wgrad_desc of a case (pointers are the caller's)"""
    sm, sn, stap, _ = wgrad_layout(c)
    return SimpleNamespace(p_ld=c.Cp + c.p_pad, g_ld=c.Cg + c.g_pad, dst_sm=sm, dst_sn=sn, dst_stap=stap, B=c.B,
                           Hs=c.Hs, Ws=c.Ws, Cp=c.Cp, Hl=c.Hl, Wl=c.Wl, Cg=c.Cg, kh=c.kh, kw=c.kw, stride=c.stride,
                           pad=c.pad, g_is_row=c.g_is_row, sq_p=0, sq_g=c.sq_g, scale=c.scale, force_tm=0, force_tn=0,
                           force_split=0)


def fill_desc(desc, fields):
    """copies wgrad_fields / a job's scalar fields into a ctypes structure"""
    for k, v in vars(fields).items():
        if hasattr(desc, k) and k not in ("src", "dst", "param", "p", "g"):
            setattr(desc, k, v)
    return desc


def _values(rng, shape, data):
    if data == "int":
        return rng.randint(-3, 4, size=shape).astype(np.float32)
    return bf16_round(rng.standard_normal(shape).astype(np.float32))


def wgrad_inputs(c):
    """P [B, Hs, Ws, Cp], G [B, Hl, Wl, Cg] as fp32 arrays of bf16-exact values"""
    r = _rng(c.name)
    return _values(r, (c.B, c.Hs, c.Ws, c.Cp), c.data), _values(r, (c.B, c.Hl, c.Wl, c.Cg), c.data)


def integer_bound(c):
    """largest magnitude any partial or final sum of an integer case can reach: Ps terms of at most 3 * 3^2"""
    return c.B * c.Hs * c.Ws * 27 * abs(c.scale)


# ---------------------------------------------------------------------------------------------
# the column-sum cases: (P, C, ld - C)
# ---------------------------------------------------------------------------------------------
COLSUM_P = (1, 31, 32, 33, 255, 256, 257, 8191, 65536, 65537, 70001)
COLSUM_C = (8, 64, 72, 640)


def _build_colsum_cases():
    cases = []
    for i, P in enumerate(COLSUM_P):
        for j, C in enumerate(COLSUM_C):
            if P > 60000 and C == 640 and P != 70001:
                continue                      # the 90 MB shape once
            cases.append((P, C, 8 * ((i + j) % 2)))
    return cases


COLSUM_CASES = _build_colsum_cases()
ELEMENTWISE_N = (8, 16, 2040, 2048, 2056, 8 * 600_001)


def colsum_inputs(P, C, pad, seed=0):
    """integer [P][C + pad] matrix; the pad columns hold 3 (a kernel that sums them is wrong)"""
    r = np.random.RandomState(1000 * seed + (P * 31 + C) % 100_000)
    a = np.full((P, C + pad), 3.0, np.float32)
    a[:, :C] = r.randint(-3, 4, size=(P, C))
    return a


# ---------------------------------------------------------------------------------------------
# the lic_reduce_batch cases
# ---------------------------------------------------------------------------------------------
SLAB_SPLITS = (1, 7, 8, 9, 15, 31, 32, 33, 40, 47, 71)
COLUMN_SPLITS = (1, 15, 16, 17, 113, 128, 129, 300)
BOUND = 0.25          # a bf16- and fp32-exact bound, so `param == bound` is an exact tie


def _job(name, kind, splitk, data, ntaps=1, Cm=1, Cn=1, sm=0, smr=0, sn=0, snr=0, stap=0, Mvalid=0, Nvalid=0, mdiv=0,
         ndiv=0, scale=1.0, epilogue=EPI_NONE, bound=0.0, extent=None):
    if extent is None:
        extent = Cn if kind == COLUMNS else 1 + (ntaps - 1) * stap + (Cm - 1) * sm + (Cn - 1) * sn
    return SimpleNamespace(name=name, kind=kind, splitk=splitk, data=data, ntaps=ntaps, Cm=Cm, Cn=Cn, sm=sm, smr=smr,
                           sn=sn, snr=snr, stap=stap, Mvalid=Mvalid, Nvalid=Nvalid, mdiv=mdiv, ndiv=ndiv, scale=scale,
                           epilogue=epilogue, bound=bound, extent=extent)


def _build_reduce_cases():
    cases = []
    for i, sk in enumerate(SLAB_SPLITS):
        for data in ("int", "real"):
            # 3 x 5 x 7 = 105 and 2 x 24 x 19 = 912 elements: one ragged block, and three blocks and a ragged fourth
            nt, cm, cn = ((3, 5, 7), (2, 24, 19))[i % 2]
            cases.append(_job(f"slabs{sk}-{data}", SLABS, sk, data, nt, cm, cn, sm=cn * nt + 3, sn=nt, stap=1,
                              scale=SCALES[i % 3]))
    cases.append(_job("slabs71-big-int", SLABS, 71, "int", 2, 24, 19, sm=19 * 2, sn=2, stap=1, scale=0.5))
    for i, sk in enumerate(COLUMN_SPLITS):
        for data in ("int", "real"):
            cases.append(_job(f"columns{sk}-{data}", COLUMNS, sk, data, Cn=(40, 23)[i % 2], scale=SCALES[i % 3]))
    # rows / columns past Mvalid / Nvalid are dropped
    cases.append(_job("valid", SLABS, 9, "real", 2, 24, 19, sm=19 * 2 + 1, sn=2, stap=1, Mvalid=21, Nvalid=16, scale=-2.0))
    # the RGB layers' maps (functional_bf16.py): stem = rows (tap, c) of an 80-row column matrix to dw[co][c][tap];
    # head = columns (tap, c) to dw[ci][c][tap]; 3 channels, 25 taps, 75 live of 80
    cases.append(_job("stem-map", SLABS, 9, "real", 1, 80, 64, mdiv=3, sm=1, smr=25, sn=75, Mvalid=75, extent=64 * 75))
    cases.append(_job("stem-map-int", SLABS, 33, "int", 1, 80, 64, mdiv=3, sm=1, smr=25, sn=75, Mvalid=75,
                      extent=64 * 75))
    cases.append(_job("head-map", SLABS, 9, "real", 1, 64, 80, ndiv=3, sm=75, sn=1, snr=25, Nvalid=75, extent=64 * 75))
    cases.append(_job("head-map-int", SLABS, 15, "int", 1, 64, 80, ndiv=3, sm=75, sn=1, snr=25, Nvalid=75,
                      extent=64 * 75))
    # the GDN re-parametrisation's backward behind the reduction: gamma [C][C] and beta [C]
    for data in ("int", "real"):
        cases.append(_job(f"reparam-slabs-{data}", SLABS, 9, data, 1, 24, 24, sm=24, sn=1, epilogue=EPI_REPARAM,
                          bound=BOUND, scale=1.0 if data == "real" else 0.5))
        cases.append(_job(f"reparam-columns-{data}", COLUMNS, 17, data, Cn=40, epilogue=EPI_REPARAM, bound=BOUND,
                          scale=-2.0))
    return cases


REDUCE_CASES = _build_reduce_cases()


def reduce_inputs(job):
    """(src [splitk][ntaps * Cm * Cn] fp32, param [extent] fp32 or None).  The REPARAM parameters lie below, on and
    above the bound in turn; the summed gradients have both signs."""
    r = _rng(job.name)
    n = job.Cn if job.kind == COLUMNS else job.ntaps * job.Cm * job.Cn
    if job.data == "int":
        src = r.randint(-3, 4, size=(job.splitk, n)).astype(np.float32)
    else:
        src = (r.standard_normal((job.splitk, n)) * np.exp(r.uniform(-3, 3, size=(job.splitk, 1)))).astype(np.float32)
    param = None
    if job.epilogue == EPI_REPARAM:
        param = (np.float32(job.bound) + np.array([-0.125, 0.0, 0.5], np.float32)[np.arange(job.extent) % 3])
        param = param.astype(np.float32)
    return src, param


def reduce_ref(job, src, param=None):
    return (reduce_columns_ref if job.kind == COLUMNS else reduce_slabs_ref)(job, src, param)


def batch33():
    """33 jobs of mixed kind and very different depths: one more than a launch's table holds, in an order the depth
    sort has to permute"""
    slabs = [j for j in REDUCE_CASES if j.kind == SLABS]
    cols = [j for j in REDUCE_CASES if j.kind == COLUMNS]
    out = []
    for a, b in zip(slabs, cols):
        out += [a, b]
    out = (out + slabs[len(cols):])[:MAX_JOBS + 1]
    assert len(out) == MAX_JOBS + 1
    return out
