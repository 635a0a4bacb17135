#!/usr/bin/env python3
"""Per-XCD load of every fp32 MFMA launch of the config-2 step (JAH(192), batch 32, 256 x 256; shapes as in
tools/bench_layers.py and tools/sweep_latent.py).  CPU only: nothing is launched.

The hardware deals workgroup ids round-robin over the 8 XCDs (id % 8); the kernels remap the id with xcd_contiguous() and
decode it with conv_tile() / wgrad_tile() (csrc/lic_tile_map.h).  For lic_igemm the tile of every id comes from the
library itself (lic_igemm_tile_order: the kernels' own functions run on the host); for lic_wgrad the arithmetic of
wgrad_tile is repeated here on the plan lic_wgrad_plan reports.  Work of a workgroup = the K chunks it runs (0 for a
padding tile).  Printed per launch: grid, live workgroups, per-XCD work max / mean, and rounds = the most live workgroups
on an XCD over its resident slots (32 CUs x workgroups per CU, the latter from hipcc's kernel-resource-usage report of
the LDS-DMA variants: registers and LDS, whichever binds).

usage: python tools/xcd_load.py [filter ...]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_image_compression_amd import _lib as L  # noqa: E402

B, M, NXCD, CUS_PER_XCD = 32, 192, 8, 32
P16 = 0x10000        # a 16-byte aligned stand-in address: the planners read no operand
# workgroups per CU: igemm_kernel<BM, TN, true, true, false, GLDS> and wgrad_glds_kernel<TM, TN, ., .>
IGEMM_RESIDENT = {(64, 1): 6, (64, 2): 4, (64, 3): 3, (128, 1): 4, (128, 2): 2, (128, 3): 2}
WGRAD_RESIDENT = {(1, 1): 8, (1, 3): 4, (2, 1): 6, (2, 2): 3, (2, 3): 4, (3, 3): 2}
CTX_MASK = sum(1 << (r * 5 + s) for r in range(5) for s in range(5) if r < 2 or (r == 2 and s < 2))

# name, Hi, Cin, Ho, Cout, k, stride, pad, transposed, tap_mask.  A workspace is offered to every launch, as
# functional.py does: the planner splits K where the geometry asks for it
LAYERS = [
    ("enc conv2 128->64", 128, M, 64, M, 5, 2, 2, False, 0),
    ("enc conv3 64->32", 64, M, 32, M, 5, 2, 2, False, 0),
    ("enc conv4 32->16", 32, M, 16, M, 5, 2, 2, False, 0),
    ("dec convT1 16->32", 16, M, 32, M, 5, 2, 2, True, 0),
    ("dec convT2 32->64", 32, M, 64, M, 5, 2, 2, True, 0),
    ("dec convT3 64->128", 64, M, 128, M, 5, 2, 2, True, 0),
    ("gdn 128 (1x1)", 128, M, 128, M, 1, 1, 0, False, 0),
    ("gdn 64 (1x1)", 64, M, 64, M, 1, 1, 0, False, 0),
    ("gdn 32 (1x1)", 32, M, 32, M, 1, 1, 0, False, 0),
    ("henc1 3x3", 16, M, 16, M, 3, 1, 1, False, 0),
    ("henc2 5x5s2", 16, M, 8, M, 5, 2, 2, False, 0),
    ("henc3 5x5s2", 8, M, 4, M, 5, 2, 2, False, 0),
    ("hdec1 T5x5", 4, M, 8, M, 5, 2, 2, True, 0),
    ("hdec2 T5x5", 8, M, 16, M * 3 // 2, 5, 2, 2, True, 0),
    ("hdec3 3x3", 16, M * 3 // 2, 16, 2 * M, 3, 1, 1, False, 0),
    ("ctx 5x5m", 16, M, 16, 2 * M, 5, 1, 2, False, CTX_MASK),
    ("ep1 1x1", 16, 4 * M, 16, 640, 1, 1, 0, False, 0),
    ("ep2 1x1", 16, 640, 16, 640, 1, 1, 0, False, 0),
    ("ep3 1x1", 16, 640, 16, 2 * M, 1, 1, 0, False, 0),
]
# the RGB stem / head as dense GEMMs over column matrices [B * 128 * 128][80]: name, K, N
IMAGE_GEMMS = [("stem fwd / head dx K80 N192", 80, 192), ("head fwd K192 N80", 192, 80)]


def igemm_desc(Bn, Hi, Wi, Cin, Ho, Wo, Cout, k, stride, pad, tr, mask):
    d = L.IgemmDesc()
    d.in_, d.w, d.out = P16, P16, P16
    d.in_ld, d.out_ld = Cin, Cout
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = Bn, Hi, Wi, Cin, Ho, Wo, Cout
    d.kh = d.kw = k
    d.stride, d.pad, d.transposed, d.tap_mask = stride, pad, int(tr), mask
    d.workspace, d.workspace_bytes = P16, 1 << 50
    return d


def per_xcd(n, weight):
    return np.bincount(np.arange(n) % NXCD, weights=weight, minlength=NXCD)


def report(name, kernel, nwg, work, resident):
    live = work > 0
    w, cnt = per_xcd(nwg, work), per_xcd(nwg, live.astype(float))
    ratio = w.max() / w.mean() if w.mean() > 0 else 1.0
    rounds = cnt.max() / (CUS_PER_XCD * resident)
    flag = "  <-- above 1.1" if ratio > 1.1 else ""
    print(f"{name:34s} {kernel:22s} {nwg:6d} wg {int(live.sum()):6d} live  per-XCD chunks {int(w.min()):7d}..{int(w.max()):7d}"
          f"  max/mean {ratio:5.3f}  rounds {rounds:5.2f}{flag}")


def igemm_load(name, d):
    so = L.load()
    n, taps, shape = C.c_int64(0), (C.c_int32 * 4)(), (C.c_int32 * 4)()
    L.check(so.lic_igemm_tile_order(C.byref(d), None, 0, C.byref(n), taps, shape), "lic_igemm_tile_order")
    order = np.zeros((n.value, 4), dtype=np.int32)
    L.check(so.lic_igemm_tile_order(C.byref(d), order.ctypes.data, n.value, None, None, None), "lic_igemm_tile_order")
    bn = C.c_int32(0)
    L.check(so.lic_igemm_plan(C.byref(d), None, C.byref(bn), None), "lic_igemm_plan")
    BM, S, cps, cpt = shape
    four = bool(d.transposed and d.stride == 2)
    rows = [d.B * ((d.Ho - py + 1) // 2) * ((d.Wo - px + 1) // 2) for py in (0, 1) for px in (0, 1)] if four else \
        [d.B * d.Ho * d.Wo] * 4
    ks, ph, mt = order[:, 0].astype(np.int64), order[:, 2], order[:, 3].astype(np.int64)
    live = mt * BM < np.array(rows)[ph]
    chunks = np.array(list(taps))[ph] * cpt
    work = np.clip(np.minimum(chunks, (ks + 1) * cps) - ks * cps, 0, None) * live
    report(name, f"igemm<{BM},{bn.value // 64}> x{S}", n.value, work, IGEMM_RESIDENT.get((BM, bn.value // 64), 2))


def wgrad_load(name, Bn, Hs, Ws, Cp, Hl, Wl, Cg, k, stride, pad, g_is_row):
    so = L.load()
    d = L.WgradDesc()
    d.p, d.g, d.dst = P16, P16, P16
    d.p_ld, d.g_ld = Cp, Cg
    d.B, d.Hs, d.Ws, d.Cp, d.Hl, d.Wl, d.Cg = Bn, Hs, Ws, Cp, Hl, Wl, Cg
    d.kh = d.kw = k
    d.stride, d.pad, d.g_is_row, d.scale = stride, pad, int(g_is_row), 1.0
    tm, tn, sk = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(so.lic_wgrad_plan(C.byref(d), C.byref(tm), C.byref(tn), C.byref(sk)), "lic_wgrad_plan")
    Cm, Cn = (Cg, Cp) if g_is_row else (Cp, Cg)
    tiles = -(-Cm // (64 * tm.value)) * -(-Cn // (64 * tn.value))
    ntaps, nchunks = k * k, -(-(Bn * Hs * Ws) // 16)
    cps = -(-nchunks // sk.value)
    assert -(-nchunks // cps) == sk.value
    nwg = tiles * ntaps * sk.value
    # xcd_contiguous, then wgrad_tile: tile fastest, then tap, then split
    i = np.arange(nwg)
    q, r, xcd, idx = nwg // 8, nwg % 8, i % 8, i // 8
    wg = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + idx
    split = wg // tiles // ntaps
    work = np.minimum(nchunks, (split + 1) * cps) - split * cps
    report(name, f"wgrad<{tm.value},{tn.value}> x{sk.value}", nwg, work, WGRAD_RESIDENT.get((tm.value, tn.value), 2))


def main():
    only = sys.argv[1:] or None
    for name, Hi, Cin, Ho, Cout, k, stride, pad, tr, mask in LAYERS:
        if only and not any(o in name for o in only):
            continue
        igemm_load(name + " fwd", igemm_desc(B, Hi, Hi, Cin, Ho, Ho, Cout, k, stride, pad, tr, mask))
        igemm_load(name + " dgrad", igemm_desc(B, Ho, Ho, Cout, Hi, Hi, Cin, k, stride, pad, not tr, mask))
        if tr:   # weight [Cin, Cout, k, k]: the small grid is the input
            wgrad_load(name + " wgrad", B, Hi, Hi, Cin, Ho, Ho, Cout, k, stride, pad, False)
        else:    # weight [Cout, Cin, k, k]: the small grid is the output gradient, the input is gathered
            wgrad_load(name + " wgrad", B, Ho, Ho, Cout, Hi, Hi, Cin, k, stride, pad, True)
    P = B * 128 * 128
    for name, K, N in IMAGE_GEMMS:
        if only and not any(o in name for o in only):
            continue
        igemm_load(name, igemm_desc(1, 1, P, K, 1, P, N, 1, 1, 0, False, 0))
        wgrad_load(name + " wgrad", 1, 1, P, K, 1, P, N, 1, 1, 0, False)


if __name__ == "__main__":
    main()
