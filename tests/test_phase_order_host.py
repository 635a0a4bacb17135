"""The workgroup order of lic_igemm's four-phase (transposed, stride 2) launches, read on the CPU through
lic_igemm_tile_order: the library evaluates conv_tile(xcd_contiguous(id, nwg)) -- the very inline functions the kernels
call (csrc/lic_tile_map.h) -- for every hardware workgroup id and launches nothing.

The hardware deals workgroup ids round-robin over the 8 XCDs (XCD = id % 8, arrival order id / 8) and xcd_contiguous()
hands XCD x the x-th contiguous eighth of the logical ids.  phase_order() (csrc/lic_conv_plan.h) sorts the phases of a
launch with at least 128 M tiles per phase by tap count inside groups of g M tiles.  The rule held here:

    k = ceil(MT / 512) groups per XCD,  g = ceil(MT / 8k) <= 64 tiles per group,  MT padded to 8 k g

so that every XCD's eighth is k whole groups: the same number of M tiles of every phase on every XCD.  With the parent's
fixed g = 64 an eighth was half a group at MT = 256 (enc conv3 data gradient, dec convT2 forward at batch 32: 960 tap-tiles
on the even XCDs, 640 on the odd, max / mean 1.2) and a quarter group at MT = 128 (enc conv4 data gradient, dec convT1
forward: one tap class per XCD, 9 6 6 4 9 6 6 4, max / mean 576 / 400 = 1.44).  On this tree both are 1.0."""
import ctypes as C
import os

import numpy as np
import pytest

P16 = 0x10000                     # a 16-byte aligned address that nothing reads
NXCD = 8
SORT_FROM = 128                   # M tiles per phase from which a four-phase launch is phase-sorted
TAPS = {5: [9, 6, 6, 4], 3: [1, 2, 2, 4]}     # live taps of phase 2 py + px: 5x5 pad 2, 3x3 pad 1, stride 2


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def convt_desc(L, B, Hi, Wi, Ho, Wo, cin, cout, k, tile=(0, 0), split=0):
    d = L.IgemmDesc()
    d.in_, d.w, d.out = P16, P16, P16
    d.in_ld, d.out_ld = cin, cout
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = B, Hi, Wi, cin, Ho, Wo, cout
    d.kh = d.kw = k
    d.stride, d.pad, d.transposed = 2, k // 2, 1
    d.force_bm, d.force_tn = tile
    d.force_split = split
    if split > 1:
        d.workspace, d.workspace_bytes = P16, 1 << 50
    return d


def tile_order(lib, d):
    """(order [nwg, 4] = (ks, nt, phase, mt) per hardware id, taps of the four phases, BM, ksplit, cps, cpt)"""
    so = lib.load()
    n, taps, shape = C.c_int64(-1), (C.c_int32 * 4)(), (C.c_int32 * 4)()
    assert so.lic_igemm_tile_order(C.byref(d), None, 0, C.byref(n), taps, shape) == 0
    order = np.full((max(n.value, 1), 4), -1, dtype=np.int32)
    assert so.lic_igemm_tile_order(C.byref(d), order.ctypes.data, n.value, None, None, None) == 0
    return order[:n.value], list(taps), tuple(shape)


def phase_rows(B, Ho, Wo):
    """rows of the four phase GEMMs: the pixels of the output with row parity py and column parity px"""
    return [B * ((Ho - py + 1) // 2) * ((Wo - px + 1) // 2) for py in (0, 1) for px in (0, 1)]


def group_rule(MT):
    """(groups per XCD, M tiles per group) of a phase-sorted launch of MT tiles per phase"""
    k = -(-MT // 512)
    return k, -(-MT // (NXCD * k))


def shape_for(MT, BM, parity):
    """(B, Hi, Wi, Ho, Wo) whose largest phase has exactly MT tiles of BM rows, the last one ragged where MT % 4 != 0;
    parity "ee": all phases equal, "oo" / "eo": odd Ho and Wo / odd Wo alone, so that the phases differ in Hq * Wq"""
    total = 4 * MT - (MT % 4)                       # B * Hq0 rows of Wq0 = BM / 4 pixels: (4 MT - 4, 4 MT] quarter tiles
    B = 3 if total % 3 == 0 else (2 if total % 2 == 0 else 1)
    Hq, Wq = total // B, BM // 4
    Ho = 2 * Hq - (1 if parity == "oo" else 0)
    Wo = 2 * Wq - (1 if parity in ("oo", "eo") else 0)
    assert -(-phase_rows(B, Ho, Wo)[0] // BM) == MT
    return B, Hq, Wq, Ho, Wo


def per_xcd(order, weight):
    return np.bincount(np.arange(len(order)) % NXCD, weights=weight, minlength=NXCD)


def check_launch(lib, MT, BM, NT, split, k, parity):
    B, Hi, Wi, Ho, Wo = shape_for(MT, BM, parity)
    d = convt_desc(lib, B, Hi, Wi, Ho, Wo, 16, 64 * NT, k, (BM, 1), split)
    order, taps, (bm, S, cps, cpt) = tile_order(lib, d)
    tag = (MT, BM, NT, split, k, parity)
    assert bm == BM and taps == TAPS[k] and cpt == 1, tag
    chunks = max(taps)                                                   # 3x3: 4 chunks, 5x5: 9
    assert S == (-(-chunks // -(-chunks // min(split, chunks))) if split > 1 else 1), tag      # lic.h: force_split
    P = phase_rows(B, Ho, Wo)
    MTp = np.array([-(-p // BM) for p in P])
    sorted_ = MT >= SORT_FROM
    kx, g = group_rule(MT)
    MTpad = NXCD * kx * g if sorted_ else MT
    assert g <= 64 and MTpad - MT < NXCD * kx
    nwg = len(order)
    assert nwg == MTpad * 4 * NT * S, tag
    ks, nt, ph, mt = (order[:, i].astype(np.int64) for i in range(4))
    assert ks.min() >= 0 and ks.max() < S and nt.min() >= 0 and nt.max() < NT and ph.min() >= 0 and ph.max() < 4, tag
    assert mt.min() >= 0 and mt.max() < MTpad, tag
    # ---- bijection: every live (ks, nt, phase, mt) exactly once; whatever else is there is a padding tile
    live = mt * BM < np.array(P)[ph]
    assert (mt[live] < MTp[ph[live]]).all()
    key = ((mt * 4 + ph) * NT + nt) * S + ks
    assert len(np.unique(key)) == nwg, tag                            # no tile twice, live or padding
    assert int(live.sum()) == int(MTp.sum()) * NT * S, tag            # ... so the live ones are all of them, once
    if not sorted_:
        return
    # ---- balance: the same number of M tiles of every phase on every XCD ...
    assert nwg % NXCD == 0
    tp = np.array(taps)
    for p in range(4):
        assert (per_xcd(order, (ph == p).astype(float)) == kx * g * NT * S).all(), tag
    # ... so an XCD's live work falls short of a full share only by padding tiles it holds, and no two XCDs differ by
    # more than the work of all the padding: the MTpad - MTp[phase] tiles past each phase's last row
    work = per_xcd(order, tp[ph] * live)
    bound = int((tp * (MTpad - MTp)).sum()) * NT * S
    assert work.max() - work.min() <= bound, (tag, work, bound)
    assert work.max() <= kx * g * int(tp.sum()) * NT * S
    # ---- order: inside each group, in arrival order on the XCD, tap counts do not increase
    arrivals = tp[ph].reshape(nwg // NXCD, NXCD).T                    # [xcd][idx], idx = id / 8
    groups = arrivals.reshape(NXCD, kx, 4 * g * NT * S)
    assert (np.diff(groups, axis=2) <= 0).all(), tag
    assert (groups[:, :, 0] == tp.max()).all() and (groups[:, :, -1] == tp.min()).all()


@pytest.mark.parametrize("k", [5, 3])
@pytest.mark.parametrize("BM", [64, 128])
def test_every_tile_once_balanced_and_sorted(lib, BM, k):
    """MT = 1 .. 600 per phase x NT 1 2 3 x forced split 0 2 3, phases equal ("ee") and unequal ("oo", "eo")"""
    for MT in range(1, 601):
        for parity in ("ee", "oo", "eo"):
            for NT in (1, 2, 3):
                for split in (0, 2, 3):
                    check_launch(lib, MT, BM, NT, split, k, parity)


def test_the_sweep_meets_its_edges(lib):
    """a phase without rows, a launch of padding beyond one group's eighth, both sides of the threshold"""
    assert phase_rows(*[shape_for(1, 64, "oo")[i] for i in (0, 3, 4)])[2:] == [0, 0]
    assert group_rule(128) == (1, 16) and group_rule(162) == (1, 21) and group_rule(256) == (1, 32)
    assert group_rule(512) == (1, 64) and group_rule(513) == (2, 33) and group_rule(600) == (2, 38)
    assert group_rule(1024) == (2, 64) and group_rule(1536) == (3, 64)
    for MT, sorted_ in ((127, False), (128, True)):
        order, _, _ = tile_order(lib, convt_desc(lib, *shape_for(MT, 64, "ee"), 16, 64, 5, (64, 1)))
        first_eight = order[::NXCD][:8, 2]                            # the phases XCD 0 receives first
        assert (len(set(first_eight.tolist())) == 1) == sorted_


def parent_tile(wg_id, nwg, NT, S, MT64, porder=(0, 1, 2, 3)):
    """the parent's decode, written out: xcd_contiguous, then K split fastest, N tile, and phases sorted inside groups
    of a fixed 64 M tiles (MT64 = MT rounded up to 64)"""
    q, r, xcd, idx = nwg // 8, nwg % 8, wg_id % 8, wg_id // 8
    wg = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
    ks, wg = wg % S, wg // S
    nt, kq = wg % NT, wg // NT
    grp, loc = divmod(kq, 4 * 64)
    rank = loc // 64
    return ks, nt, porder[rank], grp * 64 + (loc - rank * 64)


@pytest.mark.parametrize("MT,BM,NT,split", [(512, 64, 1, 0), (512, 128, 3, 0), (512, 64, 2, 3), (1024, 128, 1, 0),
                                            (1024, 64, 1, 2), (1536, 64, 1, 0)])
def test_launches_of_whole_groups_of_64_keep_their_order(lib, MT, BM, NT, split):
    """MT a multiple of 512 -- the 128 x 128 layers of the training step -- decodes exactly as the parent did"""
    B, Hi, Wi, Ho, Wo = shape_for(MT, BM, "ee")
    order, taps, (_, S, _, _) = tile_order(lib, convt_desc(lib, B, Hi, Wi, Ho, Wo, 16, 64 * NT, 5, (BM, 1), split))
    nwg = MT * 4 * NT * S
    assert len(order) == nwg
    want = np.array([parent_tile(i, nwg, NT, S, MT) for i in range(nwg)], dtype=np.int32)
    assert (order == want).all()
    if (MT, NT, split) == (512, 1, 0):
        # read off the parent's formula by hand: q = 256 ids per XCD, one group of 4 x 64 each
        pins = {0: (0, 0, 0, 0), 1: (0, 0, 0, 64), 8: (0, 0, 0, 1), 512: (0, 0, 1, 0), 1024: (0, 0, 2, 0),
                1543: (0, 0, 3, 448), 2047: (0, 0, 3, 511)}
        for i, t in pins.items():
            assert tuple(order[i]) == t, (i, tuple(order[i]), t)


# enc conv3 / conv4 data gradients and dec convT2 / convT1 forward of the config-2 step (JAH(192), batch 32, 256 x 256):
# transposed 5x5 stride 2, 192 -> 192 channels, on 32 x 32 -> 64 x 64 and 16 x 16 -> 32 x 32, the automatic plan
STEP_LAUNCHES = [("enc conv3 dgrad / dec convT2 fwd", 32, 64), ("enc conv4 dgrad / dec convT1 fwd", 16, 32)]


@pytest.mark.parametrize("name,hi,ho", STEP_LAUNCHES, ids=[s[0] for s in STEP_LAUNCHES])
def test_the_step_launches_are_balanced(lib, name, hi, ho):
    """per-XCD work (K chunks summed over the XCD's live workgroups): max / mean is 1.0 (the parent: 1.2 at 64 x 64,
    1.44 at 32 x 32, see the module text)"""
    d = convt_desc(lib, 32, hi, hi, ho, ho, 192, 192, 5)
    order, taps, (BM, S, cps, cpt) = tile_order(lib, d)
    assert S == 1 and cpt == 12 and taps == [9, 6, 6, 4]
    P = phase_rows(32, ho, ho)
    MT = -(-P[0] // BM)
    assert MT >= SORT_FROM and MT in (128, 256, 512) and len(order) == MT * 4       # N tile 192: NT = 1, no padding
    live = order[:, 3].astype(np.int64) * BM < np.array(P)[order[:, 2]]
    assert live.all()
    work = per_xcd(order, np.array(taps)[order[:, 2]] * cpt * live)
    print(f"{name}: BM {BM}, MT {MT}, per-XCD chunks {work.astype(int).tolist()}")
    assert work.max() / work.mean() == 1.0
