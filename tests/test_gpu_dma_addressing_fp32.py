"""The LDS-DMA addressing of the fp32 GEMM loops (csrc/lic_gemm.hip: the GLDS loop of igemm_kernel, wgrad_glds_kernel):
both operands reach LDS by `buffer_load ... lds` on a descriptor, a lane contributes a 32-bit byte offset, and a lane that
must read zeros is given an offset past num_records.  A kernel of this kind can go wrong only where an address or a
zero-fill decision is made, so the cases are the smallest shapes that meet every such decision: border taps, tail rows of
an M tile, channels that end inside a chunk, K splits that begin inside a tap, pixel counts that end inside a chunk, chunks
without a live pixel, clamped duplicate chunks, pitched and offset views, and a view whose last pixel lies beyond 4 GB.

Operands are integers (x in [-3, 3], w in [-2, 2], S < 2^24: conv_ref64.exact_ok), for which fp32 is exact in any order,
and the required relation is equality with float64, bit for bit.  They live in tests/guarded.py buffers: a quiet-NaN
pattern behind the pitch and around the allocation, so a lane that fetches where it should have been zero-filled poisons
the result.  The launch helpers are those of tests/test_gpu_conv_fp32.py.

The one banded statement is y of the fused conv + GDN launch: y = x * v_rsq_f32(norm) with x and norm exact; v_rsq_f32 is
good to 1 ulp (2^-23 relative) and the product rounds once (2^-24), together below 2^-22 |y|."""
import ctypes

import pytest
import torch

import conv_ref64 as R
from guarded import Guarded
from test_gpu_conv_fp32 import OK, IgemmOperands, WgradOperands, env, igemm_desc, run_igemm, run_wgrad, sync_clean, wgrad_result  # noqa: F401

pytestmark = pytest.mark.gpu

BIG_PITCH = 1 << 20          # floats between pixels of the > 4 GB views


def _name(env, fn, d):
    buf = ctypes.create_string_buffer(128)
    assert fn(ctypes.byref(d), buf, 128) == OK
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------
# lic_igemm
# ---------------------------------------------------------------------------------------------
_ic = R.ICase
IG = [
    # 5x5 stride 2 pad 2 on 9 x 9: every border tap; 2 * 5 * 5 = 50 rows, so the M tile has tail rows; Cin = 20 ends inside
    # its second chunk, behind it the pitch holds NaNs
    _ic("dma-c5s2-20-192", "conv", 5, 2, 2, 0, 2, 9, 9, 20, 192, tiles="all", in_extra=4),
    # (its mirrored launch is a four-phase transposed convolution 64 -> 192 on the 5 x 5 gradient)
    _ic("dma-c5s2-192-64", "conv", 5, 2, 2, 0, 2, 9, 9, 192, 64, tiles="all", dgrad=True),
    # the transposed twin: four phases of 9 / 6 / 6 / 4 taps on 18 x 18 outputs
    _ic("dma-t5s2-20-192", "convT", 5, 2, 2, 1, 2, 9, 9, 20, 192, tiles="all", in_extra=12),
    _ic("dma-t5s2-192-64", "convT", 5, 2, 2, 1, 2, 9, 9, 192, 64, tiles="all"),
    # ... and phase-sorted: 2 * 72 * 72 / 64 = 162 M tiles per phase (phase_order sorts from 128 on)
    _ic("dma-t5s2-pgroup", "convT", 5, 2, 2, 1, 2, 72, 72, 16, 64, tiles=[(64, 1)]),
    _ic("dma-c3-128-128", "conv", 3, 1, 1, 0, 2, 9, 9, 128, 128, tiles="all"),                 # TN 1 and 2
    _ic("dma-c3-192-192", "conv", 3, 1, 1, 0, 2, 9, 9, 192, 192, tiles="all"),                 # TN 1 and 3
    _ic("dma-m5-64-64", "conv", 5, 1, 2, 0, 2, 9, 9, 64, 64, mask=True, tiles="all"),          # tap_mask A: 12 live taps
    # K splits of 27 chunks, 3 per tap: slices of 14, 7 and 4 chunks begin inside a tap
    _ic("dma-split-48-64", "conv", 3, 1, 1, 0, 2, 9, 9, 48, 64, tiles="all", splits=R.M_SPLITS),
    _ic("dma-split-48-192", "conv", 3, 1, 1, 0, 2, 9, 9, 48, 192, tiles=[(64, 3), (128, 3)], splits=(2, 7)),
]
IGC = {c.name: c for c in IG}


def _assert_dma_kernel(env, c, ops, which, tile):
    """a forced tile of these cases is the LDS-DMA instantiation: igemm_kernel<BM, TN, true, true, false, true>"""
    F_, L, lib, dev = env
    d = igemm_desc(env, c, ops, which, tile, 0, Guarded(1, 4, dev))
    nm = _name(env, lib.lic_igemm_kernel_name, d)
    assert nm == f"igemm_kernel<{tile[0]}, {tile[1]}, true, true, false, true>", (c, which, tile, nm)


def _igemm_all(env, c, ops, inp):
    ref = R.igemm_reference(c, inp)
    dref = R.igemm_reference(c, inp, "dgrad") if c.dgrad else None
    assert R.exact_ok(ref["S"]) and (dref is None or R.exact_ok(dref["S"]))
    bad = []
    for which, tile, split in c.launches():
        if tile != (0, 0):
            _assert_dma_kernel(env, c, ops, which, tile)
        out, _, _ = run_igemm(env, c, ops, which, tile, split)
        want = ref if which == "fwd" else dref
        if not R.same_bits(out, want["out"]):
            bad.append((which, tile, split, int((out.double() != want["out"]).sum())))
    print(f"DMA {c.name}: {len(c.launches())} launches, {len(bad)} differ")
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in IG])
def test_igemm_dma_exact(env, name):
    c = IGC[name]
    inp = R.igemm_inputs(c, True)
    _igemm_all(env, c, IgemmOperands(env, c, inp), inp)


def test_igemm_dma_1x1_on_a_pitched_offset_view(env):
    """in_ld = Cin + 64 and the view begins 32 floats into its rows: NaNs on both sides of every pixel"""
    F_, L, lib, dev = env
    for cin, cout in ((192, 192), (20, 64)):
        c = _ic(f"dma-c1-view-{cin}", "conv", 1, 1, 0, 0, 2, 9, 9, cin, cout, tiles="all", in_extra=64)
        inp = R.igemm_inputs(c, True)
        ops = IgemmOperands(env, c, inp)
        ops.x = Guarded.holding(inp["x"].reshape(-1, cin), dev, ld=cin + 64, col0=32)
        _igemm_all(env, c, ops, inp)


def test_igemm_dma_fused_conv_gdn(env):
    """LIC_EPI_CONV_GDN at Cout = 192 (igemm_kernel<64, 3, true, true, true, true>): the convolution output (out3) and the
    pool (out2) are integers and exact; y within 2^-22 |y| (see the module text)"""
    F_, L, lib, dev = env
    C = 192
    c = _ic("dma-fuse-16-192", "conv", 3, 1, 1, 0, 2, 9, 9, 16, C, in_extra=8)
    inp = R.igemm_inputs(c, True)
    x, w = inp["x"].clamp(-1, 1), inp["w"].clamp(-1, 1)              # |conv + bias| <= 148, pool < 192 * 148^2 < 2^24
    g_ = torch.Generator().manual_seed(77)
    gamma = torch.randint(0, 2, (C, C), generator=g_).float()
    beta = torch.randint(1, 5, (C,), generator=g_).float()
    v, _ = R.igemm(x, R.logical_weight(w, "conv", False), c.geom(), inp["b"])
    norm = beta.double() + torch.einsum("ij,bhwj->bhwi", gamma.double(), v * v)
    assert float(norm.max()) < R.EXACT_LIMIT
    yref = v / norm.sqrt()
    npix = c.B * c.Ho * c.Wo
    xg = Guarded.holding(x.reshape(-1, c.cin), dev, ld=c.cin + c.in_extra)
    wd = w.to(dev).contiguous()
    wp = F_._pack(wd, *R.pack_strides("conv", False, c.cin, C, 9))
    gT = F_._pack(gamma.to(dev).contiguous(), 1, C, C, 0, 1, C)
    y, nrm, cv = Guarded(npix, C, dev), Guarded(npix, C, dev), Guarded(npix, C, dev)
    bias_d, beta_d = inp["b"].to(dev), beta.to(dev)        # (held: the descriptor keeps addresses only)
    d = F_._igemm_desc(xg.t, wp, y.t, c.B, c.H, c.W, c.cin, c.Ho, c.Wo, C, 3, 3, 1, 1, False, bias_d, 0,
                       L.EPI_CONV_GDN, 0.0, 0, nrm.t, gT, beta_d, None, cv.t, None, None, c.cin + c.in_extra)
    assert _name(env, lib.lic_igemm_kernel_name, d) == "igemm_kernel<64, 3, true, true, true, true>"
    got = []
    for _ in range(2):
        assert lib.lic_igemm(ctypes.byref(d), F_._stream()) == OK
        sync_clean(lib)
        for o in (y, nrm, cv, xg):
            o.check("fused conv + GDN")
        got.append((y.cpu(), nrm.cpu(), cv.cpu()))
    shape = (c.B, c.Ho, c.Wo, C)
    assert R.same_bits(got[0][2].reshape(shape), v), "out3: the convolution output"
    assert R.same_bits(got[0][1].reshape(shape), norm), "out2: the pool"
    err = (got[0][0].reshape(shape).double() - yref).abs()
    print(f"FUSED worst |y - ref| / |ref| = {float((err / yref.abs().clamp_min(1e-30)).max()):.3e}")
    assert bool((err <= 2.0 ** -22 * yref.abs()).all())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[0], got[1])), "second launch"


# ---------------------------------------------------------------------------------------------
# lic_wgrad
# ---------------------------------------------------------------------------------------------
# (TM, TN) -> (Cm, Cn) that fill the tile, (Cm, Cn) that do not (None: the 192 x 192 tile is for multiples of 192 only)
WG_TILES = {
    (1, 1): ((64, 64), (80, 64)),
    (1, 3): ((64, 192), (80, 288)),
    (2, 1): ((128, 64), (192, 80)),
    (2, 2): ((128, 128), (192, 80)),
    (2, 3): ((128, 192), (288, 288)),
    (3, 3): ((192, 192), None),
}
WG_PIXELS = ((1, 1, 1), (1, 3, 5), (1, 1, 17), (2, 9, 9))     # Ps = 1, 15, 17, 162: (B, Hs, Ws)
WG_SPLITS = (1, 2, 3, 7)


def _wcase(tile, Cm, Cn, B, Hs, Ws, stride, g_is_row, sq_g=0):
    Cg, Cp = (Cm, Cn) if g_is_row else (Cn, Cm)
    name = f"dma-w{tile[0]}{tile[1]}-{Cm}x{Cn}-{B}x{Hs}x{Ws}-s{stride}-{'row' if g_is_row else 'col'}{'-sq' if sq_g else ''}"
    # 3x3, pad 1: tap (0, 0) of pixel (0, 0) is padding -- with Ps = 1 a chunk without a live pixel
    return R.WCase(name, B, Hs, Ws, Cp, Hs * stride, Ws * stride, Cg, 3, stride, 1, g_is_row, sq_g=sq_g, tile=tile,
                   splits=WG_SPLITS, layout="dense")


def _wgrad_all(env, c, want_kernel, splits=None):
    F_, L, lib, dev = env
    inp = R.wgrad_inputs(c, True)
    ref = R.wgrad_reference(c, inp)
    assert R.exact_ok(ref["S"])
    ops = WgradOperands(env, c, inp)
    d = R.fill_wgrad_desc(L.WgradDesc(), c, 1, {"p": ops.P.ptr(), "g": ops.G.ptr(), "dst": ops.P.ptr()})
    nm = _name(env, lib.lic_wgrad_kernel_name, d)
    assert nm == want_kernel, (c, nm)
    bad = []
    for split in (splits or c.splits):
        dst, _, rc = run_wgrad(env, c, ops, split)
        assert rc == OK
        got, touched = wgrad_result(c, dst)
        if touched or not R.same_bits(got, ref["R"]):
            bad.append((c.name, split, touched, int((got.double() != ref["R"]).sum())))
    return bad


@pytest.mark.parametrize("tile,full", [(t, f) for t in WG_TILES for f in (True, False) if WG_TILES[t][0 if f else 1]],
                         ids=lambda v: ("full" if v else "ragged") if isinstance(v, bool) else f"{v[0]}{v[1]}")
def test_wgrad_dma_exact(env, tile, full):
    """every forced (TM, TN) of wgrad_glds_kernel, whole and ragged tiles: pixel counts 1 / 15 / 17 / 162 (a partial last
    chunk; with 3x3 taps on one pixel, chunks without a live pixel), splits 1 / 2 / 3 / 7 (the prefetch past a split's end
    is a clamped duplicate), the gathered operand on either side, stride 1 and 2"""
    dims = WG_TILES[tile][0 if full else 1]
    want = f"wgrad_glds_kernel<{tile[0]}, {tile[1]}, false, {'true' if full else 'false'}>"
    bad, n = [], 0
    for (B, Hs, Ws) in WG_PIXELS:
        for stride in (1, 2):
            for g_is_row in (1, 0):
                c = _wcase(tile, dims[0], dims[1], B, Hs, Ws, stride, g_is_row)
                bad += _wgrad_all(env, c, want)
                n += len(c.splits)
    print(f"DMA wgrad {tile} {'full' if full else 'ragged'}: {n} launches, {len(bad)} differ")
    assert not bad, bad


def test_wgrad_dma_squared_column(env):
    """SQB: the column operand squared at the fragment read, here the gathered one"""
    c = _wcase((2, 3), 128, 192, 2, 9, 9, 2, 0, sq_g=1)
    assert not _wgrad_all(env, c, "wgrad_glds_kernel<2, 3, true, true>")
    c = _wcase((1, 1), 80, 64, 1, 1, 17, 1, 0, sq_g=1)
    assert not _wgrad_all(env, c, "wgrad_glds_kernel<1, 1, true, false>")


def test_wgrad_dma_both_operands_linear(env):
    """1x1, stride 1, same grids: neither operand is gathered (the GDN d-gamma and RGB launches); pitched operands"""
    for tile, (Cp, Cg) in (((1, 1), (64, 64)), ((2, 3), (128, 192)), ((3, 3), (192, 192))):
        for pixels in (1, 15, 17, 162):
            c = R.WCase(f"dma-dense-{tile[0]}{tile[1]}-{pixels}", 1, 1, pixels, Cp, 1, pixels, Cg, 1, 1, 0, 0, tile=tile,
                        splits=WG_SPLITS, p_extra=8, g_extra=68)
            assert not _wgrad_all(env, c, f"wgrad_glds_kernel<{tile[0]}, {tile[1]}, false, true>")


# ---------------------------------------------------------------------------------------------
# offsets beyond 32 bits: B = 2, 24 x 24 pixels, 16 channels, a pixel pitch of 2^20 floats -- the last pixel lies 4.8 GB from
# the base.  The view is allocated with torch.empty and only the pixels' own 64 bytes are written.
# ---------------------------------------------------------------------------------------------
class Pitched:
    """[rows][C] fp32 view with a pitch of BIG_PITCH floats (the interface of a Guarded operand; nothing to check)"""

    def __init__(self, src, dev):
        rows, C = src.shape
        try:
            self.buf = torch.empty(((rows - 1) * BIG_PITCH + C,), dtype=torch.float32, device=dev)
        except RuntimeError as e:     # (torch.OutOfMemoryError is one)
            pytest.skip(f"cannot allocate the {4 * rows * BIG_PITCH / 2 ** 30:.1f} GiB view: {e}")
        self.t = self.buf.as_strided((rows, C), (BIG_PITCH, 1))
        self.t.copy_(src)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        pass


def test_igemm_dma_beyond_4_gigabytes(env):
    F_, L, lib, dev = env
    c = _ic("dma-big-pitch-16-64", "conv", 3, 1, 1, 0, 2, 24, 24, 16, 64, tiles="all", in_extra=BIG_PITCH - 16)
    inp = R.igemm_inputs(c, True)
    ops = IgemmOperands.__new__(IgemmOperands)
    ops.c, ops.x = c, Pitched(inp["x"].reshape(-1, c.cin), dev)
    ops.w = inp["w"].to(dev).contiguous()
    ops.wp = F_._pack(ops.w, *R.pack_strides(c.kind, False, c.cin, c.cout, 9))
    ops.wp_d, ops.b, ops.dy, ops.res, ops.aux = None, inp["b"].to(dev), None, None, None
    assert (c.B * c.H * c.W - 1) * BIG_PITCH * 4 > 2 ** 32
    _igemm_all(env, c, ops, inp)


@pytest.mark.parametrize("which", ["gathered", "linear"])
def test_wgrad_dma_beyond_4_gigabytes(env, which):
    """the gathered operand (3x3, pad 1, on the row side), then the linear one, behind the 2^20-float pitch"""
    F_, L, lib, dev = env
    big_g = which == "gathered"
    c = R.WCase(f"dma-big-pitch-w-{which}", 2, 24, 24, 16, 24, 24, 16, 3, 1, 1, 1, tile=(1, 1), splits=(1, 7),
                g_extra=BIG_PITCH - 16 if big_g else 0, p_extra=0 if big_g else BIG_PITCH - 16)
    inp = R.wgrad_inputs(c, True)
    ref = R.wgrad_reference(c, inp)
    assert R.exact_ok(ref["S"])
    ops = WgradOperands.__new__(WgradOperands)
    P2, G2 = inp["P"].reshape(-1, 16), inp["G"].reshape(-1, 16)
    ops.P = Guarded.holding(P2, dev) if big_g else Pitched(P2, dev)
    ops.G = Pitched(G2, dev) if big_g else Guarded.holding(G2, dev)
    d = R.fill_wgrad_desc(L.WgradDesc(), c, 1, {"p": ops.P.ptr(), "g": ops.G.ptr(), "dst": ops.P.ptr()})
    assert _name(env, lib.lic_wgrad_kernel_name, d) == "wgrad_glds_kernel<1, 1, false, false>"
    for split in c.splits:
        dst, _, rc = run_wgrad(env, c, ops, split)
        assert rc == OK
        got, touched = wgrad_result(c, dst)
        assert not touched and R.same_bits(got, ref["R"]), (which, split, int((got.double() != ref["R"]).sum()))


# ---------------------------------------------------------------------------------------------
# stated equality: the same launches give the same bits a second time
# ---------------------------------------------------------------------------------------------
def test_a_second_launch_gives_the_same_bits(env):
    c = IGC["dma-c5s2-20-192"]
    inp = R.igemm_inputs(c, False)
    ops = IgemmOperands(env, c, inp)
    for tile in ((64, 3), (128, 3)):
        a, _, _ = run_igemm(env, c, ops, "fwd", tile, 0)
        b, _, _ = run_igemm(env, c, ops, "fwd", tile, 0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tile
    for tile, dims in (((2, 3), (288, 288)), ((3, 3), (192, 192))):
        w = _wcase(tile, dims[0], dims[1], 2, 9, 9, 2, 1)
        wops = WgradOperands(env, w, R.wgrad_inputs(w, False))
        for split in (1, 3):
            a, _, rc = run_wgrad(env, w, wops, split)
            b, _, rc2 = run_wgrad(env, w, wops, split)
            assert rc == OK and rc2 == OK
            assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), (tile, split)
