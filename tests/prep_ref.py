"""The buffers of lic_prep_run (csrc/lic_prep.hip) stated in numpy from include/lic.h's words, and the case table of
tests/test_gpu_prep_layouts.py.  CPU only; imports gdn_bf16_ref (round-to-nearest-even to bf16 in integer arithmetic)
and no product code.  tests/test_prep_ref.py checks this file.

Every layout is a FORWARD map: logical element (tap, k, n) -> its index in the packed buffer; every other slot of the
buffer is +0.0.  The words of include/lic.h this file restates:

  fp32   [tap][ceil(K/16)][npad/32][2][64][4], npad = 32 if N <= 32 else ceil64(N): element (k, n) of a chunk sits at
         lane (n%32) + 32*((k%16)/8), load q = (k%8)/4, float k%4.
  bf16   [tap][ceil(K/32)][ceil64(N)/32][2][64 lanes][8]: a chunk holds two k-steps of 16; slot (h = 0..1, e = 0..7) of
         a group of 16, at lane (n%32) + 32*h, holds k = 8*h + e.
  kperm  ... holds k = 8*(e/4) + 4*h + e%4 instead.
  stem   the bf16 layout with taps = 1 of the [80][N] matrix whose row 16*r + 3*s + c is w[n][c][r][s] of a [N][3][5][5]
         weight (slot 15 of every 16 is zero; K = 80 is padded to 96, so is "row 5").
  job    element (tap, k, n) = value(src[tap*s_tap + koff(k) + noff(n)]), koff(k) = kdiv ? (k/kdiv)*s_kq + (k%kdiv)*s_kr
         : k*s_kq (same for n); value(v) = v * mask, then transform 1 = max(v, bound)^2 - pedestal;
         MAP: dst[i] = value(src[i]); MASK_INPLACE: src[i] *= mask[i].

All results are BIT PATTERNS (uint32 / uint16): -0.0 (a masked negative weight) and +0.0 (padding) are different."""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from gdn_bf16_ref import rne_bf16

PACK_F32, PACK_BF16, MAP, MASK_INPLACE, PACK_BF16_KPERM, PACK_BF16_STEM = range(6)   # enum lic_prep_kind
HALF_KINDS = (PACK_BF16, PACK_BF16_KPERM, PACK_BF16_STEM)
PACK_KINDS = (PACK_F32,) + HALF_KINDS
MAP_BLOCK = 2048          # elements per block of the MAP / MASK_INPLACE kinds
POISON16 = 0x7FC1         # a NaN as bf16, and 0x7FC17FC1 a NaN as fp32: what every destination holds before a launch


def _ceil(a, b):
    return (a + b - 1) // b


def npad_f32(N):
    return 32 if N <= 32 else _ceil(N, 64) * 64


def npad_bf16(N):
    return _ceil(N, 64) * 64


def packed_elems(kind, taps, K, N):
    if kind == PACK_F32:
        return taps * _ceil(K, 16) * npad_f32(N) * 16
    return taps * _ceil(K, 32) * npad_bf16(N) * 32


def _grid(taps, K, N):
    return np.ogrid[0:taps, 0:K, 0:N]


def dest_f32(taps, K, N):
    """int64 [taps][K][N]: index of (tap, k, n) in the fp32 packed buffer"""
    tap, k, n = _grid(taps, K, N)
    cpt, ntile = _ceil(K, 16), npad_f32(N) // 32
    lane = n % 32 + 32 * ((k % 16) // 8)
    q = (k % 8) // 4
    return (((((tap * cpt + k // 16) * ntile + n // 32) * 2 + q) * 64 + lane) * 4 + k % 4).astype(np.int64)


def dest_bf16(taps, K, N, kperm=False):
    """int64 [taps][K][N]: index of (tap, k, n) in the bf16 packed buffer, plain or kperm K order"""
    tap, k, n = _grid(taps, K, N)
    cpt, ntile = _ceil(K, 32), npad_bf16(N) // 32
    kstep, g = (k % 32) // 16, k % 16
    if kperm:     # slot (h, e) holds 8*(e/4) + 4*h + e%4: e/4 = g/8, h = (g%8)/4, e%4 = g%4
        h, e = (g % 8) // 4, 4 * (g // 8) + g % 4
    else:         # slot (h, e) holds 8*h + e
        h, e = g // 8, g % 8
    lane = n % 32 + 32 * h
    return (((((tap * cpt + k // 32) * ntile + n // 32) * 2 + kstep) * 64 + lane) * 8 + e).astype(np.int64)


def dest(kind, taps, K, N):
    return dest_f32(taps, K, N) if kind == PACK_F32 else dest_bf16(taps, K, N, kperm=kind == PACK_BF16_KPERM)


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(a):
    """uint16 bf16 patterns of fp32 values: round to nearest, ties to even, on the bit pattern (gdn_bf16_ref.rne_bf16;
    fp32 -> float64 is exact, so this rounds the fp32 value once)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    r = rne_bf16(torch.from_numpy(a.astype(np.float64))).numpy().astype(np.float32)   # exact: r is bf16-representable
    bits = r.view(np.uint32)
    assert not (bits & 0xFFFF).any()
    return (bits >> 16).astype(np.uint16)


def pack(kind, vals):
    """fp32 [taps][K][N] -> the packed buffer's bit patterns (uint32 for PACK_F32, else uint16), padding +0.0"""
    taps, K, N = vals.shape
    idx = dest(kind, taps, K, N)
    if kind == PACK_F32:
        out = np.zeros(packed_elems(kind, taps, K, N), np.uint32)
        out[idx.reshape(-1)] = f32_bits(vals).reshape(-1)
    else:
        out = np.zeros(packed_elems(kind, taps, K, N), np.uint16)
        out[idx.reshape(-1)] = bf16_bits(vals).reshape(-1)
    return out


def unpack(kind, packed, taps, K, N):
    """the [taps][K][N] bit patterns a packed buffer holds"""
    return np.asarray(packed)[dest(kind, taps, K, N)]


def stem_logical(w):
    """[N][3][5][5] -> fp32 [1][80][N]: row 16*r + 3*s + c = w[n][c][r][s], every other row zero"""
    N = w.shape[0]
    assert w.shape == (N, 3, 5, 5)
    out = np.zeros((1, 80, N), np.float32)
    for r in range(5):
        for s in range(5):
            for c in range(3):
                out[0, 16 * r + 3 * s + c, :] = w[:, c, r, s]
    return out


# ---------------------------------------------------------------------------------------------
# job semantics
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    """one lic_prep_job: `src` / `mask` name buffers of the source arena, `off` is an element offset into `src`"""
    name: str
    kind: int
    src: str
    off: int = 0
    taps: int = 1
    K: int = 1
    N: int = 1
    s_tap: int = 0
    s_kq: int = 0
    s_kr: int = 0
    s_nq: int = 0
    s_nr: int = 0
    kdiv: int = 0
    ndiv: int = 0
    mask: Optional[str] = None
    transform: int = 0
    bound: float = 0.0
    pedestal: float = 0.0
    expect: Optional[Tuple[int, int]] = None    # (tiled, v4) the planner must derive, where the issue's probe states it

    @property
    def half(self):
        return self.kind in HALF_KINDS

    def dst_bytes(self):
        if self.kind == MASK_INPLACE:
            return 0
        if self.kind == MAP:
            return 4 * self.N
        K = 80 if self.kind == PACK_BF16_STEM else self.K
        return packed_elems(self.kind, self.taps, K, self.N) * (2 if self.half else 4)


def _split(i, div, sq, sr):
    return (i // div) * sq + (i % div) * sr if div > 0 else i * sq


def src_offsets(c: Case):
    """int64 [taps][K][N]: tap*s_tap + koff(k) + noff(n), relative to the job's src pointer"""
    tap, k, n = _grid(c.taps, c.K, c.N)
    return (tap * c.s_tap + _split(k, c.kdiv, c.s_kq, c.s_kr) + _split(n, c.ndiv, c.s_nq, c.s_nr)).astype(np.int64)


def masked(src, mask):
    """value before the transform: v * mask in fp32 (one IEEE multiply: the same float on any machine)"""
    src = np.ascontiguousarray(src, np.float32)
    return src if mask is None else (src * np.ascontiguousarray(mask, np.float32)).astype(np.float32)


def _round_diff32(a, b):
    """fp32(a - b) for float64 a, b, rounded ONCE: where the float64 difference is inexact and sits on an fp32 tie, it is
    moved one float64 ulp towards the lost remainder first (a sticky bit), so the second rounding cannot tie wrongly"""
    d = a - b
    bb = d - a
    err = (a - (d - bb)) + (-b - bb)                       # two-sum: a - b = d + err exactly
    tie = (d.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)
    up = np.nextafter(d, np.where(err > 0, np.inf, -np.inf))
    d = np.where(tie & (err != 0), up, d)
    return d.astype(np.float32)


def reparam_candidates(v, bound, pedestal):
    """max(v, bound)^2 - pedestal in fp32, both ways a compiler may emit it: (fused, unfused) = (one rounding of the exact
    value as v_fma does, the product rounded to fp32 first).  v*v is exact in float64 (24 x 24 significant bits)."""
    v = np.ascontiguousarray(v, np.float32)
    m = np.maximum(v, np.float32(bound)).astype(np.float64)
    ped = np.full_like(m, np.float64(np.float32(pedestal)))
    p = m * m
    return _round_diff32(p, ped), _round_diff32(p.astype(np.float32).astype(np.float64), ped)


def gather(c: Case, flat):
    """fp32 [taps][K][N] of a job from the flat VALUE array of its source (value() already applied element-wise;
    `flat` starts at the buffer's first element, c.off is added here)"""
    if c.kind == PACK_BF16_STEM:
        return stem_logical(np.asarray(flat)[c.off:c.off + c.N * 75].reshape(c.N, 3, 5, 5))
    return np.asarray(flat)[src_offsets(c) + c.off]


def expected(c: Case, flat):
    """bit patterns of the job's destination, given the flat value array of its source (see gather)"""
    if c.kind == MAP:
        return f32_bits(np.asarray(flat)[c.off:c.off + c.N])
    assert c.kind in PACK_KINDS
    return pack(c.kind, gather(c, flat))


# ---------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_prep_layouts.py (planned on the host by tests/test_prep_ref.py)
# ---------------------------------------------------------------------------------------------
# weight [d0][d1][kh][kw] -> ((tiled, v4) of the fp32 forward, dgrad), the same for bf16 where the probe of the planner
# recorded it: stated for a non-transposed weight, a convT weight swaps the pair
CONV_ROWS = [
    ((64, 32, 3, 3), ((1, 1), (2, 1)), ((1, 1), (2, 1))),
    ((24, 32, 3, 3), ((1, 1), (2, 0)), None),              # fp32 forward: npad 32 > N 24, whole zero-filled blocks
    ((24, 16, 3, 3), ((1, 1), (2, 0)), ((1, 0), (2, 0))),
    ((33, 20, 3, 3), ((1, 0), (2, 0)), None),              # npad 64
    ((40, 40, 5, 5), ((1, 0), (2, 0)), None),              # K > 16 with a partial last chunk
    ((100, 100, 5, 5), ((1, 0), (2, 0)), None),
    ((64, 64, 2, 2), ((1, 1), (2, 1)), None),
    ((8, 8, 4, 7), ((1, 0), (2, 0)), None),                # taps = 28, the most the tiled packer stages
    ((8, 8, 5, 6), ((0, 0), (0, 0)), None),                # taps = 30: element-wise
    ((16, 16, 1, 3), ((0, 0), (0, 0)), None),
    ((72, 48, 1, 1), ((0, 0), (0, 0)), None),
    # not in the probe: the transpose of the second row, so that the s_n == taps packer zero-fills whole blocks too
    ((32, 24, 3, 3), ((1, 0), (2, 1)), ((1, 0), (2, 1))),
]
OFFSET_ROW = ((64, 32, 3, 3), ((1, 0), None), None)        # the same weight 4 bytes off 16-byte alignment
GAMMA_C = (8, 40, 64, 100)
RGB_C = (24, 40, 64)
STEM16_N = (24, 64, 100)
EDGE_N = (1, 2047, 2048, 2049, 4097)                       # around the 2048-element block of MAP / MASK_INPLACE
# (bound, pedestal): compressai's gamma and beta pairs, and one whose pedestal is no power of two (v*v - pedestal then
# differs between the fused and the unfused form for many elements)
REPARAMS = ((2.0 ** -18, 2.0 ** -36), (float(np.float32(np.sqrt(1e-6 + 2.0 ** -36))), 2.0 ** -36), (0.3, 0.1))


def _rng(name):
    return np.random.default_rng([ord(ch) for ch in name])


def _planted(n, r):
    """fp32 normals with planted bf16 rounding ties (even and odd lower neighbour, both signs) and large magnitudes"""
    a = r.standard_normal(n).astype(np.float32)
    hi = np.array([0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4012, 0x4013, 0xC2FE, 0xC2FF, 0x3A00, 0x3A01], np.uint32)
    ties = ((hi << 16) | 0x8000).view(np.float32)
    near = np.concatenate([np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    big = np.array([1e30, -1e30, 1e38, -1e38, 3e-38, -3e-38, 65504.0, -2.0 ** 100], np.float32)
    special = np.concatenate([ties, near, big])
    if n >= 4 * special.size:
        pos = r.choice(n, special.size, replace=False)
        a[pos] = special
    elif n >= 2:
        a[0], a[n - 1] = ties[1], ties[2]
    return a


def _conv_jobs(name, kind, src, off, shape, transposed, mask=None, expect=(None, None)):
    """the forward and dgrad jobs of a conv / convT weight, as prep.py fills them"""
    d0, d1, kh, kw = shape
    taps = kh * kw
    cin, cout = (d0, d1) if transposed else (d1, d0)
    s_ci, s_co = (d1 * taps, taps) if transposed else (taps, d1 * taps)
    return [Case(f"{name}.fwd", kind, src, off, taps=taps, K=cin, N=cout, s_tap=1, s_kq=s_ci, s_nq=s_co, mask=mask,
                 expect=expect[0]),
            Case(f"{name}.dgrad", kind, src, off, taps=taps, K=cout, N=cin, s_tap=1, s_kq=s_co, s_nq=s_ci, mask=mask,
                 expect=expect[1])]


def build_table():
    """(cases, sources): the job list in launch order and name -> flat fp32 array of every source / mask buffer.
    Deterministic; a MASK_INPLACE case's source is changed by the launch, every other source is not."""
    cases, sources = [], {}

    def src(name, n):
        sources[name] = _planted(n, _rng(name))
        return name

    def mask01(name, n):
        sources[name] = (_rng(name).random(n) < 0.6).astype(np.float32)
        return name

    kn = {PACK_F32: "f32", PACK_BF16: "bf16", PACK_BF16_KPERM: "kperm"}
    # 1. conv / convT weights, forward and dgrad, fp32 and bf16
    for shape, e32, e16 in CONV_ROWS + [OFFSET_ROW]:
        off = 1 if (shape, e32, e16) == OFFSET_ROW else 0
        tag = "x".join(map(str, shape)) + ("+4B" if off else "")
        s = src(f"w{tag}", off + int(np.prod(shape)))
        for kind, e in ((PACK_F32, e32), (PACK_BF16, e16)):
            e = e or (None, None)
            cases += _conv_jobs(f"conv{tag}.{kn[kind]}", kind, s, off, shape, False, expect=e)
            cases += _conv_jobs(f"convT{tag}.{kn[kind]}", kind, s, off, shape, True, expect=(e[1], e[0]))
    # 2. a padded pitch: [N = 64][K = 32][9] rows s_n = K*taps + 1 apart (v4 is lost to the pitch alone), and the
    #    transposed view of it, whose K pitch is the odd one
    K, N, taps = 32, 64, 9
    s = src("pitch", N * (K * taps + 1))
    for kind in (PACK_F32, PACK_BF16):
        cases.append(Case(f"pitch.runk.{kn[kind]}", kind, s, taps=taps, K=K, N=N, s_tap=1, s_kq=taps, s_nq=K * taps + 1))
        cases.append(Case(f"pitch.runn.{kn[kind]}", kind, s, taps=taps, K=N, N=K, s_tap=1, s_kq=K * taps + 1, s_nq=taps))
    # 3. s_tap != 1: a [taps][K][N] source
    taps, K, N = 9, 20, 40
    s = src("tapmajor", taps * K * N)
    for kind in (PACK_F32, PACK_BF16, PACK_BF16_KPERM):
        cases.append(Case(f"tapmajor.{kn[kind]}", kind, s, taps=taps, K=K, N=N, s_tap=K * N, s_kq=N, s_nq=1))
    # 4. GDN: beta_eff (MAP) and the gamma panels in both orientations, values on both sides of the bound
    for i, C in enumerate(GAMMA_C):
        bound, ped = REPARAMS[(0, 2, 2, 0)[i]]
        name = f"gamma{C}"
        r = _rng(name)
        g = (bound + (0.2 if bound > 0.1 else 1e-3) * r.standard_normal(C * C)).astype(np.float32)
        g[r.choice(C * C, max(1, C // 4), replace=False)] = np.float32(bound)      # exactly on it
        sources[name] = g
        kw = dict(K=C, N=C, transform=1, bound=bound, pedestal=ped)
        for kind in (PACK_F32, PACK_BF16, PACK_BF16_KPERM):
            cases.append(Case(f"{name}.gT.{kn[kind]}", kind, name, s_kq=1, s_nq=C, **kw))
            cases.append(Case(f"{name}.g.{kn[kind]}", kind, name, s_kq=C, s_nq=1, **kw))
    # 5. the RGB stem and head column matrices (split indices), with and without a 0/1 mask
    for C in RGB_C:
        s = src(f"rgb{C}", C * 75)
        m = mask01(f"rgbmask{C}", C * 75)
        for mk, mt in ((None, ""), (m, ".masked")):
            for kind in (PACK_F32, PACK_BF16):
                t = f"{C}{mt}.{kn[kind]}"
                # conv weight [Cout = C][3][5][5]: K = 25*3 rows k = 3*tap + colour
                cases.append(Case(f"stem{t}", kind, s, K=75, N=C, kdiv=3, s_kq=1, s_kr=25, s_nq=75, mask=mk))
                # convT weight [Cin = C][3][5][5]: columns n = 3*tap + colour, and the transpose of that
                cases.append(Case(f"head{t}", kind, s, K=C, N=75, s_kq=75, ndiv=3, s_nq=1, s_nr=25, mask=mk))
                cases.append(Case(f"head_dx{t}", kind, s, K=75, N=C, kdiv=3, s_kq=1, s_kr=25, s_nq=75, mask=mk))
    # split index, mask and transform together
    C = 40
    bound, ped = REPARAMS[2]
    r = _rng("rgbgamma")
    sources["rgbgamma"] = (bound + 0.2 * r.standard_normal(C * 75)).astype(np.float32)
    cases.append(Case("head.masked.reparam.f32", PACK_F32, "rgbgamma", K=C, N=75, s_kq=75, ndiv=3, s_nq=1, s_nr=25,
                      mask="rgbmask40", transform=1, bound=bound, pedestal=ped))
    cases.append(Case("stem.masked.reparam.bf16", PACK_BF16, "rgbgamma", K=75, N=C, kdiv=3, s_kq=1, s_kr=25, s_nq=75,
                      mask="rgbmask40", transform=1, bound=bound, pedestal=ped))
    # 6. the one-launch stem operand
    for n in STEM16_N:
        cases.append(Case(f"stem16.{n}", PACK_BF16_STEM, src(f"stemw{n}", n * 75), N=n))
    # 7. MAP with the transform and MASK_INPLACE around the block edge
    for i, n in enumerate(EDGE_N):
        bound, ped = REPARAMS[1 + i % 2]
        name = f"beta{n}"
        r = _rng(name)
        sources[name] = (bound * (1.0 + r.standard_normal(n))).astype(np.float32)
        cases.append(Case(f"map.{n}", MAP, name, N=n, transform=1, bound=bound, pedestal=ped))
        cases.append(Case(f"mask_inplace.{n}", MASK_INPLACE, src(f"ctxw{n}", n), N=n, mask=mask01(f"ctxmask{n}", n)))
    # 8. masked pack jobs of a tensor that a MASK_INPLACE job of the same launch masks (the context model's weight)
    shape = (24, 16, 5, 5)
    s, m = src("ctx", int(np.prod(shape))), mask01("ctx.mask", int(np.prod(shape)))
    for kind in (PACK_F32, PACK_BF16):
        cases += _conv_jobs(f"ctx.masked.{kn[kind]}", kind, s, 0, shape, False, mask=m)
    cases.append(Case("ctx.mask_inplace", MASK_INPLACE, s, N=int(np.prod(shape)), mask=m))
    cases += _conv_jobs("ctx.masked.after.f32", PACK_F32, s, 0, shape, True, mask=m)
    # the last job of the table: a single block
    cases.append(Case("map.last", MAP, "beta1", N=1, transform=1, bound=REPARAMS[1][0], pedestal=REPARAMS[1][1]))
    assert len({c.name for c in cases}) == len(cases)
    return cases, sources


GAP = 4                  # poisoned floats between two buffers of an arena: 16 bytes, so every buffer stays aligned
TAIL = 128 * 1024        # poisoned floats behind the last source: a read past a source stays inside the arena


def source_layout(sources):
    """name -> first element of the buffer in ONE fp32 arena (16-byte aligned, poisoned gaps between), and its size"""
    at, pos = {}, GAP
    for name, a in sources.items():
        at[name] = pos
        pos = _ceil(pos + a.size + GAP, 4) * 4
    return at, pos + TAIL


def dest_layout(cases):
    """case index -> byte offset of its destination in ONE arena (16-byte aligned, poisoned gaps), and the arena's bytes"""
    at, pos = [], 16 * GAP
    for c in cases:
        at.append(pos)
        pos = _ceil(pos + c.dst_bytes() + 4 * GAP, 16) * 16
    return at, pos


def fill_job(j, c: Case, src_base, at, dst_ptr):
    """fills a lic_prep_job (any object with its fields); src_base: address of the source arena's first element"""
    j.src = src_base + 4 * (at[c.src] + c.off)
    j.mask = None if c.mask is None else src_base + 4 * at[c.mask]   # (read at the same offsets as src)
    j.dst = None if c.kind == MASK_INPLACE else dst_ptr
    j.s_tap, j.s_kq, j.s_kr, j.s_nq, j.s_nr = c.s_tap, c.s_kq, c.s_kr, c.s_nq, c.s_nr
    j.kind, j.taps, j.K, j.N, j.kdiv, j.ndiv = c.kind, c.taps, c.K, c.N, c.kdiv, c.ndiv
    j.transform, j.bound, j.pedestal = c.transform, c.bound, c.pedestal
    return j
