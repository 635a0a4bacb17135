// Device half of lic_conv_plan.h, shared by the fp32 and bf16 GEMM families: the integer arithmetic that turns a
// workgroup id into a tile and a tile row into a pixel.  It consumes what the host half computes (`porder`, `pgroup`,
// `dHW`, `dW`, `MTt`, `chunks_per_split`); a change to phase_order() or wgrad_fill() has its device counterpart here
// and nowhere else.  Everything is a stateless function of the parameter block, inlined into the calling kernel.
#pragma once
#include "lic_conv_plan.h"

// operands of the LDS-DMA builtins (`global_load_lds_dwordx4`, `buffer_load ... lds`)
typedef const __attribute__((address_space(1))) void* lic_gptr_t;
typedef __attribute__((address_space(3))) void* lic_lptr_t;

// XCD-contiguous workgroup remap (bijective on [0, n)).  The hardware deals workgroup ids round-robin over the chip's
// 8 XCDs, each with an L2 of its own: id i runs on XCD i % 8.  Launch-order neighbours -- which is how every kernel
// here lays out the workgroups that read the same memory -- would therefore land in eight different L2s and each pull
// the shared data through the fabric.  The remap hands XCD x the contiguous range of logical ids
// [x * q + min(x, r), +q + (x < r)), q = n / 8, r = n % 8 (the first r XCDs hold one id more), and walks it in the
// order the XCD receives its workgroups (idx = id / 8).  What the neighbours share is said at each call site.
// (__host__ too, like conv_tile below: lic_igemm_tile_order evaluates the pair on the host.)
__host__ __device__ __forceinline__ int xcd_contiguous(int id, int n) {
  const int q = n >> 3, r = n & 7, xcd = id & 7, idx = id >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- implicit-GEMM convolutions (IgemmParams / IgemmHParams: the same field names, as for store_phases) ---------
// Tile of logical workgroup `wg`: K split fastest (the splits of a tile share its A rows in L2), then the N tile,
// then phase and M tile.  Phases interleave under one M tile index so that every XCD's contiguous id range holds all
// phases (their K lengths differ up to 2.25x: 9/6/6/4 taps for 5x5 stride 2).
struct ConvTile {
  int ks, nt, phase, mt;
};
template <class Params>
__host__ __device__ __forceinline__ ConvTile conv_tile(const Params& p, int wg) {
  ConvTile t;
  t.ks = 0;
  if (p.ksplit > 1) {
    t.ks = wg % p.ksplit;
    wg /= p.ksplit;
  }
  t.nt = wg % p.NT;
  const int kq = wg / p.NT;
  t.phase = 0;
  t.mt = kq;
  if (p.nphase == 4) {
    if (p.pgroup > 0) {
      // phases sorted by tap count inside groups of `pgroup` M tiles (phase_order()): an XCD's slots run a round
      // of 9-tap workgroups, then the 6-tap ones, then the 4-tap ones -- homogeneous rounds, short tail (all-equal
      // neighbours also avoid the period-4 pattern described below).  phase_order() sizes the groups so that each
      // XCD's range under xcd_contiguous() is a whole number of them, and pads MT to that: the caller's `m0 >= P`
      // exit retires the padding tiles.
      const int span = 4 * p.pgroup;
      const int grp = kq / span, loc = kq - grp * span;
      const int rank = loc / p.pgroup;
      t.phase = (p.porder >> (2 * rank)) & 3;
      t.mt = grp * p.pgroup + (loc - rank * p.pgroup);
    } else {
      // Rotate the phase order from one M tile to the next.  Phase durations differ (9/6/6/4 taps) and the
      // hardware deals consecutive workgroups round-robin over its shader engines / CUs: with a fixed period-4
      // order one engine would receive only 9-tap workgroups and pace all the others (measured: 1.2 instead of
      // 1.9 resident waves per SIMD).
      t.phase = (kq + (kq >> 2) + (kq >> 4) + (kq >> 6) + (kq >> 8)) & 3;
      t.mt = kq / p.nphase;
    }
  }
  return t;
}

// One output phase of a launch: rows of the phase's GEMM are the pixels of its Hq x Wq quotient grid, batch-major.
// Rows must be in range (0 <= prow < P); what a kernel does with the rows past P is its own business.
struct PhaseView {
  int nphase, Hq, Wq, P;
  int sph;     // output step between rows of this phase
  int py, px;  // the phase's offset on the output grid
  int Ho, Wo;
  FastDiv dHW, dW;
  struct Origin {
    int b, oy, ox;  // image and output coordinates of a row
  };
  template <class Params>
  __device__ __forceinline__ PhaseView(const Params& p, int phase)
      : nphase(p.nphase), Hq(p.Hq[phase]), Wq(p.Wq[phase]), P(p.B * p.Hq[phase] * p.Wq[phase]),
        sph(p.nphase > 1 ? p.stride : 1), py(p.nphase > 1 ? phase / p.stride : 0),
        px(p.nphase > 1 ? phase % p.stride : 0), Ho(p.Ho), Wo(p.Wo), dHW(p.dHW[phase]), dW(p.dW[phase]) {}
  __device__ __forceinline__ Origin origin(int prow) const {
    const int b = fdiv(prow, dHW);
    const int rem = prow - b * Hq * Wq;
    const int i = fdiv(rem, dW), jj = rem - i * Wq;
    return {b, i * sph + py, jj * sph + px};
  }
  // flat output pixel of a row (a single phase covers the output in row order)
  __device__ __forceinline__ long out_pixel(int prow) const {
    if (nphase == 1) return prow;
    const Origin o = origin(prow);
    return ((long)o.b * Ho + o.oy) * Wo + o.ox;
  }
};

// Where the gather of a row starts: first pixel of its image and the input coordinate tap (0, 0) reads -- a transposed
// convolution walks the taps backwards from it (and halves the result at stride 2), a forward one forwards.
struct GatherOrigin {
  int base, hy, wx;
};
template <class Params>
__device__ __forceinline__ GatherOrigin gather_origin(const Params& p, const PhaseView& pv, int prow) {
  const PhaseView::Origin o = pv.origin(prow);
  const int base = o.b * p.Hi * p.Wi;
  if (p.transposed) return {base, o.oy + p.pad, o.ox + p.pad};
  return {base, o.oy * p.stride - p.pad, o.ox * p.stride - p.pad};
}

// ---- weight gradients (WgradParams / WgradHParams) -------------------------------------------------------------
// Logical workgroup -> (BMt x BNt tile, tap, K split), tile fastest: the workgroups of a split stream the same pixels.
struct WgradTile {
  int mt, nt, m0, n0;
  int tap, r, s;
  int split, c_begin, c_end;  // this split's chunks [c_begin, c_end)
};
template <class Params>
__device__ __forceinline__ WgradTile wgrad_tile(const Params& p, int wg, int BMt, int BNt) {
  WgradTile t;
  const int tiles = p.MTt * p.NTt;
  const int tile = wg % tiles;
  wg /= tiles;
  t.tap = wg % p.ntaps;
  t.split = wg / p.ntaps;
  t.mt = tile / p.NTt;
  t.nt = tile - t.mt * p.NTt;
  t.m0 = t.mt * BMt;
  t.n0 = t.nt * BNt;
  t.r = t.tap / p.kw;
  t.s = t.tap - t.r * p.kw;
  t.c_begin = t.split * p.chunks_per_split;
  t.c_end = min(p.nchunks, t.c_begin + p.chunks_per_split);
  return t;
}
// Pixel `pk` of the small grid (the contraction index; past Ps it reads pixel 0 and `inb` is false) and the pixel of
// the large grid that tap (r, s) pairs it with, for whichever operand is gathered (`gok`: it exists).
struct WgradPixel {
  bool inb, gok;
  int pix;  // (the launch checks refuse Ps >= 2^31)
  long gpix;
};
template <class Params>
__device__ __forceinline__ WgradPixel wgrad_pixel(const Params& p, long pk, int r, int s) {
  WgradPixel w;
  w.inb = pk < p.Ps;
  w.pix = w.inb ? (int)pk : 0;
  const int b = fdiv(w.pix, p.dHW);
  const int rem = w.pix - b * p.Hs * p.Ws;
  const int hs = fdiv(rem, p.dW), ws = rem - hs * p.Ws;
  const int hl = hs * p.stride - p.pad + r, wl = ws * p.stride - p.pad + s;
  w.gok = w.inb && hl >= 0 && wl >= 0 && hl < p.Hl && wl < p.Wl;
  w.gpix = ((long)b * p.Hl + hl) * p.Wl + wl;
  return w;
}
