// Host-side planning shared by the fp32 and bf16 GEMM families (lic_gemm.hip, lic_gemm_bf16.hip): the fast divider,
// descriptor checks, the phase geometry of transposed convolutions, the phase order, the workspace query, the wgrad
// parameter fill and the kernel-variant tables.  Everything here is a pure function of the descriptor.
#pragma once
#include "lic_common.h"

// division of 0 <= n < 2^31 by a launch-constant d via multiply-high (host precomputes m, s)
struct FastDiv {
  unsigned m, s;
};
static inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  if (d == 0) d = 1;
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  f.s = s;
  f.m = (unsigned)(((1ull << (31 + s)) + d - 1) / d);
  return f;
}
__device__ __forceinline__ int fdiv(int n, FastDiv f) {
  return (int)(((unsigned long long)(unsigned)n * f.m) >> (31 + f.s));
}

static inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
static inline bool null_or_aligned16(const void* q) { return q == nullptr || aligned16(q); }

long lic_pick_splits(long base, long slots, long max_sk);  // lic_gemm.hip

// ---- kernel-variant tables ------------------------------------------------------------------------------------
// One row per instantiated kernel: the key the planner's choice is matched against, the kernel, its block size and
// its name.  LIC_VARIANT makes pointer and name from ONE token sequence, so the name a *_kernel_name entry reports is
// by construction the instantiation the launch entry runs (the demangled symbol without `void ` and the parameter
// list; tests/test_variant_tables.py holds every name against the library's symbols).  Rows spell out every
// template argument: a defaulted one would be missing from the name.
template <class Params>
struct KernelVariant {
  unsigned key;
  void (*kernel)(Params);
  unsigned block;
  const char* name;
};
constexpr unsigned lic_variant_key(int a, int b, int c = 0, int d = 0, int e = 0, int f = 0) {
  return (unsigned)a | (unsigned)b << 10 | (unsigned)c << 14 | (unsigned)d << 18 | (unsigned)e << 22 | (unsigned)f << 26;
}
#define LIC_VARIANT(key, block, ...) {key, __VA_ARGS__, block, #__VA_ARGS__}

template <class Params, size_t N>
static inline const KernelVariant<Params>* lic_find_variant(const KernelVariant<Params> (&table)[N], unsigned key) {
  for (const KernelVariant<Params>& v : table)
    if (v.key == key) return &v;
  return nullptr;  // the caller answers LIC_ERR_UNSUPPORTED and launches nothing
}
// the body of every lic_*_kernel_name entry point
template <class Params>
static inline int lic_variant_name(const KernelVariant<Params>* v, char* buf, size_t n) {
  if (!v) return LIC_ERR_UNSUPPORTED;
  if (!buf || n == 0) return LIC_ERR_INVALID;
  size_t i = 0;
  for (; i + 1 < n && v->name[i]; ++i) buf[i] = v->name[i];
  buf[i] = 0;
  return LIC_OK;
}

// ---- convolution descriptors ----------------------------------------------------------------------------------
// the checks both igemm planners start with
static inline int conv_desc_check(const lic_igemm_desc* d) {
  if (!d || !d->in || !d->w || !d->out) return LIC_ERR_INVALID;
  if (d->B <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Cin <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Cout <= 0 ||
      d->kh <= 0 || d->kw <= 0)
    return LIC_ERR_INVALID;
  if (d->kh * d->kw > 28 || d->stride < 1 || d->stride > 2) return LIC_ERR_UNSUPPORTED;
  return LIC_OK;
}

// Output phases of a launch: one, or the stride^2 phases of a transposed convolution (output pixels of one parity
// share their live taps).  Per phase the quotient grid Hq x Wq, its dividers and the live taps.
struct PhaseGeometry {
  int nphase;
  int ntaps[4];
  int Hq[4], Wq[4];
  FastDiv dHW[4], dW[4];  // divide by Hq*Wq and by Wq
  unsigned char taps[4][28];
  long maxP;          // most output pixels of any phase
  int max_taps;       // most live taps of any phase ...
  int max_chunks;     // ... and its K chunks, at `cpt` chunks per tap
  int64_t live_macs;  // multiply-adds on live taps
};
static inline PhaseGeometry phase_geometry(const lic_igemm_desc* d, int cpt) {
  PhaseGeometry g = {};
  const uint32_t mask = d->tap_mask ? d->tap_mask : 0xFFFFFFFFu;
  g.nphase = (d->transposed && d->stride > 1) ? d->stride * d->stride : 1;
  for (int ph = 0; ph < 4; ++ph) g.dHW[ph] = g.dW[ph] = make_fastdiv(1);
  for (int ph = 0; ph < g.nphase; ++ph) {
    const int py = (g.nphase > 1) ? ph / d->stride : 0, px = (g.nphase > 1) ? ph % d->stride : 0;
    const int st = (g.nphase > 1) ? d->stride : 1;
    g.Hq[ph] = (d->Ho - py + st - 1) / st;
    g.Wq[ph] = (d->Wo - px + st - 1) / st;
    if (g.Hq[ph] < 0) g.Hq[ph] = 0;
    if (g.Wq[ph] < 0) g.Wq[ph] = 0;
    const long Pp = (long)d->B * g.Hq[ph] * g.Wq[ph];
    g.dHW[ph] = make_fastdiv((unsigned)(g.Hq[ph] * g.Wq[ph]));
    g.dW[ph] = make_fastdiv((unsigned)g.Wq[ph]);
    if (Pp > g.maxP) g.maxP = Pp;
    int n = 0;
    for (int r = 0; r < d->kh; ++r)
      for (int s = 0; s < d->kw; ++s) {
        const int t = r * d->kw + s;
        if (!((mask >> t) & 1u)) continue;
        if (g.nphase > 1)
          if (((py + d->pad - r) % d->stride) != 0 || ((px + d->pad - s) % d->stride) != 0) continue;
        g.taps[ph][n++] = (unsigned char)t;
      }
    g.ntaps[ph] = n;
    if (n > g.max_taps) g.max_taps = n;
    g.live_macs += (int64_t)Pp * n * d->Cin * d->Cout;
  }
  g.max_chunks = g.max_taps * cpt;
  return g;
}
// copies the per-phase fields into a kernel parameter block (IgemmParams / IgemmHParams)
template <class Params>
static inline void store_phases(Params& p, const PhaseGeometry& g) {
  p.nphase = g.nphase;
  for (int ph = 0; ph < 4; ++ph) {
    p.ntaps[ph] = g.ntaps[ph];
    p.Hq[ph] = g.Hq[ph];
    p.Wq[ph] = g.Wq[ph];
    p.dHW[ph] = g.dHW[ph];
    p.dW[ph] = g.dW[ph];
    for (int t = 0; t < 28; ++t) p.taps[ph][t] = g.taps[ph][t];
  }
}

// Phase order of a 4-phase launch of MT tiles in M.  From 128 tiles on, phases are sorted by tap count inside groups
// of `pgroup` M tiles (an XCD's slots run a round of 9-tap workgroups, then the 6-tap ones, then the 4-tap ones).  The
// groups are sized to the XCD ranges of xcd_contiguous(): every XCD takes k = ceil(MT / 512) whole groups of
// pgroup = ceil(MT / 8k) <= 64 tiles, MT is rounded up to 8 * k * pgroup (at most 8k - 1 padding tiles, which exit at
// once) and the grid is a multiple of 8, so all eight XCDs get the same number of M tiles of every phase whatever NT
// and the K split are.  (Groups of a fixed 64 tiles left an XCD half a group at MT = 256 -- nine- and six-tap
// workgroups on the even XCDs, six- and four-tap ones on the odd: 960 against 640 tap-tiles -- and one tap class per
// XCD at MT = 128.)  MT a multiple of 512 gives groups of 64, k per XCD.  Below 128 tiles the kernels rotate phases
// tile by tile (pgroup 0).
struct PhaseOrder {
  int porder;  // phase ids by decreasing tap count, 2 bits each
  int pgroup;  // M tiles per phase-sorted group
  int MT;
};
static inline PhaseOrder phase_order(int nphase, const int ntaps[4], int MT) {
  PhaseOrder o = {0, 0, MT};
  if (nphase != 4 || MT < 128) return o;
  int ord[4] = {0, 1, 2, 3};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (ntaps[ord[j]] > ntaps[ord[i]]) {
        const int t = ord[i];
        ord[i] = ord[j];
        ord[j] = t;
      }
  o.porder = ord[0] | (ord[1] << 2) | (ord[2] << 4) | (ord[3] << 6);
  const int per_xcd = (MT + 511) / 512;  // groups in each XCD's range
  o.pgroup = (MT + 8 * per_xcd - 1) / (8 * per_xcd);
  o.MT = 8 * per_xcd * o.pgroup;
  return o;
}

// Workspace that lets the planner split K for `d`: plans a copy of the descriptor with stand-in pointers (planners
// never dereference them) and an unlimited workspace.  ksplit_of(q) returns the plan's K split, 0 when it failed.
template <class KsplitOf>
static inline size_t conv_workspace_bytes(const lic_igemm_desc* d, KsplitOf ksplit_of) {
  if (!d) return 0;
  if (d->epilogue != LIC_EPI_NONE && d->epilogue != LIC_EPI_LEAKY) return 0;
  lic_igemm_desc q = *d;
  static float dummy[4] __attribute__((aligned(16)));
  q.in = q.w = dummy;
  q.out = dummy;
  q.bias = q.aux = q.aux2 = q.aux3 = q.res = nullptr;
  q.out2 = q.out3 = nullptr;
  q.workspace = dummy;
  q.workspace_bytes = ~(size_t)0;
  const int ksplit = ksplit_of(q);
  if (ksplit <= 1) return 0;
  return (size_t)ksplit * d->B * d->Ho * d->Wo * d->Cout * sizeof(float);
}

// ---- weight gradients -----------------------------------------------------------------------------------------
struct WgPlan {
  int TM, TN, vec, MTt, NTt, ntaps, nchunks, splitk, cps;
  int Cm, Cn;
  int dma;  // fp32: both operands within reach of the LDS-DMA kernel's 32-bit lane offsets (wgrad_dma_addressable)
};
static inline int wgrad_desc_check(const lic_wgrad_desc* d) {
  if (!d || d->B <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->Cp <= 0 || d->Cg <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->Hl <= 0 || d->Wl <= 0)
    return LIC_ERR_INVALID;
  return LIC_OK;
}
static inline size_t wgrad_slab_bytes(const WgPlan& pl) {
  return (size_t)pl.splitk * pl.ntaps * pl.Cm * pl.Cn * sizeof(float);
}
// the checks of a launch that follow the plan; `operands` is the precision's own verdict on the operands (stride,
// alignment), which ranks after the null checks
static inline int wgrad_launch_check(const lic_wgrad_desc* d, const WgPlan& pl, const void* workspace,
                                     size_t workspace_bytes, int operands) {
  if (!d->p || !d->g || !d->dst || !workspace) return LIC_ERR_INVALID;
  if (operands != LIC_OK) return operands;
  if (workspace_bytes < wgrad_slab_bytes(pl)) return LIC_ERR_WORKSPACE;
  if ((long)d->B * d->Hs * d->Ws > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
  return LIC_OK;
}
// fills WgradParams / WgradHParams (the two stay distinct types: their element types differ)
template <class Params>
static inline Params wgrad_fill(const lic_wgrad_desc* d, const WgPlan& pl, void* workspace) {
  using Operand = decltype(Params::row);
  using Ptr = decltype(Operand::ptr);
  Operand P, G;
  P.ptr = (Ptr)d->p;
  P.ld = d->p_ld;
  P.C = d->Cp;
  P.gathered = 0;
  P.sq = d->sq_p;
  G.ptr = (Ptr)d->g;
  G.ld = d->g_ld;
  G.C = d->Cg;
  G.gathered = !(d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0 && d->Hl == d->Hs && d->Wl == d->Ws);
  G.sq = d->sq_g;
  Params p;
  p.row = d->g_is_row ? G : P;
  p.col = d->g_is_row ? P : G;
  p.slabs = (float*)workspace;
  p.B = d->B;
  p.Hs = d->Hs;
  p.Ws = d->Ws;
  p.Hl = d->Hl;
  p.Wl = d->Wl;
  p.kw = d->kw;
  p.stride = d->stride;
  p.pad = d->pad;
  p.ntaps = pl.ntaps;
  p.MTt = pl.MTt;
  p.NTt = pl.NTt;
  p.chunks_per_split = pl.cps;
  p.nchunks = pl.nchunks;
  p.Ps = (long)d->B * d->Hs * d->Ws;
  p.dHW = make_fastdiv((unsigned)(d->Hs * d->Ws));
  p.dW = make_fastdiv((unsigned)d->Ws);
  return p;
}
