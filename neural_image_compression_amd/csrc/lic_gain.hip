// Gain units of the variable-rate model (Cui et al. 2021): a per-channel scale in front of a quantiser
// and its inverse behind it.  Two HBM-bound entries of liblic_hip.so (gfx950):
//   lic_gain_quantize  vg = v * s and, in the same launch, the quantised vg, its anchors and the bf16 copies;
//   lic_gain_bwd       dv = t * s and ds[b][c] = sum_pixels t * v, a two-stage sum in a fixed order.
// Each has a 16-byte path (C % 4 == 0, aligned operands) and a single-float path that write the same bytes.  No
// multiply is contracted with the add behind it (gain_point, gain_grad_point): the rounding points are lic.h's.
// And the scales themselves from qualities that stay on the device (a few thousand elements, one launch each):
//   lic_gain_rows_fwd  rows[t][b] = exp((1 - l_b) T_t[i_b] + l_b T_t[i_b + 1]) for up to four stacked tables;
//   lic_gain_rows_bwd  the tables' gradient, one thread per element summing over the images in rising order.
#include "lic_common.h"

#define GAIN_BLOCK 256
#define GAIN_LANES 64  // channel units side by side in a workgroup of lic_gain_bwd: one wave per running sum
static_assert(GAIN_LANES * LIC_GAIN_SLAB_ROWS == GAIN_BLOCK, "one wave per running sum of a slab");
static_assert(LIC_GAIN_SLAB_PIXELS % LIC_GAIN_SLAB_ROWS == 0, "a full slab gives every running sum as many pixels");

typedef __bf16 gain_bf16_t;
typedef gain_bf16_t gain_bf16x4 __attribute__((ext_vector_type(4)));

static bool gain_al(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

template <int VEC>
__device__ __forceinline__ void gain_load(const float* p, float (&a)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = t[e];
  } else {
    a[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void gain_store(float* p, const float (&a)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = a[e];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = a[0];
  }
}
template <int VEC>
__device__ __forceinline__ void gain_store_bf16(gain_bf16_t* p, const float (&a)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = a[e];
    *reinterpret_cast<gain_bf16x4*>(p) = __builtin_convertvector(t, gain_bf16x4);
  } else {
    *p = (gain_bf16_t)a[0];
  }
}

// vg = fl32(v * s); out = fl32(vg + fl32(u - 0.5f)) or rint(vg): the product is rounded before it is used
__device__ __forceinline__ void gain_point(float v, float s, float u, int mode, float& vg, float& out) {
#pragma clang fp contract(off)
  vg = v * s;
  out = mode == LIC_GAIN_NOISE ? vg + (u - 0.5f) : rintf(vg);
}

// one thread: VEC consecutive channels of one pixel (C % VEC == 0).  Workgroups [b * bpi, (b + 1) * bpi) cover image b.
template <int VEC>
__global__ __launch_bounds__(GAIN_BLOCK) void gain_quantize_kernel(const float* __restrict__ v, const float* __restrict__ u,
                                                                   const float* __restrict__ s, long s_stride,
                                                                   float* __restrict__ vg, float* __restrict__ out,
                                                                   float* __restrict__ anc, gain_bf16_t* __restrict__ vg16,
                                                                   gain_bf16_t* __restrict__ out16,
                                                                   gain_bf16_t* __restrict__ anc16, unsigned upi,
                                                                   unsigned bpi, unsigned w, unsigned cu, int mode) {
  const unsigned b = blockIdx.x / bpi;
  const unsigned j = (blockIdx.x - b * bpi) * GAIN_BLOCK + threadIdx.x;
  if (j >= upi) return;
  const unsigned pix = j / cu, c = (j - pix * cu) * VEC;
  const long at = ((long)b * upi + j) * VEC;
  float a[VEC], sc[VEC], r[VEC], g[VEC], o[VEC];
  gain_load<VEC>(v + at, a);
  gain_load<VEC>(s + (long)b * s_stride + c, sc);
  if (mode == LIC_GAIN_NOISE) {
    gain_load<VEC>(u + at, r);
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) r[e] = 0.0f;
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) gain_point(a[e], sc[e], r[e], mode, g[e], o[e]);
  gain_store<VEC>(vg + at, g);
  if (vg16) gain_store_bf16<VEC>(vg16 + at, g);
  if (mode == LIC_GAIN_SCALE) return;
  gain_store<VEC>(out + at, o);
  if (out16) gain_store_bf16<VEC>(out16 + at, o);
  if (anc || anc16) {
    const unsigned row = pix / w;
    if ((row + (pix - row * w)) & 1) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = 0.0f;
    }
    if (anc) gain_store<VEC>(anc + at, o);
    if (anc16) gain_store_bf16<VEC>(anc16 + at, o);
  }
}

// the extents both entries accept; *hw = h * w
static int gain_extents(const float* s, int64_t s_stride, int32_t B, int32_t h, int32_t w, int32_t C, int64_t* hw) {
  if (!s || B <= 0 || h <= 0 || w <= 0 || C <= 0 || s_stride < 0 || (s_stride > 0 && s_stride < C)) return LIC_ERR_INVALID;
  *hw = (int64_t)h * w;
  if (*hw * C >= 0x7FFFFFFFLL) return LIC_ERR_UNSUPPORTED;
  return LIC_OK;
}

LIC_EXPORT int lic_gain_quantize(const float* v, const float* u, const float* s, int64_t s_stride, float* vg, float* out,
                                 float* out_anchor, void* vg_bf16, void* out_bf16, void* anchor_bf16, int32_t B, int32_t h,
                                 int32_t w, int32_t C, int32_t mode, lic_stream_t stream) {
  int64_t hw = 0;
  if (!v || !vg) return LIC_ERR_INVALID;
  if (mode == LIC_GAIN_SCALE) {
    if (u || out || out_anchor || out_bf16 || anchor_bf16) return LIC_ERR_INVALID;
  } else if (mode == LIC_GAIN_NOISE || mode == LIC_GAIN_ROUND) {
    if (!out || (mode == LIC_GAIN_NOISE && !u)) return LIC_ERR_INVALID;
  } else {
    return LIC_ERR_INVALID;
  }
  if (const int rc = gain_extents(s, s_stride, B, h, w, C, &hw)) return rc;
  for (const void* p : {(const void*)v, (const void*)u, (const void*)s, (const void*)vg, (const void*)out,
                        (const void*)out_anchor})
    if (!gain_al(p, 4)) return LIC_ERR_INVALID;
  for (const void* p : {(const void*)vg_bf16, (const void*)out_bf16, (const void*)anchor_bf16})
    if (!gain_al(p, 2)) return LIC_ERR_INVALID;
  if (mode == LIC_GAIN_ROUND) u = nullptr;
  bool vec = C % 4 == 0 && s_stride % 4 == 0;
  for (const void* p : {(const void*)v, (const void*)u, (const void*)s, (const void*)vg, (const void*)out,
                        (const void*)out_anchor})
    vec = vec && gain_al(p, 16);
  for (const void* p : {(const void*)vg_bf16, (const void*)out_bf16, (const void*)anchor_bf16}) vec = vec && gain_al(p, 8);
  const int per = vec ? 4 : 1;
  const int64_t upi = hw * C / per, bpi = cdiv64(upi, GAIN_BLOCK);
  if (bpi * B > 0x7FFFFFFFLL) return LIC_ERR_UNSUPPORTED;
  auto kern = vec ? gain_quantize_kernel<4> : gain_quantize_kernel<1>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(bpi * B)), dim3(GAIN_BLOCK), 0, (hipStream_t)stream, v, u, s, (long)s_stride, vg,
                     out, out_anchor, (gain_bf16_t*)vg_bf16, (gain_bf16_t*)out_bf16, (gain_bf16_t*)anchor_bf16,
                     (unsigned)upi, (unsigned)bpi, (unsigned)w, (unsigned)(C / per), mode);
  return lic_check_launch();
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// t = d_vg + d_out + anchor(d_anchor) in that order (an absent term is left out); dv = fl32(t * s); the running sum
// takes fl32(t * v)
__device__ __forceinline__ void gain_grad_point(bool has_g, float g, bool has_o, float o, bool has_a, float a, float s,
                                                float v, float& dv, float& acc) {
#pragma clang fp contract(off)
  float t = has_g ? g : (has_o ? o : a);
  if (has_g && has_o) t = t + o;
  if ((has_g || has_o) && has_a) t = t + a;
  dv = t * s;
  const float tv = t * v;
  acc = acc + tv;
}

// stage 1: workgroup (b, slab); wave r of it keeps running sum r of every channel unit, over the slab's pixels r, r + ROWS,
// ...; the ROWS sums are added r = 0, 1, ... into the slab's partial row.  dv is written on the way.
template <int VEC>
__global__ __launch_bounds__(GAIN_BLOCK) void gain_bwd_kernel(const float* __restrict__ v, const float* __restrict__ s,
                                                              long s_stride, const float* __restrict__ d_vg,
                                                              const float* __restrict__ d_out,
                                                              const float* __restrict__ d_anchor, float* __restrict__ dv,
                                                              float* __restrict__ part, unsigned hw, unsigned w, unsigned C,
                                                              unsigned nslab) {
  __shared__ float red[LIC_GAIN_SLAB_ROWS][GAIN_LANES * VEC];
  const unsigned b = blockIdx.x / nslab, slab = blockIdx.x - b * nslab;
  const unsigned tx = threadIdx.x % GAIN_LANES, ty = threadIdx.x / GAIN_LANES;
  const unsigned p0 = slab * LIC_GAIN_SLAB_PIXELS;
  const unsigned p1 = p0 + LIC_GAIN_SLAB_PIXELS < hw ? p0 + LIC_GAIN_SLAB_PIXELS : hw;
  const unsigned ncu = C / VEC;
  const long image = (long)b * hw * C;
  for (unsigned cu0 = 0; cu0 < ncu; cu0 += GAIN_LANES) {  // (uniform trip count: the barriers below are reached by all)
    const unsigned cu = cu0 + tx;
    const bool live = cu < ncu;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
    if (live) {
      float sc[VEC];
      gain_load<VEC>(s + (long)b * s_stride + cu * VEC, sc);
      for (unsigned p = p0 + ty; p < p1; p += LIC_GAIN_SLAB_ROWS) {
        const long at = image + (long)p * C + cu * VEC;
        const unsigned row = p / w;
        const bool anchor = ((row + (p - row * w)) & 1) == 0;
        float a[VEC], g[VEC], o[VEC], m[VEC], d[VEC];
        gain_load<VEC>(v + at, a);
#pragma unroll
        for (int e = 0; e < VEC; ++e) g[e] = o[e] = m[e] = 0.0f;
        if (d_vg) gain_load<VEC>(d_vg + at, g);
        if (d_out) gain_load<VEC>(d_out + at, o);
        if (d_anchor && anchor) gain_load<VEC>(d_anchor + at, m);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          gain_grad_point(d_vg != nullptr, g[e], d_out != nullptr, o[e], d_anchor != nullptr, m[e], sc[e], a[e], d[e],
                          acc[e]);
        gain_store<VEC>(dv + at, d);
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[ty][tx * VEC + e] = acc[e];
    __syncthreads();
    if (ty == 0 && live) {
      float sum[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        sum[e] = red[0][tx * VEC + e];
#pragma unroll
        for (int r = 1; r < LIC_GAIN_SLAB_ROWS; ++r) sum[e] += red[r][tx * VEC + e];
      }
      gain_store<VEC>(part + (long)blockIdx.x * C + cu * VEC, sum);
    }
    __syncthreads();
  }
}

// stage 2: ds[b][c] = partial rows of image b added slab 0, 1, ...
__global__ __launch_bounds__(GAIN_BLOCK) void gain_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ ds,
                                                                     long BC, unsigned C, unsigned nslab) {
  const long i = (long)blockIdx.x * GAIN_BLOCK + threadIdx.x;
  if (i >= BC) return;
  const long b = i / C;
  const unsigned c = (unsigned)(i - b * C);
  const float* row = part + b * nslab * C + c;
  float sum = row[0];
  for (unsigned k = 1; k < nslab; ++k) sum += row[(long)k * C];
  ds[i] = sum;
}

LIC_EXPORT size_t lic_gain_bwd_workspace_bytes(int32_t B, int64_t hw, int32_t C) {
  if (B <= 0 || hw <= 0 || C <= 0) return 0;
  return (size_t)B * (size_t)cdiv64(hw, LIC_GAIN_SLAB_PIXELS) * (size_t)C * sizeof(float);
}

LIC_EXPORT int lic_gain_bwd(const float* v, const float* s, int64_t s_stride, const float* d_vg, const float* d_out,
                            const float* d_anchor, float* dv, float* ds, int32_t B, int32_t h, int32_t w, int32_t C,
                            void* workspace, size_t workspace_bytes, lic_stream_t stream) {
  int64_t hw = 0;
  if (!v || !dv || !ds || !workspace || (!d_vg && !d_out && !d_anchor)) return LIC_ERR_INVALID;
  if (const int rc = gain_extents(s, s_stride, B, h, w, C, &hw)) return rc;
  if (workspace_bytes < lic_gain_bwd_workspace_bytes(B, hw, C)) return LIC_ERR_INVALID;
  for (const void* p : {(const void*)v, (const void*)s, (const void*)d_vg, (const void*)d_out, (const void*)d_anchor,
                        (const void*)dv, (const void*)ds, (const void*)workspace})
    if (!gain_al(p, 4)) return LIC_ERR_INVALID;
  const int64_t nslab = cdiv64(hw, LIC_GAIN_SLAB_PIXELS);
  if (nslab * B > 0x7FFFFFFFLL) return LIC_ERR_UNSUPPORTED;
  float* part = nslab == 1 ? ds : (float*)workspace;
  bool vec = C % 4 == 0 && s_stride % 4 == 0;
  for (const void* p : {(const void*)v, (const void*)s, (const void*)d_vg, (const void*)d_out, (const void*)d_anchor,
                        (const void*)dv, (const void*)part})
    vec = vec && gain_al(p, 16);
  auto kern = vec ? gain_bwd_kernel<4> : gain_bwd_kernel<1>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nslab * B)), dim3(GAIN_BLOCK), 0, (hipStream_t)stream, v, s, (long)s_stride, d_vg,
                     d_out, d_anchor, dv, part, (unsigned)hw, (unsigned)w, (unsigned)C, (unsigned)nslab);
  if (const int rc = lic_check_launch()) return rc;
  if (nslab == 1) return LIC_OK;
  const int64_t BC = (int64_t)B * C;
  hipLaunchKernelGGL(gain_bwd_finish_kernel, dim3((unsigned)cdiv64(BC, GAIN_BLOCK)), dim3(GAIN_BLOCK), 0, (hipStream_t)stream,
                     (const float*)part, ds, (long)BC, (unsigned)C, (unsigned)nslab);
  return lic_check_launch();
}

// ---------------------------------------------------------------------------------------------
// gain rows from device qualities (lic.h: lic_gain_rows_fwd / lic_gain_rows_bwd)
// ---------------------------------------------------------------------------------------------
// the level i and the weight l of one image: qc = min(max(q, 0), Q-1) (NaN -> 0), i = min(floor(qc), Q-2), l = qc - i
__device__ __forceinline__ void gain_level(float q, int Q, int& i, float& l) {
  const float top = (float)(Q - 1);
  const float qc = q != q ? 0.0f : (q < 0.0f ? 0.0f : (q > top ? top : q));
  const int f = (int)floorf(qc);
  i = f < Q - 2 ? f : Q - 2;
  l = qc - (float)i;
}

// rows = expf(fl32(fl32(fl32(1 - l) * T[i]) + fl32(l * T[i+1]))): no product is contracted with the sum
__device__ __forceinline__ float gain_row_point(float l, float t0, float t1) {
#pragma clang fp contract(off)
  const float w0 = 1.0f - l;
  const float a = w0 * t0;
  const float b = l * t1;
  const float e = a + b;
  return expf(e);
}

// one thread per element of rows [k][B][M]; the threads of table 0, channel 0 write their image's level
__global__ __launch_bounds__(GAIN_BLOCK) void gain_rows_fwd_kernel(const float* __restrict__ q, const float* __restrict__ tables,
                                                                   float* __restrict__ rows, int* __restrict__ lvl_i,
                                                                   float* __restrict__ lvl_l, long total, int Q, int M,
                                                                   int B) {
  const long e = (long)blockIdx.x * GAIN_BLOCK + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % M);
  const long kb = e / M;
  const int b = (int)(kb % B), kk = (int)(kb / B);
  int i;
  float l;
  gain_level(q[b], Q, i, l);
  const float* T = tables + ((long)kk * Q + i) * M + c;
  rows[e] = gain_row_point(l, T[0], T[M]);
  if (kk == 0 && c == 0) {
    lvl_i[b] = i;
    lvl_l[b] = l;
  }
}

struct gain_rows_grads {
  const float* p[LIC_GAIN_ROWS_MAX_TABLES];
};

// one thread per element of d_tables [k][Q][M]: a running sum over the images in rising order, level i first, then i + 1
__global__ __launch_bounds__(GAIN_BLOCK) void gain_rows_bwd_kernel(const int* __restrict__ lvl_i, const float* __restrict__ lvl_l,
                                                                   const float* __restrict__ rows, gain_rows_grads d_rows,
                                                                   float* __restrict__ d_tables, long total, int Q, int M,
                                                                   int B) {
#pragma clang fp contract(off)
  const long e = (long)blockIdx.x * GAIN_BLOCK + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % M);
  const long kj = e / M;
  const int j = (int)(kj % Q), kk = (int)(kj / Q);
  const float* g = d_rows.p[kk];
  float sum = 0.0f;
  if (g) {
    const float* r = rows + (long)kk * B * M + c;
    for (int b = 0; b < B; ++b) {
      const int i = lvl_i[b];
      if (i != j && i + 1 != j) continue;
      const float l = lvl_l[b], rv = r[(long)b * M], gv = g[(long)b * M + c];
      if (i == j) {
        const float w0 = 1.0f - l;
        const float t = w0 * rv;
        const float u = t * gv;
        sum = sum + u;
      }
      if (i + 1 == j) {
        const float t = l * rv;
        const float u = t * gv;
        sum = sum + u;
      }
    }
  }
  d_tables[e] = sum;
}

static int gain_rows_extents(int32_t k, int32_t Q, int32_t M, int32_t B) {
  if (k < 1 || k > LIC_GAIN_ROWS_MAX_TABLES || Q < 2 || M < 1 || B < 1) return LIC_ERR_INVALID;
  if ((int64_t)k * M * (B > Q ? B : Q) >= 0x7FFFFFFFLL) return LIC_ERR_UNSUPPORTED;
  return LIC_OK;
}

LIC_EXPORT int lic_gain_rows_fwd(const float* q, const float* tables, float* rows, void* lvl, int32_t k, int32_t Q, int32_t M,
                                 int32_t B, lic_stream_t stream) {
  if (!q || !tables || !rows || !lvl) return LIC_ERR_INVALID;
  if (const int rc = gain_rows_extents(k, Q, M, B)) return rc;
  for (const void* p : {(const void*)q, (const void*)tables, (const void*)rows, (const void*)lvl})
    if (!gain_al(p, 4)) return LIC_ERR_INVALID;
  const int64_t total = (int64_t)k * B * M;
  hipLaunchKernelGGL(gain_rows_fwd_kernel, dim3((unsigned)cdiv64(total, GAIN_BLOCK)), dim3(GAIN_BLOCK), 0, (hipStream_t)stream,
                     q, tables, rows, (int*)lvl, (float*)lvl + B, (long)total, (int)Q, (int)M, (int)B);
  return lic_check_launch();
}

LIC_EXPORT int lic_gain_rows_bwd(const void* lvl, const float* rows, const float* d_rows0, const float* d_rows1,
                                 const float* d_rows2, const float* d_rows3, float* d_tables, int32_t k, int32_t Q, int32_t M,
                                 int32_t B, lic_stream_t stream) {
  if (!lvl || !rows || !d_tables) return LIC_ERR_INVALID;
  if (const int rc = gain_rows_extents(k, Q, M, B)) return rc;
  gain_rows_grads g = {{d_rows0, d_rows1, d_rows2, d_rows3}};
  for (int t = k; t < LIC_GAIN_ROWS_MAX_TABLES; ++t)
    if (g.p[t]) return LIC_ERR_INVALID;
  for (const void* p : {(const void*)lvl, (const void*)rows, (const void*)d_rows0, (const void*)d_rows1, (const void*)d_rows2,
                        (const void*)d_rows3, (const void*)d_tables})
    if (!gain_al(p, 4)) return LIC_ERR_INVALID;
  const int64_t total = (int64_t)k * Q * M;
  hipLaunchKernelGGL(gain_rows_bwd_kernel, dim3((unsigned)cdiv64(total, GAIN_BLOCK)), dim3(GAIN_BLOCK), 0, (hipStream_t)stream,
                     (const int*)lvl, (const float*)lvl + B, rows, g, d_tables, (long)total, (int)Q, (int)M, (int)B);
  return lic_check_launch();
}
