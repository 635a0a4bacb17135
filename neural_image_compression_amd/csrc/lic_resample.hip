// lic_resample: a window of an image RESIZED with Pillow's 8-bit bicubic filter -- resize, crop, flip and
// ToTensor() as one launch.
//
// The reference draws a downscale factor per image, resizes with Image.BICUBIC and cuts one crop, once,
// offline, on the host (preprocess.py:23-33).  Pillow's 8-bit resize is integer arithmetic on integer
// coefficients (22 fractional bits), the coefficients being rounded from IEEE doubles, so the device result
// equals Pillow's byte for byte: include/lic.h holds the definition this file implements.
//
// A workgroup of 256 threads owns one RS_TH x RS_TW tile of one output image:
//   1. wave 0 computes the tile's column coefficients (first tap, tap count, <= 9 integer taps), wave 1 its row
//      coefficients, in fp64 with every operation rounded on its own, into LDS;
//   2. horizontal pass: a thread owns one (column, channel) of the tile, keeps that column's taps in registers
//      and walks the source rows the tile's output rows read (<= RS_ROWS), writing uint8 into LDS;
//   3. vertical pass: a wave owns every 4th output row (its taps are wave-uniform LDS broadcasts), a lane 4
//      consecutive floats of it, placed so that the lane's global address is 16-byte aligned whatever the row
//      length: one 16-byte store per lane, scalar stores only for a row's unaligned head and tail.
// An axis that is not resized (n_out == n_in, or a size outside the supported range in a table the host did
// not validate) is one tap of weight 2^22 on the clamped coordinate: the same passes copy it.
//
// Like lic_window.hip, every source index is resolved to an in-range index before any load: first taps are
// clamped into [0, n_in), tap counts into [0, min(9, n_in - first)], LDS row indices into [0, RS_ROWS), so no
// address leaves an image's [src_offset, src_offset + Hs*Ws*C) whatever the table holds.
#include "lic_common.h"

// Pillow's coefficients are products and sums of doubles each rounded on its own; a fused multiply-add
// changes a coefficient by one count in rare cases.
#pragma clang fp contract(off)

namespace {

constexpr int RS_TH = 32;                       // tile rows
constexpr int RS_TW = 64;                       // tile columns
constexpr int RS_MAXC = 4;                      // channels the LDS row holds
constexpr int RS_TAPS = 9;                      // downscale by at most 2: support 4, at most 9 taps
constexpr int RS_ROWS = 72;                     // source rows of a tile: (RS_TH - 1) * 2 + 2 * 4 + 1 = 71
constexpr int RS_LD = RS_TW * RS_MAXC;          // bytes per LDS row
constexpr int RS_ONE = 1 << 22;                 // PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ double rs_bicubic(double t) {  // a = -0.5
  const double a = -0.5;
  if (t < 0.0) t = -t;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}

// taps of output sample `xx` of an axis resized from n_in to n_out samples: k[0..cnt) on source samples
// first .. first + cnt - 1, all in [0, n_in)
__device__ __forceinline__ void rs_coef(long long xx, int n_in, int n_out, int* __restrict__ k, int& first, int& cnt) {
  n_in = max(n_in, 1);
#pragma unroll
  for (int x = 0; x < RS_TAPS; ++x) k[x] = 0;
  if (!(n_out >= 1 && n_out < n_in && 2LL * n_out >= n_in)) {  // copied axis (and every size outside the range)
    first = (int)min(max(xx, 0LL), (long long)n_in - 1);
    cnt = 1;
    k[0] = RS_ONE;
    return;
  }
  const double scale = (double)n_in / (double)n_out;  // > 1: filterscale
  const double support = 2.0 * scale, ss = 1.0 / scale;
  const double center = ((double)xx + 0.5) * scale;
  // (the bounds only keep the conversion defined for a window the host did not validate)
  const double lo = fmin(fmax(center - support + 0.5, -2.0e9), 2.0e9);
  const double hi = fmin(fmax(center + support + 0.5, -2.0e9), 2.0e9);
  int xmin = max(0, (int)lo);
  int xmax = min(n_in, (int)hi) - xmin;
  xmin = min(xmin, n_in - 1);
  xmax = min(max(xmax, 0), min(RS_TAPS, n_in - xmin));
  double wt[RS_TAPS];
  double ww = 0.0;
#pragma unroll
  for (int x = 0; x < RS_TAPS; ++x) {
    wt[x] = x < xmax ? rs_bicubic(((double)(x + xmin) - center + 0.5) * ss) : 0.0;
    if (x < xmax) ww = ww + wt[x];
  }
#pragma unroll
  for (int x = 0; x < RS_TAPS; ++x) {
    double v = wt[x];
    if (ww != 0.0) v = v / ww;
    k[x] = x < xmax ? (int)(v * 4194304.0 + (v < 0.0 ? -0.5 : 0.5)) : 0;
  }
  first = xmin;
  cnt = xmax;
}

__device__ __forceinline__ int rs_clip8(int acc) { return min(max(acc >> 22, 0), 255); }

__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ pool,
                                                          const lic_resample_job* __restrict__ jobs, int h, int w, int C,
                                                          int tiles_x, int tiles_per_image, float* __restrict__ out) {
  __shared__ int s_ck[RS_TW * RS_TAPS], s_cfirst[RS_TW], s_ccnt[RS_TW];
  __shared__ int s_rk[RS_TH * RS_TAPS], s_rfirst[RS_TH], s_rcnt[RS_TH];
  __shared__ __attribute__((aligned(16))) uint8_t s_mid[RS_ROWS * RS_LD];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles_per_image, tile = blockIdx.x - b * tiles_per_image;
  const int ty0 = (tile / tiles_x) * RS_TH, tx0 = (tile % tiles_x) * RS_TW;
  const int th = min(RS_TH, h - ty0), tw = min(RS_TW, w - tx0);
  const lic_resample_job j = jobs[b];
  const int Hs = max(j.Hs, 1), Ws = max(j.Ws, 1);

  // 1. coefficients: wave 0 the columns, wave 1 the rows
  if (tid < RS_TW) {
    const int ox = tx0 + min(tid, tw - 1);
    const int oxf = (j.flags & 1) ? w - 1 - ox : ox;
    int k[RS_TAPS], first, cnt;
    rs_coef((long long)j.x0 + oxf, Ws, j.Wn, k, first, cnt);
#pragma unroll
    for (int t = 0; t < RS_TAPS; ++t) s_ck[tid * RS_TAPS + t] = k[t];
    s_cfirst[tid] = first;
    s_ccnt[tid] = cnt;
  } else if (tid < RS_TW + RS_TH) {
    const int r = tid - RS_TW;
    int k[RS_TAPS], first, cnt;
    rs_coef((long long)j.y0 + ty0 + min(r, th - 1), Hs, j.Hn, k, first, cnt);
#pragma unroll
    for (int t = 0; t < RS_TAPS; ++t) s_rk[r * RS_TAPS + t] = k[t];
    s_rfirst[r] = first;
    s_rcnt[r] = cnt;
  }
  __syncthreads();

  // the source rows this tile reads: first taps and ends are nondecreasing in the output row
  const int row0 = s_rfirst[0];
  const int nrows = min(max(s_rfirst[th - 1] + s_rcnt[th - 1] - row0, 0), RS_ROWS);
  const int ne = tw * C;                                              // floats per tile row
  const uint8_t* img = pool + j.src_offset;

  // 2. horizontal pass, uint8 -> uint8 in LDS
  if (tid < ne) {
    const int col = tid / C, c = tid - col * C;
    int k[RS_TAPS];
#pragma unroll
    for (int t = 0; t < RS_TAPS; ++t) k[t] = s_ck[col * RS_TAPS + t];
    const int cnt = s_ccnt[col];
    const uint8_t* p = img + ((long)row0 * Ws + s_cfirst[col]) * C + c;
    for (int r = 0; r < nrows; ++r, p += (long)Ws * C) {
      int acc = 1 << 21;
#pragma unroll
      for (int t = 0; t < RS_TAPS; ++t)
        if (t < cnt) acc += (int)p[t * C] * k[t];
      s_mid[r * RS_LD + tid] = (uint8_t)rs_clip8(acc);
    }
  }
  __syncthreads();

  // 3. vertical pass and store: wave `wv` owns rows wv, wv + 4, ...; lane q owns floats [4q - a, 4q - a + 4)
  //    of the row, a = the row start's misalignment in floats, so that its address is 16-byte aligned
  const int wv = tid >> 6, lane = tid & 63;
  for (int oy = wv; oy < th; oy += 4) {
    const long rowstart = (((long)b * h + ty0 + oy) * w + tx0) * C;
    float* orow = out + rowstart;
    const int a = (int)(rowstart & 3);
    const int cnt = s_rcnt[oy];
    const int rel0 = s_rfirst[oy] - row0;
    int kr[RS_TAPS];
#pragma unroll
    for (int t = 0; t < RS_TAPS; ++t) kr[t] = s_rk[oy * RS_TAPS + t];
    for (int e0 = 4 * lane - a; e0 < ne; e0 += 256) {
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      int ecl[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ecl[i] = min(max(e0 + i, 0), ne - 1);
#pragma unroll
      for (int t = 0; t < RS_TAPS; ++t) {
        if (t < cnt) {
          const uint8_t* m = s_mid + min(max(rel0 + t, 0), RS_ROWS - 1) * RS_LD;
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] += (int)m[ecl[i]] * kr[t];
        }
      }
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (float)rs_clip8(acc[i]) / 255.0f;  // lic_u8_to_f32's division
      if (e0 >= 0 && e0 + 3 < ne) {
        *reinterpret_cast<f32x4*>(orow + e0) = o;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (e0 + i >= 0 && e0 + i < ne) orow[e0 + i] = o[i];
      }
    }
  }
}

}  // namespace

LIC_EXPORT int lic_resample_u8_to_f32(const uint8_t* pool, const lic_resample_job* jobs_device, int32_t B, int32_t h,
                                      int32_t w, int32_t C, float* out, lic_stream_t stream) {
  if (!pool || !jobs_device || !out || B <= 0 || h <= 0 || w <= 0 || C <= 0) return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(jobs_device) & 7) return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(out) & 15) return LIC_ERR_INVALID;
  if (C > RS_MAXC) return LIC_ERR_UNSUPPORTED;
  if ((int64_t)B * h * w * C > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
  const int tiles_x = (w + RS_TW - 1) / RS_TW, tiles_y = (h + RS_TH - 1) / RS_TH;
  const int64_t blocks = (int64_t)B * tiles_x * tiles_y;
  if (blocks > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(resample_u8_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, pool, jobs_device,
                     h, w, C, tiles_x, tiles_x * tiles_y, out);
  return lic_check_launch();
}
