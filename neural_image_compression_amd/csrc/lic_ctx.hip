// lic_ctx_gather: the rows the per-pixel context GEMM and entropy-parameter MLP of codec.ContextCodec read, in one
// launch.  For each listed latent pixel (i, j) of each image it writes
//   win[row][t*M + c]    = y_hat[i + dr_t, j + ds_t, c]  for the live taps t of the masked convolution
//                          (ContextModels.py:18-20), zero where the tap leaves the image or the pixel's slice;
//   comb[row][c]         = psi[pixel][c], the hyper-decoder's columns of the `cat` of Models.py:73 (optional),
// row = b * n + k for entry k of the list.  The slice rule: a tap with dr < 0 is live only if
// (i mod R) + dr >= 0, so no context crosses a boundary between bands of R latent rows.
//
// Pure data movement: one workgroup per output row, grid-stride over rows; inside a row the 256 lanes walk the
// tap-major pieces, so consecutive lanes read consecutive addresses of one source pixel and write consecutive
// addresses of the row -- 16 bytes per lane when M, Cpsi and every base and pitch allow it, one float otherwise.
// Both paths write the same bytes.  Every address is decided from (i, j, dr, ds, R, h, w) before the load: nothing
// outside the h x w pixels of the plane is read, whatever surrounds them, and a pixel index outside [0, h*w) reads
// nothing and writes a row of zeros.
#include "lic_common.h"

namespace {

struct CtxGatherParams {
  const float* y;
  const int32_t* taps;
  const int64_t* pix;
  const float* psi;
  float* win;
  float* comb;
  int64_t y_batch, y_row, y_pix, y_origin, comb_ld, n, rows;
  int32_t h, w, M, nt, R, Cpsi;
};

// V: floats per piece (4: 16-byte moves, 1: element by element)
template <int V>
__global__ __launch_bounds__(256) void ctx_gather_kernel(const CtxGatherParams p) {
  typedef float piece __attribute__((ext_vector_type(V)));
  const int Mq = p.M / V, Cq = p.psi ? p.Cpsi / V : 0;
  const int nwin = p.nt * Mq, per_row = nwin + Cq;
  const int64_t hw = (int64_t)p.h * p.w;
  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t b = row / p.n, k = row - b * p.n;
    const int64_t px = p.pix[k];
    const bool ok = px >= 0 && px < hw;  // a bad index: zeros out, nothing in
    const int i = ok ? (int)(px / p.w) : 0, j = ok ? (int)(px - (int64_t)i * p.w) : 0;
    const int ri = i % p.R;  // row inside the pixel's slice
    const float* yb = p.y + b * p.y_batch + p.y_origin;
    float* wrow = p.win + row * ((int64_t)p.nt * p.M);
    for (int e = threadIdx.x; e < per_row; e += 256) {
      if (e < nwin) {
        const int t = e / Mq, c = (e - t * Mq) * V;
        const int dr = p.taps[2 * t], ds = p.taps[2 * t + 1];
        const int si = i + dr, sj = j + ds;
        const bool live = ok && si >= 0 && si < p.h && sj >= 0 && sj < p.w && (dr >= 0 || ri + dr >= 0);
        piece v = {};
        if (live) v = *reinterpret_cast<const piece*>(yb + si * p.y_row + sj * p.y_pix + c);
        *reinterpret_cast<piece*>(wrow + (int64_t)e * V) = v;
      } else {
        const int c = (e - nwin) * V;
        piece v = {};
        if (ok) v = *reinterpret_cast<const piece*>(p.psi + (b * hw + px) * p.Cpsi + c);
        *reinterpret_cast<piece*>(p.comb + row * p.comb_ld + c) = v;
      }
    }
  }
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

LIC_EXPORT int lic_ctx_gather(const float* y, int64_t y_batch, int64_t y_row, int64_t y_pix, int64_t y_origin,
                              int32_t B, int32_t h, int32_t w, int32_t M, const int32_t* taps, int32_t nt,
                              int32_t slice_rows, const int64_t* pix, int64_t n, float* win, const float* psi,
                              int32_t Cpsi, float* comb, int64_t comb_ld, int32_t path, lic_stream_t stream) {
  if (!y || !taps || !pix || !win) return LIC_ERR_INVALID;
  if (B <= 0 || h <= 0 || w <= 0 || M <= 0 || n <= 0 || nt < 1 || slice_rows < 1) return LIC_ERR_INVALID;
  if (y_batch < 0 || y_row < 0 || y_pix < M || y_origin < 0) return LIC_ERR_INVALID;
  if (psi && (!comb || Cpsi <= 0 || comb_ld < Cpsi)) return LIC_ERR_INVALID;
  if (path != LIC_CTX_AUTO && path != LIC_CTX_VECTOR && path != LIC_CTX_ELEMENT) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(win) | reinterpret_cast<uintptr_t>(psi) |
       reinterpret_cast<uintptr_t>(comb) | reinterpret_cast<uintptr_t>(taps)) & 3)
    return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(pix) & 7) return LIC_ERR_INVALID;
  // rows and row lengths the kernel's 32-bit piece counters and 64-bit offsets hold
  if ((int64_t)nt * M + (psi ? Cpsi : 0) > 0x7FFFFFFFL - 256 || n > 0x7FFFFFFFL || (int64_t)B * n > (1LL << 40))
    return LIC_ERR_UNSUPPORTED;
  const bool can_vec = M % 4 == 0 && aligned16(y) && aligned16(win) && y_batch % 4 == 0 && y_row % 4 == 0 &&
                       y_pix % 4 == 0 && y_origin % 4 == 0 &&
                       (!psi || (Cpsi % 4 == 0 && comb_ld % 4 == 0 && aligned16(psi) && aligned16(comb)));
  if (path == LIC_CTX_VECTOR && !can_vec) return LIC_ERR_INVALID;
  CtxGatherParams p;
  p.y = y;
  p.taps = taps;
  p.pix = pix;
  p.psi = psi;
  p.win = win;
  p.comb = psi ? comb : nullptr;
  p.y_batch = y_batch;
  p.y_row = y_row;
  p.y_pix = y_pix;
  p.y_origin = y_origin;
  p.comb_ld = comb_ld;
  p.n = n;
  p.rows = (int64_t)B * n;
  p.h = h;
  p.w = w;
  p.M = M;
  p.nt = nt;
  p.R = slice_rows;
  p.Cpsi = psi ? Cpsi : 0;
  const dim3 grid(ew_grid(p.rows, 1));
  if (can_vec && path != LIC_CTX_ELEMENT)
    hipLaunchKernelGGL(ctx_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(ctx_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
  return lic_check_launch();
}
