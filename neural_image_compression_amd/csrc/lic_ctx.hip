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
//
// lic_ctx_gather_ragged: the same rows for pixels of DIFFERENT images in one launch (codec.ContextCodec.decompress_images:
// step t of many bitstreams at once).  Every row names its image and its pixel; an image's geometry (plane base, row
// pitch, origin, psi base, h, w, R) comes from a device table of LIC_CTX_IMAGE_WORDS int64 per image, which the kernel
// checks against the buffers' lengths before it addresses anything: a descriptor that fails, like a bad image or pixel
// index, gives a row of zeros and no read.  The 16-byte kernel moves a row float by float when its image's bases are
// not multiples of 4 floats: the same bytes either way.
//
// lic_ctx_gather_layers / lic_ctx_gather_layers_ragged: the two launches above for a latent whose channels are split
// into layers (codec.ScalableCodec), every layer's rows in one launch; both at the end of this file.
#include "lic_common.h"

namespace {

// What the walk of one row reads and writes, whichever launch names the row; comb is null and Cpsi 0 without psi
struct CtxRowParams {
  const float* y;
  const int32_t* taps;
  const float* psi;
  float* win;
  float* comb;
  int64_t y_pix, comb_ld;
  int32_t M, nt, Cpsi;
};

// The plane a row's pixel lies in: built from the launch's uniform geometry in ctx_gather_kernel, read from the image's
// descriptor in ctx_gather_ragged_kernel
struct CtxImage {
  int64_t y_base, y_row, y_origin, psi_base, h, w, R;
};

// one row in pieces of V floats (4: 16-byte moves, 1: element by element); `ok` false: zeros, nothing read
template <int V>
__device__ __forceinline__ void ctx_row(const CtxRowParams& p, int64_t row, bool ok, const CtxImage& g, int64_t px) {
  typedef float piece __attribute__((ext_vector_type(V)));
  const int Mq = p.M / V, Cq = p.psi ? p.Cpsi / V : 0;
  const int nwin = p.nt * Mq, per_row = nwin + Cq;
  const int h = ok ? (int)g.h : 1, w = ok ? (int)g.w : 1;
  const int i = ok ? (int)(px / w) : 0, j = ok ? (int)(px - (int64_t)i * w) : 0;
  const int64_t ri = ok ? i % g.R : 0;  // row inside the pixel's slice
  const float* yb = p.y + (ok ? g.y_base + g.y_origin : 0);
  float* wrow = p.win + row * ((int64_t)p.nt * p.M);
  for (int e = threadIdx.x; e < per_row; e += 256) {
    if (e < nwin) {
      const int t = e / Mq, c = (e - t * Mq) * V;
      const int dr = p.taps[2 * t], ds = p.taps[2 * t + 1];
      // 64 bits: a tap table with absurd offsets must not wrap back into the plane
      const int64_t si = (int64_t)i + dr, sj = (int64_t)j + ds;
      const bool live = ok && si >= 0 && si < h && sj >= 0 && sj < w && (dr >= 0 || ri + dr >= 0);
      piece v = {};
      if (live) v = *reinterpret_cast<const piece*>(yb + si * g.y_row + sj * p.y_pix + c);
      *reinterpret_cast<piece*>(wrow + (int64_t)e * V) = v;
    } else {
      const int c = (e - nwin) * V;
      piece v = {};
      if (ok) v = *reinterpret_cast<const piece*>(p.psi + g.psi_base + px * p.Cpsi + c);
      *reinterpret_cast<piece*>(p.comb + row * p.comb_ld + c) = v;
    }
  }
}

struct CtxGatherParams {
  CtxRowParams row;
  const int64_t* pix;
  int64_t y_batch, y_row, y_origin, n, rows;
  int32_t h, w, R;
};

// V as in ctx_row
template <int V>
__global__ __launch_bounds__(256) void ctx_gather_kernel(const CtxGatherParams p) {
  const int64_t hw = (int64_t)p.h * p.w;
  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t b = row / p.n, k = row - b * p.n;
    const int64_t px = p.pix[k];
    const CtxImage g{b * p.y_batch, p.y_row, p.y_origin, b * hw * p.row.Cpsi, p.h, p.w, p.R};
    ctx_row<V>(p.row, row, px >= 0 && px < hw, g, px);  // a bad index: zeros out, nothing in
  }
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// ---- rows of different images ------------------------------------------------------------------------------------
constexpr int64_t kMaxSide = 1 << 15;            // h, w of one latent plane: keeps every product below in 64 bits
constexpr int64_t kMaxFloats = (int64_t)1 << 40;  // y_len, psi_len

struct CtxRaggedParams {
  CtxRowParams row;
  const int64_t* images;
  const int64_t* row_image;
  const int64_t* row_pix;
  int64_t y_len, psi_len, rows;
  int32_t nimg;
};

// the descriptor of image b if every address it can produce lies inside y[0, y_len) and psi[0, psi_len)
__device__ __forceinline__ bool ctx_image(const CtxRaggedParams& p, int64_t b, CtxImage& g) {
  if (b < 0 || b >= p.nimg) return false;
  const int64_t* d = p.images + b * LIC_CTX_IMAGE_WORDS;
  g.y_base = d[LIC_CTX_IMAGE_Y_BASE];
  g.y_row = d[LIC_CTX_IMAGE_Y_ROW];
  g.y_origin = d[LIC_CTX_IMAGE_Y_ORIGIN];
  g.psi_base = d[LIC_CTX_IMAGE_PSI_BASE];
  g.h = d[LIC_CTX_IMAGE_H];
  g.w = d[LIC_CTX_IMAGE_W];
  g.R = d[LIC_CTX_IMAGE_R];
  if (g.h < 1 || g.h > kMaxSide || g.w < 1 || g.w > kMaxSide || g.R < 1) return false;
  if (g.y_base < 0 || g.y_base > p.y_len || g.y_row < 0 || g.y_row > p.y_len || g.y_origin < 0 || g.y_origin > p.y_len)
    return false;
  // the last float of the last pixel: every term is below 2^55
  if (g.y_base + g.y_origin + (g.h - 1) * g.y_row + (g.w - 1) * p.row.y_pix + p.row.M > p.y_len) return false;
  if (p.row.psi && (g.psi_base < 0 || g.psi_base > p.psi_len || g.psi_base + g.h * g.w * p.row.Cpsi > p.psi_len))
    return false;
  return true;
}

// V as in ctx_row; with V = 4 a row whose image is not laid out in multiples of 4 floats goes by floats
template <int V>
__global__ __launch_bounds__(256) void ctx_gather_ragged_kernel(const CtxRaggedParams p) {
  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t b = p.row_image[row], px = p.row_pix[row];
    CtxImage g = {};
    const bool ok = ctx_image(p, b, g) && px >= 0 && px < g.h * g.w;
    if (V == 1 || (ok && ((g.y_base | g.y_row | g.y_origin | g.psi_base) & 3)))
      ctx_row<1>(p.row, row, ok, g, px);
    else
      ctx_row<V>(p.row, row, ok, g, px);
  }
}

// the fields both launches fill the same way
CtxRowParams ctx_row_params(const float* y, const int32_t* taps, const float* psi, float* win, float* comb,
                            int64_t y_pix, int64_t comb_ld, int32_t M, int32_t nt, int32_t Cpsi) {
  return CtxRowParams{y, taps, psi, win, psi ? comb : nullptr, y_pix, comb_ld, M, nt, psi ? Cpsi : 0};
}

// ---- the layers of one latent ------------------------------------------------------------------------------------
// Layer l is lic_ctx_gather on the channel range [c0, c0 + M): row[l].y points at channel c0 of the plane, row[l].M
// is the layer's width, y_pix stays the plane's.  vec bit l: the layer moves in 16-byte pieces.
struct CtxLayersParams {
  CtxRowParams row[LIC_MAX_LAYERS];
  const int64_t* pix;
  int64_t y_batch, y_row, y_origin, n, rows;
  int32_t h, w, R, L;
  uint32_t vec;
};

// one workgroup per row walks the row of every layer; the layer loop is unrolled so that the by-value table is read
// with constant indices
__global__ __launch_bounds__(256) void ctx_gather_layers_kernel(const CtxLayersParams p) {
  const int64_t hw = (int64_t)p.h * p.w;
  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t b = row / p.n, k = row - b * p.n;
    const int64_t px = p.pix[k];
    const bool ok = px >= 0 && px < hw;  // a bad index: zeros out, nothing in
#pragma unroll
    for (int l = 0; l < LIC_MAX_LAYERS; ++l) {
      if (l < p.L) {
        const CtxImage g{b * p.y_batch, p.y_row, p.y_origin, b * hw * p.row[l].Cpsi, p.h, p.w, p.R};
        if ((p.vec >> l) & 1u)
          ctx_row<4>(p.row[l], row, ok, g, px);
        else
          ctx_row<1>(p.row[l], row, ok, g, px);
      }
    }
  }
}

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
  p.row = ctx_row_params(y, taps, psi, win, comb, y_pix, comb_ld, M, nt, Cpsi);
  p.pix = pix;
  p.y_batch = y_batch;
  p.y_row = y_row;
  p.y_origin = y_origin;
  p.n = n;
  p.rows = (int64_t)B * n;
  p.h = h;
  p.w = w;
  p.R = slice_rows;
  const dim3 grid(ew_grid(p.rows, 1));
  if (can_vec && path != LIC_CTX_ELEMENT)
    hipLaunchKernelGGL(ctx_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(ctx_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
  return lic_check_launch();
}

LIC_EXPORT int lic_ctx_gather_ragged(const float* y, int64_t y_len, int64_t y_pix, const int64_t* images, int32_t nimg,
                                     int32_t M, const int32_t* taps, int32_t nt, const int64_t* row_image,
                                     const int64_t* row_pix, int64_t rows, float* win, const float* psi,
                                     int64_t psi_len, int32_t Cpsi, float* comb, int64_t comb_ld, int32_t path,
                                     lic_stream_t stream) {
  if (!y || !images || !taps || !row_image || !row_pix || !win) return LIC_ERR_INVALID;
  if (nimg <= 0 || M <= 0 || rows <= 0 || nt < 1 || y_len <= 0 || y_pix < M) return LIC_ERR_INVALID;
  if (psi && (!comb || Cpsi <= 0 || comb_ld < Cpsi || psi_len <= 0)) return LIC_ERR_INVALID;
  if (path != LIC_CTX_AUTO && path != LIC_CTX_VECTOR && path != LIC_CTX_ELEMENT) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(win) | reinterpret_cast<uintptr_t>(psi) |
       reinterpret_cast<uintptr_t>(comb) | reinterpret_cast<uintptr_t>(taps)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(row_image) |
       reinterpret_cast<uintptr_t>(row_pix)) & 7)
    return LIC_ERR_INVALID;
  if ((int64_t)nt * M + (psi ? Cpsi : 0) > 0x7FFFFFFFL - 256 || rows > (1LL << 40) || y_len > kMaxFloats ||
      y_pix > kMaxFloats || (psi && psi_len > kMaxFloats))
    return LIC_ERR_UNSUPPORTED;
  const bool can_vec = M % 4 == 0 && aligned16(y) && aligned16(win) && y_pix % 4 == 0 &&
                       (!psi || (Cpsi % 4 == 0 && comb_ld % 4 == 0 && aligned16(psi) && aligned16(comb)));
  if (path == LIC_CTX_VECTOR && !can_vec) return LIC_ERR_INVALID;
  CtxRaggedParams p;
  p.row = ctx_row_params(y, taps, psi, win, comb, y_pix, comb_ld, M, nt, Cpsi);
  p.images = images;
  p.row_image = row_image;
  p.row_pix = row_pix;
  p.y_len = y_len;
  p.psi_len = psi ? psi_len : 0;
  p.rows = rows;
  p.nimg = nimg;
  const dim3 grid(ew_grid(rows, 1));
  if (can_vec && path != LIC_CTX_ELEMENT)
    hipLaunchKernelGGL(ctx_gather_ragged_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(ctx_gather_ragged_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
  return lic_check_launch();
}

LIC_EXPORT int lic_ctx_gather_layers(const float* y, int64_t y_batch, int64_t y_row, int64_t y_pix, int64_t y_origin,
                                     int32_t B, int32_t h, int32_t w, const int32_t* taps, int32_t nt,
                                     int32_t slice_rows, const int64_t* pix, int64_t n, const float* psi, int32_t Cpsi,
                                     const lic_ctx_layer* layers, int32_t L, int32_t path, lic_stream_t stream) {
  if (!y || !taps || !pix || !layers) return LIC_ERR_INVALID;
  if (L < 1 || L > LIC_MAX_LAYERS) return LIC_ERR_INVALID;
  if (B <= 0 || h <= 0 || w <= 0 || n <= 0 || nt < 1 || slice_rows < 1) return LIC_ERR_INVALID;
  if (y_batch < 0 || y_row < 0 || y_pix < 1 || y_origin < 0) return LIC_ERR_INVALID;
  if (psi && Cpsi <= 0) return LIC_ERR_INVALID;
  if (path != LIC_CTX_AUTO && path != LIC_CTX_VECTOR && path != LIC_CTX_ELEMENT) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(psi) | reinterpret_cast<uintptr_t>(taps)) & 3)
    return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(pix) & 7) return LIC_ERR_INVALID;
  for (int l = 0; l < L; ++l) {
    const lic_ctx_layer& a = layers[l];
    if (!a.win || a.M <= 0 || a.c0 < 0 || (int64_t)a.c0 + a.M > y_pix) return LIC_ERR_INVALID;
    if (psi && (!a.comb || a.comb_ld < Cpsi)) return LIC_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a.win) | reinterpret_cast<uintptr_t>(a.comb)) & 3) return LIC_ERR_INVALID;
    for (int m = 0; m < l; ++m)  // channel ranges must not overlap
      if (a.c0 < layers[m].c0 + layers[m].M && layers[m].c0 < a.c0 + a.M) return LIC_ERR_INVALID;
  }
  // rows and row lengths the kernel's 32-bit piece counters and 64-bit offsets hold
  if (n > 0x7FFFFFFFL || (int64_t)B * n > (1LL << 40)) return LIC_ERR_UNSUPPORTED;
  for (int l = 0; l < L; ++l)
    if ((int64_t)nt * layers[l].M + (psi ? Cpsi : 0) > 0x7FFFFFFFL - 256) return LIC_ERR_UNSUPPORTED;
  const bool plane_vec = aligned16(y) && y_batch % 4 == 0 && y_row % 4 == 0 && y_pix % 4 == 0 && y_origin % 4 == 0 &&
                         (!psi || (Cpsi % 4 == 0 && aligned16(psi)));
  CtxLayersParams p = {};
  for (int l = 0; l < L; ++l) {
    const lic_ctx_layer& a = layers[l];
    const bool can_vec = plane_vec && a.c0 % 4 == 0 && a.M % 4 == 0 && aligned16(a.win) &&
                         (!psi || (a.comb_ld % 4 == 0 && aligned16(a.comb)));
    if (path == LIC_CTX_VECTOR && !can_vec) return LIC_ERR_INVALID;
    if (can_vec && path != LIC_CTX_ELEMENT) p.vec |= 1u << l;
    p.row[l] = ctx_row_params(y + a.c0, taps, psi, a.win, a.comb, y_pix, a.comb_ld, a.M, nt, Cpsi);
  }
  p.pix = pix;
  p.y_batch = y_batch;
  p.y_row = y_row;
  p.y_origin = y_origin;
  p.n = n;
  p.rows = (int64_t)B * n;
  p.h = h;
  p.w = w;
  p.R = slice_rows;
  p.L = L;
  hipLaunchKernelGGL(ctx_gather_layers_kernel, dim3(ew_grid(p.rows, 1)), dim3(256), 0, (hipStream_t)stream, p);
  return lic_check_launch();
}

// ---- the layers of one latent, rows of different images (lic_ctx_gather_layers_ragged, codec.ScalableCodec) ---------
// ctx_gather_ragged_kernel's row walk once per layer: `chk` is the launch lic_ctx_gather_ragged would be given for the
// whole plane -- its row.M is the widest c0 + M of the layers, so ctx_image passes a descriptor only if every layer's
// last float lies inside y -- and row[l] is the layer's own walk, row[l].y at channel c0 of the buffer's first float.
namespace {

struct CtxLayersRaggedParams {
  CtxRaggedParams chk;
  CtxRowParams row[LIC_MAX_LAYERS];
  int32_t L;
  uint32_t vec;
};

// one workgroup per row checks the row's image once and walks the row of every layer; unrolled as in
// ctx_gather_layers_kernel.  A layer in 16-byte pieces moves a row float by float when its image's bases are not
// multiples of 4 floats.
__global__ __launch_bounds__(256) void ctx_gather_layers_ragged_kernel(const CtxLayersRaggedParams p) {
  for (int64_t row = blockIdx.x; row < p.chk.rows; row += gridDim.x) {
    const int64_t b = p.chk.row_image[row], px = p.chk.row_pix[row];
    CtxImage g = {};
    const bool ok = ctx_image(p.chk, b, g) && px >= 0 && px < g.h * g.w;
    const bool by_float = ok && ((g.y_base | g.y_row | g.y_origin | g.psi_base) & 3);
#pragma unroll
    for (int l = 0; l < LIC_MAX_LAYERS; ++l) {
      if (l < p.L) {
        if (((p.vec >> l) & 1u) && !by_float)
          ctx_row<4>(p.row[l], row, ok, g, px);
        else
          ctx_row<1>(p.row[l], row, ok, g, px);
      }
    }
  }
}

}  // namespace

LIC_EXPORT int lic_ctx_gather_layers_ragged(const float* y, int64_t y_len, int64_t y_pix, const int64_t* images,
                                            int32_t nimg, const int32_t* taps, int32_t nt, const int64_t* row_image,
                                            const int64_t* row_pix, int64_t rows, const float* psi, int64_t psi_len,
                                            int32_t Cpsi, const lic_ctx_layer* layers, int32_t L, int32_t path,
                                            lic_stream_t stream) {
  if (!y || !images || !taps || !row_image || !row_pix || !layers) return LIC_ERR_INVALID;
  if (L < 1 || L > LIC_MAX_LAYERS) return LIC_ERR_INVALID;
  if (nimg <= 0 || rows <= 0 || nt < 1 || y_len <= 0 || y_pix < 1) return LIC_ERR_INVALID;
  if (psi && (Cpsi <= 0 || psi_len <= 0)) return LIC_ERR_INVALID;
  if (path != LIC_CTX_AUTO && path != LIC_CTX_VECTOR && path != LIC_CTX_ELEMENT) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(psi) | reinterpret_cast<uintptr_t>(taps)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(row_image) |
       reinterpret_cast<uintptr_t>(row_pix)) & 7)
    return LIC_ERR_INVALID;
  int32_t widest = 0;
  for (int l = 0; l < L; ++l) {
    const lic_ctx_layer& a = layers[l];
    if (!a.win || a.M <= 0 || a.c0 < 0 || (int64_t)a.c0 + a.M > y_pix) return LIC_ERR_INVALID;
    if (psi && (!a.comb || a.comb_ld < Cpsi)) return LIC_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a.win) | reinterpret_cast<uintptr_t>(a.comb)) & 3) return LIC_ERR_INVALID;
    for (int m = 0; m < l; ++m)  // channel ranges must not overlap
      if (a.c0 < layers[m].c0 + layers[m].M && layers[m].c0 < a.c0 + a.M) return LIC_ERR_INVALID;
    widest = a.c0 + a.M > widest ? a.c0 + a.M : widest;
  }
  // rows and row lengths the kernel's 32-bit piece counters and 64-bit offsets hold
  if (rows > (1LL << 40) || y_len > kMaxFloats || y_pix > kMaxFloats || (psi && psi_len > kMaxFloats))
    return LIC_ERR_UNSUPPORTED;
  for (int l = 0; l < L; ++l)
    if ((int64_t)nt * layers[l].M + (psi ? Cpsi : 0) > 0x7FFFFFFFL - 256) return LIC_ERR_UNSUPPORTED;
  const bool plane_vec = aligned16(y) && y_pix % 4 == 0 && (!psi || (Cpsi % 4 == 0 && aligned16(psi)));
  CtxLayersRaggedParams p = {};
  for (int l = 0; l < L; ++l) {
    const lic_ctx_layer& a = layers[l];
    const bool can_vec = plane_vec && a.c0 % 4 == 0 && a.M % 4 == 0 && aligned16(a.win) &&
                         (!psi || (a.comb_ld % 4 == 0 && aligned16(a.comb)));
    if (path == LIC_CTX_VECTOR && !can_vec) return LIC_ERR_INVALID;
    if (can_vec && path != LIC_CTX_ELEMENT) p.vec |= 1u << l;
    p.row[l] = ctx_row_params(y + a.c0, taps, psi, a.win, a.comb, y_pix, a.comb_ld, a.M, nt, Cpsi);
  }
  // what ctx_image reads: y_pix, the widest channel end as M, psi and Cpsi; it writes nothing
  p.chk.row = ctx_row_params(y, taps, psi, nullptr, nullptr, y_pix, 0, widest, nt, Cpsi);
  p.chk.images = images;
  p.chk.row_image = row_image;
  p.chk.row_pix = row_pix;
  p.chk.y_len = y_len;
  p.chk.psi_len = psi ? psi_len : 0;
  p.chk.rows = rows;
  p.chk.nimg = nimg;
  p.L = L;
  hipLaunchKernelGGL(ctx_gather_layers_ragged_kernel, dim3(ew_grid(rows, 1)), dim3(256), 0, (hipStream_t)stream, p);
  return lic_check_launch();
}
