// lic_window: a window of an image with a rule for what lies outside it -- crop and pad as ONE gather.
//
// The reference crops on the host, once, offline (preprocess.py:30-32: one fixed 256x256 window per source
// image) and converts with ToTensor() per item (Dataloader.py:23-27, 39-43).  Here a pool of uint8 [Hs][Ws][C]
// images of any size stays resident in HBM and a training batch is one launch over a 32-byte-per-image job
// table: out[b, oy, ox, c] = float(src_b(border(y0 + oy), border(x0 + ox'), c)) / 255 with ox' = w-1-ox when
// the job's flip bit is set.  The same rule over strided fp32 (lic_window_f32) pads an evaluation image to
// the multiple of 64 the model needs and crops the reconstruction back.
//
// HBM-bound, shaped like lic_elementwise.hip: grid-stride, <= 2048 blocks, a lane owns 4 consecutive output
// floats and stores 16 bytes.  Within an output row the source bytes of an interior, unflipped run are
// consecutive too ((x0 + ox) * C + c = x0 * C + r for the row offset r), so such a run is read with the widest
// aligned loads its byte address allows (rows start at arbitrary byte offsets: 3 * Ws is odd for odd widths).
// Everything else -- border, flipped, row-crossing and tail elements -- resolves each coordinate to an
// in-range index plus a keep/zero flag BEFORE the load and selects afterwards: no load is conditional and no
// address leaves [src_offset, src_offset + Hs*Ws*C).
#include "lic_common.h"

namespace {

// border rule for one coordinate of a side of n >= 1 samples: in-range index, and whether the sample is kept
// (border 0 zeroes what lies outside).  Reflect is torch's 'reflect' (edge not repeated); its result is
// clamped as well, so a table the host did not validate still cannot leave the image.
__device__ __forceinline__ int win_resolve(int v, int n, int border, bool& keep) {
  const bool inside = v >= 0 && v < n;
  keep = inside || border != LIC_WINDOW_ZERO;
  if (border == LIC_WINDOW_REFLECT) v = v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v);
  return min(max(v, 0), n - 1);
}

__device__ __forceinline__ float win_u8(uint32_t v) { return (float)v / 255.0f; }  // lic_u8_to_f32's division

__global__ __launch_bounds__(256) void window_u8_kernel(const uint8_t* __restrict__ pool,
                                                        const lic_window_job* __restrict__ jobs, uint32_t total,
                                                        uint32_t per_image, uint32_t rowlen, int w, int C, int border,
                                                        float* __restrict__ out) {
  const uint32_t nquad = (total + 3) >> 2;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < nquad; q += gridDim.x * 256u) {
    const uint32_t e0 = q << 2;
    const uint32_t b = e0 / per_image, rem = e0 - b * per_image;
    const uint32_t oy = rem / rowlen, r = rem - oy * rowlen;
    const lic_window_job j = jobs[b];
    const uint8_t* img = pool + j.src_offset;
    const int y = j.y0 + (int)oy;
    const long xs = (long)j.x0 * C + (long)r;                          // source row offset of this run, if interior
    f32x4 o;
    if (e0 + 3 < total && r + 3 < rowlen && !(j.flags & 1) && y >= 0 && y < j.Hs && xs >= 0 &&
        xs + 3 < (long)j.Ws * C) {
      const uint8_t* p = img + (long)y * j.Ws * C + xs;
      const uintptr_t a = reinterpret_cast<uintptr_t>(p);
      uint32_t v;
      if ((a & 3) == 0) {
        v = *reinterpret_cast<const uint32_t*>(p);
      } else if ((a & 1) == 0) {
        v = (uint32_t) * reinterpret_cast<const uint16_t*>(p) | ((uint32_t) * reinterpret_cast<const uint16_t*>(p + 2) << 16);
      } else {
        v = (uint32_t)p[0] | ((uint32_t) * reinterpret_cast<const uint16_t*>(p + 1) << 8) | ((uint32_t)p[3] << 24);
      }
      o = f32x4{win_u8(v & 255u), win_u8((v >> 8) & 255u), win_u8((v >> 16) & 255u), win_u8(v >> 24)};
      *reinterpret_cast<f32x4*>(out + e0) = o;
      continue;
    }
    // general path: the 4 elements may cross a row or an image; each resolves its own coordinates
    lic_window_job jj = j;
    uint32_t bb = b, yy = oy, rr = r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // (elements past `total` repeat the last valid one: their loads stay in range and they are not stored)
      const bool live = e0 + e < total;
      if (e > 0 && live) {
        if (++rr == rowlen) {
          rr = 0;
          if ((++yy) * rowlen == per_image) {
            yy = 0;
            jj = jobs[++bb];
          }
        }
      }
      const int ox = (int)(rr / (uint32_t)C), c = (int)(rr - (uint32_t)ox * C);
      const int oxf = (jj.flags & 1) ? w - 1 - ox : ox;
      bool ky, kx;
      const int sy = win_resolve(jj.y0 + (int)yy, jj.Hs, border, ky);
      const int sx = win_resolve(jj.x0 + oxf, jj.Ws, border, kx);
      const uint8_t v = pool[jj.src_offset + ((long)sy * jj.Ws + sx) * C + c];
      o[e] = (ky && kx) ? win_u8(v) : 0.0f;
    }
    if (e0 + 3 < total) {
      *reinterpret_cast<f32x4*>(out + e0) = o;
    } else {
      for (int e = 0; e < 4; ++e)
        if (e0 + e < total) out[e0 + e] = o[e];
    }
  }
}

// strided fp32 source, one window for the whole batch.  Always the clamped-index + select path: the source
// may be NCHW-contiguous (a lane's 4 floats are then C-strided gathers), channels_last or a view of either.
__global__ __launch_bounds__(256) void window_f32_kernel(const float* __restrict__ src, long sb, long sc, long sh,
                                                         long sw, uint32_t total, uint32_t per_image,
                                                         uint32_t rowlen, int C, int Hs, int Ws, int y0, int x0,
                                                         int border, float* __restrict__ out) {
  const uint32_t nquad = (total + 3) >> 2;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < nquad; q += gridDim.x * 256u) {
    const uint32_t e0 = q << 2;
    uint32_t b = e0 / per_image;
    const uint32_t rem = e0 - b * per_image;
    uint32_t oy = rem / rowlen, r = rem - oy * rowlen;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e > 0 && e0 + e < total) {
        if (++r == rowlen) {
          r = 0;
          if ((++oy) * rowlen == per_image) {
            oy = 0;
            ++b;
          }
        }
      }
      const int ox = (int)(r / (uint32_t)C), c = (int)(r - (uint32_t)ox * C);
      bool ky, kx;
      const int sy = win_resolve(y0 + (int)oy, Hs, border, ky);
      const int sx = win_resolve(x0 + ox, Ws, border, kx);
      const float v = src[(long)b * sb + (long)c * sc + (long)sy * sh + (long)sx * sw];
      o[e] = (ky && kx) ? v : 0.0f;
    }
    if (e0 + 3 < total) {
      *reinterpret_cast<f32x4*>(out + e0) = o;
    } else {
      for (int e = 0; e < 4; ++e)
        if (e0 + e < total) out[e0 + e] = o[e];
    }
  }
}

// output geometry shared by both entries: [B][h][w][C] fp32 of at most 2^31 - 1 elements (32-bit index math)
int win_geometry(int32_t B, int32_t h, int32_t w, int32_t C, int32_t border, const float* out, uint32_t* total,
                 uint32_t* per_image, uint32_t* rowlen) {
  if (!out || B <= 0 || h <= 0 || w <= 0 || C <= 0) return LIC_ERR_INVALID;
  if (border != LIC_WINDOW_ZERO && border != LIC_WINDOW_REPLICATE && border != LIC_WINDOW_REFLECT) return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(out) & 15) return LIC_ERR_INVALID;
  const int64_t row = (int64_t)w * C, img = row * h, all = img * B;
  if (all > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
  *total = (uint32_t)all;
  *per_image = (uint32_t)img;
  *rowlen = (uint32_t)row;
  return LIC_OK;
}

}  // namespace

LIC_EXPORT int lic_window_u8_to_f32(const uint8_t* pool, const lic_window_job* jobs_device, int32_t B, int32_t h,
                                    int32_t w, int32_t C, int32_t border, float* out, lic_stream_t stream) {
  if (!pool || !jobs_device) return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(jobs_device) & 7) return LIC_ERR_INVALID;
  uint32_t total, per_image, rowlen;
  const int rc = win_geometry(B, h, w, C, border, out, &total, &per_image, &rowlen);
  if (rc != LIC_OK) return rc;
  hipLaunchKernelGGL(window_u8_kernel, dim3(ew_grid(((int64_t)total + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     pool, jobs_device, total, per_image, rowlen, w, C, border, out);
  return lic_check_launch();
}

LIC_EXPORT int lic_window_f32(const float* src, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B, int32_t C,
                              int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t h, int32_t w, int32_t border,
                              float* out, lic_stream_t stream) {
  if (!src || Hs <= 0 || Ws <= 0 || sb < 0 || sc < 0 || sh < 0 || sw < 0) return LIC_ERR_INVALID;
  uint32_t total, per_image, rowlen;
  const int rc = win_geometry(B, h, w, C, border, out, &total, &per_image, &rowlen);
  if (rc != LIC_OK) return rc;
  if (border == LIC_WINDOW_REFLECT) {
    // overhang on each side; torch's 'reflect' needs every one smaller than the side it reflects about
    const int64_t top = -(int64_t)y0, bottom = (int64_t)y0 + h - Hs, left = -(int64_t)x0, right = (int64_t)x0 + w - Ws;
    if (top >= Hs || bottom >= Hs || left >= Ws || right >= Ws) return LIC_ERR_INVALID;
  }
  hipLaunchKernelGGL(window_f32_kernel, dim3(ew_grid(((int64_t)total + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     src, (long)sb, (long)sc, (long)sh, (long)sw, total, per_image, rowlen, C, Hs, Ws, y0, x0, border,
                     out);
  return lic_check_launch();
}
