// lic_rans_decode_step / lic_rans_decode_step_groups: one wavefront step of the "rANS-64" and "rANS-64 x G" y
// streams (include/lic_codec.h) decoded where the tables are built, so codec.ContextCodec's step loop needs no copy
// to the host, no synchronisation and no host arithmetic.
//
// One wave per (image, group), each a workgroup of its own with its own LDS rows: lane l owns coder state l of the
// block, and the wave of group g decodes rounds g, g + G, ... of the step (G = 1: one wave per image, every round).  A round decodes 64 symbols: each lane searches its own table
// row for the 16-bit slot of its state, updates the state, and the lanes that fell below 2^16 share the stream
// with one ballot (who needs a word), one popcount (rank among them) and a wave-uniform cursor.
//
// Latency, not bandwidth, paces this kernel, so every global load is issued ahead of its use:
//  * a round's 64 table rows are contiguous (64 * (S+1) * 4 bytes); they are fetched with 16-byte loads into
//    registers one round ahead (the tables do not depend on what this step decodes) and dropped into LDS after the
//    current round has been searched;
//  * the next 64 stream words (a round consumes at most 64) are loaded at the start of the round, one per lane,
//    and a needing lane takes the word of lane `rank` by shuffle: no load depends on the search;
//  * centres and destination indices depend on the symbol number only.
// LDS row stride is S+2 dwords: S+1 = 2W+2 is even, and with an even stride the 64 lanes' first probe (the same
// column of 64 rows) would land on 16 of ds_read_b32's 32 banks; an odd stride spreads a 32-lane group over all 32.
// With that stride element `rel` of the round (row rel / (S+1)) sits at LDS dword rel + row.
//
// lic_rans_decode_step_ragged is that step for images that contribute different numbers of rows, or none, to the launch
// (rans_step_ragged_kernel below).  lic_rans_decode_step_layers and lic_rans_decode_step_layers_ragged are the two
// steps for the L layers of a latent, all layers' waves in one launch (the last two kernels of this file).
//
// Nothing outside the given buffers is ever read: a word or escape is read only after cursor + rank has been
// compared with the block's length; otherwise the block's error word is set and every later symbol of the block
// decodes as its table centre.  Destination indices outside [0, pixels) are not written and set the error word too.
#include "lic_common.h"

namespace {

constexpr int kLanes = 64;
constexpr int kStateWords = LIC_RANS_STATE_WORDS;

// NQ: 16-byte table pieces a lane holds for one round; S1MAX: largest S+1 that fits; kGrouped == false: one group,
// G is the constant 1 and the code is the one-wave-per-image kernel it always was
template <int NQ, int S1MAX, bool kGrouped>
__global__ __launch_bounds__(64) void rans_step_kernel(const uint8_t* __restrict__ streams,
                                                       const int64_t* __restrict__ stream_off,
                                                       const int64_t* __restrict__ stream_bytes,
                                                       const uint32_t* __restrict__ escapes,
                                                       const int64_t* __restrict__ esc_off, uint32_t* state,
                                                       const uint32_t* __restrict__ tables,
                                                       const int32_t* __restrict__ center, int32_t groups, int32_t nsym,
                                                       int32_t M, int32_t W, const int64_t* __restrict__ dest,
                                                       float* ypad, int64_t pixels, int64_t total_dwords) {
  __shared__ uint32_t lds[kLanes * (S1MAX + 1)];
  // blk: the state block, stream and escape list of (image b, group g); tables, centres and ypad go by image
  const int G = kGrouped ? groups : 1;
  const int blk = blockIdx.x, b = blk / G, g = blk - b * G, lane = threadIdx.x;
  const int rounds = (nsym + kLanes - 1) / kLanes;
  if (g >= rounds) return;  // no round of this step is this group's: the state block stays as it is
  const int S1 = 2 * W + 2, S = S1 - 1, stride = S1 + 1;
  const uint32_t inv = ((1u << 24) + S1 - 1) / S1;  // rel / S1 == (rel * inv) >> 24 for rel < 64 * S1 <= 2^14

  uint32_t* st = state + (size_t)blk * kStateWords;
  uint32_t x = st[lane];
  uint32_t ptr = st[kLanes], eptr = st[kLanes + 1], err = st[kLanes + 2];
  const int64_t o0 = stream_off[blk], room = stream_off[blk + 1] - o0;
  int64_t len = stream_bytes[blk];
  if (len > room || len < kLanes * 4 || o0 < 0) {
    err |= LIC_RANS_ERR_STREAM;
    len = kLanes * 4;
  }
  const uint16_t* words = reinterpret_cast<const uint16_t*>(streams + (o0 < 0 ? 0 : o0) + kLanes * 4);
  const uint64_t nwords = (uint64_t)(len - kLanes * 4) >> 1;
  const int64_t e0 = esc_off[blk], e1 = esc_off[blk + 1];
  const uint64_t nesc = (e0 >= 0 && e1 >= e0) ? (uint64_t)(e1 - e0) : 0;
  const uint32_t* esc = escapes + (e0 < 0 ? 0 : e0);

  const int64_t gbase = (int64_t)b * nsym * S1;  // this image's first table dword
  uint4 pre[NQ];

  // global -> registers: the dwords [g0, g1) of round r, fetched as the 16-byte pieces that cover them
  auto fetch = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int64_t a0 = g0 & ~(int64_t)3;
    const int nq = (int)((g0 + (int64_t)rows * S1 - a0 + 3) >> 2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int64_t e = a0 + 4 * (int64_t)q;
        if (e + 4 <= total_dwords) {
          pre[i] = *reinterpret_cast<const uint4*>(tables + e);
        } else {  // the buffer's last, partial piece
          pre[i].x = e < total_dwords ? tables[e] : 0u;
          pre[i].y = e + 1 < total_dwords ? tables[e + 1] : 0u;
          pre[i].z = e + 2 < total_dwords ? tables[e + 2] : 0u;
          pre[i].w = 0u;
        }
      }
    }
  };
  // registers -> LDS rows of S1 dwords at a pitch of S1 + 1
  auto drop = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int head = (int)(g0 & 3), lim = rows * S1;
    const int nq = (head + lim + 3) >> 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int rel0 = 4 * q - head;  // >= -3
        int row = rel0 > 0 ? (int)(((uint32_t)rel0 * inv) >> 24) : 0;
        int col = rel0 - row * S1;
        const uint32_t v[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rel = rel0 + j;
          if (rel >= 0 && rel < lim) lds[rel + row] = v[j];
          if (++col == S1) {
            col = 0;
            ++row;
          }
        }
      }
    }
  };

  fetch(g);
  drop(g);
  __syncthreads();
  for (int r = g; r < rounds; r += G) {
    const int k = r * kLanes + lane;
    const bool active = k < nsym;
    // loads that do not depend on the search, oldest first so that waiting for them leaves the prefetch in flight
    const uint64_t wi = (uint64_t)ptr + lane;
    const uint32_t wpre = (err == 0 && wi < nwords) ? (uint32_t)words[wi] : 0u;
    const int32_t c = active ? center[(int64_t)b * nsym + k] : 0;
    const int64_t d = active ? dest[k / M] : 0;
    if (r + G < rounds) fetch(r + G);

    int s = W;  // the table centre: what an image in error decodes
    bool bad = false;
    uint32_t excess = 0;
    if (err == 0) {
      const uint32_t slot = x & 0xFFFFu;
      const uint32_t* row = lds + lane * stride;
      int lo = 0, hi = S;  // largest s with cum[s] <= slot
      if (active) {
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (row[mid] <= slot)
            lo = mid;
          else
            hi = mid;
        }
        const uint32_t start = row[lo], freq = row[lo + 1] - start;
        x = freq * (x >> 16) + slot - start;
        s = lo;
      }
      // renormalisation: one ballot, one popcount, one shuffle of the prefetched words
      const bool need = active && x < 65536u;
      const unsigned long long mask = __ballot(need);
      const int rank = __popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t w = __shfl(wpre, rank, kLanes);
      if (need) {
        if ((uint64_t)ptr + rank < nwords)
          x = (x << 16) | w;
        else
          bad = true;
      }
      ptr += (uint32_t)__popcll(mask);
      // escapes: the same rule on a second cursor; rare, so their load may depend on the search
      const bool edge = active && (s == 0 || s == S - 1);
      const unsigned long long emask = __ballot(edge);
      if (emask != 0ull) {
        const int erank = __popcll(emask & ((1ull << lane) - 1ull));
        if (edge) {
          if ((uint64_t)eptr + erank < nesc)
            excess = esc[(uint64_t)eptr + erank];
          else
            bad = true;
        }
        eptr += (uint32_t)__popcll(emask);
      }
    }
    if (active) {
      int64_t v = (int64_t)s + c - W;
      if (s == 0) v -= excess;
      if (s == S - 1) v += excess;
      if (d >= 0 && d < pixels)
        ypad[((int64_t)b * pixels + d) * M + (k % M)] = (float)v;
      else
        bad = true;
    }
    if (__any(bad)) err |= LIC_RANS_ERR_RANGE;
    __syncthreads();  // every lane has finished searching this round's rows
    if (r + G < rounds) {
      drop(r + G);
      __syncthreads();
    }
  }
  st[lane] = x;
  if (lane == 0) {
    st[kLanes] = ptr;
    st[kLanes + 1] = eptr;
    st[kLanes + 2] = err;
  }
}

// The same step for images whose rows of this step differ in number (lic_rans_decode_step_ragged): wave (b, g) takes
// its rows from seg[b] = (first row, rows) of the step's concatenated tables, centres and dest, and its plane from
// y_base[b], pixels[b].  Written beside rans_step_kernel and not as a parameter of it: that kernel's registers and time
// are held where they are, and the two differ only in where the wave's rows start.  An image's first
// table dword first * M * (S+1) sits at any offset mod 4; fetch / drop take a misaligned g0 as they always did.
template <int NQ, int S1MAX>
__global__ __launch_bounds__(64) void rans_step_ragged_kernel(
    const uint8_t* __restrict__ streams, const int64_t* __restrict__ stream_off,
    const int64_t* __restrict__ stream_bytes, const uint32_t* __restrict__ escapes,
    const int64_t* __restrict__ esc_off, uint32_t* state, const uint32_t* __restrict__ tables,
    const int32_t* __restrict__ center, const int32_t* __restrict__ seg, int32_t G, int64_t total_rows, int32_t M,
    int32_t W, const int64_t* __restrict__ dest_all, float* ypad_all, const int64_t* __restrict__ y_base,
    const int64_t* __restrict__ pixels_of, int64_t ypad_len) {
  __shared__ uint32_t lds[kLanes * (S1MAX + 1)];
  // blk: the state block, stream and escape list of (image b, group g); tables, centres and ypad go by image
  const int blk = blockIdx.x, b = blk / G, g = blk - b * G, lane = threadIdx.x;
  const int64_t first = seg[2 * b], nrows = seg[2 * b + 1];
  if (nrows == 0) return;  // the image has finished, or sits this step out: the state block stays as it is
  uint32_t* st = state + (size_t)blk * kStateWords;
  if (first < 0 || nrows < 0 || first + nrows > total_rows) {  // a segment outside the step: nothing is read
    if (lane == 0) st[kLanes + 2] |= LIC_RANS_ERR_RANGE;
    return;
  }
  const int nsym = (int)(nrows * M);  // <= total_rows * M, which the entry holds below 2^31
  const int rounds = (nsym + kLanes - 1) / kLanes;
  if (g >= rounds) return;  // no round of this step is this group's: the state block stays as it is
  const int S1 = 2 * W + 2, S = S1 - 1, stride = S1 + 1;
  const uint32_t inv = ((1u << 24) + S1 - 1) / S1;  // rel / S1 == (rel * inv) >> 24 for rel < 64 * S1 <= 2^14

  uint32_t x = st[lane];
  uint32_t ptr = st[kLanes], eptr = st[kLanes + 1], err = st[kLanes + 2];
  const int64_t o0 = stream_off[blk], room = stream_off[blk + 1] - o0;
  int64_t len = stream_bytes[blk];
  if (len > room || len < kLanes * 4 || o0 < 0) {
    err |= LIC_RANS_ERR_STREAM;
    len = kLanes * 4;
  }
  const uint16_t* words = reinterpret_cast<const uint16_t*>(streams + (o0 < 0 ? 0 : o0) + kLanes * 4);
  const uint64_t nwords = (uint64_t)(len - kLanes * 4) >> 1;
  const int64_t e0 = esc_off[blk], e1 = esc_off[blk + 1];
  const uint64_t nesc = (e0 >= 0 && e1 >= e0) ? (uint64_t)(e1 - e0) : 0;
  const uint32_t* esc = escapes + (e0 < 0 ? 0 : e0);

  const int64_t gbase = first * M * S1;  // this image's first table dword of the step
  const int64_t total_dwords = total_rows * M * S1;
  const int32_t* cen = center + first * M;
  const int64_t* dest = dest_all + first;
  // the image's plane, inside ypad_all or empty: with pixels == 0 every destination is refused below
  int64_t yb = y_base[b], pixels = pixels_of[b];
  if (yb < 0 || pixels < 0 || pixels > ypad_len / M || yb > ypad_len - pixels * M) yb = 0, pixels = 0;
  float* ypad = ypad_all + yb;
  uint4 pre[NQ];

  // global -> registers: the dwords [g0, g1) of round r, fetched as the 16-byte pieces that cover them
  auto fetch = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int64_t a0 = g0 & ~(int64_t)3;
    const int nq = (int)((g0 + (int64_t)rows * S1 - a0 + 3) >> 2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int64_t e = a0 + 4 * (int64_t)q;
        if (e + 4 <= total_dwords) {
          pre[i] = *reinterpret_cast<const uint4*>(tables + e);
        } else {  // the buffer's last, partial piece
          pre[i].x = e < total_dwords ? tables[e] : 0u;
          pre[i].y = e + 1 < total_dwords ? tables[e + 1] : 0u;
          pre[i].z = e + 2 < total_dwords ? tables[e + 2] : 0u;
          pre[i].w = 0u;
        }
      }
    }
  };
  // registers -> LDS rows of S1 dwords at a pitch of S1 + 1
  auto drop = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int head = (int)(g0 & 3), lim = rows * S1;
    const int nq = (head + lim + 3) >> 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int rel0 = 4 * q - head;  // >= -3
        int row = rel0 > 0 ? (int)(((uint32_t)rel0 * inv) >> 24) : 0;
        int col = rel0 - row * S1;
        const uint32_t v[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rel = rel0 + j;
          if (rel >= 0 && rel < lim) lds[rel + row] = v[j];
          if (++col == S1) {
            col = 0;
            ++row;
          }
        }
      }
    }
  };

  fetch(g);
  drop(g);
  __syncthreads();
  for (int r = g; r < rounds; r += G) {
    const int k = r * kLanes + lane;
    const bool active = k < nsym;
    // loads that do not depend on the search, oldest first so that waiting for them leaves the prefetch in flight
    const uint64_t wi = (uint64_t)ptr + lane;
    const uint32_t wpre = (err == 0 && wi < nwords) ? (uint32_t)words[wi] : 0u;
    const int32_t c = active ? cen[k] : 0;
    const int64_t d = active ? dest[k / M] : 0;
    if (r + G < rounds) fetch(r + G);

    int s = W;  // the table centre: what an image in error decodes
    bool bad = false;
    uint32_t excess = 0;
    if (err == 0) {
      const uint32_t slot = x & 0xFFFFu;
      const uint32_t* row = lds + lane * stride;
      int lo = 0, hi = S;  // largest s with cum[s] <= slot
      if (active) {
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (row[mid] <= slot)
            lo = mid;
          else
            hi = mid;
        }
        const uint32_t start = row[lo], freq = row[lo + 1] - start;
        x = freq * (x >> 16) + slot - start;
        s = lo;
      }
      // renormalisation: one ballot, one popcount, one shuffle of the prefetched words
      const bool need = active && x < 65536u;
      const unsigned long long mask = __ballot(need);
      const int rank = __popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t w = __shfl(wpre, rank, kLanes);
      if (need) {
        if ((uint64_t)ptr + rank < nwords)
          x = (x << 16) | w;
        else
          bad = true;
      }
      ptr += (uint32_t)__popcll(mask);
      // escapes: the same rule on a second cursor; rare, so their load may depend on the search
      const bool edge = active && (s == 0 || s == S - 1);
      const unsigned long long emask = __ballot(edge);
      if (emask != 0ull) {
        const int erank = __popcll(emask & ((1ull << lane) - 1ull));
        if (edge) {
          if ((uint64_t)eptr + erank < nesc)
            excess = esc[(uint64_t)eptr + erank];
          else
            bad = true;
        }
        eptr += (uint32_t)__popcll(emask);
      }
    }
    if (active) {
      int64_t v = (int64_t)s + c - W;
      if (s == 0) v -= excess;
      if (s == S - 1) v += excess;
      if (d >= 0 && d < pixels)
        ypad[d * M + (k % M)] = (float)v;
      else
        bad = true;
    }
    if (__any(bad)) err |= LIC_RANS_ERR_RANGE;
    __syncthreads();  // every lane has finished searching this round's rows
    if (r + G < rounds) {
      drop(r + G);
      __syncthreads();
    }
  }
  st[lane] = x;
  if (lane == 0) {
    st[kLanes] = ptr;
    st[kLanes + 1] = eptr;
    st[kLanes + 2] = err;
  }
}

}  // namespace

static int decode_step(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                       const uint32_t* escapes, const int64_t* esc_off, uint32_t* state, const uint32_t* tables,
                       const int32_t* center, int32_t B, int32_t G, int32_t n, int32_t M, int32_t W,
                       const int64_t* dest, float* ypad, int64_t pixels, lic_stream_t stream) {
  if (!streams || !stream_off || !stream_bytes || !escapes || !esc_off || !state || !tables || !center || !dest || !ypad)
    return LIC_ERR_INVALID;
  if (B <= 0 || n <= 0 || M <= 0 || W <= 0 || pixels <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) & 15) || (reinterpret_cast<uintptr_t>(streams) & 3)) return LIC_ERR_INVALID;
  if (W > 64) return LIC_ERR_UNSUPPORTED;
  const int64_t nsym = (int64_t)n * M;
  if (nsym > 0x7FFFFFFFL - kLanes || (int64_t)B * G > 65535) return LIC_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)B * nsym * (2 * W + 2);
  // a round spans 64 * (S+1) dwords plus up to 3 of misalignment: 17 pieces per lane for S+1 <= 66, 33 for <= 130
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B * G), dim3(kLanes), 0, (hipStream_t)stream, streams, stream_off, stream_bytes,
                       escapes, esc_off, state, tables, center, G, (int32_t)nsym, M, W, dest, ypad, pixels, total);
  };
  if (W <= 32)
    G == 1 ? launch(rans_step_kernel<17, 66, false>) : launch(rans_step_kernel<17, 66, true>);
  else
    G == 1 ? launch(rans_step_kernel<33, 130, false>) : launch(rans_step_kernel<33, 130, true>);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_decode_step(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                    const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                    const uint32_t* tables, const int32_t* center, int32_t B, int32_t n, int32_t M,
                                    int32_t W, const int64_t* dest, float* ypad, int64_t pixels,
                                    lic_stream_t stream) {
  return decode_step(streams, stream_off, stream_bytes, escapes, esc_off, state, tables, center, B, 1, n, M, W, dest,
                     ypad, pixels, stream);
}

LIC_EXPORT int lic_rans_decode_step_groups(const uint8_t* streams, const int64_t* stream_off,
                                           const int64_t* stream_bytes, const uint32_t* escapes,
                                           const int64_t* esc_off, uint32_t* state, const uint32_t* tables,
                                           const int32_t* center, int32_t B, int32_t G, int32_t n, int32_t M,
                                           int32_t W, const int64_t* dest, float* ypad, int64_t pixels,
                                           lic_stream_t stream) {
  return decode_step(streams, stream_off, stream_bytes, escapes, esc_off, state, tables, center, B, G, n, M, W, dest,
                     ypad, pixels, stream);
}

LIC_EXPORT int lic_rans_decode_step_ragged(const uint8_t* streams, const int64_t* stream_off,
                                           const int64_t* stream_bytes, const uint32_t* escapes,
                                           const int64_t* esc_off, uint32_t* state, const uint32_t* tables,
                                           const int32_t* center, const int32_t* seg, int32_t nimg, int32_t G,
                                           int64_t total_rows, int32_t M, int32_t W, const int64_t* dest, float* ypad,
                                           const int64_t* y_base, const int64_t* pixels, int64_t ypad_len,
                                           lic_stream_t stream) {
  if (!streams || !stream_off || !stream_bytes || !escapes || !esc_off || !state || !tables || !center || !seg ||
      !dest || !ypad || !y_base || !pixels)
    return LIC_ERR_INVALID;
  if (nimg <= 0 || total_rows <= 0 || M <= 0 || W <= 0 || ypad_len <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) & 15) || (reinterpret_cast<uintptr_t>(streams) & 3)) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(seg) | reinterpret_cast<uintptr_t>(center) | reinterpret_cast<uintptr_t>(ypad) |
       reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(dest) | reinterpret_cast<uintptr_t>(y_base) | reinterpret_cast<uintptr_t>(pixels)) & 7)
    return LIC_ERR_INVALID;
  if (W > 64) return LIC_ERR_UNSUPPORTED;
  if (total_rows * (int64_t)M > 0x7FFFFFFFL - kLanes || total_rows > 0x7FFFFFFFL || (int64_t)nimg * G > 65535 ||
      ypad_len > ((int64_t)1 << 40))
    return LIC_ERR_UNSUPPORTED;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nimg * G), dim3(kLanes), 0, (hipStream_t)stream, streams, stream_off, stream_bytes,
                       escapes, esc_off, state, tables, center, seg, G, total_rows, M, W, dest, ypad, y_base, pixels,
                       ypad_len);
  };
  if (W <= 32)
    launch(rans_step_ragged_kernel<17, 66>);
  else
    launch(rans_step_ragged_kernel<33, 130>);
  return lic_check_launch();
}

// ---- the layers of one latent (lic_rans_decode_step_layers, codec.ScalableCodec) ------------------------------------
// L * B * G waves, layer-major: wave (l, b, g) is rans_step_kernel's wave (b, g) on layer l's tables, centres and
// blocks, and writes channel c0 + k % M of the shared plane, whose pixels are y_pix floats apart.  The waves of the
// layers do not depend on each other, so one launch carries them side by side instead of one behind the other.
// A fourth kernel beside the three above, for the reason the ragged one is the third: their
// registers and time are held where they are, and the shared inlined round loop that was tried cost time.  What
// differs from rans_step_kernel: where the wave finds its layer (the by-value table, read with constant indices),
// `total_dwords` per layer, and the destination's pitch and channel offset.
namespace {

struct RansLayers {
  lic_rans_layer layer[LIC_MAX_LAYERS];
};

template <int NQ, int S1MAX>
__global__ __launch_bounds__(64) void rans_step_layers_kernel(
    const uint8_t* __restrict__ streams, const int64_t* __restrict__ stream_off,
    const int64_t* __restrict__ stream_bytes, const uint32_t* __restrict__ escapes,
    const int64_t* __restrict__ esc_off, uint32_t* state, const RansLayers layers, int32_t B, int32_t G, int32_t n,
    int32_t W, const int64_t* __restrict__ dest, float* ypad, int64_t pixels, int64_t y_pix) {
  __shared__ uint32_t lds[kLanes * (S1MAX + 1)];
  // blk: the state block, stream and escape list of (layer l, image b, group g); tables and centres go by layer and
  // image, ypad by image
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int l = blk / (B * G), ib = blk - l * (B * G), b = ib / G, g = ib - b * G;
  const uint32_t* tables = layers.layer[0].tables;
  const int32_t* center = layers.layer[0].center;
  int c0 = layers.layer[0].c0, M = layers.layer[0].M;
#pragma unroll
  for (int i = 1; i < LIC_MAX_LAYERS; ++i)
    if (l == i) {
      tables = layers.layer[i].tables;
      center = layers.layer[i].center;
      c0 = layers.layer[i].c0;
      M = layers.layer[i].M;
    }
  const int nsym = n * M;  // the entry holds it below 2^31 - 64
  const int rounds = (nsym + kLanes - 1) / kLanes;
  if (g >= rounds) return;  // no round of this step is this group's: the state block stays as it is
  const int S1 = 2 * W + 2, S = S1 - 1, stride = S1 + 1;
  const uint32_t inv = ((1u << 24) + S1 - 1) / S1;  // rel / S1 == (rel * inv) >> 24 for rel < 64 * S1 <= 2^14
  const int64_t total_dwords = (int64_t)B * nsym * S1;

  uint32_t* st = state + (size_t)blk * kStateWords;
  uint32_t x = st[lane];
  uint32_t ptr = st[kLanes], eptr = st[kLanes + 1], err = st[kLanes + 2];
  const int64_t o0 = stream_off[blk], room = stream_off[blk + 1] - o0;
  int64_t len = stream_bytes[blk];
  if (len > room || len < kLanes * 4 || o0 < 0) {
    err |= LIC_RANS_ERR_STREAM;
    len = kLanes * 4;
  }
  const uint16_t* words = reinterpret_cast<const uint16_t*>(streams + (o0 < 0 ? 0 : o0) + kLanes * 4);
  const uint64_t nwords = (uint64_t)(len - kLanes * 4) >> 1;
  const int64_t e0 = esc_off[blk], e1 = esc_off[blk + 1];
  const uint64_t nesc = (e0 >= 0 && e1 >= e0) ? (uint64_t)(e1 - e0) : 0;
  const uint32_t* esc = escapes + (e0 < 0 ? 0 : e0);

  const int64_t gbase = (int64_t)b * nsym * S1;  // this image's first table dword in the layer's tables
  uint4 pre[NQ];

  // global -> registers: the dwords [g0, g1) of round r, fetched as the 16-byte pieces that cover them
  auto fetch = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int64_t a0 = g0 & ~(int64_t)3;
    const int nq = (int)((g0 + (int64_t)rows * S1 - a0 + 3) >> 2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int64_t e = a0 + 4 * (int64_t)q;
        if (e + 4 <= total_dwords) {
          pre[i] = *reinterpret_cast<const uint4*>(tables + e);
        } else {  // the buffer's last, partial piece
          pre[i].x = e < total_dwords ? tables[e] : 0u;
          pre[i].y = e + 1 < total_dwords ? tables[e + 1] : 0u;
          pre[i].z = e + 2 < total_dwords ? tables[e + 2] : 0u;
          pre[i].w = 0u;
        }
      }
    }
  };
  // registers -> LDS rows of S1 dwords at a pitch of S1 + 1
  auto drop = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int head = (int)(g0 & 3), lim = rows * S1;
    const int nq = (head + lim + 3) >> 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int rel0 = 4 * q - head;  // >= -3
        int row = rel0 > 0 ? (int)(((uint32_t)rel0 * inv) >> 24) : 0;
        int col = rel0 - row * S1;
        const uint32_t v[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rel = rel0 + j;
          if (rel >= 0 && rel < lim) lds[rel + row] = v[j];
          if (++col == S1) {
            col = 0;
            ++row;
          }
        }
      }
    }
  };

  fetch(g);
  drop(g);
  __syncthreads();
  for (int r = g; r < rounds; r += G) {
    const int k = r * kLanes + lane;
    const bool active = k < nsym;
    // loads that do not depend on the search, oldest first so that waiting for them leaves the prefetch in flight
    const uint64_t wi = (uint64_t)ptr + lane;
    const uint32_t wpre = (err == 0 && wi < nwords) ? (uint32_t)words[wi] : 0u;
    const int32_t c = active ? center[(int64_t)b * nsym + k] : 0;
    const int64_t d = active ? dest[k / M] : 0;
    if (r + G < rounds) fetch(r + G);

    int s = W;  // the table centre: what a block in error decodes
    bool bad = false;
    uint32_t excess = 0;
    if (err == 0) {
      const uint32_t slot = x & 0xFFFFu;
      const uint32_t* row = lds + lane * stride;
      int lo = 0, hi = S;  // largest s with cum[s] <= slot
      if (active) {
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (row[mid] <= slot)
            lo = mid;
          else
            hi = mid;
        }
        const uint32_t start = row[lo], freq = row[lo + 1] - start;
        x = freq * (x >> 16) + slot - start;
        s = lo;
      }
      // renormalisation: one ballot, one popcount, one shuffle of the prefetched words
      const bool need = active && x < 65536u;
      const unsigned long long mask = __ballot(need);
      const int rank = __popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t w = __shfl(wpre, rank, kLanes);
      if (need) {
        if ((uint64_t)ptr + rank < nwords)
          x = (x << 16) | w;
        else
          bad = true;
      }
      ptr += (uint32_t)__popcll(mask);
      // escapes: the same rule on a second cursor; rare, so their load may depend on the search
      const bool edge = active && (s == 0 || s == S - 1);
      const unsigned long long emask = __ballot(edge);
      if (emask != 0ull) {
        const int erank = __popcll(emask & ((1ull << lane) - 1ull));
        if (edge) {
          if ((uint64_t)eptr + erank < nesc)
            excess = esc[(uint64_t)eptr + erank];
          else
            bad = true;
        }
        eptr += (uint32_t)__popcll(emask);
      }
    }
    if (active) {
      int64_t v = (int64_t)s + c - W;
      if (s == 0) v -= excess;
      if (s == S - 1) v += excess;
      if (d >= 0 && d < pixels)
        ypad[((int64_t)b * pixels + d) * y_pix + c0 + (k % M)] = (float)v;
      else
        bad = true;
    }
    if (__any(bad)) err |= LIC_RANS_ERR_RANGE;
    __syncthreads();  // every lane has finished searching this round's rows
    if (r + G < rounds) {
      drop(r + G);
      __syncthreads();
    }
  }
  st[lane] = x;
  if (lane == 0) {
    st[kLanes] = ptr;
    st[kLanes + 1] = eptr;
    st[kLanes + 2] = err;
  }
}

}  // namespace

LIC_EXPORT int lic_rans_decode_step_layers(const uint8_t* streams, const int64_t* stream_off,
                                           const int64_t* stream_bytes, const uint32_t* escapes,
                                           const int64_t* esc_off, uint32_t* state, const lic_rans_layer* layers,
                                           int32_t L, int32_t B, int32_t G, int32_t n, int32_t W, const int64_t* dest,
                                           float* ypad, int64_t pixels, int64_t y_pix, lic_stream_t stream) {
  if (!streams || !stream_off || !stream_bytes || !escapes || !esc_off || !state || !layers || !dest || !ypad)
    return LIC_ERR_INVALID;
  if (L < 1 || L > LIC_MAX_LAYERS) return LIC_ERR_INVALID;
  if (B <= 0 || n <= 0 || W <= 0 || pixels <= 0 || y_pix <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(streams) | reinterpret_cast<uintptr_t>(escapes) | reinterpret_cast<uintptr_t>(ypad) |
       reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(stream_off) | reinterpret_cast<uintptr_t>(stream_bytes) |
       reinterpret_cast<uintptr_t>(esc_off) | reinterpret_cast<uintptr_t>(dest)) & 7)
    return LIC_ERR_INVALID;
  RansLayers table = {};
  for (int l = 0; l < L; ++l) {
    const lic_rans_layer& a = layers[l];
    if (!a.tables || !a.center || a.M <= 0 || a.c0 < 0 || (int64_t)a.c0 + a.M > y_pix) return LIC_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a.tables) & 15) || (reinterpret_cast<uintptr_t>(a.center) & 3))
      return LIC_ERR_INVALID;
    for (int m = 0; m < l; ++m)  // channel ranges must not overlap: two waves would write one element
      if (a.c0 < layers[m].c0 + layers[m].M && layers[m].c0 < a.c0 + a.M) return LIC_ERR_INVALID;
    table.layer[l] = a;
  }
  if (W > 64) return LIC_ERR_UNSUPPORTED;
  for (int l = 0; l < L; ++l)
    if ((int64_t)n * layers[l].M > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  if ((int64_t)L * B * G > 65535 || pixels > ((int64_t)1 << 40) / y_pix) return LIC_ERR_UNSUPPORTED;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(L * B * G), dim3(kLanes), 0, (hipStream_t)stream, streams, stream_off, stream_bytes,
                       escapes, esc_off, state, table, B, G, n, W, dest, ypad, pixels, y_pix);
  };
  if (W <= 32)
    launch(rans_step_layers_kernel<17, 66>);
  else
    launch(rans_step_layers_kernel<33, 130>);
  return lic_check_launch();
}

// ---- the layers of many latents of different sizes (lic_rans_decode_step_layers_ragged) -----------------------------
// L * nimg * G waves, layer-major: wave (l, b, g) is rans_step_ragged_kernel's wave (b, g) on layer l's tables, centres
// and blocks -- seg, dest, y_base and pixels are shared by the layers, which share the schedule -- and writes channel
// c0 + k % M of its image's plane, whose pixels are y_pix floats apart.  A fifth kernel beside the four above, for the
// reason each of them stands alone: their registers and time are held where they are.  What
// differs from rans_step_ragged_kernel: where the wave finds its layer (the by-value table, read with constant
// indices), `total_dwords` per layer, and the plane's extent and the destination in y_pix and c0.
namespace {

template <int NQ, int S1MAX>
__global__ __launch_bounds__(64) void rans_step_layers_ragged_kernel(
    const uint8_t* __restrict__ streams, const int64_t* __restrict__ stream_off,
    const int64_t* __restrict__ stream_bytes, const uint32_t* __restrict__ escapes,
    const int64_t* __restrict__ esc_off, uint32_t* state, const RansLayers layers, const int32_t* __restrict__ seg,
    int32_t nimg, int32_t G, int64_t total_rows, int32_t W, const int64_t* __restrict__ dest_all, float* ypad_all,
    const int64_t* __restrict__ y_base, const int64_t* __restrict__ pixels_of, int64_t ypad_len, int64_t y_pix) {
  __shared__ uint32_t lds[kLanes * (S1MAX + 1)];
  // blk: the state block, stream and escape list of (layer l, image b, group g); tables and centres go by layer,
  // seg, dest and the plane by image
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int l = blk / (nimg * G), ib = blk - l * (nimg * G), b = ib / G, g = ib - b * G;
  const int64_t first = seg[2 * b], nrows = seg[2 * b + 1];
  if (nrows == 0) return;  // the image has finished, or sits this step out: the state block stays as it is
  uint32_t* st = state + (size_t)blk * kStateWords;
  if (first < 0 || nrows < 0 || first + nrows > total_rows) {  // a segment outside the step: nothing is read
    if (lane == 0) st[kLanes + 2] |= LIC_RANS_ERR_RANGE;
    return;
  }
  const uint32_t* tables = layers.layer[0].tables;
  const int32_t* center = layers.layer[0].center;
  int c0 = layers.layer[0].c0, M = layers.layer[0].M;
#pragma unroll
  for (int i = 1; i < LIC_MAX_LAYERS; ++i)
    if (l == i) {
      tables = layers.layer[i].tables;
      center = layers.layer[i].center;
      c0 = layers.layer[i].c0;
      M = layers.layer[i].M;
    }
  const int nsym = (int)(nrows * M);  // <= total_rows * M, which the entry holds below 2^31
  const int rounds = (nsym + kLanes - 1) / kLanes;
  if (g >= rounds) return;  // no round of this step is this group's: the state block stays as it is
  const int S1 = 2 * W + 2, S = S1 - 1, stride = S1 + 1;
  const uint32_t inv = ((1u << 24) + S1 - 1) / S1;  // rel / S1 == (rel * inv) >> 24 for rel < 64 * S1 <= 2^14

  uint32_t x = st[lane];
  uint32_t ptr = st[kLanes], eptr = st[kLanes + 1], err = st[kLanes + 2];
  const int64_t o0 = stream_off[blk], room = stream_off[blk + 1] - o0;
  int64_t len = stream_bytes[blk];
  if (len > room || len < kLanes * 4 || o0 < 0) {
    err |= LIC_RANS_ERR_STREAM;
    len = kLanes * 4;
  }
  const uint16_t* words = reinterpret_cast<const uint16_t*>(streams + (o0 < 0 ? 0 : o0) + kLanes * 4);
  const uint64_t nwords = (uint64_t)(len - kLanes * 4) >> 1;
  const int64_t e0 = esc_off[blk], e1 = esc_off[blk + 1];
  const uint64_t nesc = (e0 >= 0 && e1 >= e0) ? (uint64_t)(e1 - e0) : 0;
  const uint32_t* esc = escapes + (e0 < 0 ? 0 : e0);

  const int64_t gbase = first * M * S1;  // this image's first table dword of the step in the layer's tables
  const int64_t total_dwords = total_rows * M * S1;
  const int32_t* cen = center + first * M;
  const int64_t* dest = dest_all + first;
  // the image's plane, inside ypad_all or empty: with pixels == 0 every destination is refused below
  int64_t yb = y_base[b], pixels = pixels_of[b];
  if (yb < 0 || pixels < 0 || pixels > ypad_len / y_pix || yb > ypad_len - pixels * y_pix) yb = 0, pixels = 0;
  float* ypad = ypad_all + yb + c0;
  uint4 pre[NQ];

  // global -> registers: the dwords [g0, g1) of round r, fetched as the 16-byte pieces that cover them
  auto fetch = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int64_t a0 = g0 & ~(int64_t)3;
    const int nq = (int)((g0 + (int64_t)rows * S1 - a0 + 3) >> 2);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int64_t e = a0 + 4 * (int64_t)q;
        if (e + 4 <= total_dwords) {
          pre[i] = *reinterpret_cast<const uint4*>(tables + e);
        } else {  // the buffer's last, partial piece
          pre[i].x = e < total_dwords ? tables[e] : 0u;
          pre[i].y = e + 1 < total_dwords ? tables[e + 1] : 0u;
          pre[i].z = e + 2 < total_dwords ? tables[e + 2] : 0u;
          pre[i].w = 0u;
        }
      }
    }
  };
  // registers -> LDS rows of S1 dwords at a pitch of S1 + 1
  auto drop = [&](int r) {
    const int64_t g0 = gbase + (int64_t)r * kLanes * S1;
    const int rows = min(kLanes, nsym - r * kLanes);
    const int head = (int)(g0 & 3), lim = rows * S1;
    const int nq = (head + lim + 3) >> 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = lane + kLanes * i;
      if (q < nq) {
        const int rel0 = 4 * q - head;  // >= -3
        int row = rel0 > 0 ? (int)(((uint32_t)rel0 * inv) >> 24) : 0;
        int col = rel0 - row * S1;
        const uint32_t v[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rel = rel0 + j;
          if (rel >= 0 && rel < lim) lds[rel + row] = v[j];
          if (++col == S1) {
            col = 0;
            ++row;
          }
        }
      }
    }
  };

  fetch(g);
  drop(g);
  __syncthreads();
  for (int r = g; r < rounds; r += G) {
    const int k = r * kLanes + lane;
    const bool active = k < nsym;
    // loads that do not depend on the search, oldest first so that waiting for them leaves the prefetch in flight
    const uint64_t wi = (uint64_t)ptr + lane;
    const uint32_t wpre = (err == 0 && wi < nwords) ? (uint32_t)words[wi] : 0u;
    const int32_t c = active ? cen[k] : 0;
    const int64_t d = active ? dest[k / M] : 0;
    if (r + G < rounds) fetch(r + G);

    int s = W;  // the table centre: what a block in error decodes
    bool bad = false;
    uint32_t excess = 0;
    if (err == 0) {
      const uint32_t slot = x & 0xFFFFu;
      const uint32_t* row = lds + lane * stride;
      int lo = 0, hi = S;  // largest s with cum[s] <= slot
      if (active) {
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (row[mid] <= slot)
            lo = mid;
          else
            hi = mid;
        }
        const uint32_t start = row[lo], freq = row[lo + 1] - start;
        x = freq * (x >> 16) + slot - start;
        s = lo;
      }
      // renormalisation: one ballot, one popcount, one shuffle of the prefetched words
      const bool need = active && x < 65536u;
      const unsigned long long mask = __ballot(need);
      const int rank = __popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t w = __shfl(wpre, rank, kLanes);
      if (need) {
        if ((uint64_t)ptr + rank < nwords)
          x = (x << 16) | w;
        else
          bad = true;
      }
      ptr += (uint32_t)__popcll(mask);
      // escapes: the same rule on a second cursor; rare, so their load may depend on the search
      const bool edge = active && (s == 0 || s == S - 1);
      const unsigned long long emask = __ballot(edge);
      if (emask != 0ull) {
        const int erank = __popcll(emask & ((1ull << lane) - 1ull));
        if (edge) {
          if ((uint64_t)eptr + erank < nesc)
            excess = esc[(uint64_t)eptr + erank];
          else
            bad = true;
        }
        eptr += (uint32_t)__popcll(emask);
      }
    }
    if (active) {
      int64_t v = (int64_t)s + c - W;
      if (s == 0) v -= excess;
      if (s == S - 1) v += excess;
      if (d >= 0 && d < pixels)
        ypad[d * y_pix + (k % M)] = (float)v;
      else
        bad = true;
    }
    if (__any(bad)) err |= LIC_RANS_ERR_RANGE;
    __syncthreads();  // every lane has finished searching this round's rows
    if (r + G < rounds) {
      drop(r + G);
      __syncthreads();
    }
  }
  st[lane] = x;
  if (lane == 0) {
    st[kLanes] = ptr;
    st[kLanes + 1] = eptr;
    st[kLanes + 2] = err;
  }
}

}  // namespace

LIC_EXPORT int lic_rans_decode_step_layers_ragged(const uint8_t* streams, const int64_t* stream_off,
                                                  const int64_t* stream_bytes, const uint32_t* escapes,
                                                  const int64_t* esc_off, uint32_t* state,
                                                  const lic_rans_layer* layers, int32_t L, const int32_t* seg,
                                                  int32_t nimg, int32_t G, int64_t total_rows, int32_t W,
                                                  const int64_t* dest, float* ypad, const int64_t* y_base,
                                                  const int64_t* pixels, int64_t ypad_len, int64_t y_pix,
                                                  lic_stream_t stream) {
  if (!streams || !stream_off || !stream_bytes || !escapes || !esc_off || !state || !layers || !seg || !dest ||
      !ypad || !y_base || !pixels)
    return LIC_ERR_INVALID;
  if (L < 1 || L > LIC_MAX_LAYERS) return LIC_ERR_INVALID;
  if (nimg <= 0 || total_rows <= 0 || W <= 0 || ypad_len <= 0 || y_pix <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(streams) | reinterpret_cast<uintptr_t>(escapes) | reinterpret_cast<uintptr_t>(ypad) |
       reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(seg)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(stream_off) | reinterpret_cast<uintptr_t>(stream_bytes) |
       reinterpret_cast<uintptr_t>(esc_off) | reinterpret_cast<uintptr_t>(dest) | reinterpret_cast<uintptr_t>(y_base) |
       reinterpret_cast<uintptr_t>(pixels)) & 7)
    return LIC_ERR_INVALID;
  RansLayers table = {};
  for (int l = 0; l < L; ++l) {
    const lic_rans_layer& a = layers[l];
    if (!a.tables || !a.center || a.M <= 0 || a.c0 < 0 || (int64_t)a.c0 + a.M > y_pix) return LIC_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a.tables) & 15) || (reinterpret_cast<uintptr_t>(a.center) & 3))
      return LIC_ERR_INVALID;
    for (int m = 0; m < l; ++m)  // channel ranges must not overlap: two waves would write one element
      if (a.c0 < layers[m].c0 + layers[m].M && layers[m].c0 < a.c0 + a.M) return LIC_ERR_INVALID;
    table.layer[l] = a;
  }
  if (W > 64) return LIC_ERR_UNSUPPORTED;
  if (total_rows > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
  for (int l = 0; l < L; ++l)
    if (total_rows * (int64_t)layers[l].M > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  if ((int64_t)L * nimg * G > 65535 || ypad_len > ((int64_t)1 << 40)) return LIC_ERR_UNSUPPORTED;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(L * nimg * G), dim3(kLanes), 0, (hipStream_t)stream, streams, stream_off,
                       stream_bytes, escapes, esc_off, state, table, seg, nimg, G, total_rows, W, dest, ypad, y_base,
                       pixels, ypad_len, y_pix);
  };
  if (W <= 32)
    launch(rans_step_layers_ragged_kernel<17, 66>);
  else
    launch(rans_step_layers_ragged_kernel<33, 130>);
  return lic_check_launch();
}
