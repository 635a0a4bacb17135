// lic_rans_z_pick / lic_rans_z_decode: the hyper-latent z as "rANS-64 x G" streams (include/lic_codec.h), coded by
// kernels, for codec.ContextCodec(z_coder="rans").  The z prior has no parameters: the whole stream has M tables, and
// symbol k of an image (pixel by pixel, channel by channel) uses table k % M.  An image is ONE step of all its
// symbols, dealt to G sub-streams round by round.
//
// The y kernels of lic_rans.hip fetch 64 table rows per round, one per symbol.  Here the M tables are staged ONCE per
// wave and stay in LDS for the whole stream: cum[0..S-1] of a valid table are below 65536 and cum[S] is implied, so a
// row is S 16-bit entries.  Lane l of round r holds symbol k = 64 r + l and searches row k % M: consecutive lanes,
// consecutive rows.  The row pitch is the smallest P >= S with P % 4 == 2 (in 16-bit entries): P / 2 is then odd, so
// the 32 lanes of a half wave, probing the same column of 32 consecutive rows, land on 32 different dwords modulo 32,
// i.e. on all 32 banks of ds_read_u16 (an even P / 2 would pile them onto 16 banks or fewer; see the stride comment at
// the top of lic_rans.hip).  When M * P entries exceed the LDS budget (LIC_RANS_Z_LDS_BYTES) the second instantiation
// searches the rows in global memory instead (they stay in L2); both write the same bytes.
//
// The wave validates the tables while it stages them (pick's rules: cum[0] == 0, cum[S] == 65536, 0 < freq < 65536);
// a malformed table sets LIC_RANS_ERR_RANGE in the block and decodes nothing.  Stream words are prefetched one per lane
// at the top of each round and handed out by ballot, popcount and shuffle, as in rans_step_kernel.  Every cursor is
// compared with its length before it indexes; a block in error decodes its later symbols as lo + S / 2.
//
// The encoder's serial half is lic_rans_encode_ragged, unchanged: a z "image" is a descriptor of P rows of M with one
// step of P * M symbols.  lic_rans_z_pick is its parallel half: no order array (coding order is raster order), no
// centres, M shared tables.
#include "lic_common.h"

namespace {

constexpr int kLanes = LIC_RANS_LANES;
constexpr int kStateWords = LIC_RANS_STATE_WORDS;
constexpr uint32_t kNoEscape = 0xFFFFFFFFu;  // the largest real excess is 2^31
constexpr uint32_t kHarmless = 1u;           // start 0, freq 1: what a symbol in error codes

// smallest pitch >= S, in 16-bit entries, whose half is odd
inline int z_pitch(int S) { return S + ((6 - (S & 3)) & 3); }

__global__ __launch_bounds__(256) void rans_z_pick_kernel(const uint32_t* __restrict__ tables, int32_t M, int32_t lo,
                                                          int32_t S, const int32_t* __restrict__ z, int64_t n,
                                                          uint32_t* __restrict__ sf, uint32_t* __restrict__ exc,
                                                          uint32_t* err) {
  const int S1 = S + 1;
  bool bad = false;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    // two's complement, as the host path's int32 tensor arithmetic
    const int32_t idx = (int32_t)((uint32_t)z[k] - (uint32_t)lo);
    const int32_t s = idx <= 0 ? 0 : (idx >= S - 1 ? S - 1 : idx);
    uint32_t word = kHarmless, excess = kNoEscape;
    if (idx <= 0) excess = (uint32_t)(-(int64_t)idx);
    if (idx >= S - 1) excess = (uint32_t)((int64_t)idx - (S - 1));
    const uint32_t* row = tables + (int64_t)(k % M) * S1;
    const uint32_t first = row[0], last = row[S], start = row[s], end = row[s + 1];
    if (first == 0u && last == 65536u && end > start && end - start < 65536u && start < 65536u) {
      word = (start << 16) | (end - start);
    } else {
      bad = true;
      excess = kNoEscape;
    }
    sf[k] = word;
    exc[k] = excess;
  }
  // one atomic per wave at the most; the loop has ended for every lane here
  if (__any(bad) && (threadIdx.x & (kLanes - 1)) == 0) atomicOr(err, LIC_RANS_ERR_RANGE);
}

// kResident: the M rows live in LDS as 16-bit entries at `pitch`; otherwise they are read where they are
template <bool kResident>
__global__ __launch_bounds__(64) void rans_z_decode_kernel(
    const uint8_t* __restrict__ streams, const int64_t* __restrict__ stream_off,
    const int64_t* __restrict__ stream_bytes, const uint32_t* __restrict__ escapes,
    const int64_t* __restrict__ esc_off, uint32_t* state, const uint32_t* __restrict__ tables, int32_t M, int32_t lo,
    int32_t S, int32_t pitch, int32_t G, const int64_t* __restrict__ nsym_of, const int64_t* __restrict__ z_base,
    float* z, int64_t z_len) {
  extern __shared__ uint16_t lds[];
  // blk: the state block, stream and escape list of (image b, group g)
  const int blk = blockIdx.x, b = blk / G, g = blk - b * G, lane = threadIdx.x;
  const int64_t n64 = nsym_of[b];
  if (n64 == 0) return;  // no z symbol of this image in the call: the state block stays as it is
  uint32_t* st = state + (size_t)blk * kStateWords;
  const int64_t zb = z_base[b];
  // a count that cannot be right, or a plane that does not lie inside [0, z_len): nothing is read or written
  if (n64 < 0 || n64 > 0x7FFFFFFFL - kLanes || zb < 0 || zb > z_len || n64 > z_len - zb) {
    if (lane == 0) st[kLanes + 2] |= LIC_RANS_ERR_RANGE;
    return;
  }
  const int nsym = (int)n64;
  const int rounds = (nsym + kLanes - 1) / kLanes;
  if (g >= rounds) return;  // the image has fewer rounds than groups: the state block stays as it is
  const int S1 = S + 1;

  // the tables: validated by pick's rules, entry by entry, and (kResident) dropped into LDS on the way
  {
    bool badl = false;
    const int total = M * S;
    int row = 0, col = lane;
    while (col >= S) col -= S, ++row;
    for (int e = lane; e < total; e += kLanes) {
      const uint32_t* t = tables + (int64_t)row * S1 + col;
      const uint32_t v = t[0], nx = t[1];
      if (nx <= v || nx - v >= 65536u || (col == 0 && v != 0u) || (col == S - 1 && nx != 65536u) || v >= 65536u)
        badl = true;
      if (kResident) lds[row * pitch + col] = (uint16_t)v;
      col += kLanes;
      while (col >= S) col -= S, ++row;
    }
    if (kResident) __syncthreads();
    if (__any(badl)) {
      if (lane == 0) st[kLanes + 2] |= LIC_RANS_ERR_RANGE;
      return;
    }
  }

  uint32_t x = st[lane];
  uint32_t ptr = st[kLanes], eptr = st[kLanes + 1], err = st[kLanes + 2];
  const int64_t o0 = stream_off[blk], room = stream_off[blk + 1] - o0;
  int64_t len = stream_bytes[blk];
  if (len > room || len < kLanes * 4 || o0 < 0 || (o0 & 3)) {
    err |= LIC_RANS_ERR_STREAM;
    len = kLanes * 4;
  }
  const uint16_t* words = reinterpret_cast<const uint16_t*>(streams + ((o0 < 0 || (o0 & 3)) ? 0 : o0) + kLanes * 4);
  const uint64_t nwords = (uint64_t)(len - kLanes * 4) >> 1;
  const int64_t e0 = esc_off[blk], e1 = esc_off[blk + 1];
  const uint64_t nesc = (e0 >= 0 && e1 >= e0) ? (uint64_t)(e1 - e0) : 0;
  const uint32_t* esc = escapes + (e0 < 0 ? 0 : e0);
  float* out = z + zb;

  // the lane's table row of round g; a round moves it on by 64 G rows modulo M
  int c = (int)(((int64_t)g * kLanes + lane) % M);
  const int dc = (int)(((int64_t)G * kLanes) % M);
  for (int r = g; r < rounds; r += G) {
    const int k = r * kLanes + lane;
    const bool active = k < nsym;
    // the load that does not depend on the search
    const uint64_t wi = (uint64_t)ptr + lane;
    const uint32_t wpre = (err == 0 && wi < nwords) ? (uint32_t)words[wi] : 0u;

    int s = S >> 1;  // what a block in error decodes
    bool bad = false;
    uint32_t excess = 0;
    if (err == 0) {
      const uint32_t slot = x & 0xFFFFu;
      if (active) {
        int l = 0, h = S;  // largest s with cum[s] <= slot; cum[S] = 65536 is above every slot
        uint32_t start, end;
        if (kResident) {
          const uint16_t* row = lds + c * pitch;
          while (h - l > 1) {
            const int mid = (l + h) >> 1;
            if ((uint32_t)row[mid] <= slot)
              l = mid;
            else
              h = mid;
          }
          start = row[l];
          end = l + 1 == S ? 65536u : (uint32_t)row[l + 1];
        } else {
          const uint32_t* row = tables + (int64_t)c * S1;
          while (h - l > 1) {
            const int mid = (l + h) >> 1;
            if (row[mid] <= slot)
              l = mid;
            else
              h = mid;
          }
          start = row[l];
          end = row[l + 1];
        }
        x = (end - start) * (x >> 16) + slot - start;
        s = l;
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
      // escapes: the same rule on a second cursor
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
      int64_t v = (int64_t)s + lo;
      if (s == 0) v -= excess;
      if (s == S - 1) v += excess;
      out[k] = (float)v;  // k < nsym <= z_len - zb
    }
    if (__any(bad)) err |= LIC_RANS_ERR_RANGE;
    c += dc;
    if (c >= M) c -= M;
  }
  st[lane] = x;
  if (lane == 0) {
    st[kLanes] = ptr;
    st[kLanes + 1] = eptr;
    st[kLanes + 2] = err;
  }
}

}  // namespace

LIC_EXPORT int lic_rans_z_pick(const uint32_t* tables, int32_t M, int32_t lo, int32_t S, const int32_t* z, int64_t n,
                               uint32_t* sf, uint32_t* exc, uint32_t* err, lic_stream_t stream) {
  if (!tables || !z || !sf || !exc || !err) return LIC_ERR_INVALID;
  if (M <= 0 || S < 2 || n <= 0 || n % M) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(sf) |
       reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(err)) & 3)
    return LIC_ERR_INVALID;
  if (S > LIC_RANS_Z_MAX_S || M > LIC_RANS_Z_MAX_M || n > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rans_z_pick_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, tables, M, lo, S, z,
                     n, sf, exc, err);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_z_decode_path(int32_t M, int32_t S) {
  if (M <= 0 || S < 2) return LIC_ERR_INVALID;
  if (S > LIC_RANS_Z_MAX_S || M > LIC_RANS_Z_MAX_M) return LIC_ERR_UNSUPPORTED;
  return (int64_t)M * z_pitch(S) * 2 <= LIC_RANS_Z_LDS_BYTES ? LIC_RANS_Z_RESIDENT : LIC_RANS_Z_GLOBAL;
}

LIC_EXPORT int lic_rans_z_decode(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                 const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                 const uint32_t* tables, int32_t M, int32_t lo, int32_t S, int32_t nimg, int32_t G,
                                 const int64_t* nsym, const int64_t* z_base, float* z, int64_t z_len, int32_t path,
                                 lic_stream_t stream) {
  if (!streams || !stream_off || !stream_bytes || !escapes || !esc_off || !state || !tables || !nsym || !z_base || !z)
    return LIC_ERR_INVALID;
  if (M <= 0 || S < 2 || nimg <= 0 || z_len <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if (path != LIC_RANS_Z_AUTO && path != LIC_RANS_Z_RESIDENT && path != LIC_RANS_Z_GLOBAL) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(streams) | reinterpret_cast<uintptr_t>(escapes) |
       reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(z)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(stream_off) | reinterpret_cast<uintptr_t>(stream_bytes) |
       reinterpret_cast<uintptr_t>(esc_off) | reinterpret_cast<uintptr_t>(nsym) | reinterpret_cast<uintptr_t>(z_base)) & 7)
    return LIC_ERR_INVALID;
  if (S > LIC_RANS_Z_MAX_S || M > LIC_RANS_Z_MAX_M || (int64_t)nimg * G > 65535 || z_len > ((int64_t)1 << 40))
    return LIC_ERR_UNSUPPORTED;
  const int pitch = z_pitch(S);
  const int64_t lds_bytes = (int64_t)M * pitch * 2;
  const bool fits = lds_bytes <= LIC_RANS_Z_LDS_BYTES;
  if (path == LIC_RANS_Z_RESIDENT && !fits) return LIC_ERR_INVALID;
  auto launch = [&](auto kernel, size_t shared) {
    hipLaunchKernelGGL(kernel, dim3(nimg * G), dim3(kLanes), shared, (hipStream_t)stream, streams, stream_off,
                       stream_bytes, escapes, esc_off, state, tables, M, lo, S, pitch, G, nsym, z_base, z, z_len);
  };
  if (path == LIC_RANS_Z_GLOBAL || !fits)
    launch(rans_z_decode_kernel<false>, 0);
  else
    launch(rans_z_decode_kernel<true>, (size_t)lds_bytes);
  return lic_check_launch();
}
