// Host side of the interleaved rANS coder behind include/lic_codec.h ("rANS-64"): 64 coder
// states of 32 bits in [2^16, 2^32), 16-bit probabilities, renormalisation by 16-bit words, at most one word per
// symbol per lane.  Inside a wavefront step symbol k belongs to lane k % 64 and round k / 64; rounds never
// straddle steps.  The encoder is the decoder run backwards (steps, rounds and lanes last to first, words written
// towards lower addresses); the device decoder of the same format is lic_rans_decode_step (lic_rans.hip).
// Out-of-window values code the edge symbol and put their excess into a separate list of uint32, in symbol order.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "lic_codec.h"

#define LIC_CODEC_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kLanes = 64;
constexpr uint32_t kLow = 1u << 16;  // lower bound of a state

inline bool table_ok(const uint32_t* t, int S) { return t[0] == 0 && t[S] == 65536u; }

inline void put_u32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}
inline uint32_t get_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the step lengths must be non-negative and add up to n
bool steps_ok(const int64_t* step_len, int64_t nsteps, int64_t n) {
  if (nsteps < 0 || (nsteps > 0 && !step_len)) return false;
  int64_t sum = 0;
  for (int64_t t = 0; t < nsteps; ++t) {
    if (step_len[t] < 0 || step_len[t] > n - sum) return false;
    sum += step_len[t];
  }
  return sum == n;
}

// every table_of entry must name one of the T tables before anything is indexed with it (NULL: table i, no T)
bool table_of_ok(const int32_t* table_of, int32_t T, int64_t n) {
  if (!table_of) return true;
  if (T < 1) return n == 0;
  for (int64_t i = 0; i < n; ++i)
    if (table_of[i] < 0 || table_of[i] >= T) return false;
  return true;
}

// The one encoder: symbol i codes with table table_of[i] of `tables` (table_of == NULL: table i).
int encode(const uint32_t* tables, const int32_t* table_of, int32_t T, int32_t S, const int32_t* idx, int64_t n,
           const int64_t* step_len, int64_t nsteps, uint8_t* out, size_t cap, size_t* nbytes, uint32_t* esc_out,
           size_t esc_cap, size_t* nesc) {
  if (!out || !nbytes || !nesc || S < 2 || n < 0 || (n > 0 && (!tables || !idx))) return LIC_CODEC_ERR_INVALID;
  if (!steps_ok(step_len, nsteps, n)) return LIC_CODEC_ERR_INVALID;
  if (!table_of_ok(table_of, T, n)) return LIC_CODEC_ERR_INVALID;
  if (cap < (size_t)kLanes * 4) return LIC_CODEC_ERR_OVERFLOW;
  // escapes leave in symbol order: a forward pass of their own
  size_t ne = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t v = idx[i];
    if (v > 0 && v < S - 1) continue;
    if (ne >= esc_cap || !esc_out) return LIC_CODEC_ERR_OVERFLOW;
    esc_out[ne++] = v <= 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)((int64_t)v - (S - 1));
  }
  uint32_t x[kLanes];
  for (int l = 0; l < kLanes; ++l) x[l] = kLow;
  // words are written from the end of `out` towards lower addresses and moved behind the states afterwards
  size_t wpos = cap & ~(size_t)1;
  const size_t wfloor = (size_t)kLanes * 4;
  int64_t base = n;
  for (int64_t t = nsteps - 1; t >= 0; --t) {
    base -= step_len[t];
    for (int64_t k = step_len[t] - 1; k >= 0; --k) {  // rounds last to first, lanes 63 down to 0
      const int64_t i = base + k;
      const uint32_t* tb = tables + (size_t)(table_of ? table_of[i] : i) * (size_t)(S + 1);
      if (!table_ok(tb, S)) return LIC_CODEC_ERR_INVALID;
      const int32_t v = idx[i];
      const int32_t s = v <= 0 ? 0 : (v >= S - 1 ? S - 1 : v);
      if (tb[s + 1] <= tb[s] || tb[s + 1] - tb[s] >= 65536u) return LIC_CODEC_ERR_INVALID;
      const uint32_t start = tb[s], freq = tb[s + 1] - start;
      uint32_t xl = x[k % kLanes];
      if ((uint64_t)xl >= ((uint64_t)freq << 16)) {
        if (wpos < wfloor + 2) return LIC_CODEC_ERR_OVERFLOW;
        wpos -= 2;
        out[wpos] = (uint8_t)xl, out[wpos + 1] = (uint8_t)(xl >> 8);
        xl >>= 16;
      }
      x[k % kLanes] = ((xl / freq) << 16) + (xl % freq) + start;
    }
  }
  const size_t wbytes = (cap & ~(size_t)1) - wpos;
  memmove(out + wfloor, out + wpos, wbytes);
  for (int l = 0; l < kLanes; ++l) put_u32(out + 4 * l, x[l]);
  *nbytes = wfloor + wbytes;
  *nesc = ne;
  return LIC_CODEC_OK;
}

// The one decoder, with encode's table rule.
int decode(const uint8_t* in, size_t nbytes, const uint32_t* esc, size_t nesc, const uint32_t* tables,
           const int32_t* table_of, int32_t T, int32_t S, int64_t n, const int64_t* step_len, int64_t nsteps,
           int32_t* idx_out) {
  if (!in || S < 2 || n < 0 || (n > 0 && (!tables || !idx_out)) || (nesc > 0 && !esc)) return LIC_CODEC_ERR_INVALID;
  if (!steps_ok(step_len, nsteps, n)) return LIC_CODEC_ERR_INVALID;
  if (!table_of_ok(table_of, T, n)) return LIC_CODEC_ERR_INVALID;
  if (nbytes < (size_t)kLanes * 4 || (nbytes & 1)) return LIC_CODEC_ERR_CORRUPT;
  uint32_t x[kLanes];
  for (int l = 0; l < kLanes; ++l) {
    x[l] = get_u32(in + 4 * l);
    if (x[l] < kLow) return LIC_CODEC_ERR_CORRUPT;
  }
  const uint8_t* words = in + (size_t)kLanes * 4;
  const size_t nwords = (nbytes - (size_t)kLanes * 4) / 2;
  size_t ptr = 0, eptr = 0;
  int64_t base = 0;
  for (int64_t t = 0; t < nsteps; ++t) {
    // lanes in ascending order within a round is ascending k: the rank rule of the format, serialised
    for (int64_t k = 0; k < step_len[t]; ++k) {
      const int64_t i = base + k;
      const uint32_t* tb = tables + (size_t)(table_of ? table_of[i] : i) * (size_t)(S + 1);
      if (!table_ok(tb, S)) return LIC_CODEC_ERR_INVALID;
      uint32_t xl = x[k % kLanes];
      const uint32_t slot = xl & 0xFFFFu;
      int lo = 0, hi = S;  // largest s with tb[s] <= slot
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb[mid] <= slot)
          lo = mid;
        else
          hi = mid;
      }
      if (tb[lo + 1] <= tb[lo] || slot >= tb[lo + 1]) return LIC_CODEC_ERR_INVALID;
      xl = (tb[lo + 1] - tb[lo]) * (xl >> 16) + slot - tb[lo];
      if (xl < kLow) {
        if (ptr >= nwords) return LIC_CODEC_ERR_CORRUPT;
        xl = (xl << 16) | (uint32_t)words[2 * ptr] | ((uint32_t)words[2 * ptr + 1] << 8);
        ++ptr;
      }
      x[k % kLanes] = xl;
      int64_t v = lo;
      if (lo == 0 || lo == S - 1) {
        if (eptr >= nesc) return LIC_CODEC_ERR_CORRUPT;
        const uint32_t ex = esc[eptr++];
        v = lo == 0 ? -(int64_t)ex : (int64_t)(S - 1) + ex;
        if (v < INT32_MIN || v > INT32_MAX) return LIC_CODEC_ERR_CORRUPT;
      }
      idx_out[i] = (int32_t)v;
    }
    base += step_len[t];
  }
  // an intact stream is used up exactly and leaves every state where the encoder started it
  if (ptr != nwords || eptr != nesc) return LIC_CODEC_ERR_CORRUPT;
  for (int l = 0; l < kLanes; ++l)
    if (x[l] != kLow) return LIC_CODEC_ERR_CORRUPT;
  return LIC_CODEC_OK;
}

}  // namespace

LIC_CODEC_EXPORT size_t lic_rans_bound(int64_t n) {
  // the 64 final states + at most one 16-bit word per symbol
  return n < 0 ? 0 : (size_t)kLanes * 4 + (size_t)n * 2;
}

LIC_CODEC_EXPORT int lic_rans_encode(const uint32_t* tables, int32_t S, const int32_t* idx, int64_t n,
                                     const int64_t* step_len, int64_t nsteps, uint8_t* out, size_t cap,
                                     size_t* nbytes, uint32_t* esc_out, size_t esc_cap, size_t* nesc) {
  return encode(tables, nullptr, 0, S, idx, n, step_len, nsteps, out, cap, nbytes, esc_out, esc_cap, nesc);
}

LIC_CODEC_EXPORT int lic_rans_decode(const uint8_t* in, size_t nbytes, const uint32_t* esc, size_t nesc,
                                     const uint32_t* tables, int32_t S, int64_t n, const int64_t* step_len,
                                     int64_t nsteps, int32_t* idx_out) {
  return decode(in, nbytes, esc, nesc, tables, nullptr, 0, S, n, step_len, nsteps, idx_out);
}

LIC_CODEC_EXPORT int lic_rans_encode_shared(const uint32_t* tables, const int32_t* table_of, int32_t T, int32_t S,
                                            const int32_t* idx, int64_t n, const int64_t* step_len, int64_t nsteps,
                                            uint8_t* out, size_t cap, size_t* nbytes, uint32_t* esc_out,
                                            size_t esc_cap, size_t* nesc) {
  return encode(tables, table_of, T, S, idx, n, step_len, nsteps, out, cap, nbytes, esc_out, esc_cap, nesc);
}

LIC_CODEC_EXPORT int lic_rans_decode_shared(const uint8_t* in, size_t nbytes, const uint32_t* esc, size_t nesc,
                                            const uint32_t* tables, const int32_t* table_of, int32_t T, int32_t S,
                                            int64_t n, const int64_t* step_len, int64_t nsteps, int32_t* idx_out) {
  return decode(in, nbytes, esc, nesc, tables, table_of, T, S, n, step_len, nsteps, idx_out);
}

LIC_CODEC_EXPORT double lic_rans_ideal_bits(const uint32_t* tables, const int32_t* table_of, int32_t S,
                                            const int32_t* idx, int64_t n) {
  if (!tables || !idx || S < 2 || n < 0) return -1.0;
  double bits = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t* t = tables + (size_t)(table_of ? table_of[i] : i) * (size_t)(S + 1);
    const int32_t v = idx[i];
    const int32_t s = v <= 0 ? 0 : (v >= S - 1 ? S - 1 : v);
    bits += 16.0 - log2((double)(t[s + 1] - t[s]));
    if (s == 0 || s == S - 1) bits += 32.0;
  }
  return bits;
}
