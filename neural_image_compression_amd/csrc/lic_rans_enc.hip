// lic_rans_encode_pick + lic_rans_encode / lic_rans_encode_groups: the encoder of the "rANS-64" and "rANS-64 x G" y
// streams (include/lic_codec.h) run where lic_gmm_cdf_tables has left the tables, so codec.ContextCodec.compress
// copies streams, not tables, to the host.  Byte for byte the host encoder of lic_rans.cpp: same streams, same
// escape lists.
// lic_rans_encode_pick_ragged + lic_rans_encode_ragged, at the end of the file, are the same pair for images of different
// sizes in one launch each (codec.ContextCodec.compress_images).
//
// An rANS encoder never searches: symbol k needs cum[s] and cum[s+1] of its own table, and neither its table nor
// its symbol depends on a coder state.  So the work splits in two launches:
//  * pick (one thread per symbol, any grid) resolves wavefront order -> raster pixel, clamps the symbol, validates
//    the table as the host does and leaves one uint32 (start << 16 | freq) and one escape word per symbol, in
//    coding order;
//  * encode (one wave per image, lane l owns state l; in rans_encode_groups_kernel one wave per image and group, the
//    wave of group g visiting the rounds whose index inside their step is g, g + G, ...) walks those words.
//    Escapes first, forward: ballot, rank, a wave-uniform cursor.  Then the states, backward: steps and rounds
//    last to first; the lanes whose state
//    would overflow share the stream with one ballot (who emits), one popcount below the lane (rank) and a
//    wave-uniform cursor that moves towards lower addresses.  Ascending lane id is reading order, which is what the
//    host's "lanes 63 down to 0, towards lower addresses" produces.
//
// Latency on a single wave paces the second kernel, so nothing but the compare, the ballot, the word store and the
// divide sits on the state's dependent chain: the start|freq words of the next kRing rounds are already in
// registers (a ring the unrolled loop indexes statically), and the step lengths are read by the producer side of
// that ring, kRing rounds ahead of their use.  An inactive lane of a partial round carries the word 0 (a real one
// has freq >= 1), so the consumer needs no round geometry at all.
//
// Nothing outside the given buffers is read or written: pick checks every order entry before it indexes with it,
// encode checks the step lengths (non-negative, summing to nsym) before it walks them and compares the word cursor
// with the slot's first word, and the escape cursor with the list's capacity, before every store.
#include "lic_common.h"

namespace {

constexpr int kLanes = LIC_RANS_LANES;
constexpr int kStateWords = LIC_RANS_STATE_WORDS;
constexpr int kRing = 8;                    // rounds of start|freq words in flight
constexpr uint32_t kNoEscape = 0xFFFFFFFFu;  // the largest real excess is 2^31
constexpr uint32_t kHarmless = 1u;           // start 0, freq 1: what a symbol in error codes

__global__ __launch_bounds__(256) void rans_pick_kernel(const uint32_t* __restrict__ tables,
                                                        const int32_t* __restrict__ center,
                                                        const int32_t* __restrict__ y,
                                                        const int64_t* __restrict__ order, int32_t P, int32_t M,
                                                        int32_t W, int32_t nsym, uint32_t* __restrict__ sf,
                                                        uint32_t* __restrict__ exc, uint32_t* state) {
  const int b = blockIdx.y;
  const int S1 = 2 * W + 2, S = S1 - 1;
  bool bad = false;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nsym; k += (int64_t)gridDim.x * blockDim.x) {
    const int pos = (int)k / M, c = (int)k - pos * M;
    const int64_t pix = order[pos];
    uint32_t word = kHarmless, excess = kNoEscape;
    if (pix >= 0 && pix < P) {
      const int64_t i = ((int64_t)b * P + pix) * M + c;
      // two's complement, as the host path's int32 tensor arithmetic
      const int32_t idx = (int32_t)((uint32_t)y[i] - (uint32_t)center[i] + (uint32_t)W);
      const int32_t s = idx <= 0 ? 0 : (idx >= S - 1 ? S - 1 : idx);
      if (idx <= 0) excess = (uint32_t)(-(int64_t)idx);
      if (idx >= S - 1) excess = (uint32_t)((int64_t)idx - (S - 1));
      const uint32_t* row = tables + i * S1;
      const uint32_t first = row[0], last = row[S], start = row[s], end = row[s + 1];
      if (first == 0u && last == 65536u && end > start && end - start < 65536u && start < 65536u)
        word = (start << 16) | (end - start);
      else
        bad = true;
    } else {
      bad = true;
    }
    sf[(int64_t)b * nsym + k] = word;
    exc[(int64_t)b * nsym + k] = excess;
  }
  // one atomic per wave at the most; the loop has ended for every lane here
  if (__any(bad) && (threadIdx.x & (kLanes - 1)) == 0)
    atomicOr(state + (size_t)b * kStateWords + kLanes + 2, LIC_RANS_ERR_RANGE);
}

// Producer side of the ring: the rounds of an image last to first, as (first symbol, active lanes).  Wave-uniform.
struct RoundWalk {
  const int64_t* step_len;
  int64_t t;     // steps [0, t) are still whole
  int32_t base;  // first symbol of step t
  int32_t rem;   // symbols of step t not yet handed out, counted from its start
  __device__ __forceinline__ bool next(int32_t& k0, int32_t& n) {
    while (rem == 0 && t > 0) {
      --t;
      rem = (int32_t)step_len[t];
      base -= rem;
    }
    if (rem == 0) return false;
    const int32_t head = (rem - 1) & ~(kLanes - 1);  // where the step's last remaining round starts
    k0 = base + head;
    n = rem - head;
    rem = head;
    return true;
  }
};

// The step lengths must be non-negative and add up to nsym before anything is indexed with them.  True if they do;
// rounds is then the wave's number of rounds, count(n) of them in a step of n symbols.  Wave-uniform.
template <class Count>
__device__ __forceinline__ bool step_lengths_ok(const int64_t* __restrict__ step_len, int64_t nsteps, int32_t nsym,
                                                int lane, Count count, int64_t& rounds) {
  int64_t sum = 0;
  bool okl = true;
  rounds = 0;
  for (int64_t t = lane; t < nsteps; t += kLanes) {
    const int64_t n = step_len[t];
    if (n < 0 || n > nsym)
      okl = false;
    else
      sum += n, rounds += count(n);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, kLanes);
    rounds += __shfl_xor(rounds, o, kLanes);
  }
  return __all(okl) && sum == nsym;
}

// What a wave leaves of lengths it refuses: the initial state, no word, no escape and the error word
__device__ __forceinline__ void refuse_steps(uint32_t* st, int lane, uint32_t err) {
  st[lane] = 1u << 16;
  if (lane == 0) st[kLanes] = 0u, st[kLanes + 1] = 0u, st[kLanes + 2] = err | LIC_RANS_ERR_RANGE;
}

// States, backward: the wave codes the `rounds` rounds that walk hands out, last to first, into the slot's words
// [.., wend) and stores its state, word count, escape count (nesc, counted by the caller) and error word.
template <class Walk>
__device__ __forceinline__ void encode_states(const uint32_t* __restrict__ sf, Walk walk, int64_t rounds,
                                              uint16_t* __restrict__ wbuf, uint32_t wend, uint32_t nesc, uint32_t err,
                                              uint32_t* st, int lane) {
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t wpos = wend;  // in 16-bit words from the slot's start; the words so far are [wpos, wend)
  uint32_t x = 1u << 16;
  // the ring: a round's raw words and its number of active lanes.  Exactly one load per round, taken or not (an
  // idle lane reads word 0; it is dropped where the round is consumed): a load under a branch cannot be counted,
  // and every wait for the ring would then wait for all of it
  uint32_t ring[kRing];
  int32_t live[kRing];
  auto fetch = [&](int j) {
    int32_t k0 = 0, n = 0;
    walk.next(k0, n);  // leaves (0, 0) once the walk is over
    ring[j] = sf[lane < n ? k0 + lane : 0];
    live[j] = n;
  };
#pragma unroll
  for (int j = 0; j < kRing; ++j) fetch(j);
  for (int64_t r = 0; r < rounds; r += kRing) {
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      const uint32_t w = lane < live[j] ? ring[j] : 0u;
      fetch(j);  // the round kRing ahead; no lane is live once the walk is over
      const uint32_t freq = w & 0xFFFFu, start = w >> 16;
      const bool active = freq != 0u;
      const bool emit = active && (x >> 16) >= freq;
      const unsigned long long mask = __ballot(emit);
      const uint32_t cnt = (uint32_t)__popcll(mask);
      if (cnt > wpos) {  // cannot happen in a slot of one word per symbol of the wave's rounds (lic_rans_bound)
        err |= LIC_RANS_ERR_RANGE;
      } else {
        wpos -= cnt;
        if (emit) {
          wbuf[wpos + (uint32_t)__popcll(mask & below)] = (uint16_t)x;
          x >>= 16;
        }
      }
      const uint32_t f = active ? freq : 1u;
      const uint32_t q = x / f;
      if (active) x = (q << 16) + (x - q * f) + start;
    }
  }
  st[lane] = x;
  if (lane == 0) st[kLanes] = wend - wpos, st[kLanes + 1] = nesc, st[kLanes + 2] = err;
}

__global__ __launch_bounds__(64) void rans_encode_kernel(const uint32_t* __restrict__ sf,
                                                         const uint32_t* __restrict__ exc,
                                                         const int64_t* __restrict__ step_len, int64_t nsteps,
                                                         int32_t nsym, uint8_t* __restrict__ words, int64_t slot,
                                                         uint32_t* __restrict__ esc_out, uint32_t* state) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  sf += (int64_t)b * nsym;
  exc += (int64_t)b * nsym;
  esc_out += (int64_t)b * nsym;
  uint32_t* st = state + (size_t)b * kStateWords;
  uint32_t err = st[kLanes + 2];

  int64_t rounds;
  if (!step_lengths_ok(step_len, nsteps, nsym, lane, [](int64_t n) { return (n + kLanes - 1) / kLanes; }, rounds))
    return refuse_steps(st, lane, err);

  // escapes, forward, in symbol order: rounds play no part in their order
  uint32_t nesc = 0;
  for (uint32_t k0 = 0; k0 < (uint32_t)nsym; k0 += kRing * kLanes) {
    uint32_t e[kRing];
#pragma unroll
    for (int j = 0; j < kRing; ++j) {  // all loads first: none depends on the cursor
      const uint32_t k = k0 + j * kLanes + lane;
      e[j] = k < (uint32_t)nsym ? exc[k] : kNoEscape;
    }
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      const bool edge = e[j] != kNoEscape;
      const unsigned long long mask = __ballot(edge);
      if (edge) esc_out[nesc + (uint32_t)__popcll(mask & below)] = e[j];
      nesc += (uint32_t)__popcll(mask);
    }
  }

  encode_states(sf, RoundWalk{step_len, nsteps, nsym, 0}, rounds,
                reinterpret_cast<uint16_t*>(words + (int64_t)b * slot), (uint32_t)(slot >> 1), nesc, err, st, lane);
}

// The rounds of one group, as (first symbol, active lanes): round r of a step is the group's if r % G == g.
// Wave-uniform.
struct GroupRounds {
  const int64_t* step_len;
  int32_t g, G;
  __device__ __forceinline__ int32_t count(int32_t n) const {  // the group's rounds in a step of n symbols
    const int32_t R = (n + kLanes - 1) / kLanes;
    return R > g ? (int32_t)((uint32_t)(R - 1 - g) / (uint32_t)G) + 1 : 0;
  }
};

// RoundWalk for one group: its rounds last to first.
struct GroupWalk {
  GroupRounds of;
  int64_t t;     // steps [0, t) are still whole
  int32_t base;  // first symbol of step t
  int32_t len;   // symbols of step t
  int32_t r;     // the group's last round of step t not yet handed out; below 0: none
  __device__ __forceinline__ bool next(int32_t& k0, int32_t& n) {
    while (r < 0 && t > 0) {
      --t;
      len = (int32_t)of.step_len[t];
      base -= len;
      r = of.g + (of.count(len) - 1) * of.G;  // g - G < 0 for a step without a round of this group
    }
    if (r < 0) return false;
    k0 = base + r * kLanes;
    n = min(kLanes, len - r * kLanes);
    r -= of.G;
    return true;
  }
};

// The same rounds first to last: the order of the escape list.
struct GroupWalkForward {
  GroupRounds of;
  int64_t nsteps;
  int64_t t;     // the next step to open
  int32_t base;  // first symbol of the open step
  int32_t len;   // symbols of the open step
  int32_t R;     // its rounds
  int32_t r;     // the group's first round of the open step not yet handed out; R or above: none
  __device__ __forceinline__ bool next(int32_t& k0, int32_t& n) {
    while (r >= R && t < nsteps) {
      base += len;
      len = (int32_t)of.step_len[t++];
      R = (len + kLanes - 1) / kLanes;
      r = of.g;
    }
    if (r >= R) return false;
    k0 = base + r * kLanes;
    n = min(kLanes, len - r * kLanes);
    r += of.G;
    return true;
  }
};

// rans_encode_kernel with one wave per (image, group).  The same length check, ring and divide; the two walks hand out
// the group's rounds only, and the escape list has a capacity of its own to compare with
__global__ __launch_bounds__(64) void rans_encode_groups_kernel(const uint32_t* __restrict__ sf,
                                                         const uint32_t* __restrict__ exc,
                                                         const int64_t* __restrict__ step_len, int64_t nsteps,
                                                         int32_t G, int32_t nsym, uint8_t* __restrict__ words,
                                                         int64_t slot, uint32_t* __restrict__ esc_out,
                                                         uint32_t esc_cap, uint32_t* state) {
  // blk: the slot, escape list and state block of (image b, group g); sf and exc go by image
  const int blk = blockIdx.x, b = blk / G, g = blk - b * G, lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const GroupRounds of{step_len, g, G};
  sf += (int64_t)b * nsym;
  exc += (int64_t)b * nsym;
  esc_out += (int64_t)blk * esc_cap;
  uint32_t* st = state + (size_t)blk * kStateWords;
  uint32_t err = st[kLanes + 2];

  int64_t rounds;
  if (!step_lengths_ok(step_len, nsteps, nsym, lane, [&](int64_t n) { return (int64_t)of.count((int32_t)n); }, rounds))
    return refuse_steps(st, lane, err);

  // escapes, forward, in the symbol order of the group's rounds
  uint32_t nesc = 0;
  GroupWalkForward fwd{of, nsteps, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < rounds; r += kRing) {
    uint32_t e[kRing];
#pragma unroll
    for (int j = 0; j < kRing; ++j) {  // all loads first: none depends on the cursor, none sits under a branch
      int32_t k0 = 0, n = 0;
      fwd.next(k0, n);  // leaves (0, 0) once the walk is over
      const uint32_t v = exc[lane < n ? k0 + lane : 0];
      e[j] = lane < n ? v : kNoEscape;
    }
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      const bool edge = e[j] != kNoEscape;
      const unsigned long long mask = __ballot(edge);
      const uint32_t cnt = (uint32_t)__popcll(mask);
      // the list has room for the round's escapes or takes none of them; it cannot run out with one entry per symbol
      // of the group.  No branch around the store: the waits for e[] stay counted
      const bool room = cnt <= esc_cap - nesc;
      if (edge && room) esc_out[nesc + (uint32_t)__popcll(mask & below)] = e[j];
      nesc += room ? cnt : 0u;
      err |= room ? 0u : LIC_RANS_ERR_RANGE;
    }
  }

  encode_states(sf, GroupWalk{of, nsteps, nsym, 0, -1}, rounds,
                reinterpret_cast<uint16_t*>(words + (int64_t)blk * slot), (uint32_t)(slot >> 1), nesc, err, st, lane);
}

// ---- many images of different sizes in one launch each (codec.ContextCodec.compress_images) ----------------------
// Every image brings its own rows, steps, slots and lists; where they lie is read from descriptors on the device, so
// both kernels compare a descriptor with the lengths the entry was given before they address anything with it.

// rans_pick_kernel for the rows of a whole chunk: position q of the coding order belongs to image row_image[q], whose
// rows of tables, centres and symbols are [ROW0, ROW0 + P), and stands for raster pixel order[q] of that image.  The
// lanes of a wave may belong to different images, so every symbol in error reports for itself
__global__ __launch_bounds__(256) void rans_pick_ragged_kernel(
    const uint32_t* __restrict__ tables, const int32_t* __restrict__ center, const int32_t* __restrict__ y,
    int64_t total_rows, const int64_t* __restrict__ images, int32_t nimg, const int64_t* __restrict__ row_image,
    const int64_t* __restrict__ order, int32_t M, int32_t W, int32_t nsym, uint32_t* __restrict__ sf,
    uint32_t* __restrict__ exc, uint32_t* state) {
  const int S1 = 2 * W + 2, S = S1 - 1;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nsym; k += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = (int32_t)k / M, c = (int32_t)k - q * M;
    const int64_t b = row_image[q];
    uint32_t word = kHarmless, excess = kNoEscape;
    if (b >= 0 && b < nimg) {  // a row of no image has no error block to name
      const int64_t row0 = images[b * LIC_RANS_IMAGE_WORDS + LIC_RANS_IMAGE_ROW0];
      const int64_t P = images[b * LIC_RANS_IMAGE_WORDS + LIC_RANS_IMAGE_P];
      const int64_t pix = order[q];
      bool bad = true;
      if (row0 >= 0 && P >= 1 && row0 <= total_rows && P <= total_rows - row0 && q >= row0 && q - row0 < P &&
          pix >= 0 && pix < P) {
        const int64_t i = (row0 + pix) * M + c;
        // two's complement, as the host path's int32 tensor arithmetic
        const int32_t idx = (int32_t)((uint32_t)y[i] - (uint32_t)center[i] + (uint32_t)W);
        const int32_t s = idx <= 0 ? 0 : (idx >= S - 1 ? S - 1 : idx);
        if (idx <= 0) excess = (uint32_t)(-(int64_t)idx);
        if (idx >= S - 1) excess = (uint32_t)((int64_t)idx - (S - 1));
        const uint32_t* row = tables + i * S1;
        const uint32_t first = row[0], last = row[S], start = row[s], end = row[s + 1];
        if (first == 0u && last == 65536u && end > start && end - start < 65536u && start < 65536u) {
          word = (start << 16) | (end - start);
          bad = false;
        }
      }
      if (bad) atomicOr(state + (size_t)b * kStateWords + kLanes + 2, LIC_RANS_ERR_RANGE);
    }
    sf[k] = word;
    exc[k] = excess;
  }
}

// rans_encode_groups_kernel with one wave per (image, group) of images that differ in size: the image's range of sf /
// exc / step_len and the block's slot and escape list come from the two descriptor tables.  A wave whose descriptors
// do not fit the given lengths leaves what a wave leaves of step lengths it refuses; otherwise the same length check,
// walks, ring and divide
__global__ __launch_bounds__(64) void rans_encode_ragged_kernel(
    const uint32_t* __restrict__ sf, const uint32_t* __restrict__ exc, const int64_t* __restrict__ step_len,
    int64_t steps_len, const int64_t* __restrict__ images, const int64_t* __restrict__ blocks, int32_t G,
    int64_t total_rows, int32_t M, uint8_t* __restrict__ words, int64_t words_len, uint32_t* __restrict__ esc_out,
    int64_t esc_len, uint32_t* state) {
  const int blk = blockIdx.x, b = blk / G, g = blk - b * G, lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t* st = state + (size_t)blk * kStateWords;
  uint32_t err = st[kLanes + 2];

  const int64_t* im = images + (int64_t)b * LIC_RANS_IMAGE_WORDS;
  const int64_t* bl = blocks + (int64_t)blk * LIC_RANS_BLOCK_WORDS;
  const int64_t row0 = im[LIC_RANS_IMAGE_ROW0], P = im[LIC_RANS_IMAGE_P], step0 = im[LIC_RANS_IMAGE_STEP0],
                nsteps = im[LIC_RANS_IMAGE_NSTEPS];
  const int64_t word_off = bl[LIC_RANS_BLOCK_WORD_OFF], slot = bl[LIC_RANS_BLOCK_SLOT],
                esc_off = bl[LIC_RANS_BLOCK_ESC_OFF], cap = bl[LIC_RANS_BLOCK_ESC_CAP];
  // wave-uniform; every sum is written as a difference of checked terms, so none can overflow
  const bool fits = row0 >= 0 && P >= 1 && step0 >= 0 && nsteps >= 0 && word_off >= 0 && slot >= 4 && esc_off >= 0 &&
                    cap >= 1 && row0 <= total_rows && P <= total_rows - row0 && P <= (0x7FFFFFFFL - kLanes) / M &&
                    step0 <= steps_len && nsteps <= steps_len - step0 && (word_off & 3) == 0 && (slot & 3) == 0 &&
                    slot <= 0xFFFFFFFFL && word_off <= words_len && slot <= words_len - word_off &&
                    cap <= 0x7FFFFFFFL && esc_off <= esc_len && cap <= esc_len - esc_off;
  if (!fits) return refuse_steps(st, lane, err);

  const int32_t nsym = (int32_t)(P * M);
  const uint32_t esc_cap = (uint32_t)cap;
  step_len += step0;
  sf += row0 * M;
  exc += row0 * M;
  esc_out += esc_off;
  const GroupRounds of{step_len, g, G};

  int64_t rounds;
  if (!step_lengths_ok(step_len, nsteps, nsym, lane, [&](int64_t n) { return (int64_t)of.count((int32_t)n); }, rounds))
    return refuse_steps(st, lane, err);

  // escapes, forward, in the symbol order of the group's rounds: rans_encode_groups_kernel's loop
  uint32_t nesc = 0;
  GroupWalkForward fwd{of, nsteps, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < rounds; r += kRing) {
    uint32_t e[kRing];
#pragma unroll
    for (int j = 0; j < kRing; ++j) {  // all loads first: none depends on the cursor, none sits under a branch
      int32_t k0 = 0, n = 0;
      fwd.next(k0, n);  // leaves (0, 0) once the walk is over
      const uint32_t v = exc[lane < n ? k0 + lane : 0];
      e[j] = lane < n ? v : kNoEscape;
    }
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      const bool edge = e[j] != kNoEscape;
      const unsigned long long mask = __ballot(edge);
      const uint32_t cnt = (uint32_t)__popcll(mask);
      const bool room = cnt <= esc_cap - nesc;  // the round's escapes all fit or none is stored
      if (edge && room) esc_out[nesc + (uint32_t)__popcll(mask & below)] = e[j];
      nesc += room ? cnt : 0u;
      err |= room ? 0u : LIC_RANS_ERR_RANGE;
    }
  }

  encode_states(sf, GroupWalk{of, nsteps, nsym, 0, -1}, rounds, reinterpret_cast<uint16_t*>(words + word_off),
                (uint32_t)(slot >> 1), nesc, err, st, lane);
}

}  // namespace

LIC_EXPORT int lic_rans_encode_pick(const uint32_t* tables, const int32_t* center, const int32_t* y,
                                    const int64_t* order, int32_t B, int64_t P, int32_t M, int32_t W, uint32_t* sf,
                                    uint32_t* exc, uint32_t* state, lic_stream_t stream) {
  if (!tables || !center || !y || !order || !sf || !exc || !state) return LIC_ERR_INVALID;
  if (B <= 0 || P <= 0 || M <= 0 || W <= 0) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(center) | reinterpret_cast<uintptr_t>(y) |
       reinterpret_cast<uintptr_t>(sf) | reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(order) & 7) return LIC_ERR_INVALID;
  if (W > 64 || B > 65535) return LIC_ERR_UNSUPPORTED;
  if (P > 0x7FFFFFFFL || P * M > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  const int32_t nsym = (int32_t)(P * M);
  hipLaunchKernelGGL(rans_pick_kernel, dim3(ew_grid(nsym, 256), B), dim3(256), 0, (hipStream_t)stream, tables, center,
                     y, order, (int32_t)P, M, W, nsym, sf, exc, state);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_encode(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len, int64_t nsteps,
                               int32_t B, int64_t nsym, uint8_t* words, int64_t slot, uint32_t* esc_out,
                               uint32_t* state, lic_stream_t stream) {
  if (!sf || !exc || !step_len || !words || !esc_out || !state) return LIC_ERR_INVALID;
  if (B <= 0 || nsym <= 0 || nsteps <= 0) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(sf) | reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(words) |
       reinterpret_cast<uintptr_t>(esc_out) | reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(step_len) & 7) return LIC_ERR_INVALID;
  if (nsym > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  // a slot holds the words only: at most one per symbol, whole dwords so that every image's slot is aligned
  if (slot < 2 * nsym || (slot & 3) || slot > 0xFFFFFFFFL) return LIC_ERR_INVALID;
  hipLaunchKernelGGL(rans_encode_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, sf, exc, step_len, nsteps,
                     (int32_t)nsym, words, slot, esc_out, state);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_encode_groups(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len,
                                      int64_t nsteps, int32_t B, int32_t G, int64_t nsym, uint8_t* words,
                                      int64_t slot, uint32_t* esc_out, int64_t esc_cap, uint32_t* state,
                                      lic_stream_t stream) {
  if (!sf || !exc || !step_len || !words || !esc_out || !state) return LIC_ERR_INVALID;
  if (B <= 0 || nsym <= 0 || nsteps <= 0) return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(sf) | reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(words) |
       reinterpret_cast<uintptr_t>(esc_out) | reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(step_len) & 7) return LIC_ERR_INVALID;
  if (nsym > 0x7FFFFFFFL - kLanes || (int64_t)B * G > 65535) return LIC_ERR_UNSUPPORTED;
  // whole dwords, so that every block's slot is aligned; what the two sizes must be at least is the caller's to know
  // (lic.h): the kernel compares before every store
  if (slot < 4 || (slot & 3) || slot > 0xFFFFFFFFL || esc_cap < 1 || esc_cap > 0x7FFFFFFFL) return LIC_ERR_INVALID;
  hipLaunchKernelGGL(rans_encode_groups_kernel, dim3(B * G), dim3(kLanes), 0, (hipStream_t)stream, sf, exc, step_len,
                     nsteps, G, (int32_t)nsym, words, slot, esc_out, (uint32_t)esc_cap, state);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_encode_pick_ragged(const uint32_t* tables, const int32_t* center, const int32_t* y,
                                           int64_t total_rows, const int64_t* images, int32_t nimg,
                                           const int64_t* row_image, const int64_t* order, int32_t M, int32_t W,
                                           uint32_t* sf, uint32_t* exc, uint32_t* state, lic_stream_t stream) {
  if (!tables || !center || !y || !images || !row_image || !order || !sf || !exc || !state) return LIC_ERR_INVALID;
  if (total_rows <= 0 || nimg <= 0 || M <= 0 || W <= 0) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(center) | reinterpret_cast<uintptr_t>(y) |
       reinterpret_cast<uintptr_t>(sf) | reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(row_image) |
       reinterpret_cast<uintptr_t>(order)) & 7)
    return LIC_ERR_INVALID;
  if (W > 64 || nimg > 65535) return LIC_ERR_UNSUPPORTED;
  if (total_rows > 0x7FFFFFFFL || total_rows * M > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  const int32_t nsym = (int32_t)(total_rows * M);
  hipLaunchKernelGGL(rans_pick_ragged_kernel, dim3(ew_grid(nsym, 256)), dim3(256), 0, (hipStream_t)stream, tables,
                     center, y, total_rows, images, nimg, row_image, order, M, W, nsym, sf, exc, state);
  return lic_check_launch();
}

LIC_EXPORT int lic_rans_encode_ragged(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len,
                                      int64_t steps_len, const int64_t* images, const int64_t* blocks, int32_t nimg,
                                      int32_t G, int64_t total_rows, int32_t M, uint8_t* words, int64_t words_len,
                                      uint32_t* esc_out, int64_t esc_len, uint32_t* state, lic_stream_t stream) {
  if (!sf || !exc || !step_len || !images || !blocks || !words || !esc_out || !state) return LIC_ERR_INVALID;
  if (nimg <= 0 || total_rows <= 0 || M <= 0 || steps_len <= 0 || words_len <= 0 || esc_len <= 0)
    return LIC_ERR_INVALID;
  if (G < 1 || G > LIC_RANS_MAX_GROUPS) return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(sf) | reinterpret_cast<uintptr_t>(exc) | reinterpret_cast<uintptr_t>(words) |
       reinterpret_cast<uintptr_t>(esc_out) | reinterpret_cast<uintptr_t>(state)) & 3)
    return LIC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(step_len) | reinterpret_cast<uintptr_t>(images) |
       reinterpret_cast<uintptr_t>(blocks)) & 7)
    return LIC_ERR_INVALID;
  if ((int64_t)nimg * G > 65535) return LIC_ERR_UNSUPPORTED;
  if (total_rows > 0x7FFFFFFFL || total_rows * M > 0x7FFFFFFFL - kLanes) return LIC_ERR_UNSUPPORTED;
  // what every image's and block's descriptor must satisfy is the kernel's to check: they live on the device
  hipLaunchKernelGGL(rans_encode_ragged_kernel, dim3(nimg * G), dim3(kLanes), 0, (hipStream_t)stream, sf, exc,
                     step_len, steps_len, images, blocks, G, total_rows, M, words, words_len, esc_out, esc_len, state);
  return lic_check_launch();
}
