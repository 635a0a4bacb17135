// The transposed-tile epilogue of the bf16 direct and fused kernels: igemm_bf16_kernel<FUSE> (lic_gemm_bf16.hip),
// stem_gdn_bf16_kernel (lic_stem_bf16.hip), halo_conv_bf16_kernel / halo_convt_bf16_kernel (lic_halo_bf16.h,
// lic_halot_bf16.h) and, for the primitives, gdn_bwd_bf16_kernel (lic_gdn_bf16.hip).  Inlined device code only: no
// state, no LDS of its own, no kernels.
//
// These kernels run their MFMAs with the operands swapped, so the accumulators hold the TRANSPOSED tile: lane
// (li, lh) = (lane & 31, lane >> 5) owns pixel li and, of every 32-channel tile, channels 8 g + 4 lh + {0..3}
// (g = 0..3; accumulator register 4 g + j).  Bias, rounding, LeakyReLU and the GDN finish are then element-wise, and
// one v_permlane32_swap per dword pair turns a lane's 4 + 4 channels into 8 consecutive ones: 16-byte stores, and --
// the same exchange -- one lane's share of a 16-deep MFMA B operand in lic_pack_weight_bf16_kperm's K order.
//
// conv -> GDN / IGDN in one launch (LIC_EPI_CONV_GDN / CONV_IGDN; Components.py:10-15) is three steps per pixel:
//   1. x = conv + bias rounded to bf16 (what the backward pass reads), kept in the accumulators as the rounded
//      value; x^2 rounded to bf16 again: the pool's B operand;
//   2. norm^T = gamma_eff . (x^2)^T, an MFMA contraction in fp32 (the caller's: operands from L2, LDS or registers);
//   3. norm + beta_eff in fp32 (stored rounded to bf16 where asked for), y = x * norm^-1/2 (IGDN: ^+1/2) from the
//      fp32 norm, rounded to bf16.
// These ROUNDING POINTS are what makes the fused and the two-launch paths agree, what lic_gdn_bwd_bf16_recompute
// reproduces and what every declared bf16 tolerance rests on: they are defined here and nowhere else
// (tests/test_gpu_bf16_epilogue_bits.py pins the bits).  The element-wise parts are written with 2-wide vectors
// (v_pk_add/mul_f32, v_cvt_pk_bf16_f32): at 2^26 outputs per launch every VALU instruction per element is 1.7 us.
//
// Register arrays: tiles and packs are passed by reference to fixed-size arrays and indexed with compile-time
// constants only (every loop below unrolls), so nothing here is runtime-indexed or address-taken -- that would move
// it to scratch, and the halo kernels run one wave per SIMD on all 512 registers.
#pragma once
#include "lic_common.h"

typedef __bf16 bf16_t;
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// two floats -> one dword of two bf16 (round to nearest even), element 0 in the low half
__device__ __forceinline__ unsigned pack2(f32x2 v) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// ... and back.  They take the dword BY VALUE on purpose: __builtin_bit_cast on a vector-element lvalue
// (`__builtin_bit_cast(unsigned, v[i])`) reads element 0 of the vector with this clang -- copy the element to a
// scalar first, as passing it here does.
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// Lanes li and li + 32 exchange halves of four packed dwords.  Forward (accumulator layout in): a lane's channel
// pairs of g = 2 s, 2 s + 1 become 8 consecutive channels 16 s + 8 lh + {0..7}.  Backward (8 consecutive channels
// of a 16-channel group in): the kperm operand {0..3, 8..11} / {4..7, 12..15}.  Every lane must execute it.
__device__ __forceinline__ u32x4 swap_dword_pairs(unsigned p0, unsigned p1, unsigned p2, unsigned p3) {
  const u32x2 r0 = __builtin_amdgcn_permlane32_swap(p0, p2, false, false);
  const u32x2 r1 = __builtin_amdgcn_permlane32_swap(p1, p3, false, false);
  return u32x4{r0[0], r1[0], r0[1], r1[1]};
}

// a lane's 16 channels of the 32-channel tile at channel `cb` as 8 bf16 pairs -> two 16-byte stores
__device__ __forceinline__ void store_tile_swapped(bf16_t* base, long ld, long opix, bool rok, int cb, int lh,
                                                   const unsigned (&pk)[8]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u32x4 o = swap_dword_pairs(pk[4 * s], pk[4 * s + 1], pk[4 * s + 2], pk[4 * s + 3]);
    if (rok) *reinterpret_cast<u32x4*>(base + opix * ld + cb + 16 * s + 8 * lh) = o;
  }
}

// step 1 of one tile.  bias(g) = the f32x4 of channels 8 g + 4 lh + {0..3}; it is called once per g, in order, right
// in front of the group's arithmetic, so a caller that loads there keeps its loads where they were (loading the
// four up front cost the 192-channel stem 18 spilled registers) and a caller that has them in registers returns them.
template <class Bias>
__device__ __forceinline__ void gdn_fwd_square_tile(f32x16& acc, Bias bias, unsigned (&xpk)[8], unsigned (&sqpk)[8]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 bs = bias(g);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x2 v = {acc[4 * g + 2 * h] + bs[2 * h], acc[4 * g + 2 * h + 1] + bs[2 * h + 1]};
      const unsigned pk = pack2(v);
      xpk[2 * g + h] = pk;
      const f32x2 xb = {bf16_lo(pk), bf16_hi(pk)};
      acc[4 * g + 2 * h] = xb[0];
      acc[4 * g + 2 * h + 1] = xb[1];
      sqpk[2 * g + h] = pack2(xb * xb);
    }
  }
}

// step 3 of one tile; beta(g) as bias(g) above, x = the tile step 1 left in the accumulators.  `inv` (IGDN) is a
// std::true_type / std::false_type where the caller dispatched on it, a bool where it is only known at run time.
template <class Beta, class Inv>
__device__ __forceinline__ void gdn_fwd_finish_tile(const f32x16& nacc, Beta beta, const f32x16& x, Inv inv,
                                                    unsigned (&npk)[8], unsigned (&ypk)[8]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 be = beta(g);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x2 nv = {nacc[4 * g + 2 * h] + be[2 * h], nacc[4 * g + 2 * h + 1] + be[2 * h + 1]};
      npk[2 * g + h] = pack2(nv);
      const f32x2 f = {inv ? __builtin_amdgcn_sqrtf(nv[0]) : __builtin_amdgcn_rsqf(nv[0]),
                       inv ? __builtin_amdgcn_sqrtf(nv[1]) : __builtin_amdgcn_rsqf(nv[1])};
      const f32x2 xv = {x[4 * g + 2 * h], x[4 * g + 2 * h + 1]};
      ypk[2 * g + h] = pack2(xv * f);
    }
  }
}

// The plain finish of one tile: + bias, LeakyReLU as max(v, slope v) (slope 1 = none), then fp32 stores of a lane's
// 4 + 4 + 4 + 4 channels or bf16 through the swap.
__device__ __forceinline__ void plain_finish_tile(const f32x16& acc, const f32x4 (&bs)[4], float sl, bool of32, void* out,
                                                  long ld, long opix, bool rok, int cb, int lh) {
  f32x4 v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    v[g] = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]} + bs[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[g][e] = __builtin_fmaxf(v[g][e], v[g][e] * sl);
  }
  if (of32) {
    if (rok) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + opix * ld + cb + 8 * g + 4 * lh) = v[g];
    }
  } else {
    unsigned pk[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      pk[2 * g] = pack2(f32x2{v[g][0], v[g][1]});
      pk[2 * g + 1] = pack2(f32x2{v[g][2], v[g][3]});
    }
    store_tile_swapped(reinterpret_cast<bf16_t*>(out), ld, opix, rok, cb, lh, pk);
  }
}

// ---- the epilogues of the halo-resident kernels (2 x 2 waves; wave (wm, wn) holds 4 row tiles x TW channel tiles:
// tile (a, t) = pixel li of the workgroup tile's row 4 wm + a, channels 32 (wn TW + t) ..).  `p` is the kernel's
// parameter block (IgemmHParams); out_pixel(a, rok) maps row tile a of this lane to its output pixel index and says
// whether it lies inside the image (0 otherwise: the address is formed, the store is not made).  lh, wn, wm are the
// callers' OPAQUE copies: hipcc otherwise hoists every address below out of the tile loop and spills it across the
// main loop.

// a wave's bias (or zeros) in ONE batch: a load per tile would drain the stores in flight every time
template <int TW, class Params>
__device__ __forceinline__ void halo_load_bias(const Params& p, int lh, int wn, f32x4 (&bs)[TW][4]) {
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) bs[t][g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (p.bias) {
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) bs[t][g] = *reinterpret_cast<const f32x4*>(p.bias + (wn * TW + t) * 32 + 4 * lh + 8 * g);
  }
}

// Plain: bias / LeakyReLU / bf16 or fp32 out, straight from the registers -- no LDS (the halo buffers already hold
// the next tile's first chunk).
template <int TW, class Params, class OutPixel>
__device__ __forceinline__ void halo_epilogue_plain(const f32x16 (&acc)[4][TW], const Params& p, int lh, int wn,
                                                    OutPixel out_pixel) {
  f32x4 bs[TW][4];
  halo_load_bias<TW>(p, lh, wn, bs);
  const float sl = p.epilogue == LIC_EPI_LEAKY ? p.slope : 1.0f;
  const bool of32 = p.out_f32 != 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    bool rok;
    const long opix = out_pixel(a, rok);
#pragma unroll
    for (int t = 0; t < TW; ++t)
      plain_finish_tile(acc[a][t], bs[t], sl, of32, p.out, p.out_ld, opix, rok, (wn * TW + t) * 32, lh);
  }
}

// Fused conv -> GDN / IGDN.  A wave holds only HALF the channels of its pixels, so the x^2 fragments are exchanged
// through LDS: every wave writes its 16 fragments (4 row tiles x TW channel tiles x 2 k steps, lane-linear 1 KiB
// each) into the exchange area `xch` ([wm][a][channel tile 0..2TW-1][k step][64 lanes][16 B], 64 KiB at TW = 2, 96 at
// 3: LDS the main loop does not have in flight now), one barrier, and reads back all the fragments of its pixel
// half -- its partner's lanes own the same pixels, so the exchange is a lane-wise copy.  The barrier at the end keeps
// the next writer (the caller's halo DMA, or the next call) out of the area until every wave has read.
//   * gamma_eff^T fragments and beta_eff are requested up front, all at once: a load in front of each pool MFMA /
//     each finish tile was one exposed L2 round trip after the other at one wave per SIMD -- the fused epilogue took
//     14 us per tile that way;
//   * pool and finish run two row tiles at a time: the register budget (the conv accumulators stay live as x).
template <int TW, class Params, class OutPixel>
__device__ __forceinline__ void halo_epilogue_fused(f32x16 (&acc)[4][TW], const Params& p, unsigned char* xch, int lane,
                                                    int lh, int wn, int wm, OutPixel out_pixel) {
  const bool inv = p.epilogue == LIC_EPI_CONV_IGDN;
  auto frag_at = [&](int wmi, int a, int tt, int s2) { return xch + ((((wmi * 4 + a) * (2 * TW) + tt) * 2 + s2) * 64 + lane) * 16; };
  f32x4 bs[TW][4];
  halo_load_bias<TW>(p, lh, wn, bs);
  const bf16_t* gA = p.aux + lane * 8;
  const int ntile = p.Npad >> 5;
  bf16x8 gfr[2 * TW][2][TW];
#pragma unroll
  for (int tt = 0; tt < 2 * TW; ++tt)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int t = 0; t < TW; ++t)
        gfr[tt][s2][t] = *reinterpret_cast<const bf16x8*>(gA + ((long)tt * ntile + (wn * TW + t)) * 1024 + s2 * 512);
  f32x4 be[TW][4];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) be[t][g] = *reinterpret_cast<const f32x4*>(p.beta + (wn * TW + t) * 32 + 4 * lh + 8 * g);
  // 1. x -> bf16 (kept in the accumulators), x^2 -> bf16 -> LDS; the conv output if asked for
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    bool rok;
    const long opix = out_pixel(a, rok);
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      unsigned xpk[8], sqpk[8];
      gdn_fwd_square_tile(acc[a][t], [&](int g) { return bs[t][g]; }, xpk, sqpk);
      if (p.out3) store_tile_swapped(p.out3, p.out3_ld, opix, rok, (wn * TW + t) * 32, lh, xpk);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
        *reinterpret_cast<u32x4*>(frag_at(wm, a, wn * TW + t, s2)) =
            u32x4{sqpk[4 * s2], sqpk[4 * s2 + 1], sqpk[4 * s2 + 2], sqpk[4 * s2 + 3]};
    }
  }
  __syncthreads();
  // 2. + 3. two row tiles at a time: pool over all 2 TW input channel tiles, then finish
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    f32x16 nacc[2][TW];
#pragma unroll
    for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) nacc[a2][t][r] = 0.0f;
#pragma unroll
    for (int tt = 0; tt < 2 * TW; ++tt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 b2[2];
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2) b2[a2] = *reinterpret_cast<const bf16x8*>(frag_at(wm, 2 * hh + a2, tt, s2));
#pragma unroll
        for (int t = 0; t < TW; ++t) {
          const bf16x8 a2f = gfr[tt][s2][t];
#pragma unroll
          for (int a2 = 0; a2 < 2; ++a2)
            nacc[a2][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2f, b2[a2], nacc[a2][t], 0, 0, 0);
        }
      }
#pragma unroll
    for (int a2 = 0; a2 < 2; ++a2) {
      const int a = 2 * hh + a2;
      bool rok;
      const long opix = out_pixel(a, rok);
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const int cb = (wn * TW + t) * 32;
        unsigned npk[8], ypk[8];
        gdn_fwd_finish_tile(nacc[a2][t], [&](int g) { return be[t][g]; }, acc[a][t], inv, npk, ypk);
        if (p.out2) store_tile_swapped(p.out2, p.out2_ld, opix, rok, cb, lh, npk);
        store_tile_swapped(reinterpret_cast<bf16_t*>(p.out), p.out_ld, opix, rok, cb, lh, ypk);
      }
    }
  }
  __syncthreads();
}
