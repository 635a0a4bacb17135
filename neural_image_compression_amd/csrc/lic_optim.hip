// lic_adam_run: the Adam update of EVERY parameter of a model in one launch.
//
// The reference trains with torch.optim.Adam (Main.ipynb; Trainer.py:81-86 calls optimizer.step()); on the GPU
// that is nine multi-tensor launches per step that read / write each of the four per-parameter streams several
// times (measured 0.25 ms for the 57 MB of config 2: 7 streams x 57 MB would take 0.07 ms at HBM speed).  This
// kernel does torch's arithmetic (non-amsgrad, L2 weight decay) for all parameters in one pass: block b looks
// up its job (parameter, gradient, exp_avg, exp_avg_sq, length) in a device-resident table, as lic_prep_run does.
//   g' = g + weight_decay * p;   m += (1 - beta1) * (g' - m);   v = beta2 * v + (1 - beta2) * g' * g';
//   p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps)
// The bias corrections are computed on the host from the step count, as torch's default (non-capturable) path does.
#include "lic_common.h"
#include <math.h>

#include <type_traits>

namespace {
constexpr int AD_ITEMS = 4096;  // elements per block

// Gradient tensors are new allocations every step, so their addresses travel as kernel arguments (copied at
// launch time: no host -> device table copy that a host running several steps ahead could overwrite too early).
template <int NG>
struct AdamGrads {
  const float* g[NG];
};

// the one rounding of g * coefficient that an unfused `grad.mul_(coefficient)` performs.  The empty asm makes the
// product a value the optimiser cannot look into: hipcc would otherwise contract it into the multiply-adds of the
// update, or pair it with `weight_decay * p` in one packed multiply and so undo the contraction adam_kernel gets
// there -- either way other bits than the unfused order gives
__device__ __forceinline__ float scale_once(float g, float coef) {
  float r = g * coef;
  asm volatile("" : "+v"(r));
  return r;
}

// e + w * (p - e) in three separately rounded fp32 operations (lic.h: lic_adam_run_ema).  `p` arrives as a value
// the optimiser cannot look into, so nothing of the average reaches back into how p itself was formed, and the
// product is opaque as in scale_once: a fused multiply-add would round once where the statement rounds twice
__device__ __forceinline__ float ema_once(float e, float p, float w) {
  asm volatile("" : "+v"(p));
  float s = __fmul_rn(w, __fsub_rn(p, e));
  asm volatile("" : "+v"(s));
  return __fadd_rn(e, s);
}

struct AdamScalars {
  float lerp_w, beta2, one_minus_beta2, eps, weight_decay, step_size, bc2_sqrt;
};

// the job whose block range [block0, block0 + nblocks) holds this block (asked by thread 0 of every kernel here)
__device__ __forceinline__ int adam_job_of_block(const lic_adam_job* jobs, int njobs) {
  int lo = 0, hi = njobs - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].block0 <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// What a block works on: its job, that job's gradient and average (nullptr where the kernel reads no such table, or
// the table has no entry), and the block's elements [begin, end) of the job's n.
struct AdamWork {
  float *p, *m, *v, *e;
  const float* g;
  long begin, end;
};

// The ONE prologue of every kernel on the lic_adam_plan partition: thread 0 finds the job, hands it to the block
// through shared memory with the addresses that travel beside the table (GRADS / EMA: which of the two tables the
// kernel reads), and every thread derives its range.
template <bool GRADS, bool EMA>
__device__ __forceinline__ AdamWork adam_work_of_block(const lic_adam_job* jobs, int njobs, const float* const* grads,
                                                       float* const* ema) {
  __shared__ lic_adam_job job;
  __shared__ int s_blk;
  __shared__ const float* s_g;
  __shared__ float* s_e;
  if (threadIdx.x == 0) {
    const int lo = adam_job_of_block(jobs, njobs);
    job = jobs[lo];
    s_blk = blockIdx.x - jobs[lo].block0;
    s_g = GRADS ? grads[lo] : nullptr;
    s_e = EMA ? ema[lo] : nullptr;
  }
  __syncthreads();
  const long n = job.n;
  const long begin = (long)s_blk * AD_ITEMS, end = begin + AD_ITEMS < n ? begin + AD_ITEMS : n;
  return AdamWork{job.p, job.m, job.v, s_e, s_g, begin, end};
}

// The update of one block's <= AD_ITEMS elements: the ONE body of every adam_kernel<NG, SCALED, EMA> (SCALED: the
// gradient times `coef`, rounded once, on the way in; EMA: one more stream `e`, read and written beside p).
// Whether p / g / m / v take the 16-byte path does not depend on `e`: a misaligned average
// is read and written element by element inside it.  (The pointers carry no __restrict__: as function arguments
// it would be honoured, unlike on the locals the kernels had before this body was shared, and the scalar loops of
// the existing kernels would be interleaved and fused differently -- other bits.)
template <bool SCALED, bool EMA>
__device__ __forceinline__ void adam_block(float* p, const float* g, float* m, float* v, float* ea, long begin,
                                           long end, const AdamScalars k, float coef, float ema_w) {
  const float lerp_w = k.lerp_w, beta2 = k.beta2, one_minus_beta2 = k.one_minus_beta2, eps = k.eps;
  const float weight_decay = k.weight_decay, step_size = k.step_size, bc2_sqrt = k.bc2_sqrt;
  auto upd = [&](float& pw, float graw, float& mw, float& vw) {
    float gw = SCALED ? scale_once(graw, coef) : graw;
    if (weight_decay != 0.0f) gw += weight_decay * pw;
    mw = lerp_w < 0.5f ? mw + lerp_w * (gw - mw) : gw - (gw - mw) * (1.0f - lerp_w);  // torch.lerp
    vw = vw * beta2;
    vw = vw + (one_minus_beta2 * gw) * gw;
    const float denom = sqrtf(vw) / bc2_sqrt + eps;
    pw = pw - step_size * (mw / denom);
  };
  auto one = [&](long i) {
    upd(p[i], g[i], m[i], v[i]);
    if (EMA) ea[i] = ema_once(ea[i], p[i], ema_w);
  };
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (vec) {
    const bool evec = EMA && (reinterpret_cast<uintptr_t>(ea) & 15) == 0;
    const long e4 = begin + ((end - begin) & ~3L);
    for (long i = begin + threadIdx.x * 4L; i < e4; i += 256 * 4) {
      // (the average is loaded in front of, and updated behind, the statements the three kernels share, under
      // branches of its own: what the compiler pairs and fuses among those statements stays what it is without it)
      f32x4 ew = {0.0f, 0.0f, 0.0f, 0.0f};
      if (evec) ew = *reinterpret_cast<const f32x4*>(ea + i);
      f32x4 pw = *reinterpret_cast<const f32x4*>(p + i), mw = *reinterpret_cast<const f32x4*>(m + i);
      f32x4 vw = *reinterpret_cast<const f32x4*>(v + i);
      const f32x4 gw = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pw[e], me = mw[e], ve = vw[e];
        upd(pe, gw[e], me, ve);
        pw[e] = pe;
        mw[e] = me;
        vw[e] = ve;
      }
      *reinterpret_cast<f32x4*>(p + i) = pw;
      *reinterpret_cast<f32x4*>(m + i) = mw;
      *reinterpret_cast<f32x4*>(v + i) = vw;
      if (evec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ew[e] = ema_once(ew[e], pw[e], ema_w);
        *reinterpret_cast<f32x4*>(ea + i) = ew;
      } else if (EMA) {  // an average off the 16-byte grid: element by element, from the p just stored
#pragma unroll 1
        for (int e = 0; e < 4; ++e) ea[i + e] = ema_once(ea[i + e], p[i + e], ema_w);
      }
    }
    for (long i = e4 + threadIdx.x; i < end; i += 256) one(i);
  } else {
    for (long i = begin + threadIdx.x; i < end; i += 256) one(i);
  }
}

// lic_adam_run (neither), lic_adam_run_scaled (SCALED) and lic_adam_run_ema (EMA, with or without SCALED).
// SCALED: the gradient is scaled by clip_state[1] (layout below, at grad_norm_finish_kernel) on the way in, and
// nothing is done at all when the caller asked for non-finite steps to be skipped and clip_state[2] says this one is.
// EMA: the exponential moving average of every parameter is updated from the new p while it is in registers.  The
// averages are persistent buffers: their addresses live in a device table `ema` (one per job, NULL = no average for
// that tensor) and do not travel per step.  36 bytes per element instead of 28: e is read and written once.
// (The seven scalars travel as seven arguments: with an AdamScalars passed by value hipcc contracts a multiply and
// an add of the scalar loops into a multiply-add in every instantiation -- other bits.)
template <int NG, bool SCALED, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(const lic_adam_job* jobs, int njobs, const AdamGrads<NG> grads,
                                                   float lerp_w, float beta2, float one_minus_beta2, float eps,
                                                   float weight_decay, float step_size, float bc2_sqrt,
                                                   const float* __restrict__ clip_state, int skip_nonfinite,
                                                   float* const* __restrict__ ema, float ema_w) {
  const AdamScalars k{lerp_w, beta2, one_minus_beta2, eps, weight_decay, step_size, bc2_sqrt};
  float coef = 1.0f;
  if (SCALED) {
    if (skip_nonfinite && reinterpret_cast<const unsigned*>(clip_state)[2] != 0u) return;  // (uniform over the grid)
    coef = clip_state[1];
  }
  const AdamWork w = adam_work_of_block<true, EMA>(jobs, njobs, grads.g, ema);
  if (EMA && w.e) adam_block<SCALED, true>(w.p, w.g, w.m, w.v, w.e, w.begin, w.end, k, coef, ema_w);
  else adam_block<SCALED, false>(w.p, w.g, w.m, w.v, nullptr, w.begin, w.end, k, coef, 0.0f);
}

// lic_grad_norm_partial / lic_grad_norm_finish / lic_adam_run_scaled: the global-norm clipping of the usual recipe
// for these models (torch.nn.utils.clip_grad_norm_ before optimizer.step(): a handful of foreach launches that
// read every gradient twice and write it once, and ~240 small host-side calls) as one more read of the gradients
// over the block partition lic_adam_run already has, a one-workgroup sum, and a scale applied inside the update.
// Every sum is a double sum of fixed shape: thread t of a block takes elements at a fixed stride, the 64 lanes of
// a wave combine in a butterfly, thread 0 adds the 4 wave sums in wave order; no atomics.  The norm is therefore
// a function of the gradients, the job order and AD_ITEMS only, bitwise the same from run to run.
__device__ __forceinline__ double block_sum_d(double acc, double* s_wave) {
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];  // (wave order; every thread forms the same sum)
}

template <int NG>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const lic_adam_job* jobs, int njobs,
                                                                const AdamGrads<NG> grads, double* partials) {
  __shared__ double s_wave[4];
  const AdamWork w = adam_work_of_block<true, false>(jobs, njobs, grads.g, nullptr);
  const float* __restrict__ g = w.g;
  const long begin = w.begin, end = w.end;
  double acc = 0.0;
  auto add = [&](float gw) { acc += (double)gw * (double)gw; };  // (the product of two floats is exact in double)
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const long e4 = begin + ((end - begin) & ~3L);
    for (long i = begin + threadIdx.x * 4L; i < e4; i += 256 * 4) {
      const f32x4 gw = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) add(gw[e]);
    }
    for (long i = e4 + threadIdx.x; i < end; i += 256) add(g[i]);
  } else {
    for (long i = begin + threadIdx.x; i < end; i += 256) add(g[i]);
  }
  const double total = block_sum_d(acc, s_wave);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// clip_state: [0] fp32 norm, [1] fp32 coefficient, [2] u32 norm-is-not-finite, [3] u32 skipped steps so far
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, long nparts,
                                                               float max_norm, int unbounded, int count_skip,
                                                               float* clip_state) {
  __shared__ double s_wave[4];
  double acc = 0.0;
  for (long i = threadIdx.x; i < nparts; i += 256) acc += partials[i];
  const double total = block_sum_d(acc, s_wave);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);  // (correctly rounded double sqrt, then ONE rounding to fp32)
    // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0) on an fp32 tensor; like torch.clamp, a NaN stays a NaN
    const float c = max_norm / (norm + 1e-6f);
    const float coef = unbounded ? 1.0f : (c > 1.0f ? 1.0f : c);
    const unsigned bad = isfinite(norm) ? 0u : 1u;
    unsigned* flags = reinterpret_cast<unsigned*>(clip_state);
    const unsigned skipped = flags[3] + (count_skip ? bad : 0u);
    clip_state[0] = norm;
    clip_state[1] = coef;
    flags[2] = bad;
    flags[3] = skipped;
  }
}

// lic_swap_run: p <-> e for every job that has an average, on the lic_adam_plan partition; loads and stores only
__global__ __launch_bounds__(256) void swap_kernel(const lic_adam_job* jobs, int njobs, float* const* __restrict__ ema) {
  const AdamWork w = adam_work_of_block<false, true>(jobs, njobs, nullptr, ema);
  float* __restrict__ p = w.p;
  float* __restrict__ e = w.e;
  if (!e) return;  // (uniform over the block)
  const long begin = w.begin, end = w.end;
  auto one = [&](long i) {
    const float t = p[i];
    p[i] = e[i];
    e[i] = t;
  };
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(e)) & 15) == 0) {
    const long e4 = begin + ((end - begin) & ~3L);
    for (long i = begin + threadIdx.x * 4L; i < e4; i += 256 * 4) {
      const f32x4 pw = *reinterpret_cast<const f32x4*>(p + i), ew = *reinterpret_cast<const f32x4*>(e + i);
      *reinterpret_cast<f32x4*>(p + i) = ew;
      *reinterpret_cast<f32x4*>(e + i) = pw;
    }
    for (long i = e4 + threadIdx.x; i < end; i += 256) one(i);
  } else {
    for (long i = begin + threadIdx.x; i < end; i += 256) one(i);
  }
}
}  // namespace

// fills block0 / nblocks of a host-side job array; returns the grid size of lic_adam_run (or a negative status)
LIC_EXPORT int64_t lic_adam_plan(lic_adam_job* jobs, int32_t njobs) {
  if (!jobs || njobs <= 0) return LIC_ERR_INVALID;
  long blocks = 0;
  for (int i = 0; i < njobs; ++i) {
    if (!jobs[i].p || !jobs[i].m || !jobs[i].v || jobs[i].n <= 0) return LIC_ERR_INVALID;  // (g is passed per launch)
    jobs[i].nblocks = (int)((jobs[i].n + AD_ITEMS - 1) / AD_ITEMS);
    if (blocks + jobs[i].nblocks > 0x7FFFFFFFL) return LIC_ERR_UNSUPPORTED;
    jobs[i].block0 = (int)blocks;
    blocks += jobs[i].nblocks;
  }
  return blocks;
}

namespace {
// the kernel-argument block of one launch: njobs gradient addresses (HOST array of DEVICE pointers), the rest null
template <int NG>
AdamGrads<NG> adam_grads(const float* const* grads, int njobs) {
  AdamGrads<NG> a;
  for (int i = 0; i < NG; ++i) a.g[i] = i < njobs ? grads[i] : nullptr;
  return a;
}

// f(std::integral_constant<int, NG>) for the smallest argument block that holds njobs (<= 448) addresses
template <class F>
void with_grads_tier(int njobs, F&& f) {
  if (njobs <= 96) f(std::integral_constant<int, 96>{});
  else if (njobs <= 224) f(std::integral_constant<int, 224>{});
  else f(std::integral_constant<int, 448>{});
}

// What the entries refuse.  Where two rules apply to one call: every null pointer, size and range of an entry's own
// arguments is LIC_ERR_INVALID and is looked at before grads_status, whose LIC_ERR_UNSUPPORTED for more than 448
// jobs in turn comes before a null entry among the gradients.
bool bad_partition(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks) {
  return !jobs_device || njobs <= 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFFL;
}

bool bad_ema_table(float* const* ema_device) {
  return !ema_device || (reinterpret_cast<uintptr_t>(ema_device) & (sizeof(float*) - 1)) != 0;
}

int grads_status(const float* const* grads_host, int32_t njobs) {
  if (njobs > 448) return LIC_ERR_UNSUPPORTED;
  for (int i = 0; i < njobs; ++i)
    if (!grads_host[i]) return LIC_ERR_INVALID;
  return LIC_OK;
}

// The one launch path of lic_adam_run, lic_adam_run_scaled and lic_adam_run_ema: clip_state and ema_device may each
// be NULL, and pick the kernel.  grads_host: njobs gradient pointers, in job order; njobs <= 448.
// (scalars are doubles: torch derives 1 - beta, lr / bias_correction1 and sqrt(bias_correction2) in Python doubles
// and rounds once to fp32; 1.0f - 0.999f is 1.7e-5 away from float(0.001))
int adam_run(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks, const float* const* grads_host,
             double lr, double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
             double bias_correction2, float* const* ema_device, double ema_weight, const float* clip_state,
             int32_t skip_nonfinite, lic_stream_t stream) {
  if (bad_partition(jobs_device, njobs, total_blocks) || !grads_host) return LIC_ERR_INVALID;
  if (!(bias_correction1 > 0.0) || !(bias_correction2 > 0.0)) return LIC_ERR_INVALID;
  if (const int status = grads_status(grads_host, njobs)) return status;
  const AdamScalars k{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay,
                      (float)(lr / bias_correction1), (float)sqrt(bias_correction2)};
  const float w = (float)ema_weight;
  const int skip = clip_state && skip_nonfinite ? 1 : 0;
  with_grads_tier(njobs, [&](auto tier) {
    constexpr int NG = decltype(tier)::value;
    const AdamGrads<NG> a = adam_grads<NG>(grads_host, njobs);
    auto launch = [&](auto scaled, auto ema) {
      hipLaunchKernelGGL((adam_kernel<NG, decltype(scaled)::value, decltype(ema)::value>), dim3((unsigned)total_blocks),
                         dim3(256), 0, (hipStream_t)stream, jobs_device, (int)njobs, a, k.lerp_w, k.beta2,
                         k.one_minus_beta2, k.eps, k.weight_decay, k.step_size, k.bc2_sqrt, clip_state, skip, ema_device,
                         w);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (clip_state) ema_device ? launch(yes, yes) : launch(yes, no);
    else ema_device ? launch(no, yes) : launch(no, no);
  });
  return lic_check_launch();
}
}  // namespace

LIC_EXPORT int lic_adam_run(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                            const float* const* grads_host, double lr, double beta1, double beta2, double eps,
                            double weight_decay, double bias_correction1, double bias_correction2, lic_stream_t stream) {
  return adam_run(jobs_device, njobs, total_blocks, grads_host, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                  bias_correction2, nullptr, 0.0, nullptr, 0, stream);
}

// the first half of torch.nn.utils.clip_grad_norm_ (torch._foreach_norm over every gradient): block b of the
// lic_adam_plan partition writes the double sum of squares of its <= 4096 gradient elements to partials[b].
// Same job table, same grads_host as lic_adam_run; partials: total_blocks doubles (DEVICE)
LIC_EXPORT int lic_grad_norm_partial(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                                     const float* const* grads_host, double* partials, lic_stream_t stream) {
  if (bad_partition(jobs_device, njobs, total_blocks) || !grads_host || !partials) return LIC_ERR_INVALID;
  if (const int status = grads_status(grads_host, njobs)) return status;
  with_grads_tier(njobs, [&](auto tier) {
    constexpr int NG = decltype(tier)::value;
    hipLaunchKernelGGL((grad_norm_partial_kernel<NG>), dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       jobs_device, (int)njobs, adam_grads<NG>(grads_host, njobs), partials);
  });
  return lic_check_launch();
}

// the second half (vector_norm of the per-tensor norms, max_norm / (total_norm + 1e-6), clamp): one workgroup sums
// the nparts partials of ALL groups in a fixed order and writes the 4 dwords of clip_state (DEVICE; see lic.h).
// max_norm +inf: the norm is computed and the coefficient is exactly 1
LIC_EXPORT int lic_grad_norm_finish(const double* partials, int64_t nparts, double max_norm, int32_t count_skip,
                                    float* clip_state, lic_stream_t stream) {
  if (!partials || !clip_state || nparts <= 0) return LIC_ERR_INVALID;
  if (!(max_norm >= 0.0)) return LIC_ERR_INVALID;  // (negative or NaN)
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)nparts,
                     (float)max_norm, isinf(max_norm) ? 1 : 0, count_skip ? 1 : 0, clip_state);
  return lic_check_launch();
}

// lic_adam_run on gradients scaled by clip_state[1] (the `g.mul_(clip_coef_clamped)` of clip_grad_norm_, rounded to
// fp32 once as there, without the pass over memory); skip_nonfinite: leave p / m / v alone when clip_state[2] is set.
// clip_state is read on the device: the host does not wait for the norm
LIC_EXPORT int lic_adam_run_scaled(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                                   const float* const* grads_host, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, double bias_correction1, double bias_correction2,
                                   const float* clip_state, int32_t skip_nonfinite, lic_stream_t stream) {
  if (!clip_state) return LIC_ERR_INVALID;
  return adam_run(jobs_device, njobs, total_blocks, grads_host, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                  bias_correction2, nullptr, 0.0, clip_state, skip_nonfinite, stream);
}

// lic_adam_run (clip_state NULL) or lic_adam_run_scaled (clip_state given) that also moves the exponential moving
// average of every parameter: e += w * (p_new - e), w = (float)ema_weight, three fp32 roundings.  ema_device: DEVICE
// array of njobs float* (NULL entry: that tensor has no average); a skipped step leaves e alone as it does p / m / v
LIC_EXPORT int lic_adam_run_ema(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                                const float* const* grads_host, double lr, double beta1, double beta2, double eps,
                                double weight_decay, double bias_correction1, double bias_correction2,
                                float* const* ema_device, double ema_weight, const float* clip_state,
                                int32_t skip_nonfinite, lic_stream_t stream) {
  if (bad_ema_table(ema_device)) return LIC_ERR_INVALID;
  if (!(ema_weight >= 0.0 && ema_weight <= 1.0)) return LIC_ERR_INVALID;  // (a NaN too)
  return adam_run(jobs_device, njobs, total_blocks, grads_host, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                  bias_correction2, ema_device, ema_weight, clip_state, skip_nonfinite, stream);
}

// p <-> e, element by element, for every job whose ema_device entry is not NULL: the averaged weights become the
// live ones (and back).  The job table and partition of lic_adam_run; m / v / g are not touched
LIC_EXPORT int lic_swap_run(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                            float* const* ema_device, lic_stream_t stream) {
  if (bad_partition(jobs_device, njobs, total_blocks) || bad_ema_table(ema_device)) return LIC_ERR_INVALID;
  if (njobs > 448) return LIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(swap_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device,
                     njobs, ema_device);
  return lic_check_launch();
}
