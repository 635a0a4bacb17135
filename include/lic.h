/*
 * lic.h -- C ABI of liblic_hip.so: the MI355X (gfx950) implementation of the
 * analysis/synthesis + hyperprior + likelihood + rate-distortion hot path of
 * achraf-15/neural_image_compression.
 *
 * The reference has no FFI: its "operator API" for this path is torch's ATen ops reached from
 * the nn.Module surface.  Each entry point below names the reference call
 * site(s) whose device arithmetic it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *  - All pointers are DEVICE pointers to fp32 unless stated.  Activations are NHWC: element
 *    (b,h,w,c) of a tensor with row pitch `ld` (floats per pixel, ld >= C) lives at
 *    ((b*H + h)*W + w)*ld + c.  `ld` lets two producers write disjoint channel ranges of one
 *    buffer: the reference's torch.cat([phi, psi]) (Models.py:73) is not materialised in the fp32
 *    path -- the context conv and the hyper decoder's last conv write the two halves of one tensor
 *    (models.py; the backward's two gradient slices are still made contiguous by a copy each).
 *  - The library never allocates, frees or synchronises; every launch goes to `stream`
 *    (a hipStream_t passed as void*), so every call is hipGraph-capturable.  Workspaces are
 *    caller-owned; sizes come from the *_workspace_bytes queries.
 *  - Return value: LIC_OK (0) or a negative lic_status.  Nothing throws or exits.
 *  - Re-entrant: no global mutable state; safe to call from autograd's backward thread.
 */
#ifndef LIC_H
#define LIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIC_ABI_VERSION 4

typedef void* lic_stream_t; /* hipStream_t */

enum lic_status {
  LIC_OK = 0,
  LIC_ERR_INVALID = -1,     /* bad argument (null pointer, non-positive size, ...) */
  LIC_ERR_UNSUPPORTED = -2, /* geometry outside what the kernels implement */
  LIC_ERR_LAUNCH = -3,      /* hipLaunchKernel failed; see lic_last_hip_error() */
  LIC_ERR_WORKSPACE = -4    /* workspace too small */
};

/* epilogues of lic_igemm (fused into the producing kernel) */
enum lic_epilogue {
  LIC_EPI_NONE = 0,           /* v = acc + bias                                              */
  LIC_EPI_LEAKY = 1,          /* v = leaky(acc + bias); with res: out2 = v + res            */
  LIC_EPI_MUL_LEAKY_MASK = 2, /* v = acc * (aux > 0 ? 1 : slope)  (grad through in-place LeakyReLU) */
  LIC_EPI_GDN = 3,            /* n = acc + bias; out2 = n; v = aux * rsqrt(n)                 */
  LIC_EPI_IGDN = 4,           /* n = acc + bias; out2 = n; v = aux * sqrt(n)                  */
  LIC_EPI_GDN_BWD = 5,        /* v = aux * rsqrt(aux3) + 2 * aux2 * acc                       */
  LIC_EPI_IGDN_BWD = 6,       /* v = aux * sqrt(aux3)  + 2 * aux2 * acc                       */
  /* convolution + the GDN / IGDN that follows it, in one kernel (lic_igemm_fused_gdn_supported):
   *   x = acc + bias -> out3 (may be NULL);  n = aux2 + x^2 . aux -> out2 (may be NULL);  out = x * rsqrt(n) | x * sqrt(n)
   *   aux = gamma_eff^T packed by lic_pack_weight(taps=1, K=Cout, N=Cout), aux2 = beta_eff [Cout].
   *   Bitwise identical to LIC_EPI_NONE followed by a prologue=1 / LIC_EPI_GDN contraction launch. */
  LIC_EPI_CONV_GDN = 7,
  LIC_EPI_CONV_IGDN = 8
  /* for every epilogue except LEAKY a non-null `res` is added to v before the store */
};

/* ------------------------------------------------------------------------------------------
 * lic_igemm -- implicit-GEMM convolution family on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *   rows  = output pixels, cols = output channels, K = live taps x input channels.
 *   transposed == 0:  out[b,oh,ow,:] = sum_{r,s} in[b, oh*stride-pad+r, ow*stride-pad+s, :] . W[r,s]
 *   transposed == 1:  out[b,oy,ox,:] = sum_{r,s : (oy+pad-r) % stride == 0 ...}
 *                                       in[b,(oy+pad-r)/stride,(ox+pad-s)/stride,:] . W[r,s]
 *   W is the packed weight produced by lic_pack_weight: [kh*kw][ceil(Cin/16)][Npad/32][2][64][4], Npad = Cout
 *   rounded up to 64 (32 when Cout <= 32)
 *   (an opaque MFMA-operand order: element (k, n) of a chunk sits at lane (n%32) + 32*((k%16)/8),
 *   load q = (k%8)/4, float k%4)
 * Replaces: nn.Conv2d / nn.ConvTranspose2d forward and their input gradients
 *   (Components.py:10-16,39-45,69-73,99-103; Layers.py:21,38,40,43,74,76,99,101,103;
 *   ParametersModels.py:22-34; ContextModels.py:19-20 via tap_mask), the GDN/IGDN channel
 *   contraction (compressai GDN at Components.py:11,13,15,40,42,44; Layers.py:41,75) with
 *   prologue=1 (square the input), nn.LeakyReLU (Components.py:70,72,100,102; Layers.py:39,73,100;
 *   ParametersModels.py:23,25) and the residual adds (Layers.py:57,85,118) as epilogues.
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_igemm_desc {
  const float* in;
  const float* w;
  const float* bias; /* [Cout] or NULL */
  float* out;
  float* out2; /* secondary output (GDN norm, LEAKY+res sum) or NULL */
  const float* aux;
  const float* aux2;
  const float* aux3;
  const float* res;
  int64_t in_ld, out_ld, out2_ld, aux_ld, aux2_ld, aux3_ld, res_ld;
  int32_t B, Hi, Wi, Cin;
  int32_t Ho, Wo, Cout;
  int32_t kh, kw, stride, pad;
  int32_t transposed;
  int32_t prologue; /* 0: none, 1: square the gathered input, 2 / 3: GDN / IGDN backward -- the 1x1
                     * contraction's operand is t = dL/dnorm built on the fly from in = g, aux2 = x,
                     * aux3 = norm (-0.5 g x norm^-3/2, or 0.5 g x norm^-1/2 for IGDN) and also
                     * written to out2 for the d-gamma / d-beta launches (replaces lic_gdn_dnorm) */
  int32_t epilogue; /* enum lic_epilogue */
  uint32_t tap_mask; /* bit (r*kw+s) set = tap is live; 0 = all taps.  kh*kw <= 28 (LIC_ERR_UNSUPPORTED above): the
                      * kernels take each phase's taps from a 28-slot list in their parameter block (IgemmParams::taps) */
  float slope;       /* LeakyReLU negative slope */
  void* workspace;   /* optional (may be NULL): lets small layers split K across workgroups */
  size_t workspace_bytes;
  float* out3;       /* LIC_EPI_CONV_GDN / CONV_IGDN: the pre-normalisation conv output, or NULL */
  int64_t out3_ld;
  /* Overrides of the launch plan, 0 = automatic.  The automatic tile depends on the batch (a 128-row
   * tile needs >= 512 workgroups), so parity tests use these to put every kernel variant the full-size
   * workloads dispatch in front of the oracle at sizes the oracle finishes in seconds, and the entropy
   * coder pins one variant so that encoder and decoder build bit-identical tables whatever their batch.
   *   lic_igemm (fp32): force_bm in {64,128}, force_tn in {1,2,3} (both or neither; needs float4-aligned operands and
   *   Npad % (64*force_tn) == 0, else LIC_ERR_UNSUPPORTED); force_split >= 1: K splits
   *   (1 = never split; needs `workspace`). */
  int32_t force_bm, force_tn, force_split, reserved0;
} lic_igemm_desc;

/* 1 when lic_igemm can run LIC_EPI_CONV_GDN / LIC_EPI_CONV_IGDN for these channel counts
 * (all output channels in one full tile: Cout in {64,128,192}; Cin % 4 == 0) */
int lic_igemm_fused_gdn_supported(int32_t Cin, int32_t Cout);
/* 1 when fusing is also expected to be faster than two launches for this geometry (only the
 * shape fields of `d` are read) */
int lic_igemm_fused_gdn_preferred(const lic_igemm_desc* d);

/* workspace size that enables split-K for `d` (0 = the layer is large enough not to need it) */
size_t lic_igemm_workspace_bytes(const lic_igemm_desc* d);

int lic_igemm(const lic_igemm_desc* d, lic_stream_t stream);
/* name of the kernel variant lic_igemm launches for `d`, as rocprofv3 prints it (profiling aid) */
int lic_igemm_kernel_name(const lic_igemm_desc* d, char* buf, size_t n);
/* Weight packing for lic_igemm.  Logical element (tap, k, n) is read from
 * src[tap*s_tap + k*s_k + n*s_n]; dst holds lic_packed_weight_floats(taps, K, N) floats
 * (zero padded).  Any [Cout,Cin,kh,kw] / [Cin,Cout,kh,kw] weight, its transpose for the data
 * gradient, or a dense [K][N] matrix is expressed through the three strides. */
int64_t lic_packed_weight_floats(int32_t taps, int32_t K, int32_t N);
int lic_pack_weight(const float* src, float* dst, int32_t taps, int32_t K, int32_t N, int64_t s_tap,
                    int64_t s_k, int64_t s_n, lic_stream_t stream);
/* which workgroup tile lic_igemm will launch for `d` (kernel name igemm_kernel<BM,BN>) and how
 * many multiply-adds it will issue on live taps: lets a profiler attribute time and FLOPs. */
int lic_igemm_plan(const lic_igemm_desc* d, int32_t* BM, int32_t* BN, int64_t* live_macs);
/* Which tile every workgroup of lic_igemm's launch for `d` takes: order[4*id .. 4*id+3] = (K split, N tile, phase,
 * M tile) of hardware workgroup id, id = 0 .. nwg-1, computed on the host by the functions the kernel itself calls
 * (nothing is launched and no pointer of `d` is read through).  A workgroup whose M tile lies past its phase's last
 * row (M tile * BM >= pixels of the phase) exits at once.  `order` may be NULL to ask for the sizes alone; `capacity`
 * counts workgroups (LIC_ERR_INVALID when it is below nwg).  taps4 (may be NULL) receives the live taps of the four
 * phases, shape4 (may be NULL) BM, ksplit, chunks per split and chunks per tap.  The hardware deals ids round-robin
 * over the 8 XCDs (id % 8), in the order id / 8: a developer and test aid for the balance of that deal. */
int lic_igemm_tile_order(const lic_igemm_desc* d, int32_t* order, int64_t capacity, int64_t* nwg, int32_t* taps4,
                         int32_t* shape4);

/* ------------------------------------------------------------------------------------------
 * lic_wgrad -- weight-gradient contraction over pixels on fp32 MFMA, split-K + slab reduce.
 *   P ("plain") lives on the small grid [B,Hs,Ws,Cp]; G ("gathered") on the large grid
 *   [B,Hl,Wl,Cg] sampled at (hs*stride-pad+r, ws*stride-pad+s).
 *   R[tap][m][n] = sum_{b,hs,ws} (g_is_row ? G : P)[..m] * (g_is_row ? P : G)[..n]
 *   dst[m*dst_sm + n*dst_sn + tap*dst_stap] = scale * R[tap][m][n]
 * Replaces: autograd's weight gradients of every conv / convT / 1x1 on the path and the
 *   dgamma contraction of GDN (sq_g = 1 squares G on load).
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_wgrad_desc {
  const float* p;
  const float* g;
  float* dst;
  int64_t p_ld, g_ld;
  int64_t dst_sm, dst_sn, dst_stap;
  int32_t B, Hs, Ws, Cp;
  int32_t Hl, Wl, Cg;
  int32_t kh, kw, stride, pad;
  int32_t g_is_row;
  int32_t sq_p, sq_g;
  float scale;
  /* overrides of the launch plan, 0 = automatic (see lic_igemm_desc): tile in 64-channel units, one of
   * (1,1) (1,3) (2,1) (2,2) (2,3) (3,3) -- (3,3) needs both channel counts % 192 == 0 -- and the number
   * of pixel splits.  Honoured by lic_wgrad (fp32) only: lic_wgrad_bf16 plans from the shape alone (tile from
   * the channel counts, splits from the pixel count) and ignores all three. */
  int32_t force_tm, force_tn, force_split;
} lic_wgrad_desc;

size_t lic_wgrad_workspace_bytes(const lic_wgrad_desc* d);
int lic_wgrad(const lic_wgrad_desc* d, void* workspace, size_t workspace_bytes, lic_stream_t stream);
/* kernel variant wgrad_kernel<TM,TN,...> and split-K factor lic_wgrad will use (profiling aid) */
int lic_wgrad_plan(const lic_wgrad_desc* d, int32_t* TM, int32_t* TN, int32_t* splitk);
/* lic_wgrad in two steps, so a profiler can time the MFMA kernel apart from the slab reduction:
 * stage 1 = partial sums only, stage 2 = reduction only, 0 = both (== lic_wgrad) */
int lic_wgrad_stage(const lic_wgrad_desc* d, void* workspace, size_t workspace_bytes, int32_t stage,
                    lic_stream_t stream);
/* name of the MFMA kernel lic_wgrad launches for `d`, as rocprofv3 prints it */
int lic_wgrad_kernel_name(const lic_wgrad_desc* d, char* buf, size_t n);

/* column sums over pixels: out[c] = scale * sum_p in[p*ld + c]  (bias gradients, GDN dbeta) */
size_t lic_colsum_workspace_bytes(int64_t P, int32_t C);
int lic_colsum(const float* in, int64_t ld, int64_t P, int32_t C, float scale, float* out,
               void* workspace, size_t workspace_bytes, lic_stream_t stream);

/* generic 3-D strided copy: dst[i*d0+j*d1+k*d2] = src[i*s0+j*s1+k*s2]  (weight re-packing) */
int lic_permute3(const float* src, float* dst, int32_t n0, int32_t n1, int32_t n2, int64_t s0,
                 int64_t s1, int64_t s2, int64_t d0, int64_t d1, int64_t d2, lic_stream_t stream);

/* 3-channel layers (image side): patches <-> columns, C small.
 * im2col:  col[(b,oh,ow)][(r*kw+s)*C + c] = x[b, oh*stride-pad+r, ow*stride-pad+s, c] (0 outside),
 *          columns [kh*kw*C, Kpad) are zero.       (stem conv Components.py:10, Layers.py:38,43)
 * col2im:  out[b,oy,ox,c] = bias[c] + sum_{r,s} col[(b,ih,iw)][(r*kw+s)*C + c] with
 *          oy = ih*stride-pad+r.                    (last convT Components.py:45, :60)            */
int lic_im2col(const float* x, float* col, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho,
               int32_t Wo, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t Kpad,
               lic_stream_t stream);
int lic_col2im(const float* col, const float* bias, float* out, int32_t B, int32_t Hi, int32_t Wi,
               int32_t C, int32_t Ho, int32_t Wo, int32_t kh, int32_t kw, int32_t stride,
               int32_t pad, int32_t Kpad, lic_stream_t stream);

/* ---- elementwise ------------------------------------------------------------------------- */
/* w[i] *= mask[i]  (ContextModels.py:19, in place) */
int lic_mul_inplace(float* w, const float* mask, int64_t n, lic_stream_t stream);
/* dx = y > 0 ? dy : slope*dy  (LeakyReLU(inplace=True) backward from its output) */
int lic_leaky_bwd(const float* y, const float* dy, float* dx, int64_t n, float slope,
                  lic_stream_t stream);
/* out = max(p,bound)^2 - pedestal  (compressai NonNegativeParametrizer forward) */
int lic_gdn_reparam(const float* p, float* out, int64_t n, float bound, float pedestal,
                    lic_stream_t stream);
/* dp = pass ? dout*2*max(p,bound) : 0, pass = (p >= bound) | (that product < 0)  (LowerBound bwd) */
int lic_gdn_reparam_bwd(const float* p, const float* dout, float* dp, int64_t n, float bound,
                        lic_stream_t stream);
/* lic_gdn_reparam_bwd for beta [nb] and gamma [ng] of one GDN in one launch (either count may be 0) */
int lic_gdn_reparam_bwd2(const float* pb, const float* dob, float* dpb, int64_t nb, float bound_b, const float* pg,
                         const float* dog, float* dpg, int64_t ng, float bound_g, lic_stream_t stream);
/* lic_gdn_reparam_bwd2 for data-parallel ranks.  The pass-through is one-sided in the gradient's sign, so the mean of
 * the ranks' passed gradients is not the passed gradient of the whole batch: a half with its `late` flag set gets
 * dp = dout*2*max(p,bound) alone (linear in dout, so the ranks' mean is the whole batch's), and after the all-reduce
 * lic_gdn_pass_batch applies g = pass ? g : 0 in place, pass = (p >= bound) | (g < 0), to every such gradient in one
 * launch.  On one rank the two steps give the bits of lic_gdn_reparam_bwd2.  `jobs` is a HOST array, copied into the
 * kernel arguments, LIC_PASS_MAX_JOBS per launch; block0 is filled by the call. */
#define LIC_PASS_MAX_JOBS 32
typedef struct {
  const float* p; /* the parameter */
  float* g;       /* its gradient, rewritten in place */
  int64_t n;
  float bound;
  int32_t block0;
} lic_pass_job;
int lic_gdn_reparam_bwd2_late(const float* pb, const float* dob, float* dpb, int64_t nb, float bound_b, const float* pg,
                              const float* dog, float* dpg, int64_t ng, float bound_g, int32_t late_b, int32_t late_g,
                              lic_stream_t stream);
int lic_gdn_pass_batch(const lic_pass_job* jobs, int32_t njobs, lic_stream_t stream);
/* t = dL/dnorm: inverse ? 0.5*g*x*rsqrt(n) : -0.5*g*x*rsqrt(n)/n   (dense [n] tensors) */
int lic_gdn_dnorm(const float* g, const float* x, const float* norm, float* t, int64_t n,
                  int32_t inverse, lic_stream_t stream);
/* training: out = v + (u - 0.5); eval: out = rint(v)   (Models.py:55-64) */
int lic_quantize(const float* v, const float* u, float* out, int64_t n, int32_t training,
                 lic_stream_t stream);
/* The checkerboard context.  v, u, out, out_anchor: NHWC [B][h][w][C], any C; pixel (i, j) is an anchor
 * when i + j is even.  lic_quantize, and in the same launch out_anchor = anchor(out): out at the anchors, +0 elsewhere
 * (what the checkerboard context model convolves).  NULL v / out / out_anchor (u when training) or a non-positive
 * extent: LIC_ERR_INVALID, nothing launched. */
int lic_quantize_anchor(const float* v, const float* u, float* out, float* out_anchor, int32_t B, int32_t h, int32_t w,
                        int32_t C, int32_t training, lic_stream_t stream);
/* out = g + anchor(g_anchor), same layout: the backward of lic_quantize_anchor's two outputs (training: the gradient of
 * additive noise is the identity) in one launch.  NULL or non-positive arguments: LIC_ERR_INVALID. */
int lic_anchor_add(const float* g, const float* g_anchor, float* out, int32_t B, int32_t h, int32_t w, int32_t C,
                   lic_stream_t stream);

/* ---- gain units (variable rate; Cui et al. 2021) ------------------------------- */
/* A per-channel scale in front of a quantiser (gain) or behind it (inverse gain).  v, u, vg, out, out_anchor: NHWC
 * [B][h][w][C] fp32, any C >= 1.  The scale is read as s[b * s_stride + c]: s_stride = 0 is one row for every image,
 * otherwise s_stride >= C and every image has its own row.
 *   vg = fl32(v * s), always written;
 *   LIC_GAIN_SCALE: nothing else (u, out, out_anchor, out_bf16, anchor_bf16 must be NULL);
 *   LIC_GAIN_NOISE: out = fl32(vg + fl32(u - 0.5f));
 *   LIC_GAIN_ROUND: out = rint(vg), u is not read;
 *   out_anchor (may be NULL): out where pixel (i, j) has i + j even, +0 elsewhere (lic_quantize_anchor's rule);
 *   vg_bf16, out_bf16, anchor_bf16 (each may be NULL): the round-to-nearest-even bf16 of vg, out, out_anchor.
 * The product is rounded to fp32 before the sum: the multiply and the add are never contracted into one FMA, so every
 * output is a float32 numpy statement bit for bit.  16-byte pieces where C % 4 == 0, s_stride % 4 == 0 and every
 * pointer given is aligned (fp32 16 bytes, bf16 8), single floats otherwise; both write the same bytes.
 *   NULL v / s / vg (out, and u for NOISE), a non-positive extent, 0 < s_stride < C or s_stride < 0, an unknown mode:
 *   LIC_ERR_INVALID; h * w * C >= 2^31 or more than 2^31 - 1 workgroups: LIC_ERR_UNSUPPORTED.  Nothing launched then.
 *   One launch on `stream`, no allocation, no synchronisation, graph-capturable. */
#define LIC_GAIN_SCALE 0
#define LIC_GAIN_NOISE 1
#define LIC_GAIN_ROUND 2
int lic_gain_quantize(const float* v, const float* u, const float* s, int64_t s_stride, float* vg, float* out,
                      float* out_anchor, void* vg_bf16, void* out_bf16, void* anchor_bf16, int32_t B, int32_t h, int32_t w,
                      int32_t C, int32_t mode, lic_stream_t stream);
/* The backward of lic_gain_quantize.  t = d_vg + d_out + anchor(d_anchor), summed in that order; any of the three may be
 * NULL (it is left out of the sum), at least one is given.  dv = fl32(t * s);  ds[b][c] = sum over the pixels of image b
 * of fl32(t * v), accumulated in fp32 and written as [B][C] whatever s_stride is.
 * The sum has two stages in a fixed order, no float atomics, the same bits on every run and on either path (16-byte
 * pieces or single floats, chosen as above): a workgroup sums one slab of LIC_GAIN_SLAB_PIXELS consecutive pixels of one
 * image -- LIC_GAIN_SLAB_ROWS running sums, sum r over the slab's pixels r, r + ROWS, ... in rising order, then added
 * r = 0, 1, ... -- into a partial row of the workspace, [B][slabs][C] with slabs = ceil(h * w / LIC_GAIN_SLAB_PIXELS);
 * one pass then adds the partial rows of an image slab 0, 1, ...  (One slab: its row goes straight into ds.)
 *   NULL v / s / dv / ds / workspace, no gradient given, a non-positive extent, 0 < s_stride < C or s_stride < 0, a
 *   workspace below lic_gain_bwd_workspace_bytes(B, h * w, C): LIC_ERR_INVALID, nothing launched; the size limits of
 *   lic_gain_quantize: LIC_ERR_UNSUPPORTED.  No allocation, no synchronisation, graph-capturable. */
#define LIC_GAIN_SLAB_PIXELS 32
#define LIC_GAIN_SLAB_ROWS 4
size_t lic_gain_bwd_workspace_bytes(int32_t B, int64_t hw, int32_t C); /* 0 for a non-positive argument */
int lic_gain_bwd(const float* v, const float* s, int64_t s_stride, const float* d_vg, const float* d_out,
                 const float* d_anchor, float* dv, float* ds, int32_t B, int32_t h, int32_t w, int32_t C, void* workspace,
                 size_t workspace_bytes, lic_stream_t stream);
/* The gain rows of a batch from qualities that live on the device: one launch, nothing read back, nothing checked on the
 * host.  q: float[B]; tables: float[k][Q][M], the k stacked log-gain tables (1 <= k <= LIC_GAIN_ROWS_MAX_TABLES, Q >= 2);
 * rows: float[k][B][M].  Per image: qc = min(max(q, 0), Q-1), a NaN counting as 0 -- the clamp is this path's contract,
 * a quality outside [0, Q-1] is the nearest end, not an error --, i = min((int)floor(qc), Q-2), l = qc - i.  Per element
 *   rows = expf(fl32(fl32(fl32(1 - l) * T[i]) + fl32(l * T[i+1]))),
 * no product contracted with the sum.  lvl: int32[B] followed by float[B]; image b's i and l are written there for
 * lic_gain_rows_bwd.
 *   NULL q / tables / rows / lvl, k outside 1..4, Q < 2, M < 1, B < 1: LIC_ERR_INVALID; k * M * max(B, Q) >= 2^31:
 *   LIC_ERR_UNSUPPORTED.  Nothing launched then.  No allocation, no synchronisation, graph-capturable. */
#define LIC_GAIN_ROWS_MAX_TABLES 4
int lic_gain_rows_fwd(const float* q, const float* tables, float* rows, void* lvl, int32_t k, int32_t Q, int32_t M, int32_t B,
                      lic_stream_t stream);
/* The tables' gradient.  d_tables[t][j][c] (float[k][Q][M], every element written) is a running fp32 sum from zero over
 * b = 0, 1, ..., B-1: when i_b == j it takes fl32(fl32(fl32(1 - l_b) * rows[t][b][c]) * d_rows_t[b][c]), then, when
 * i_b + 1 == j, fl32(fl32(l_b * rows[t][b][c]) * d_rows_t[b][c]).  One thread per element, no atomics, nothing contracted:
 * the same bits on every run, exact zeros for a level no image touches.  d_rows0..3: float[B][M] each, the gradient of
 * table t's rows; NULL = none, that table's slice is zeros; those at index >= k must be NULL.  lvl, rows: as
 * lic_gain_rows_fwd left them.  Errors and limits as lic_gain_rows_fwd. */
int lic_gain_rows_bwd(const void* lvl, const float* rows, const float* d_rows0, const float* d_rows1, const float* d_rows2,
                      const float* d_rows3, float* d_tables, int32_t k, int32_t Q, int32_t M, int32_t B, lic_stream_t stream);

/* ---- entropy models (NHWC, P = B*h*w pixels) ------------------------------------------------ */
/* ParametersModels.py:43-64.  raw/out rows hold G*K*M channels (G = 2 if K == 1 else 3):
 * K==1: [mu | sigma]; K>1: [w | mu | sigma] with channel k*M+m inside each third. */
int lic_entropy_params_fwd(const float* raw, float* out, int64_t P, int32_t M, int32_t K,
                           lic_stream_t stream);
int lic_entropy_params_bwd(const float* raw, const float* out, const float* dout, float* draw,
                           int64_t P, int32_t M, int32_t K, lic_stream_t stream);
/* EntropyModels.py:188-233 + clamp :29-31 + log Models.py:87.  x,p,logp: [P][M]; params as above.
 * dp / dlogp may be NULL (treated as zero). */
int lic_gmm_likelihood_fwd(const float* x, const float* params, float* p, float* logp, int64_t P,
                           int32_t M, int32_t K, float bound, lic_stream_t stream);
int lic_gmm_likelihood_bwd(const float* x, const float* params, const float* dp,
                           const float* dlogp, float* dx, float* dparams, int64_t P, int32_t M,
                           int32_t K, float bound, lic_stream_t stream);
/* EntropyModels.py:49-151.  fe_params: [C][43] packed = matrices (3,9,9,3) | biases (3,3,3,1) |
 * factors (3,3,3), each in the reference's row-major (out,in) order.  x,p,logp: [P][C]. */
#define LIC_FE_NPARAM 43
int lic_factorized_fwd(const float* x, const float* fe_params, float* p, float* logp, int64_t P,
                       int32_t C, float bound, lic_stream_t stream);
int lic_factorized_bwd(const float* x, const float* fe_params, const float* dp, const float* dlogp,
                       float* dx, float* dfe_params, int64_t P, int32_t C, float bound,
                       lic_stream_t stream);
/* The factorised model's 11 parameter tensors (EntropyModels.py:62-86, each contiguous [C][out][in]) gathered into
 * the [C][43] operand above / its [C][43] gradient scattered into a parameter-major buffer (parameter k's [C][n_k]
 * block at offset C * prefix_k: each block has the parameter's own layout, so its views are the parameters'
 * gradients), one launch each.  params11_host: HOST array of the 11 device pointers in the order matrices, biases,
 * factors. */
int lic_fe_pack(const void* const* params11_host, float* packed, int32_t C, lic_stream_t stream);
int lic_fe_unpack(const float* dpacked, float* flat, int32_t C, lic_stream_t stream);
/* channel_logits_cumulative (EntropyModels.py:153-169): out[i] = L_ch(xs[i]) */
int lic_factorized_channel_logits(const float* fe_params, int32_t ch, const float* xs, float* out,
                                  int64_t n, lic_stream_t stream);

/* ---- rate-distortion loss (RateDistortionLoss.py:5-49) ---------------------------------------
 * Per-image element counts ny, nz, nx; images are contiguous blocks (layout-agnostic sums).
 * out[0..8] = loss, bpp_y, bpp_z, bpp_total, mse, psnr, bits_y, bits_z, bits_total; out[9..15] = 0 (every slot is written);
 * out[16 .. 16+B) = mse_per_image; out[16+B .. 16+2B) = psnr_per_image. */
size_t lic_rd_loss_workspace_bytes(int32_t B);
int lic_rd_loss_fwd(const float* logp_y, int64_t ny, const float* logp_z, int64_t nz,
                    const float* x_hat, const float* x, int64_t nx, int32_t B, int64_t num_pixels,
                    float lambda_rd, float* out, void* workspace, size_t workspace_bytes,
                    lic_stream_t stream);
/* gl: device pointer to the upstream gradient of `loss` (a single float) */
int lic_rd_loss_bwd(const float* x_hat, const float* x, int64_t ny, int64_t nz, int64_t nx,
                    int32_t B, int64_t num_pixels, float lambda_rd, const float* gl, float* dlogp_y,
                    float* dlogp_z, float* dx_hat, lic_stream_t stream);
/* The same loss with one lambda per image, read from device memory (lambda_img: float[B]), so that a captured launch
 * serves any lambdas.  Forward: the launches, the workspace and slots 1..8 and 16.. of lic_rd_loss_fwd;
 *   out[9] = (float)(sum_b (double)lambda_b * 65025.0 * (double)mse_b / B), the distortion term, summed as `mse` is;
 *   out[0] = fl32(out[3] + out[9]);  out[10..15] = 0.
 * Backward: dlogp_y, dlogp_z as lic_rd_loss_bwd; dx_hat of image b = (x_hat - x) * (gl[0] * kx_b) with
 *   kx_b = fl32(fl32(fl32(lambda_b * 65025f) * 2f) / fl32((float)nx * (float)B)),
 * lic_rd_loss_bwd's host expression evaluated on the device with nothing contracted: with all lambdas equal the three
 * gradients are that entry's bytes.  One launch; 16-byte pieces when nx % 4 == 0 and x_hat, x, dx_hat are 16-byte
 * aligned, single floats otherwise, the same bytes either way.
 *   NULL pointers, non-positive extents: LIC_ERR_INVALID.  No allocation, no synchronisation, graph-capturable. */
int lic_rd_loss_fwd_lam(const float* logp_y, int64_t ny, const float* logp_z, int64_t nz, const float* x_hat, const float* x,
                        int64_t nx, int32_t B, int64_t num_pixels, const float* lambda_img, float* out, void* workspace,
                        size_t workspace_bytes, lic_stream_t stream);
int lic_rd_loss_bwd_lam(const float* x_hat, const float* x, int64_t ny, int64_t nz, int64_t nx, int32_t B,
                        int64_t num_pixels, const float* lambda_img, const float* gl, float* dlogp_y, float* dlogp_z,
                        float* dx_hat, lic_stream_t stream);

/* ---- bf16-storage variants (BASELINE config 3) --------------------------------------------------
 * Activations / auxiliaries are bf16 NHWC (pitches and channel counts multiples of 8), weights are
 * packed to bf16 by lic_pack_weight_bf16 ([tap][ceil(K/32)][ceil64(N)/32][2][64 lanes][8], MFMA operand order), bias and all
 * accumulation are fp32 (v_mfma_f32_32x32x16_bf16).  lic_igemm_bf16 supports the NONE / LEAKY / GDN /
 * IGDN / GDN_BWD / IGDN_BWD epilogues (no residual) and tap_mask; `out` is bf16, or fp32 when out_f32 != 0.
 * Parameter gradients (lic_wgrad_bf16 dst, lic_colsum_bf16 out) are fp32. */
int64_t lic_packed_weight_bf16_elems(int32_t taps, int32_t K, int32_t N);
int lic_pack_weight_bf16(const float* src, void* dst, int32_t taps, int32_t K, int32_t N, int64_t s_tap,
                         int64_t s_k, int64_t s_n, lic_stream_t stream);
int lic_igemm_bf16(const lic_igemm_desc* d, int32_t out_f32, lic_stream_t stream);
/* workspace size that lets lic_igemm_bf16 split K across workgroups for `d` (0 = large enough not to need it);
 * pass the buffer in d->workspace / workspace_bytes.  The split and the choice between the tap-major tiles and the
 * chunk-major halo-resident variant (the two things that change the summation order of an output) are functions of
 * per-image geometry only: an image's bits do not depend on the batch it is computed in.  force_split of the
 * descriptor is honoured (1 = never, n > 1 = n splits); force_bm in {64, 128, 256, 512}: 256 = the 8-wave
 * ping-pong tile, 512 = the halo-resident 5x5 stride-2 kernel wherever a launch is eligible for it (other
 * launches keep their automatic tile); force_tn is not used on this path (the N tile follows from the channel
 * count; a value that contradicts it returns LIC_ERR_UNSUPPORTED). */
size_t lic_igemm_bf16_workspace_bytes(const lic_igemm_desc* d);
/* lic_igemm_bf16 also runs LIC_EPI_CONV_GDN / LIC_EPI_CONV_IGDN (the conv -> GDN pairs of Components.py:10-15,
 * 39-44 in one launch) when this returns 1 (Cout in {64,128,192}: one tile spans every output channel; bf16 `out`):
 * aux = gamma_eff^T packed by lic_pack_weight_bf16_kperm(taps=1, K=Cout, N=Cout), aux2 = beta_eff (fp32 [Cout]),
 * out3 / out2 = bf16 conv output / norm for the backward pass (either may be NULL: inference writes `out` only).
 * The rounding points are those of LIC_EPI_NONE followed by the prologue=1 / LIC_EPI_GDN launch (x and x^2 to
 * bf16, fp32 norm); the pool sums each group of 16 channels in a different order, so norms agree to fp32
 * rounding, not bitwise. */
int lic_igemm_bf16_fused_gdn_supported(int32_t Cin, int32_t Cout);
/* lic_stem_gdn_bf16 -- the RGB stem of the analysis transform and the GDN behind it (Components.py:10-11:
 * nn.Conv2d(3, C, 5, stride=2, padding=2) -> GDN(C)) in one launch that reads the fp32 NHWC image and writes the
 * normalised bf16 feature map (no column matrix).  w_packed: lic_pack_stem_weight_bf16 of the [C][3][5][5] weight
 * (lic_stem_weight_bf16_elems(C) bf16 elements); gamma_packed: gamma_eff^T by lic_pack_weight_bf16_kperm(taps 1,
 * K = N = C); beta_eff fp32 [C]; y / conv_out / norm: bf16 [B][ceil(H/2)][ceil(W/2)][C], the last two may be NULL
 * (they feed the backward pass).  Same rounding points as lic_igemm_bf16's LIC_EPI_CONV_GDN. */
int lic_stem_gdn_bf16_supported(int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad);
int64_t lic_stem_weight_bf16_elems(int32_t Cout);
int lic_pack_stem_weight_bf16(const float* w, void* dst, int32_t Cout, lic_stream_t stream);
int lic_stem_gdn_bf16(const float* x, const void* w_packed, const float* bias, const void* gamma_packed,
                      const float* beta_eff, void* y, void* conv_out, void* norm, int32_t B, int32_t H, int32_t W,
                      int32_t Cout, int32_t inverse, lic_stream_t stream);
/* lic_pack_weight_bf16 with the K index permuted inside every group of 16: slot (h = 0..1, e = 0..7) of a group
 * holds k = 8*(e/4) + 4*h + e%4 instead of 8*h + e -- the order in which a lane of the transposed accumulator
 * tile owns channels, so the fused pool reads its x^2 operand from registers */
int lic_pack_weight_bf16_kperm(const float* src, void* dst, int32_t taps, int32_t K, int32_t N, int64_t s_tap,
                               int64_t s_k, int64_t s_n, lic_stream_t stream);
/* names of the kernel variants lic_igemm_bf16 / lic_wgrad_bf16 launch for `d`, as rocprofv3 prints them
 * (force_bm of the descriptor is honoured; the N tile follows from the channel count) */
int lic_igemm_bf16_kernel_name(const lic_igemm_desc* d, char* buf, size_t n);
int lic_wgrad_bf16_kernel_name(const lic_wgrad_desc* d, char* buf, size_t n);
size_t lic_wgrad_bf16_workspace_bytes(const lic_wgrad_desc* d);
int lic_wgrad_bf16(const lic_wgrad_desc* d, void* workspace, size_t workspace_bytes, lic_stream_t stream);
/* fp32 image -> bf16 columns; bf16 columns -> fp32 image (+ fp32 bias) */
int lic_im2col_bf16(const float* x, void* col, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho,
                    int32_t Wo, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t Kpad,
                    lic_stream_t stream);
int lic_col2im_bf16(const void* col, const float* bias, float* out, int32_t B, int32_t Hi, int32_t Wi,
                    int32_t C, int32_t Ho, int32_t Wo, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                    int32_t Kpad, lic_stream_t stream);
/* GDN / IGDN backward in bf16 storage as one sweep (replaces lic_gdn_dnorm_bf16 + lic_igemm_bf16(EPI_GDN_BWD) for
 * C in {64, 128}; compressai GDN at Components.py:11-44): t = dL/dnorm (written: the d-gamma / d-beta launches read
 * it), dx = g * norm^-1/2 + 2 x (t . gamma_eff) (inverse: norm^+1/2).  g, x, norm, dx, t: dense bf16 [P][C];
 * gamma_packed = lic_pack_weight_bf16_kperm(gamma_eff, taps 1, K = C, N = C, s_k = C, s_n = 1). */
int lic_gdn_bwd_bf16_supported(int32_t C);
/* colsum_*_partial (optional, both or neither): [lic_gdn_bwd_bf16_partial_rows(P)][C] fp32 per-workgroup column sums of t
 * and of dx -- d beta and the d bias of the convolution in front need one small reduction over these rows instead of a
 * pass over the two activations */
int64_t lic_gdn_bwd_bf16_partial_rows(int64_t P);
int lic_gdn_bwd_bf16(const void* g, const void* x, const void* norm, const void* gamma_packed, void* dx, void* t,
                     float* colsum_t_partial, float* colsum_dx_partial, int64_t P, int32_t C, int32_t inverse,
                     lic_stream_t stream);
/* ... with the pool RECOMPUTED instead of read: norm = beta_eff + x^2 . gamma_eff^T formed as the forward pass forms it
 * (x^2 and the result rounded to bf16), so the forward pass writes two tensors per GDN layer instead of three and this
 * launch reads two instead of three.  gammaT_packed = lic_pack_weight_bf16_kperm(gamma_eff, taps 1, K = C, N = C,
 * s_k = 1, s_n = C) -- the fused conv + GDN kernels' operand. */
int lic_gdn_bwd_bf16_recompute(const void* g, const void* x, const void* gamma_packed, const void* gammaT_packed,
                               const float* beta_eff, void* dx, void* t, float* colsum_t_partial,
                               float* colsum_dx_partial, int64_t P, int32_t C, int32_t inverse, lic_stream_t stream);
/* column sums of two bf16 [P][ld] matrices of one shape in one launch pair (workspace: twice the single size) */
int lic_colsum2_bf16(const void* in_a, const void* in_b, int64_t ld, int64_t P, int32_t C, float scale, float* out_a,
                     float* out_b, void* workspace, size_t workspace_bytes, lic_stream_t stream);
size_t lic_colsum_bf16_workspace_bytes(int64_t P, int32_t C);
int lic_colsum_bf16(const void* in, int64_t ld, int64_t P, int32_t C, float scale, float* out,
                    void* workspace, size_t workspace_bytes, lic_stream_t stream);
/* dx = dy * (y > 0 ? 1 : slope), bf16 tensors, n % 8 == 0: backward of lic_igemm_bf16's LIC_EPI_LEAKY */
int lic_leaky_bwd_bf16(const void* y, const void* dy, void* dx, int64_t n, float slope, lic_stream_t stream);
int lic_gdn_dnorm_bf16(const void* g, const void* x, const void* norm, void* t, int64_t n, int32_t inverse,
                       lic_stream_t stream);
/* lic_quantize (Models.py:55-64) that also writes the bf16 copies the bf16-storage consumers read: v_bf16 = bf16(v) (the
 * hyper-encoder's input), out_bf16 = bf16(out) (decoder, context model, hyper-decoder); either may be NULL; n % 4 == 0 */
int lic_quantize_bf16(const float* v, const float* u, float* out, void* v_bf16, void* out_bf16, int64_t n,
                      int32_t training, lic_stream_t stream);
/* lic_quantize_anchor that also writes the bf16 copies: v_bf16 = bf16(v), out_bf16 = bf16(out), anchor_bf16 =
 * bf16(out_anchor); any of the three may be NULL.  LIC_ERR_UNSUPPORTED exactly where lic_quantize_bf16 returns it:
 * B*h*w*C % 4 != 0, an fp32 pointer off 16 bytes, a bf16 pointer off 8.  C itself need not be a multiple of 4. */
int lic_quantize_anchor_bf16(const float* v, const float* u, float* out, float* out_anchor, void* v_bf16, void* out_bf16,
                             void* anchor_bf16, int32_t B, int32_t h, int32_t w, int32_t C, int32_t training,
                             lic_stream_t stream);

/* ---- misc ---------------------------------------------------------------------------------- */
/* ------------------------------------------------------------------------------------------
 * Stand-alone GDN / IGDN (compressai GDN at Components.py:11-44, Layers.py:41,75)
 * for C in {64,128,192} (lic_gdn_supported): one sweep over the activation per launch, the C x C pool
 * on MFMA out of an LDS tile.  x, y, norm, g, dx, t: dense [P][C] fp32 (NHWC activations, P = B*H*W).
 *   lic_gdn_fwd: norm = beta_eff + x^2 . gamma_eff^T (written unless `norm` is NULL: only the backward pass reads
 *                it); y = x * rsqrt(norm) (inverse: * sqrt(norm)) (+ res)
 *                gammaT_packed = lic_pack_weight(gamma_eff, taps=1, K=C, N=C, s_k=1, s_n=C)
 *   lic_gdn_bwd: t = dL/dnorm (written: the d-gamma / d-beta launches read it),
 *                dx = g * rsqrt(norm) + 2 x (t . gamma_eff)  (inverse: g * sqrt(norm) + ...)
 *                gamma_packed = lic_pack_weight(gamma_eff, taps=1, K=C, N=C, s_k=C, s_n=1)
 * Same chunk / k order as lic_igemm's prologue-1 / prologue-2 route, which serves other channel counts: norm, y, t and
 * the pooled sums of the backward are bitwise that route's.  dx is not: lic_gdn_bwd forms g f + 2 x (t . gamma_eff) with
 * one fused multiply-add, the generic 16-byte epilogue rounds the product first (a last-bit difference in about one
 * element in seven).
 * ------------------------------------------------------------------------------------------ */
int lic_gdn_supported(int32_t C);
int lic_gdn_fwd(const float* x, const float* gammaT_packed, const float* beta_eff, const float* res, float* y,
                float* norm, int64_t P, int32_t C, int32_t inverse, lic_stream_t stream);
/* colsum_*_partial (optional, may be NULL): [lic_gdn_bwd_partial_rows(P)][C] per-workgroup column sums of
 * t and of dx, so that d beta and the d bias of the convolution in front of the GDN need one
 * lic_colsum over a few thousand rows instead of a pass over the whole activation */
int64_t lic_gdn_bwd_partial_rows(int64_t P);
int lic_gdn_bwd(const float* g, const float* x, const float* norm, const float* gamma_packed, float* dx, float* t,
                float* colsum_t_partial, float* colsum_dx_partial, int64_t P, int32_t C, int32_t inverse,
                lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2 -- tables for an entropy coder (the reference has none), built on the
 * device from the same distributions the likelihood entries evaluate and consumed by the host range
 * coder of include/lic_codec.h.  A table has S symbols (index i <-> integer value lo + i) and S+1
 * uint32 entries  cum[i] = floor(F_i * (65536 - S)) + i  with F_0 = 0, F_S = 1 and
 * F_i = CDF(lo + i - 0.5): cum[0] = 0, cum[S] = 65536, every symbol keeps frequency >= 1; indices 0
 * and S-1 carry the tails (the coder escapes out-of-window values through them).
 *   lic_factorized_cdf_tables: out[C][S+1], F = sigmoid(L_c(.))         (EntropyModels.py:153-184)
 *   lic_gmm_cdf_tables: per latent element e of [P][M]: center[e] = rint(sum_k w_k mu_k), window
 *     lo = center - W, S = 2W+1, out[P*M][S+1], F = sum_k w_k Phi((x - mu_k)/sigma_k); `params` as
 *     lic_gmm_likelihood_fwd                                    (EntropyModels.py:192-233, utils.py:6-8)
 * ------------------------------------------------------------------------------------------ */
int lic_factorized_cdf_tables(const float* fe_params, int32_t C, int32_t lo, int32_t S, uint32_t* out,
                              lic_stream_t stream);
int lic_gmm_cdf_tables(const float* params, int64_t P, int32_t M, int32_t K, int32_t W, int32_t* center,
                       uint32_t* out, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2e -- the rows the coder's per-pixel layers read, in one launch: the live taps of the masked context
 *   convolution evaluated as a gather (ContextModels.py:18-20: the mask kills taps, the zero padding of the
 *   convolution kills what leaves the image) and the hyper-decoder's half of torch.cat([phi, psi], dim=1)
 *   (Models.py:73).  codec.ContextCodec calls it once per image for the encoder and once per decode step.
 *     y             the latents, an fp32 NHWC plane: element (b, i, j, c) at
 *                   y[b * y_batch + y_origin + i * y_row + j * y_pix + c], 0 <= i < h, 0 <= j < w, c < M <= y_pix
 *                   (all in floats).  A zero-framed [B][h+2p][w+2p][M] buffer has y_row = (w+2p) M, y_pix = M,
 *                   y_origin = (p (w+2p) + p) M; a plain [B][h][w][M] one y_row = w M, y_pix = M, y_origin = 0.
 *                   Nothing but those h * w pixels is ever read: the frame is not relied on.
 *     taps          [nt][2] int32 (device): the live taps as (dr, ds) offsets from the pixel, in the order of the
 *                   packed context weight's K dimension
 *     slice_rows    R >= 1: the plane is cut into bands of R rows (the last one shorter when R does not divide h).
 *                   A tap with dr < 0 of pixel (i, j) is read only if (i mod R) + dr >= 0, else it is zero, as a
 *                   tap above the image is.  R >= h: no slices.
 *     pix           [n] int64 (device): raster indices i * w + j of the pixels wanted, the same for every image
 *     win           out, [B*n][nt*M] contiguous: row b * n + k, column t * M + c = tap t, channel c of pixel pix[k]
 *     psi, comb     optional (psi NULL: neither is touched).  psi [B][h*w][Cpsi] contiguous; row b * n + k of
 *                   comb, comb_ld floats per row, gets the Cpsi floats of pixel pix[k].  `comb` points at the first
 *                   column to write, so a column range of a wider buffer is comb = buffer + first column.
 *     path          LIC_CTX_AUTO: 16-byte pieces when M % 4 == 0 (and Cpsi % 4 == 0, comb_ld % 4 == 0 with psi),
 *                   y_batch, y_row, y_pix, y_origin are multiples of 4 and y, win (psi, comb) are 16-byte
 *                   aligned; single floats otherwise.  LIC_CTX_ELEMENT forces single floats, LIC_CTX_VECTOR the
 *                   pieces (LIC_ERR_INVALID where the conditions above do not hold).  Both write the same bytes.
 *   A pix[k] outside [0, h*w) reads nothing and writes zeros to its rows.  NULL y / taps / pix / win, psi without
 *   comb, B, h, w, M, n <= 0, nt < 1, slice_rows < 1, a pointer that is not float aligned: LIC_ERR_INVALID, nothing
 *   launched.  One launch on `stream`, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
#define LIC_CTX_AUTO 0
#define LIC_CTX_VECTOR 1
#define LIC_CTX_ELEMENT 2
int lic_ctx_gather(const float* y, int64_t y_batch, int64_t y_row, int64_t y_pix, int64_t y_origin, int32_t B,
                   int32_t h, int32_t w, int32_t M, const int32_t* taps, int32_t nt, int32_t slice_rows,
                   const int64_t* pix, int64_t n, float* win, const float* psi, int32_t Cpsi, float* comb,
                   int64_t comb_ld, int32_t path, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2f -- lic_ctx_gather for rows that belong to DIFFERENT images: codec.ContextCodec.decompress_images
 *   advances many bitstreams of different sizes together, and step t's rows of all of them are built by one launch.
 *   All planes lie in one flat buffer, all psi planes in another; row, tap and column rules are lic_ctx_gather's.
 *     y, y_len      the flat latent buffer and its length in floats; y_pix (>= M) is call-wide
 *     images        [nimg][LIC_CTX_IMAGE_WORDS] int64 (device), per image: Y_BASE the plane's first float in y,
 *                   Y_ROW its row pitch, Y_ORIGIN pixel (0, 0) behind the base (element (i, j, c) at
 *                   y[Y_BASE + Y_ORIGIN + i * Y_ROW + j * y_pix + c]), PSI_BASE the first float of its [h*w][Cpsi]
 *                   rows in psi, H, W, and R = its slice_rows (>= 1; >= H: no slices).  Word 7 is not read.
 *     row_image, row_pix   [rows] int64 each (device): output row k is pixel row_pix[k] (raster, i * W + j) of image
 *                   row_image[k]
 *     win           out, [rows][nt*M] contiguous
 *     psi, psi_len, comb   optional as in lic_ctx_gather; psi_len is the flat psi buffer's length in floats; row k of
 *                   comb gets psi[PSI_BASE + row_pix[k] * Cpsi ...], Cpsi floats
 *     path          as in lic_ctx_gather for what the entry can see: M, Cpsi, comb_ld, y_pix multiples of 4 and y, win
 *                   (psi, comb) 16-byte aligned.  An image's Y_BASE, Y_ROW, Y_ORIGIN, PSI_BASE live on the device: in
 *                   the 16-byte kernel a row whose image has one that is no multiple of 4 is moved float by float
 *                   instead -- the kernel falls back per row, the entry does not refuse -- and gets the same bytes.
 *   The kernel checks a descriptor before it addresses anything with it: bases, pitch and origin in [0, y_len]
 *   ([0, psi_len]), 1 <= H, W <= 32768, R >= 1, the plane's last float Y_BASE + Y_ORIGIN + (H-1) Y_ROW + (W-1) y_pix
 *   + M <= y_len and PSI_BASE + H W Cpsi <= psi_len.  A row whose image fails, whose row_image is outside [0, nimg) or
 *   whose row_pix is outside [0, H*W) reads nothing and is written as zeros (win and comb).  Taps are applied only
 *   where they stay inside the H x W pixels, so no address leaves y[0, y_len), psi[0, psi_len) whatever the tables say.
 *   NULL y / images / taps / row_image / row_pix / win, psi without comb, nimg, M, rows, y_len <= 0, nt < 1, y_pix < M,
 *   a float pointer that is not 4-byte or an int64 pointer that is not 8-byte aligned, LIC_CTX_VECTOR where the entry
 *   sees it cannot hold: LIC_ERR_INVALID; y_len, psi_len, y_pix above 2^40: LIC_ERR_UNSUPPORTED; nothing launched.
 *   One launch on `stream`, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
#define LIC_CTX_IMAGE_WORDS 8
#define LIC_CTX_IMAGE_Y_BASE 0
#define LIC_CTX_IMAGE_Y_ROW 1
#define LIC_CTX_IMAGE_Y_ORIGIN 2
#define LIC_CTX_IMAGE_PSI_BASE 3
#define LIC_CTX_IMAGE_H 4
#define LIC_CTX_IMAGE_W 5
#define LIC_CTX_IMAGE_R 6
int lic_ctx_gather_ragged(const float* y, int64_t y_len, int64_t y_pix, const int64_t* images, int32_t nimg, int32_t M,
                          const int32_t* taps, int32_t nt, const int64_t* row_image, const int64_t* row_pix,
                          int64_t rows, float* win, const float* psi, int64_t psi_len, int32_t Cpsi, float* comb,
                          int64_t comb_ld, int32_t path, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layered codec (codec.ScalableCodec) -- lic_ctx_gather for a latent whose channels are split into L layers, each
 *   with a context model of its own: one launch builds every layer's rows from the ONE y buffer and the one psi.
 *   y .. n and psi, Cpsi, path are lic_ctx_gather's (the plane has y_pix channels per pixel; there is no call-wide M).
 *     layers        [L] rows, 1 <= L <= LIC_MAX_LAYERS, a HOST array that is copied into the launch: layer l covers
 *                   channels [c0, c0 + M) of every pixel, writes row b * n + k of win [B*n][nt*M] (column t * M + c =
 *                   tap t, channel c0 + c) and, with psi, row b * n + k of comb (comb_ld floats per row, `comb` the
 *                   first column to write) with the pixel's Cpsi psi columns.
 *   The bytes written for layer l are exactly those of lic_ctx_gather(y + c0, ..., M, ..., win, psi, Cpsi, comb,
 *   comb_ld): zeros for taps outside the image or the slice, rows of zeros for a pix[k] outside [0, h*w).
 *   The 16-byte path is decided per layer: lic_ctx_gather's conditions with c0 and M multiples of 4 and the layer's
 *   win / comb 16-byte aligned; a layer that misses them goes float by float, the others keep their pieces, and both
 *   write the same bytes.  LIC_CTX_VECTOR: LIC_ERR_INVALID unless every layer qualifies.
 *   NULL y / taps / pix / layers / a layer's win, psi with a layer without comb (or comb_ld < Cpsi), L outside
 *   1..LIC_MAX_LAYERS, M <= 0, c0 < 0, c0 + M > y_pix, two layers whose channel ranges overlap, B, h, w, n <= 0,
 *   nt < 1, slice_rows < 1, a misaligned pointer: LIC_ERR_INVALID; lic_ctx_gather's size limits per layer:
 *   LIC_ERR_UNSUPPORTED; nothing launched.  One launch on `stream`, no allocation, no synchronisation.
 * ------------------------------------------------------------------------------------------ */
#define LIC_MAX_LAYERS 4
typedef struct lic_ctx_layer {
  float* win;
  float* comb;
  int64_t comb_ld;
  int32_t c0, M;
} lic_ctx_layer;
int lic_ctx_gather_layers(const float* y, int64_t y_batch, int64_t y_row, int64_t y_pix, int64_t y_origin, int32_t B,
                          int32_t h, int32_t w, const int32_t* taps, int32_t nt, int32_t slice_rows, const int64_t* pix,
                          int64_t n, const float* psi, int32_t Cpsi, const lic_ctx_layer* layers, int32_t L,
                          int32_t path, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layered codec, rows of DIFFERENT images (codec.ScalableCodec.decompress_images / decompress_base_images): one
 *   launch builds every layer's rows of a step of many layered bitstreams.  The arguments of lic_ctx_gather_ragged
 *   without M, win, comb, comb_ld, and lic_ctx_gather_layers' layer table (a HOST array that is copied into the
 *   launch): layer l covers channels [c0, c0 + M) of every pixel of every plane, writes row k of its own
 *   win [rows][nt*M] and, with psi, row k of its own comb.
 *   The bytes written for layer l are exactly those of lic_ctx_gather_ragged called with M = the layer's M, every
 *   descriptor's Y_ORIGIN raised by c0, and that layer's win / comb / comb_ld: tap, slice, column and psi rules, rows
 *   of zeros for a bad row_image / row_pix / descriptor, and the per-row fallback from the 16-byte path when an
 *   image's bases are no multiple of 4 floats.  The 16-byte path is decided per layer, as in lic_ctx_gather_layers
 *   (y, psi 16-byte aligned, y_pix, Cpsi, c0, M, comb_ld multiples of 4, the layer's win / comb 16-byte aligned).
 *   The kernel checks a descriptor once per row, before it addresses anything: lic_ctx_gather_ragged's check, with the
 *   plane's last float Y_BASE + Y_ORIGIN + (H-1) Y_ROW + (W-1) y_pix + max(c0 + M) <= y_len, so no address leaves
 *   y[0, y_len) or psi[0, psi_len), whatever the tables say.
 *   NULL y / images / taps / row_image / row_pix / layers / a layer's win, psi with a layer without comb (or comb_ld <
 *   Cpsi), L outside 1..LIC_MAX_LAYERS, M <= 0, c0 < 0, c0 + M > y_pix, overlapping channel ranges, nimg, rows,
 *   y_len <= 0, nt < 1, psi with Cpsi or psi_len <= 0, a float pointer that is not 4-byte or an int64 pointer that is
 *   not 8-byte aligned, LIC_CTX_VECTOR where a layer cannot hold it: LIC_ERR_INVALID; y_len, psi_len, y_pix above 2^40,
 *   rows above 2^40, nt * M + Cpsi of a layer above 2^31 - 257: LIC_ERR_UNSUPPORTED; nothing launched.
 *   One launch on `stream`, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
int lic_ctx_gather_layers_ragged(const float* y, int64_t y_len, int64_t y_pix, const int64_t* images, int32_t nimg,
                                 const int32_t* taps, int32_t nt, const int64_t* row_image, const int64_t* row_pix,
                                 int64_t rows, const float* psi, int64_t psi_len, int32_t Cpsi,
                                 const lic_ctx_layer* layers, int32_t L, int32_t path, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2 -- the device decoder of the "rANS-64" y streams (format and host coder: lic_codec.h).
 *   lic_rans_decode_step decodes ONE wavefront step of all B images in one launch, one wave per image, from the
 *   tables lic_gmm_cdf_tables has just built, and writes the values where the next step's gather reads them:
 *   codec.ContextCodec's decode loop becomes a chain of asynchronous launches with no host in it.
 *     streams       all images' streams in one buffer (4-byte aligned); image b's stream starts at byte
 *                   stream_off[b] (a multiple of 4: pad each start in this staging buffer, not in the file) and
 *                   is stream_bytes[b] long, stream_off[b] + stream_bytes[b] <= stream_off[b+1]; stream_off has
 *                   B+1 entries.  The 64 leading state words are NOT read here: they seed `state`.
 *     escapes       all images' escape lists; image b's entries are escapes[esc_off[b] .. esc_off[b+1])
 *     state         [B][LIC_RANS_STATE_WORDS] uint32: the 64 coder states (lane 0 first), the word cursor (in
 *                   16-bit words behind the 64 leading state words), the escape cursor and an error word (0 = fine,
 *                   else LIC_RANS_ERR_* bits).  Read at entry and written back at exit with ordinary stores, so
 *                   consecutive launches on one stream carry it.  Seed: the stream's 64 states, 0, 0, 0.
 *     tables        [B][n*M][2W+2] (16-byte aligned) and center [B][n*M]: lic_gmm_cdf_tables' outputs for the
 *                   step's n pixels per image; symbol k of the step is pixel k / M, channel k % M
 *     dest          [n] pixel indices (device, the step's slice of the caller's index array), each in [0, pixels)
 *     ypad          [B][pixels][M] fp32: element (b, dest[k / M], k % M) = float(idx + center - W), the escape
 *                   excess applied at the edge symbols; no other element is touched
 *   Before every read of a word or an escape the cursor plus the lane's rank is compared with the image's
 *   length: out of range reads nothing, sets LIC_RANS_ERR_RANGE in the image's error word and makes every later
 *   symbol of that image decode as its table centre.  A stream_bytes[b] below 256 or beyond its slot sets
 *   LIC_RANS_ERR_STREAM with the same effect; a dest index outside [0, pixels) is not written and sets
 *   LIC_RANS_ERR_RANGE.  After the last step an intact stream has word cursor == (stream_bytes - 256) / 2, escape
 *   cursor == its escape count and every state == 2^16: the caller's to check with the error words.
 *   W <= 64 (LIC_ERR_UNSUPPORTED above).  One launch, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
#define LIC_RANS_LANES 64
#define LIC_RANS_STATE_WORDS 67
#define LIC_RANS_ERR_RANGE 1u  /* a word, escape or destination index was out of range */
#define LIC_RANS_ERR_STREAM 2u /* stream_bytes[b] cannot be right */
int lic_rans_decode_step(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                         const uint32_t* escapes, const int64_t* esc_off, uint32_t* state, const uint32_t* tables,
                         const int32_t* center, int32_t B, int32_t n, int32_t M, int32_t W, const int64_t* dest,
                         float* ypad, int64_t pixels, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2d -- the same step for "rANS-64 x G" streams (lic_codec.h: round r of every step belongs to
 *   sub-stream r % G of its image): B * G workgroups of one wave, wave (b, g) decodes rounds g, g + G, ... of the
 *   step from block b * G + g.  The arguments of lic_rans_decode_step, with
 *     stream_off    B*G + 1 entries, stream_bytes B*G, esc_off B*G + 1: block b * G + g is sub-stream g of image b
 *     state         [B*G][LIC_RANS_STATE_WORDS], one block per sub-stream, seeded and checked as above
 *     tables, center, dest, ypad: per IMAGE, unchanged; round r's rows start at dword (b * n*M + 64 r) * (2W+2)
 *   A wave whose group has no round in this step (fewer rounds than G) leaves its state block bit for bit as it
 *   found it.  Error words are per block: a block in error decodes its later symbols as the table centre, the other
 *   blocks of the image carry on.  G = 1 is lic_rans_decode_step.  G outside 1..LIC_RANS_MAX_GROUPS:
 *   LIC_ERR_INVALID; B * G <= 65535 (LIC_ERR_UNSUPPORTED above); the other limits as above.
 * ------------------------------------------------------------------------------------------ */
#define LIC_RANS_MAX_GROUPS 8
int lic_rans_decode_step_groups(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                const uint32_t* tables, const int32_t* center, int32_t B, int32_t G, int32_t n,
                                int32_t M, int32_t W, const int64_t* dest, float* ypad, int64_t pixels,
                                lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2f -- the same step for images that bring DIFFERENT numbers of rows to it, or none
 *   (codec.ContextCodec.decompress_images): nimg * G workgroups of one wave; tables, centres and dest of the step are
 *   the images' rows one after the other, total_rows in all.  The arguments of lic_rans_decode_step_groups, with
 *     tables        [total_rows * M][2W+2] (16-byte aligned), center [total_rows * M], dest [total_rows]
 *     seg           [nimg][2] int32 (device): image b's rows of this step are seg[b][0] .. seg[b][0] + seg[b][1] of
 *                   those; its symbols number seg[b][1] * M, its tables start at dword seg[b][0] * M * (2W+2) -- any
 *                   offset mod 4 -- and dest[seg[b][0] + k / M] is symbol k's pixel INSIDE the image's plane
 *     ypad, ypad_len  one flat fp32 buffer and its length in floats; image b's plane is
 *                   ypad[y_base[b] .. y_base[b] + pixels[b] * M), element (d, c) at y_base[b] + d * M + c;
 *                   y_base, pixels: [nimg] int64 (device)
 *   A wave whose image has seg[b][1] == 0 (finished, or idle in this step), or whose group has no round in the step,
 *   returns before it reads its state block: the block stays bit for bit as it was.  Checked on the device before
 *   anything is addressed: a segment with a negative entry or an end beyond total_rows sets LIC_RANS_ERR_RANGE in the
 *   blocks of that image and decodes nothing; a plane that does not lie inside [0, ypad_len) counts as empty, so
 *   every destination of the image is refused (LIC_RANS_ERR_RANGE, nothing written); a dest outside [0, pixels[b]) is
 *   refused alike.  No table read goes beyond dword total_rows * M * (2W+2).  Cursor rules, error words and their
 *   effect are lic_rans_decode_step's, per block.  With every image at seg[b] = (b * n, n), y_base[b] = b * pixels * M
 *   this is lic_rans_decode_step_groups.
 *   NULL pointers, nimg, total_rows, M, W, ypad_len <= 0, G outside 1..LIC_RANS_MAX_GROUPS, misaligned pointers
 *   (tables 16 bytes, int64 arrays 8, the others 4): LIC_ERR_INVALID.  W > 64, total_rows * M >= 2^31 - 64,
 *   nimg * G > 65535, ypad_len > 2^40: LIC_ERR_UNSUPPORTED.  One launch, no allocation, no synchronisation.
 * ------------------------------------------------------------------------------------------ */
int lic_rans_decode_step_ragged(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                const uint32_t* tables, const int32_t* center, const int32_t* seg, int32_t nimg,
                                int32_t G, int64_t total_rows, int32_t M, int32_t W, const int64_t* dest, float* ypad,
                                const int64_t* y_base, const int64_t* pixels, int64_t ypad_len, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layered codec (codec.ScalableCodec) -- lic_rans_decode_step_groups for L layers of one latent in ONE launch:
 *   L * B * G workgroups of one wave.  Every layer is a "rANS-64 x G" stream set of its own over its own channels,
 *   with its own tables; the waves of different layers are independent and share the launch, dest and the plane.
 *     stream_off, stream_bytes, esc_off, state   LAYER-MAJOR: block (l * B + b) * G + g is sub-stream g of image b of
 *                   layer l (L*B*G + 1 offsets, L*B*G lengths and state blocks), so a call with the first layer
 *                   alone stages and launches L = 1 with no gaps
 *     layers        [L] rows, 1 <= L <= LIC_MAX_LAYERS, a HOST array that is copied into the launch: layer l has
 *                   channels [c0, c0 + M), tables [B][n*M][2W+2] (16-byte aligned) and center [B][n*M]
 *     n, W, dest, ypad, pixels   call-wide, as in lic_rans_decode_step; ypad is [B][pixels][y_pix] with
 *                   y_pix >= c0 + M for every layer.  Symbol k of a layer's step is pixel k / M, channel c0 + k % M:
 *                   element (b, dest[k / M], c0 + k % M) is written, no other
 *   Per block every rule of lic_rans_decode_step_groups holds: cursors are compared before each read, error words are
 *   per block, a group without a round in its layer's step (n * M symbols) leaves its state block bit for bit.  With
 *   L = 1, c0 = 0, y_pix = M this is lic_rans_decode_step_groups.
 *   NULL pointers, L outside 1..LIC_MAX_LAYERS, M <= 0, c0 < 0, c0 + M > y_pix, overlapping channel ranges, B, n, W,
 *   pixels <= 0, G outside 1..LIC_RANS_MAX_GROUPS, misaligned pointers (tables 16 bytes, int64 arrays 8, the others 4):
 *   LIC_ERR_INVALID.  W > 64, n * M >= 2^31 - 64, L * B * G > 65535: LIC_ERR_UNSUPPORTED.  Nothing is launched then.
 *   One launch, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_rans_layer {
  const uint32_t* tables;
  const int32_t* center;
  int32_t c0, M;
} lic_rans_layer;
int lic_rans_decode_step_layers(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                const lic_rans_layer* layers, int32_t L, int32_t B, int32_t G, int32_t n, int32_t W,
                                const int64_t* dest, float* ypad, int64_t pixels, int64_t y_pix, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layered codec, many latents of different sizes (codec.ScalableCodec.decompress_images / decompress_base_images) --
 *   lic_rans_decode_step_ragged for L layers in ONE launch: L * nimg * G workgroups of one wave.
 *     stream_off, stream_bytes, esc_off, state   LAYER-MAJOR: block (l * nimg + b) * G + g is sub-stream g of image b
 *                   of layer l (L*nimg*G + 1 offsets, L*nimg*G lengths and state blocks); a base-only call is L = 1
 *                   with no gaps
 *     layers        [L] rows, 1 <= L <= LIC_MAX_LAYERS, a HOST array that is copied into the launch: layer l has
 *                   channels [c0, c0 + M), tables [total_rows * M][2W+2] (16-byte aligned) and center [total_rows * M]
 *     seg           [nimg][2] int32 (device), shared by the layers, which share the schedule: image b's rows of this
 *                   step are seg[b][0] .. seg[b][0] + seg[b][1]; in layer l its symbols number seg[b][1] * M and its
 *                   tables start at dword seg[b][0] * M * (2W+2) of the layer's tables -- any offset mod 4
 *     dest, ypad, ypad_len, y_base, pixels   as in lic_rans_decode_step_ragged; y_pix is call-wide, >= c0 + M for
 *                   every layer: image b's plane is ypad[y_base[b] .. y_base[b] + pixels[b] * y_pix), and symbol k of
 *                   layer l writes element (dest[seg[b][0] + k / M], c0 + k % M) at y_base[b] + d * y_pix + c0 + k % M.
 *                   No other element is touched.
 *   Per block every rule of lic_rans_decode_step_ragged holds: cursors are compared before every read; error words are
 *   per block; a wave whose image has seg[b][1] == 0, or whose group has no round in its layer's step, returns before
 *   it reads its state block; a segment with a negative entry or an end beyond total_rows sets LIC_RANS_ERR_RANGE in
 *   that image's blocks of every layer and decodes nothing; a plane that does not lie inside [0, ypad_len), measured
 *   with pixels[b] * y_pix, counts as empty, so every destination of the image is refused (LIC_RANS_ERR_RANGE, nothing
 *   written); no table read goes beyond dword total_rows * M * (2W+2) of its layer.
 *   With L = 1, c0 = 0, y_pix = M this is lic_rans_decode_step_ragged.  With every image at seg[b] = (b * n, n) and
 *   y_base[b] = b * pixels * y_pix it is lic_rans_decode_step_layers.
 *   NULL pointers, L outside 1..LIC_MAX_LAYERS, M <= 0, c0 < 0, c0 + M > y_pix, overlapping channel ranges, nimg,
 *   total_rows, W, ypad_len, y_pix <= 0, G outside 1..LIC_RANS_MAX_GROUPS, misaligned pointers (tables 16 bytes, int64
 *   arrays 8, the others 4): LIC_ERR_INVALID.  W > 64, total_rows * M >= 2^31 - 64, L * nimg * G > 65535,
 *   ypad_len > 2^40: LIC_ERR_UNSUPPORTED.  Nothing is launched then.  One launch, no allocation, no synchronisation,
 *   graph-capturable.
 * ------------------------------------------------------------------------------------------ */
int lic_rans_decode_step_layers_ragged(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                                       const uint32_t* escapes, const int64_t* esc_off, uint32_t* state,
                                       const lic_rans_layer* layers, int32_t L, const int32_t* seg, int32_t nimg,
                                       int32_t G, int64_t total_rows, int32_t W, const int64_t* dest, float* ypad,
                                       const int64_t* y_base, const int64_t* pixels, int64_t ypad_len, int64_t y_pix,
                                       lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2 -- the device encoder of the same streams: byte for byte what the host encoder of lic_codec.h
 *   writes, from the tables where lic_gmm_cdf_tables left them, so no table ever travels to the host.  Two
 *   launches per batch on one stream, lic_rans_encode_pick then lic_rans_encode.  (This lic_rans_encode is the
 *   entry of the device library; the host coder of the same name lives in the host library of lic_codec.h.  The
 *   two headers describe two libraries and are not meant for one translation unit.)
 *
 *   lic_rans_encode_pick -- the parallel half, one thread per symbol.  Image b has P pixels of M channels, nsym =
 *   P * M symbols; symbol k in CODING order is pixel order[k / M], channel k % M.
 *     tables        [B][P*M][2W+2] and center [B*P][M]: lic_gmm_cdf_tables' outputs, raster pixel order, as written
 *     y             [B][P][M] int32: the integer latents, pixel-major (the rounded symbols, not fp32)
 *     order         [P] int64 (device): the raster pixel of every position of the coding order (the wavefront
 *                   steps of codec.ContextCodec, concatenated), each in [0, P)
 *     sf            [B][nsym] uint32 out, coding order: cum[s] << 16 | (cum[s+1] - cum[s]) of the coded symbol
 *                   s = clamp(idx, 0, S-1), idx = y - center + W in 32-bit two's complement, S = 2W+1
 *     exc           [B][nsym] uint32 out, coding order: the escape excess (-idx for idx <= 0, idx - (S-1) for
 *                   idx >= S-1; idx == 0 and idx == S-1 escape with excess 0) or 0xFFFFFFFF for no escape; the
 *                   largest real excess is 2^31
 *     state         [B][LIC_RANS_STATE_WORDS] uint32: only the error word (the last) is touched here, by atomic OR.
 *                   The caller ZEROES every image's error word before this launch.
 *   Every symbol's table is validated as the host does: cum[0] == 0, cum[S] == 65536, 0 < freq < 65536 (and
 *   cum[s] < 65536, which a table that passes the others can only miss by not being monotone); order entries must
 *   lie in [0, P).  A violation sets LIC_RANS_ERR_RANGE in that image's error word and codes that symbol as
 *   (start 0, freq 1) without an escape, so that lic_rans_encode never divides by zero; other images are not
 *   affected.  An order entry is compared before it indexes anything: nothing outside the buffers is read.
 *   W <= 64, B <= 65535, nsym < 2^31 - 64 (LIC_ERR_UNSUPPORTED otherwise); every buffer 4-byte aligned, order 8.
 *
 *   lic_rans_encode -- the serial half, one 64-lane wave per image, lane l owns coder state l.
 *     sf, exc       lic_rans_encode_pick's outputs
 *     step_len      [nsteps] int64 (device), in symbols; zero-length steps are allowed; non-negative, summing to nsym
 *     words         [B][slot] bytes out; slot >= 2 * nsym, a multiple of 4 (lic_rans_bound(nsym) of lic_codec.h
 *                   rounded up to 4 serves).  Image b's 16-bit words, in reading order, END at the end of its
 *                   slot: bytes [slot - 2 * count, slot) of the slot; the bytes before them are not touched.
 *     esc_out       [B][nsym] uint32 out: image b's escape list in symbol order, its first `escape count` entries;
 *                   the rest is not touched
 *     state         [B][LIC_RANS_STATE_WORDS] uint32, the decoder's block layout: the 64 FINAL coder states (lane 0
 *                   first), the word count, the escape count, the error word (read at entry: pick's bits stay).
 *   The host assembles image b's stream as  64 little-endian states + its `word count` words;  that is
 *   lic_rans_encode's stream of lic_codec.h, and esc_out[b][:escape count] its escape list.
 *   Step lengths that are negative or do not add up to nsym set LIC_RANS_ERR_RANGE and code nothing (states 2^16,
 *   counts 0).  The word cursor is compared with the slot's first byte before every store; a slot as above cannot
 *   run out (at most one word per symbol), if it did the error word would say so and the store would not happen.
 *   One launch each, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
int lic_rans_encode_pick(const uint32_t* tables, const int32_t* center, const int32_t* y, const int64_t* order,
                         int32_t B, int64_t P, int32_t M, int32_t W, uint32_t* sf, uint32_t* exc, uint32_t* state,
                         lic_stream_t stream);
int lic_rans_encode(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len, int64_t nsteps, int32_t B,
                    int64_t nsym, uint8_t* words, int64_t slot, uint32_t* esc_out, uint32_t* state,
                    lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2d -- lic_rans_encode for "rANS-64 x G" streams: B * G workgroups of one wave, wave (b, g) codes the
 *   rounds of image b whose index inside their step is g, g + G, ... into block b * G + g.  lic_rans_encode_pick is
 *   the same launch as before: sf and exc are per image, in coding order, and every group reads them there.
 *     step_len      [nsteps] the IMAGE's step lengths, as for lic_rans_encode; the kernel derives each group's rounds
 *     words         [B*G][slot] bytes out, slot a multiple of 4; block's words END at the end of its slot
 *     esc_out       [B*G][esc_cap] uint32 out: the block's escape list in the order of its own symbols
 *     state         [B*G][LIC_RANS_STATE_WORDS]: final states, word count, escape count, error word per block (read
 *                   at entry, so the caller zeroes it).  lic_rans_encode_pick strides its `state` by one block per
 *                   IMAGE, so for G > 1 it is given a [B] block buffer of its own; an image is in error if its
 *                   pick block or any of its G blocks here is.
 *   Sizes.  Sub-stream g of an image holds  n_g = sum over steps t of |{k < step_len[t] : (k / 64) % G == g}|
 *   symbols.  A symbol costs at most one 16-bit word (lic_codec.h) and at most one escape, so
 *     slot >= 2 * max_g n_g (rounded up to 4)  and  esc_cap >= max_g n_g
 *   can never run out; n_g <= nsym, so slot = 2 * nsym (rounded up to 4) and esc_cap = nsym always serve.  The
 *   entry cannot see the step lengths, so it does not check these two sizes beyond slot >= 4, slot % 4 == 0 and
 *   esc_cap >= 1; the kernel compares the word cursor with the slot's first word and the escape cursor with esc_cap
 *   before EVERY store: a block whose slot or list is too small stores nothing outside it and reports
 *   LIC_RANS_ERR_RANGE.  Bad step lengths: all G blocks of the image report, as lic_rans_encode's one does.
 *   G = 1 with esc_cap = nsym is lic_rans_encode.  G outside 1..LIC_RANS_MAX_GROUPS: LIC_ERR_INVALID; B * G <= 65535.
 * ------------------------------------------------------------------------------------------ */
int lic_rans_encode_groups(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len, int64_t nsteps,
                           int32_t B, int32_t G, int64_t nsym, uint8_t* words, int64_t slot, uint32_t* esc_out,
                           int64_t esc_cap, uint32_t* state, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2g -- the same encoder for images of DIFFERENT sizes in one launch each
 *   (codec.ContextCodec.compress_images): the tables, centres and symbols of all images are rows one after the
 *   other, total_rows rows of M values, as one lic_gmm_cdf_tables launch leaves them.  Where an image's rows, steps,
 *   slots and lists lie is said by two descriptor tables of int64 words on the device:
 *     images        [nimg][LIC_RANS_IMAGE_WORDS]: ROW0 the image's first row in tables / center / y, which is also
 *                   its first coding position (its symbols are sf / exc [ROW0 * M, (ROW0 + P) * M)); P its pixels
 *                   (>= 1); STEP0 its first entry in the flat step_len array; NSTEPS its steps
 *     blocks        [nimg*G][LIC_RANS_BLOCK_WORDS], image-major: WORD_OFF the byte offset of the block's slot in
 *                   `words` (a multiple of 4); SLOT its bytes (a multiple of 4, >= 4); ESC_OFF the first uint32 entry
 *                   of its escape list in esc_out; ESC_CAP its entries (>= 1).  Sizes as for lic_rans_encode_groups,
 *                   per image: SLOT >= 2 * max_g n_g rounded up to 4 and ESC_CAP >= max_g n_g never run out.
 *
 *   lic_rans_encode_pick_ragged -- one thread per symbol of the whole call.  Coding position q (symbol k = q * M + c)
 *   belongs to image row_image[q] and stands for raster pixel order[q] of that image: its table row is ROW0 + order[q].
 *     row_image, order   [total_rows] int64 each (device)
 *     sf, exc       [total_rows * M] uint32 out, as lic_rans_encode_pick writes them, image after image
 *     state         [nimg][LIC_RANS_STATE_WORDS]: one block per IMAGE, only the error word is touched, by atomic OR;
 *                   the caller zeroes it
 *   Checked before anything is indexed: row_image[q] in [0, nimg), ROW0 >= 0, P >= 1, ROW0 + P <= total_rows, q in
 *   [ROW0, ROW0 + P), order[q] in [0, P).  A violation, or a malformed table (lic_rans_encode_pick's rules), codes the
 *   symbol as (start 0, freq 1) and sets LIC_RANS_ERR_RANGE in the image's error word; a row whose row_image names no
 *   image is coded likewise and can report nowhere.  Other images are not affected.
 *
 *   lic_rans_encode_ragged -- nimg * G workgroups of one wave; wave (b, g) is lic_rans_encode_groups' wave on the
 *   image's own sf / exc / step_len ranges and on block b * G + g's own slot and list.  G = 1 is the same kernel.
 *     step_len, steps_len   all images' step lengths in one int64 array (device) and its length in entries
 *     words, words_len      one byte buffer for all slots and its length; a block's words END at the end of its slot
 *     esc_out, esc_len      one uint32 buffer for all escape lists and its length in entries
 *     state         [nimg*G][LIC_RANS_STATE_WORDS]: final states, word count, escape count, error word (read at
 *                   entry, so the caller zeroes it); an image is in error if its pick block or one of its G blocks is
 *   A wave compares its descriptors with the given lengths before it addresses anything: no negative entry, P >= 1,
 *   ROW0 + P <= total_rows, P * M < 2^31 - 64, STEP0 + NSTEPS <= steps_len, WORD_OFF and SLOT multiples of 4,
 *   SLOT >= 4, WORD_OFF + SLOT <= words_len, ESC_CAP >= 1, ESC_OFF + ESC_CAP <= esc_len.  A block that fails, or whose
 *   image's step lengths are negative or do not add up to P * M, reports LIC_RANS_ERR_RANGE with states 2^16 and
 *   counts 0 and reads and writes nothing else; the blocks of other images are not affected.  Word and escape cursor
 *   are compared with the slot's first word and ESC_CAP before every store, as in lic_rans_encode_groups.
 *   Both entries: NULL pointers, nimg, total_rows, M (W; steps_len, words_len, esc_len) <= 0, G outside
 *   1..LIC_RANS_MAX_GROUPS, misaligned pointers (int64 arrays 8 bytes, the others 4): LIC_ERR_INVALID.  W > 64,
 *   nimg * G > 65535 (pick: nimg > 65535), total_rows * M >= 2^31 - 64: LIC_ERR_UNSUPPORTED.  One launch each, no
 *   allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
#define LIC_RANS_IMAGE_WORDS 4
#define LIC_RANS_IMAGE_ROW0 0
#define LIC_RANS_IMAGE_P 1
#define LIC_RANS_IMAGE_STEP0 2
#define LIC_RANS_IMAGE_NSTEPS 3
#define LIC_RANS_BLOCK_WORDS 4
#define LIC_RANS_BLOCK_WORD_OFF 0
#define LIC_RANS_BLOCK_SLOT 1
#define LIC_RANS_BLOCK_ESC_OFF 2
#define LIC_RANS_BLOCK_ESC_CAP 3
int lic_rans_encode_pick_ragged(const uint32_t* tables, const int32_t* center, const int32_t* y, int64_t total_rows,
                                const int64_t* images, int32_t nimg, const int64_t* row_image, const int64_t* order,
                                int32_t M, int32_t W, uint32_t* sf, uint32_t* exc, uint32_t* state,
                                lic_stream_t stream);
int lic_rans_encode_ragged(const uint32_t* sf, const uint32_t* exc, const int64_t* step_len, int64_t steps_len,
                           const int64_t* images, const int64_t* blocks, int32_t nimg, int32_t G, int64_t total_rows,
                           int32_t M, uint8_t* words, int64_t words_len, uint32_t* esc_out, int64_t esc_len,
                           uint32_t* state, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).2h -- the hyper-latent z as "rANS-64 x G" streams, coded by kernels (codec.ContextCodec(z_coder="rans")).
 *   The z prior has no parameters: a stream has M tables [M][S+1] (lic_factorized_cdf_tables' output, any S >= 2) and
 *   symbol k of an image -- pixel by pixel, channel by channel over its [h4][w4][M] plane -- uses table k % M and
 *   codes idx = z - lo.  An image is ONE step of all its symbols: round r (symbols 64 r .. 64 r + 63) belongs to
 *   sub-stream r % G, and the edge symbols 0 and S-1 escape into the sub-stream's uint32 list, exactly as for y.
 *
 *   lic_rans_z_pick -- the parallel half of the encoder, one thread per z symbol of the whole call; all images lie
 *   flat, one after the other, each a multiple of M symbols long, so k % M is the channel everywhere.
 *     tables        [M][S+1] uint32
 *     z             [n] int32: the rounded hyper-latents of all images (the symbols, not fp32)
 *     sf, exc       [n] uint32 out, exactly lic_rans_encode_pick's words: cum[s] << 16 | freq of s = clamp(idx, 0, S-1),
 *                   idx = z - lo in 32-bit two's complement; the excess (-idx for idx <= 0, idx - (S-1) for idx >= S-1,
 *                   0 at idx == 0 and idx == S-1) or 0xFFFFFFFF for no escape
 *     err           one uint32 for the whole call, touched by atomic OR only; the caller zeroes it and folds it into
 *                   every block's error word
 *   The table of every symbol is validated as lic_rans_encode_pick does (cum[0] == 0, cum[S] == 65536, 0 < freq <
 *   65536); a violation codes (start 0, freq 1) without an escape and ORs LIC_RANS_ERR_RANGE into *err.
 *   The serial half is lic_rans_encode_ragged, unchanged: image b is the descriptor (ROW0 = its first pixel, P = its
 *   h4 * w4 pixels, NSTEPS = 1) with the step length P * M, sf and exc as written here.
 *   NULL pointers, M <= 0, S < 2, n <= 0, n % M != 0, a pointer that is not 4-byte aligned: LIC_ERR_INVALID.
 *   S > LIC_RANS_Z_MAX_S, M > LIC_RANS_Z_MAX_M, n >= 2^31 - 64: LIC_ERR_UNSUPPORTED.
 *
 *   lic_rans_z_decode -- nimg * G workgroups of one wave; wave (b, g) decodes rounds g, g + G, ... of image b's single
 *   step from block b * G + g.  streams .. state are lic_rans_decode_step_ragged's staging arguments and state blocks
 *   (seeded with the streams' 64 states, 0, 0, 0; checked by the caller afterwards: word cursor at the end, escape
 *   cursor at its count, every state 2^16, error word 0).
 *     nsym          [nimg] int64 (device): image b's symbols, >= 0.  0: the image has no z in this call, its blocks
 *                   stay bit for bit as they were.  So do the blocks of groups g >= ceil(nsym / 64).
 *     z, z_len      one flat fp32 buffer and its length in floats; z_base [nimg] int64 (device): symbol k of image b is
 *                   written to z[z_base[b] + k] as float(idx + lo), the escape excess applied at the edge symbols.
 *                   Nothing else is written.
 *     path          LIC_RANS_Z_AUTO: the M tables are staged once per wave into LDS as M rows of S 16-bit entries
 *                   (cum[0..S-1] < 65536, cum[S] implied) at a pitch of the smallest P >= S with P % 4 == 2, and stay
 *                   there for the whole stream, if M * P * 2 <= LIC_RANS_Z_LDS_BYTES (192 x 129: 49 920 bytes);
 *                   otherwise the rows are searched in global memory.  LIC_RANS_Z_RESIDENT forces the first
 *                   (LIC_ERR_INVALID above the budget), LIC_RANS_Z_GLOBAL the second.  Both write the same bytes.
 *                   lic_rans_z_decode_path(M, S) says which of the two AUTO takes (a host function, no launch).
 *   Checked on the device before anything is addressed with it: a negative nsym or one of 2^31 - 64 or more, or a plane
 *   that does not lie inside [0, z_len), sets LIC_RANS_ERR_RANGE in the image's blocks, reads and writes nothing else.
 *   Every wave validates the tables while it stages them, by pick's rules: a malformed table sets LIC_RANS_ERR_RANGE in
 *   the block and decodes nothing, no z element is written.  A stream_bytes below 256 or beyond its slot, or a
 *   stream_off that is negative or no multiple of 4: LIC_RANS_ERR_STREAM.  Word and escape cursors are compared with
 *   their lengths before every read: out of range reads nothing and sets LIC_RANS_ERR_RANGE.  A block in error decodes
 *   its later symbols as lo + S / 2; the other blocks carry on.
 *   NULL pointers, M, nimg, z_len <= 0, S < 2, G outside 1..LIC_RANS_MAX_GROUPS, an unknown path, misaligned pointers
 *   (int64 arrays 8 bytes, the others 4): LIC_ERR_INVALID.  S > LIC_RANS_Z_MAX_S, M > LIC_RANS_Z_MAX_M, nimg * G > 65535,
 *   z_len > 2^40: LIC_ERR_UNSUPPORTED.  One launch each, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
#define LIC_RANS_Z_AUTO 0
#define LIC_RANS_Z_RESIDENT 1
#define LIC_RANS_Z_GLOBAL 2
#define LIC_RANS_Z_LDS_BYTES 65536 /* the LDS budget of the resident path */
#define LIC_RANS_Z_MAX_S 4096
#define LIC_RANS_Z_MAX_M 65535
int lic_rans_z_pick(const uint32_t* tables, int32_t M, int32_t lo, int32_t S, const int32_t* z, int64_t n, uint32_t* sf,
                    uint32_t* exc, uint32_t* err, lic_stream_t stream);
int lic_rans_z_decode_path(int32_t M, int32_t S);
int lic_rans_z_decode(const uint8_t* streams, const int64_t* stream_off, const int64_t* stream_bytes,
                      const uint32_t* escapes, const int64_t* esc_off, uint32_t* state, const uint32_t* tables,
                      int32_t M, int32_t lo, int32_t S, int32_t nimg, int32_t G, const int64_t* nsym,
                      const int64_t* z_base, float* z, int64_t z_len, int32_t path, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).1 -- evaluation metric on the device.
 * Multi-scale SSIM exactly as the reference's evaluator calls it (Evaluator.py:7,38,45:
 * `ms_ssim(recon, orig, data_range=1.0, size_average=True)` of the third-party pytorch-msssim==0.2.1,
 * requirements.txt:5 -- absent offline, PARITY UNPINNED; follows the package's published algorithm:
 * 11-tap sigma-1.5 Gaussian window, valid filtering, K=(0.01,0.03), 5 scales, 2x2 average pooling with
 * zero padding of odd sides, default weights).  x, y: element (b,c,h,w) at b*sb + c*sc + h*sh + w*sw
 * (any NCHW / channels_last view).  out[B*C] = per-image per-channel MS-SSIM (the package's value is
 * its mean); level_out[5][B*C][2] = per-scale (mean ssim, mean cs).  min(H, W) must exceed 160 (the
 * package's assertion) -> LIC_ERR_UNSUPPORTED otherwise.
 * ------------------------------------------------------------------------------------------ */
size_t lic_msssim_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int lic_msssim(const float* x, const float* y, int32_t B, int32_t C, int32_t H, int32_t W, int64_t sb,
               int64_t sc, int64_t sh, int64_t sw, float data_range, float* out, float* level_out,
               void* workspace, size_t workspace_bytes, lic_stream_t stream);
/* Gradient of lic_msssim's out[B*C] with respect to x, its first argument (none for y): what training for
 * MS-SSIM needs.  x, y, the shape, the strides and data_range as in the forward call; level_out and
 * fwd_workspace (fwd_workspace_bytes >= lic_msssim_workspace_bytes) are that call's outputs, unchanged since:
 * the pooled planes of scales 1..4 are READ from the forward's workspace, not pooled again.  gout[B*C] =
 * upstream gradient of out; dx = fp32, element (b,c,h,w) at b*sb + c*sc + h*sh + w*sw like x (every element
 * is written; dx may not alias x or y).  workspace holds the gradients of the pooled planes.
 * Five launches, one per scale, coarsest first; each output pixel is a gather over the coefficient maps
 * around it (no atomics: two runs give the same bits).
 * DEVIATION, deliberate: where any per-scale term of an image-channel is <= 0 the forward value is 0 and the
 * derivative of relu(t)^w is undefined there (torch gives inf / NaN); dx of that image-channel is exactly 0.
 * Other image-channels of the batch are unaffected. */
size_t lic_msssim_bwd_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int lic_msssim_bwd(const float* x, const float* y, int32_t B, int32_t C, int32_t H, int32_t W, int64_t sb,
                   int64_t sc, int64_t sh, int64_t sw, float data_range, const float* level_out,
                   const void* fwd_workspace, size_t fwd_workspace_bytes, const float* gout, float* dx,
                   void* workspace, size_t workspace_bytes, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f).3 -- input pipeline and logging statistics.
 *   lic_u8_to_f32: out[i] = float(in[i]) / 255 (true division: bit-identical to torchvision
 *     ToTensor(), Dataloader.py:7-9) for uint8 NHWC shards; `in` 4-byte, `out` 16-byte aligned.
 *   lic_tensor_stats: stats[6] = count, sum, sum of squares, min, max, NaN count (fp64) and hist[nbins]
 *     (uint64) over [lo, hi] with outliers clamped into the edge bins -- the summary the reference's
 *     logging (Trainer.py:167-217: add_histogram / mean of whole latent tensors) needs, without the
 *     full-tensor D2H copy.  Reproducible (integer atomics + fixed-order fp64 reduction).
 * ------------------------------------------------------------------------------------------ */
int lic_u8_to_f32(const uint8_t* in, float* out, int64_t n, lic_stream_t stream);
size_t lic_tensor_stats_workspace_bytes(void);
int lic_tensor_stats(const float* x, int64_t n, int32_t nbins, float lo, float hi, double* stats,
                     uint64_t* hist, void* workspace, size_t workspace_bytes, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_window -- a window of an image with a rule for what lies outside it: crop and pad as one gather.
 *   The reference crops once, offline, on the host (preprocess.py:30-32: one fixed 256x256 window per source
 *   image) and converts every item with ToTensor() (Dataloader.py:23-27, 39-43); a `transform` argument is its
 *   only way to a random crop.  Here images of any size are windowed on the device:
 *     out[b, oy, ox, c] = src_b(border(y0 + oy), border(x0 + ox'), c),   ox' = (flags & 1) ? w - 1 - ox : ox
 *   `out` is [B][h][w][C] contiguous fp32 (16-byte aligned, at most 2^31 - 1 elements): the channels_last
 *   memory the conv kernels read.  `border`: LIC_WINDOW_ZERO = zeros outside the image, LIC_WINDOW_REPLICATE =
 *   the coordinate is clamped, LIC_WINDOW_REFLECT = torch's 'reflect' (the edge is not repeated), legal only
 *   while every overhang is smaller than the source side it reflects about.
 *   Every coordinate is resolved to an in-range index (or to a literal zero) before any load, so no address
 *   leaves an image's [src_offset, src_offset + Hs*Ws*C) whatever the window.
 *   lic_window_u8_to_f32: uint8 images anywhere in `pool` (any byte alignment), one job per output image in a
 *     device-resident table (8-byte aligned); the value is float(v) / 255, the same single division as
 *     lic_u8_to_f32, so a window that is the whole image gives lic_u8_to_f32's bits.  The table lives on the
 *     device, so the library cannot inspect it: Hs, Ws >= 1, offsets inside the pool and the reflect rule are
 *     the caller's to check before the upload (data.window_jobs does); an illegal reflect overhang is clamped.
 *   lic_window_f32: one window of a strided fp32 [B, C, Hs, Ws] tensor (element strides >= 0: NCHW-contiguous,
 *     channels_last or a view), a plain copy.  LIC_ERR_INVALID for an illegal reflect overhang.
 *   One launch each, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
enum lic_window_border { LIC_WINDOW_ZERO = 0, LIC_WINDOW_REPLICATE = 1, LIC_WINDOW_REFLECT = 2 };
typedef struct lic_window_job { /* 32 bytes, one per output image */
  int64_t src_offset;           /* bytes from `pool` to this image's [Hs][Ws][C] uint8 pixels */
  int32_t Hs, Ws;               /* source image size */
  int32_t y0, x0;               /* window origin in source coordinates; may be negative */
  int32_t flags;                /* bit 0: horizontal flip of the WINDOW (applied after the border rule) */
  int32_t reserved;
} lic_window_job;
int lic_window_u8_to_f32(const uint8_t* pool, const lic_window_job* jobs_device, int32_t B, int32_t h, int32_t w,
                         int32_t C, int32_t border, float* out, lic_stream_t stream);
int lic_window_f32(const float* src, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int32_t B, int32_t C,
                   int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t h, int32_t w, int32_t border, float* out,
                   lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_resample -- a window of an image resized with Pillow's 8-bit bicubic filter: resize, crop, flip and
 *   ToTensor() as one launch.
 *   The reference draws a downscale factor per image, resizes with Image.BICUBIC and cuts one crop, once,
 *   offline, on the host (preprocess.py:23-33).  Pillow's 8-bit resize is integer arithmetic on integer
 *   coefficients, so the result here equals Pillow's byte for byte.  The resize is defined per axis.
 *   One axis, n_in samples to n_out.  n_out == n_in: the axis is copied (Pillow skips the pass).  Otherwise,
 *   in IEEE double with every operation rounded on its own (no fused multiply-add):
 *     scale = n_in / n_out;  fs = max(scale, 1.0);  support = 2.0 * fs;  ss = 1.0 / fs
 *     for output index xx:
 *       center = (xx + 0.5) * scale
 *       xmin = max(0, (int)(center - support + 0.5));  xmax = min(n_in, (int)(center + support + 0.5)) - xmin
 *       w[x] = bicubic((x + xmin - center + 0.5) * ss), x in [0, xmax), with a = -0.5:
 *              |t| < 1: ((a + 2) t - (a + 3)) t t + 1;   |t| < 2: (((t - 5) t + 8) t - 4) a;   else 0
 *       ww = w[0] + w[1] + ... (left to right);  w[x] = w[x] / ww
 *       k[x] = (int)(w[x] * 2^22 + (w[x] < 0 ? -0.5 : 0.5))               (truncation toward zero)
 *       out = clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255)    (32-bit integers, arithmetic shift)
 *   Two axes: the horizontal pass first, to uint8; the vertical pass on those uint8 values, to uint8; the float
 *   is float(v) / 255, the single division of lic_u8_to_f32.  A window of the resized image is computed from
 *   its own rows and columns only (the horizontal pass runs over the source rows the window's rows read) and
 *   equals resize-then-crop exactly.
 *   `out` is [B][h][w][C] contiguous fp32 (16-byte aligned, at most 2^31 - 1 elements), C <= 4
 *   (LIC_ERR_UNSUPPORTED above):
 *     out[b, oy, ox, c] = resized_b(y0 + oy, x0 + ox', c) / 255,   ox' = (flags & 1) ? w - 1 - ox : ox
 *   with resized_b image b resized to Hn x Wn.  Supported per axis: n_in / 2 <= n_out <= n_in (downscale by at
 *   most 2, so at most 9 taps), the window inside the resized image.  The job table lives on the device (8-byte
 *   aligned), so the library cannot inspect it: sizes, the range of Hn / Wn, the window and the offsets are the
 *   caller's to check before the upload (data.resample_jobs does).  Every source index is still resolved to an
 *   in-range index before any load -- first taps clamped into [0, n_in), tap counts into [0, 9], an Hn or Wn
 *   outside the supported range treated as "copy" -- so a table nobody validated produces garbage but no
 *   address leaves an image's [src_offset, src_offset + Hs*Ws*C).
 *   One launch, no allocation, no synchronisation, graph-capturable.
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_resample_job { /* 40 bytes, one per output image */
  int64_t src_offset;             /* bytes from `pool` to this image's [Hs][Ws][C] uint8 pixels */
  int32_t Hs, Ws;                 /* source image size */
  int32_t Hn, Wn;                 /* size the image is resized to */
  int32_t y0, x0;                 /* window origin in the resized image */
  int32_t flags;                  /* bit 0: horizontal flip of the WINDOW */
  int32_t reserved;
} lic_resample_job;
int lic_resample_u8_to_f32(const uint8_t* pool, const lic_resample_job* jobs_device, int32_t B, int32_t h, int32_t w,
                           int32_t C, float* out, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_prep -- every parameter-derived buffer of a model refreshed by ONE launch per optimizer step.
 *   The reference keeps derived values implicit in ATen (cuDNN/oneDNN repack weights internally; compressai's
 *   GDN recomputes beta/gamma re-parametrisations in every forward, Components.py:11-44; ContextModels.py:19
 *   masks the weight in place in every forward).  Here they are explicit buffers: the packed MFMA operand
 *   of every conv / convT weight for the forward and for the data gradient (lic_pack_weight /
 *   lic_pack_weight_bf16 layouts), beta_eff and the two packed gamma_eff panels of every GDN, the
 *   column-matrix forms of the RGB stem / head weights.  A job describes one buffer:
 *     PACK_F32 / PACK_BF16: dst = packed operand of the logical [taps][K][N] tensor whose element (tap, k, n)
 *       is value(src[tap*s_tap + koff(k) + noff(n)]), koff(k) = kdiv ? (k/kdiv)*s_kq + (k%kdiv)*s_kr : k*s_kq
 *       (same for n): the split index expresses the (tap, channel) <-> column maps of the RGB layers;
 *     MAP: dst[i] = value(src[i]), i < N;   MASK_INPLACE: src[i] *= mask[i], i < N (ContextModels.py:19);
 *     value(v) = v * mask (when `mask` is set, same offset as src), then transform 1 = the GDN
 *       re-parametrisation max(v, bound)^2 - pedestal (lic_gdn_reparam).
 *   A pack job may read a tensor that a MASK_INPLACE job of the same launch is masking, provided it names the
 *   same mask: mask values are 0 or 1, so w*m and (w*m)*m are the same float whichever the read observes.
 *   Usage: fill jobs on the host, lic_prep_plan (fills the derived fields, returns the grid size), copy the
 *   array to device memory once, then lic_prep_run once per optimizer step.  Results are bit-identical to
 *   the stand-alone entry points.
 * ------------------------------------------------------------------------------------------ */
enum lic_prep_kind { LIC_PREP_PACK_F32 = 0, LIC_PREP_PACK_BF16 = 1, LIC_PREP_MAP = 2, LIC_PREP_MASK_INPLACE = 3,
                     LIC_PREP_PACK_BF16_KPERM = 4 /* lic_pack_weight_bf16_kperm's order */,
                     LIC_PREP_PACK_BF16_STEM = 5  /* lic_pack_stem_weight_bf16: src = [N][3][5][5], K = 80 */ };
typedef struct lic_prep_job {
  const float* src;
  void* dst;
  const float* mask;
  int64_t s_tap, s_kq, s_kr, s_nq, s_nr;
  int32_t kind; /* enum lic_prep_kind */
  int32_t taps, K, N, kdiv, ndiv;
  int32_t transform; /* 0 none, 1 GDN re-parametrisation */
  float bound, pedestal;
  /* derived by lic_prep_plan */
  int32_t cpt, npad, tiled, v4, block0, nblocks;
  int64_t total;
} lic_prep_job;
int64_t lic_prep_plan(lic_prep_job* jobs, int32_t njobs);
int lic_prep_run(const lic_prep_job* jobs_device, int32_t njobs, int64_t total_blocks, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_adam -- optimizer.step() (Trainer.py:86; the reference trains with torch.optim.Adam, Main.ipynb) for every
 *   parameter of a model in ONE launch: g' = g + weight_decay*p; m += (1-beta1)(g'-m); v = beta2 v + (1-beta2) g'^2;
 *   p -= (lr / bias_correction1) * m / (sqrt(v)/sqrt(bias_correction2) + eps)   -- torch's non-amsgrad arithmetic,
 *   bias_correction{1,2} = 1 - beta{1,2}^step computed by the caller.  Jobs: fill p / m / v / n on the host,
 *   lic_adam_plan (fills block0 / nblocks, returns the grid size), keep a device copy of the array; per step
 *   lic_adam_run with `grads_host`, a HOST array of the njobs (<= 448) gradient device pointers in job order --
 *   gradients are fresh allocations every step, so their addresses travel as kernel arguments.
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_adam_job {
  float* p;       /* parameter, updated in place */
  const float* g; /* unused (gradient pointers are passed to lic_adam_run) */
  float* m;       /* exp_avg */
  float* v;       /* exp_avg_sq */
  int64_t n;      /* elements */
  int32_t block0, nblocks; /* derived by lic_adam_plan */
} lic_adam_job;
int64_t lic_adam_plan(lic_adam_job* jobs, int32_t njobs);
int lic_adam_run(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks, const float* const* grads_host,
                 double lr, double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                 double bias_correction2, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_grad_norm / lic_adam_run_scaled -- torch.nn.utils.clip_grad_norm_(parameters, max_norm) in front of
 *   optimizer.step() (the usual recipe for these models: the CompressAI example trainer clips at 1.0), and a guard
 *   against a non-finite step, on the job table and `grads_host` of lic_adam_run.  Three launches, no read-back:
 *   lic_grad_norm_partial  (once per job table / parameter group) block b of the lic_adam_plan partition writes the
 *       sum of squares of its <= 4096 gradient elements, taken in double, to partials[b] (DEVICE, total_blocks
 *       doubles).  Several groups write consecutive ranges of one buffer.
 *   lic_grad_norm_finish   (once) one workgroup sums the nparts partials in a fixed order, in double, and writes
 *       clip_state (DEVICE, 4 dwords, zeroed by the owner before the first call):
 *         [0] float    total norm: the double square root, rounded once
 *         [1] float    coefficient min(max_norm / (norm + 1e-6), 1) in fp32 arithmetic (a NaN norm gives NaN, as
 *                      torch.clamp does); exactly 1 when max_norm is +inf (norm only, no clipping)
 *         [2] uint32   1 if [0] is not finite, else 0
 *         [3] uint32   running count: incremented by [2] when count_skip is set
 *   lic_adam_run_scaled    (once per group) lic_adam_run with every gradient multiplied by [1] and rounded to fp32
 *       once before the update uses it (bit for bit what `g *= coefficient` followed by lic_adam_run gives);
 *       skip_nonfinite: when [2] is set, p / m / v are left untouched.
 *   Fixed per-thread strides and fixed-shape trees, no atomics: the norm depends on the gradients, the job order and
 *   the block size only, and is bitwise the same from run to run.
 * ------------------------------------------------------------------------------------------ */
int lic_grad_norm_partial(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                          const float* const* grads_host, double* partials, lic_stream_t stream);
int lic_grad_norm_finish(const double* partials, int64_t nparts, double max_norm, int32_t count_skip, float* clip_state,
                         lic_stream_t stream);
int lic_adam_run_scaled(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                        const float* const* grads_host, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double bias_correction1, double bias_correction2, const float* clip_state,
                        int32_t skip_nonfinite, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_adam_run_ema / lic_swap_run -- the exponential moving average (EMA) of the weights that models of this kind are
 *   evaluated, checkpointed and shipped with (the usual recipe: torch._foreach_lerp_ over every parameter behind
 *   optimizer.step()), kept inside the optimizer's one launch, and its exchange with the live weights.
 *   lic_adam_run_ema   lic_adam_run (clip_state NULL: no scaling, no guard, skip_nonfinite ignored) or
 *       lic_adam_run_scaled (clip_state given) on the same job table, partition and `grads_host`, with one more
 *       stream per element.  ema_device: a DEVICE array of njobs float* in job order -- the averages are persistent
 *       buffers, so their addresses do not travel per step; a NULL entry means that tensor has no average.  After the
 *       new p has been formed exactly as those two entries form it,
 *           e = e + w * (p_new - e),   w = (float)ema_weight
 *       in three separately rounded fp32 operations (subtract, multiply, add; never a fused multiply-add), stored
 *       with the vector width of p (an average that is not 16-byte aligned is read and written element by element;
 *       which path p / g / m / v take does not depend on it).  skip_nonfinite with clip_state[2] set leaves e
 *       untouched like p / m / v.  ema_weight outside [0, 1] (or NaN), ema_device NULL or not aligned to a pointer:
 *       LIC_ERR_INVALID, nothing launched; the limits (448 jobs) and the other rules are lic_adam_run_scaled's.
 *       One launch, no allocation, no synchronisation; 36 bytes per element (p, g, m, v, e read; p, m, v, e written)
 *       where lic_adam_run moves 28.
 *   lic_swap_run       p <-> e, element by element, for every job with a non-NULL entry, in one launch on the same
 *       partition; m, v and the gradients are not touched.  Calling it twice restores both sides bit for bit.  The
 *       caller owns what is derived from p (packed weights, version counters).
 * ------------------------------------------------------------------------------------------ */
int lic_adam_run_ema(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks,
                     const float* const* grads_host, double lr, double beta1, double beta2, double eps,
                     double weight_decay, double bias_correction1, double bias_correction2, float* const* ema_device,
                     double ema_weight, const float* clip_state, int32_t skip_nonfinite, lic_stream_t stream);
int lic_swap_run(const lic_adam_job* jobs_device, int32_t njobs, int64_t total_blocks, float* const* ema_device,
                 lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_reduce_batch -- every pending reduction of a backward pass (Trainer.py:84 `loss.backward()`) in ONE launch.
 *   The weight-gradient launches end in a slab reduction and the column sums (bias / GDN beta gradients) in a second
 *   stage: 41 launches of 5-15 us per config-3 step.  lic_wgrad_bf16_partial / lic_colsum_bf16_partial /
 *   lic_colsum2_bf16_partial (bf16 operands; the fp32 path reduces right away) launch the first stage only and fill a
 *   lic_reduce_job; lic_reduce_batch(jobs, n) -- `jobs` a
 *   HOST array, copied into the kernel arguments, LIC_REDUCE_MAX_JOBS per launch -- finishes them with the arithmetic
 *   and association order of the stand-alone second stages (bitwise the same results), optionally followed per element
 *   by the GDN re-parametrisation's backward (epilogue LIC_REDUCE_EPI_REPARAM: lic_gdn_reparam_bwd with `param`, `bound`
 *   on the reduced value, `param` indexed like `dst`) and with split destination indices (mdiv / ndiv as in lic_prep_job:
 *   offset(m) = mdiv ? (m / mdiv) * sm + (m % mdiv) * smr : m * sm; rows >= Mvalid / columns >= Nvalid are dropped):
 *   the (tap, channel) <-> column maps of the RGB layers' weight gradients.  Workspaces and outputs named by a job must
 *   stay alive until the batch has been launched; block0 / nblocks are filled by lic_reduce_batch.
 * ------------------------------------------------------------------------------------------ */
enum { LIC_REDUCE_SLABS = 0, LIC_REDUCE_COLUMNS = 1 };
enum { LIC_REDUCE_EPI_NONE = 0, LIC_REDUCE_EPI_REPARAM = 1 };
#define LIC_REDUCE_MAX_JOBS 32
typedef struct lic_reduce_job {
  const float* src;   /* SLABS: [splitk][ntaps * Cm * Cn]; COLUMNS: [splitk][Cn] */
  float* dst;
  const float* param; /* epilogue REPARAM */
  int64_t sm, smr, sn, snr, stap;
  int32_t kind, epilogue;
  int32_t splitk, ntaps, Cm, Cn, Mvalid, Nvalid, mdiv, ndiv;
  float scale, bound;
  int32_t block0, nblocks;
} lic_reduce_job;
int lic_wgrad_bf16_partial(const lic_wgrad_desc* d, void* workspace, size_t workspace_bytes, lic_reduce_job* job,
                           lic_stream_t stream);
int lic_colsum_bf16_partial(const void* in, int64_t ld, int64_t P, int32_t C, float scale, float* out, void* workspace,
                            size_t workspace_bytes, lic_reduce_job* job, lic_stream_t stream);
int lic_colsum2_bf16_partial(const void* in_a, const void* in_b, int64_t ld, int64_t P, int32_t C, float scale,
                             float* out_a, float* out_b, void* workspace, size_t workspace_bytes, lic_reduce_job* jobs2,
                             lic_stream_t stream);
/* lic_leaky_bwd_bf16 on [P][C] matrices, with the column sums of dx (the bias gradient of the convolution in front of the LeakyReLU:
 * Components.py:69-73,99-103, ParametersModels.py:22-34) out of the same pass.  workspace: lic_colsum_bf16_workspace_bytes(P, C);
 * `job` NULL: out[C] is complete when the call's launches are; else the sums' second stage is left in *job for
 * lic_reduce_batch.  Same bits as lic_leaky_bwd_bf16 followed by lic_colsum_bf16 / lic_colsum_bf16_partial. */
int lic_leaky_bwd_colsum_bf16(const void* y, const void* dy, void* dx, int64_t P, int32_t C, float slope, float* out,
                              void* workspace, size_t workspace_bytes, lic_reduce_job* job, lic_stream_t stream);
int lic_reduce_batch(const lic_reduce_job* jobs, int32_t njobs, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RGB head in bf16 storage without column matrices (Components.py:45: ConvTranspose2d(C, 3, 5, stride 2, padding 2,
 *   output_padding 1); the column-matrix route of lic_igemm_bf16 + lic_col2im_bf16 / lic_im2col_bf16 remains for
 *   other geometries).
 *   lic_head_convt_bf16: out fp32 [B][2 Hi][2 Wi][3] = conv_transpose2d(x bf16 [B][Hi][Wi][Cin]) + bias; `w_packed` =
 *     lic_pack_weight_bf16(taps 1, K = Cin, N = 75..80) of the matrix w[ci][3 * (5 ky + kx) + colour] (the forward
 *     operand of the column-matrix route); Cin in {64, 128, 192}.  fp32 accumulation, nothing rounded between the
 *     channel contraction and the tap sum.
 *   lic_stem_conv_bf16: y bf16 [B][ceil(H/2)][ceil(W/2)][Cout] = conv2d(x fp32 [B][H][W][3], w, stride 2, padding 2)
 *     + bias, `w_packed` = lic_pack_stem_weight_bf16 of a [Cout][3][5][5] tensor -- the convolution of
 *     lic_stem_gdn_bf16 without the GDN.  The data gradient of the head is this convolution of dL/d(image) with the
 *     head's own weight tensor (ConvTranspose2d stores it as [Cin][3][5][5]).
 * ------------------------------------------------------------------------------------------ */
int lic_head_convt_bf16_supported(int32_t Cin, int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                                  int32_t out_pad);
int lic_head_convt_bf16(const void* x, const void* w_packed, const float* bias, float* out, int32_t B, int32_t Hi,
                        int32_t Wi, int32_t Cin, lic_stream_t stream);
int lic_stem_conv_bf16(const float* x, const void* w_packed, const float* bias, void* y, int32_t B, int32_t H, int32_t W,
                       int32_t Cout, lic_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lic_plan -- one training step (Trainer.py:75-90: forward, loss, backward) replayed on up to THREE HIP streams
 *   without Python in the loop.  The step is captured ONCE as a HIP graph (torch.cuda.graph with keep_graph=True:
 *   torch's private pool keeps every pointer fixed); lic_plan_create reads the graph's kernel / memset / memcpy /
 *   empty nodes and its edges back into a list of operations, and a SCHEDULE puts them in an issue order, each on one
 *   of the streams, with one event record + wait per cross-stream edge that stream order does not already imply;
 *   lic_plan_replay issues the schedule with plain stream launches (this ROCm walks a multi-branch graph node by node
 *   from the host: 8 ms per step instead of 0.1 ms, and a single-branch graph gives up the decoder / latent-side and
 *   data-gradient / weight-gradient overlap).  Every schedule honours every edge of the capture, so a replay computes
 *   what the captured step computed, bit for bit.
 *   `hip_graph` is a hipGraph_t and must outlive the plan (kernel arguments stay in the graph's storage).
 *   lic_plan_replay(plan, main, sides, n_sides): work queued on `main` before the call precedes the plan, work queued
 *   on it afterwards follows ALL of the plan; `sides` = up to two more, otherwise idle streams of the same device
 *   (fewer than the schedule uses: the missing ones fold onto the last one given; n_sides = 0: one stream).
 *   info[0..6] = operations, kernels, memsets, memcpys, operations not on `main`, cross-stream events, 1 when a
 *   tuned schedule is in use.
 *   lic_plan_create's schedule is the capture's own: the capture's streams are chains of the graph, and where a chain
 *   forks the successor with the longest way to go stays on the stream.  lic_plan_tune(plan, main, sides, n_sides,
 *   result) times every operation (one-stream replays with an event between operations), list-schedules them
 *   (earliest possible start first, the more critical operation on ties; long kernels of >= 192 workgroups take turns),
 *   measures capture order and three candidates end to end and keeps a tuned one only if it is >= 2 % faster;
 *   result[0..3] = sum of operation times, capture-order step, best tuned step (all us), 1 if kept.  It replays the
 *   plan a few dozen times: the capture must be idempotent (no in-place update of its own inputs -- keep the
 *   optimizer outside).
 *   Errors: LIC_ERR_UNSUPPORTED for a node kind that cannot be replayed (host, event, child-graph, allocation nodes;
 *   1-D copy nodes, whose parameters this ROCm does not hand back); lic_plan_last_error() names it.
 *   Read-back (so that a test can hold a schedule to HIP's ordering rules edge by edge, tests/plan_sched_ref.py):
 *   lic_plan_dag: sizes[0..1] = operations n, edges; with buffers of cap_ops (+1 for pred_ptr) and cap_edges entries
 *     the operations in capture order: the predecessors of k are pred_idx[pred_ptr[k] .. pred_ptr[k+1]) (all < k),
 *     kind[k] = 0 kernel, 1 memset, 2 memcpy, 3 empty, flags[k] = 1 (wide: >= 192 workgroups) | 2 (filler: the batched
 *     reduction, which capture order sends to the last stream), us[k] = the time lic_plan_tune measured (0 before).
 *   lic_plan_commands: the HIP calls lic_plan_replay makes for the schedule in use when given `n_sides` (0..2) side
 *     streams that differ from `main` and from each other, in order, as *n_cmds triples (kind, stream, argument):
 *     kind 0 = hipStreamWaitEvent, 1 = the launch of an operation, 2 = hipEventRecord; stream 0 = main, i = sides[i-1];
 *     argument = the operation for a launch, else an event id (0 the fork, 1 and 2 the joins, 3.. the schedule's
 *     cross-stream events).  `cmds` holds 3 * cap values.
 *   lic_plan_sched_host: the same list for a caller's DAG (n_ops operations in topological order, CSR predecessors,
 *     us, flags as above): mode 0 = lic_plan_create's capture-order schedule, mode 1 = lic_plan_tune's list scheduler
 *     on `ns` (1..3) streams with `wide_min_us` its bound for "long".  info (optional) [0..1] = operations not on main,
 *     cross-stream events, as lic_plan_info would report them.  Makes no HIP call: works without a GPU.
 *   All three always write the sizes; with every buffer null and every capacity 0 that is all they do (LIC_OK).  A
 *   null buffer otherwise is LIC_ERR_INVALID, one too small LIC_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------ */
typedef struct lic_plan lic_plan;
int lic_plan_create(void* hip_graph, lic_plan** out);
int lic_plan_info(const lic_plan* plan, int64_t* info);
int lic_plan_replay(lic_plan* plan, lic_stream_t main, const lic_stream_t* sides, int32_t n_sides);
int lic_plan_tune(lic_plan* plan, lic_stream_t main, const lic_stream_t* sides, int32_t n_sides, double* result);
int lic_plan_dag(const lic_plan* plan, int64_t cap_ops, int64_t cap_edges, int64_t* sizes, int32_t* pred_ptr,
                 int32_t* pred_idx, int32_t* kind, int32_t* flags, double* us);
int lic_plan_commands(lic_plan* plan, int32_t n_sides, int64_t cap, int64_t* n_cmds, int32_t* cmds);
int lic_plan_sched_host(int64_t n_ops, const int32_t* pred_ptr, const int32_t* pred_idx, const double* us,
                        const int32_t* flags, int32_t mode, int32_t ns, double wide_min_us, int32_t n_sides,
                        int64_t cap, int64_t* n_cmds, int32_t* cmds, int64_t* info);
void lic_plan_destroy(lic_plan* plan);
const char* lic_plan_last_error(void);

int lic_version(void);        /* LIC_ABI_VERSION */
int lic_last_hip_error(void); /* hipError_t of the most recent failed launch on this thread */
const char* lic_arch(void);   /* "gfx950" */

#ifdef __cplusplus
}
#endif
#endif /* LIC_H */
