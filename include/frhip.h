/* frhip -- C ABI of the MI355X (gfx950) kernels behind the Stage-3 face-recognition training step.
 *
 * Drop-in boundary.  The reference has no FFI for this path: it reaches its arithmetic
 * through torch.nn modules (cuDNN/cuBLAS underneath).  Every entry point below therefore cites the
 * reference call site (file:line under /root/reference) whose arithmetic it replaces.  The only native
 * boundary the reference does have (backbone/stylegan2/op/fused_bias_act.cpp:11-21, upfirdn2d.cpp:12-22)
 * sets the conventions copied here: contiguous device buffers, work enqueued on the caller's stream, no
 * host synchronisation, autograd kept on the Python side.
 *
 * Conventions
 *   - every function returns int: 0 ok, <0 unsupported argument (see fr_last_error_string), >0 hipError_t
 *   - pointers are device pointers borrowed for the duration of the enqueue; `stream` is a hipStream_t
 *   - no allocation, no synchronisation, no global mutable state besides the per-thread error string
 *   - activations are NHWC ("pixels x channels") in the compute dtype (FR_F32 or FR_BF16); statistics,
 *     gradients of parameters and optimizer state are always fp32; labels are int64
 */
#ifndef FRHIP_H
#define FRHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 7

enum { FR_F32 = 0, FR_BF16 = 1 };

/* prologue applied to the gathered A operand */
enum {
  FR_PRO_NONE = 0,
  FR_PRO_BN = 1,     /* x*a[c]+b[c] */
  FR_PRO_PRELU = 2,  /* x>0?x:a[c]*x */
  /* 3: FR_PRO_BNBWD2 of ABI v4 (BatchNorm backward inside the data gradient; measured +-0 on two streams, removed in v5; rebuilt
   *    and measured again in round 6 on the fragment-order kernels: +0.1 ms per step, profiles/r06_ab_bn2_in_dgrad.txt) */
  FR_PRO_RESBN = 4   /* BN1 of a residual unit applied to the OUTPUT of the unit in front of it, formed on the way:
                        o = round(a[c]*x + b[c] + x2)  (x = conv2 output of the previous unit, a / b = its BN2 coefficients, x2 =
                        src2 = that unit's input: bottleneck_IR's `res + shortcut`, backbone/model_irse.py:64-66 with the
                        MaxPool2d(1, 1) shortcut), operand = c[c]*o + d[c] (pro_c / pro_d: this unit's BN1).  o is stored to
                        pro_out (interior pixels, once each): the residual stream is materialised by its consumer and the
                        BN-apply pass behind conv2 is gone.  The batch statistics of o come from fr_bn_finalize_res.
                        Served by fr_conv3x3_strip forward launches (bf16). */
  ,
  FR_PRO_RESBN_SE = 5 /* FR_PRO_RESBN behind a squeeze-excite unit (bottleneck_IR_SE, backbone/model_irse.py:84-91):
                         o = round((a[c]*x + b[c]) * g[image][c] + x2) with the excite gates pro_g = [B][SC] fp32.  Instances
                         whose workgroups hold strips of ONE image. */
};

/* epilogue of fr_conv_igemm */
enum {
  FR_EPI_STORE = 0,     /* out = acc (+bias) */
  FR_EPI_STATS = 1,     /* + part[mtile][0][n] = sum_rows out, part[mtile][1][n] = sum_rows out^2 */
  FR_EPI_PRELU_BWD = 2, /* out = acc * (aux>0 ? 1 : epi_a[n]); part[mtile][0][n] = sum acc*aux*[aux<=0] */
  FR_EPI_BNBWD = 3,     /* out = acc; part[.][0] = sum acc; part[.][1] = sum acc*(aux-epi_a[n])*epi_b[n] */
  FR_EPI_MARGIN = 4,    /* out = scale*(n==label[m] ? phi(acc) : acc); cos_t[m] = acc[label] */
  FR_EPI_ATOMIC = 5,    /* atomicAdd(out, acc) fp32; used with splitk > 1 (summation order not reproducible) */
  FR_EPI_BIAS_RES = 7,  /* out = acc + epi_a[n] + epi_b[n] + aux[m][n]: inference with BatchNorm folded into the weights
                           (util/utils.py:254-307 runs the backbone in eval mode): epi_a / epi_b = the folded BN shifts of
                           the residual branch and of the conv shortcut (both required; pass zeros), aux = the shortcut */
  FR_EPI_STATS_X = 8,   /* FR_EPI_STATS + part[.][2][n] = sum_rows out*aux: the cross moment with the residual input (aux), from
                           which fr_bn_finalize_res derives the statistics of a*out + b + aux; part rows are [3][N] */
  FR_EPI_SLAB = 6       /* split-K slice z stores its fp32 partial (+bias in slice 0) to out[z][rows][ldc]: the caller
                           adds the splitk slabs with fr_reduce_parts(out, splitk, 1, rows*ldc, ...) -- reproducible.
                           The cut: with nk = KH*KW*SC/32 K steps of 32 channels (tap-major, then channels), slice z sums the
                           steps [nk*z/splitk, nk*(z+1)/splitk) in integer division -- uneven where splitk does not divide nk
                           (nk = 7, splitk = 3: 2, 2 and 3 steps).  splitk <= 1: one slab, all steps, with the bias.  The
                           columns N..ldc of a slab row are not written (tests/test_gpu_exact_output.py pins all of this) */
};

/* The BatchNorm arguments of fr_bn_finalize as a struct (fr_bn_finalize_res takes two of them). */
typedef struct FrBnFinArgs {
  double count;            /* elements per channel */
  const float* gamma;
  const float* beta;
  float eps, momentum;
  float* running_mean;     /* NULL: no running statistics */
  float* running_var;
  int64_t* nbt;
  float* mean;             /* outputs [C] */
  float* invstd;
  float* scale;
  float* shift;
} FrBnFinArgs;

typedef struct FrConvArgs {
  const void* src; /* A operand: NHWC [B,SH,SW,SC], pixel stride lda (elements) */
  const void* w;   /* B operand: [N][KH*KW][SC] in the compute dtype */
  void* out;       /* [B*RH*RW][ldc], compute dtype or fp32 (out_f32) */
  int32_t B, RH, RW;   /* row space: one GEMM row per (b, rh, rw) */
  int32_t SH, SW, SC;  /* source tensor geometry; SC % 32 == 0 */
  int32_t N;           /* output columns */
  int32_t KH, KW, stride, pad;
  int32_t mode;        /* 0: sh = rh*stride+kh-pad (forward); 1: sh = (rh+pad-kh)/stride (data gradient);
                          2: stride-2 3x3 data gradient for the output pixels (2i+par_h, 2j+par_w) only: rows = B*RH/2*RW/2,
                             the taps that hit no input pixel are skipped; run once per parity class */
  int32_t lda, ldc, ldaux;
  int32_t pro;         /* FR_PRO_* */
  int32_t epi;         /* FR_EPI_* */
  int32_t out_f32;
  int32_t splitk;      /* >1: K loop split over gridDim.z, requires FR_EPI_ATOMIC + out_f32 */
  int32_t stride_log2; /* filled in by the library */
  int32_t par_h, par_w; /* mode 2: parity class of the output pixels; (-1, -1) = all four classes in one launch,
                           part rows ordered [class = 2*par_h + par_w][M tile] */
  int32_t margin_kind; /* 0 ArcFace, 1 CosFace */
  int32_t easy_margin;
  float cos_m, sin_m, th, mm, scale;
  const float* pro_a; /* [SC] */
  const float* pro_b; /* [SC] */
  const float* bias;  /* [N] or NULL */
  const float* epi_a; /* [N] */
  const float* epi_b; /* [N] */
  const void* aux;    /* [rows][ldaux] compute dtype */
  float* part;        /* [ceil(rows/128)][2][N] partial column sums */
  const int64_t* label; /* [rows] */
  float* cos_t;         /* [rows] */
  /* the two-source prologues FR_PRO_RESBN / FR_PRO_RESBN_SE */
  const void* src2;    /* second source, geometry and strides of src */
  const float* pro_c;  /* [SC] */
  void* pro_out;       /* NULL or [B*SH*SW][lda]: the residual sum of every source pixel */
  const float* pro_d;  /* [SC], FR_PRO_RESBN / FR_PRO_RESBN_SE only */
  const float* pro_g;  /* [B][SC] excite gates, FR_PRO_RESBN_SE only */
  /* ABI v7: 1 = w is in MFMA-fragment order, [N / 16][taps][K / 32][64][8] with (n, tap, k) at
   * (((n / 16 * taps + tap) * (K / 32) + k / 32) * 64 + (k % 32) / 8 * 16 + n % 16) * 8 + k % 8  (N = output columns, K = SC;
   * FrPackTensor.frag writes it): the 64 lanes of a weight-fragment load then read 1024 contiguous bytes.  Taken by
   * fr_conv3x3_strip on its LDS-strip instances (fr_conv3x3_strip_takes_frag) and by fr_conv3x3_s2_strip; refused elsewhere. */
  int32_t w_frag;
  int32_t reserved_;
} FrConvArgs;

/* Convolution forward / data gradient / dense GEMM on MFMA.
 * Replaces: Conv2d 3x3 s1/s2 + neighbours in bottleneck_IR (backbone/model_irse.py:56-60), stem conv
 * (:140, through fr_stem_im2col), shortcut conv1x1 (:55), Linear(25088,512) (:147), and
 * F.linear(F.normalize(x), F.normalize(W)) + margin blend of ArcFace/CosFace (head/metrics.py:103,115-138,
 * :167,181-189); their autograd data-gradients with mode = 1. */
int fr_conv_igemm(const FrConvArgs* args, int dtype, void* stream);

/* Stride-1 3x3 convolution (bf16 only) with the input strip resident in LDS: same FrConvArgs contract as
 * fr_conv_igemm (mode 1 = data gradient: mirrored taps, w = [Cin][tap][Cout]); epilogues STORE / STATS / PRELU_BWD /
 * BNBWD.  Partial rows go to part[workgroup][2][N]; fr_conv3x3_strip_parts returns the number of workgroups for a
 * shape and epilogue, or 0 when that combination is not served (use fr_conv_igemm then).
 * Replaces Conv2d(c, d, (3,3), (1,1), 1) of bottleneck_IR (backbone/model_irse.py:57-59) fwd + data gradient. */
int fr_conv3x3_strip(const FrConvArgs* args, void* stream);
int fr_conv3x3_strip_parts(int B, int Cin, int Cout, int W, int epi);
/* 1 when fr_conv3x3_strip serves the two-source prologues (FR_PRO_RESBN[_SE]) and FR_EPI_STATS_X for a C -> C layer of width W
 * at batch B (the LDS-strip instances; not the 64-channel rolling-window kernel) */
int fr_conv3x3_strip_serves_resbn(int B, int C, int W);
/* 1 when fr_conv3x3_strip reads fragment-order weights (FrConvArgs.w_frag) for a Cin -> Cout layer of width W at batch B: the
 * shape is served and not by the 64-channel rolling-window kernel, which keeps its weights resident and takes the plain layout */
int fr_conv3x3_strip_takes_frag(int B, int Cin, int Cout, int W);

/* 1x1 convolution as a row-streaming GEMM (bf16; round 4): the weights stationary in registers, one row per output pixel,
 * stride 1 or 2 (SH = RH * stride), epilogue STORE or STATS (part[workgroup][2][N]; fr_conv1x1_stream_parts returns the number
 * of partial rows, 0 when the shape is not served: 64 -> 128, 128 -> 256, 256 -> 512 and their transposes).  Same FrConvArgs
 * fields as fr_conv_igemm (mode 0, no prologue).  Replaces shortcut_layer's Conv2d(in, depth, (1, 1), stride) of the first unit
 * of a stage (backbone/model_irse.py:52-56) forward and, with the transposed weight on dense rows, its data gradient. */
int fr_conv1x1_stream(const FrConvArgs* args, void* stream);
int fr_conv1x1_stream_parts(int B, int RH, int RW, int K, int N);

/* Stride-2 3x3 convolution (bf16, Cin == Cout: the first unit of every IR stage) on LDS-resident parity planes:
 * mode 0 = forward (SH = 2*RH), mode 2 with par_h = par_w = -1 = data gradient of all four output parity classes
 * (RH = 2*SH, w = [Cin][tap][Cout]).  Same FrConvArgs contract and epilogues as fr_conv_igemm; partial rows:
 * forward part[workgroup][2][N], gradient part[class][workgroup][2][N]; forward rows are image-major (all rows of
 * image b before those of image b + 1), the same number per image.  fr_conv3x3_s2_strip_parts returns the number of partial
 * rows for (B, channels, low-res width WL, mode), 0 when the shape is not served -- callers size and sum `part` with
 * that number and nothing else: the 64-channel layer (112 -> 56) runs on a persistent rolling-window kernel that
 * writes ONE row per work item (image x row segment) in both directions.
 * Replaces Conv2d(d, d, (3,3), stride 2, 1) of bottleneck_IR (backbone/model_irse.py:59) fwd + data gradient. */
int fr_conv3x3_s2_strip(const FrConvArgs* args, void* stream);
int fr_conv3x3_s2_strip_parts(int B, int Cin, int Cout, int WL, int mode);
/* 1 when fr_conv3x3_s2_strip reads fragment-order weights (FrConvArgs.w_frag) for (B, C -> C, low-res width WL, mode): every
 * served shape except the 64-channel layer (rolling-window kernel, weights resident, plain layout) */
int fr_conv3x3_s2_strip_takes_frag(int B, int C, int WL, int mode);

typedef struct FrWgradArgs {
  const void* g;   /* gradient of the conv output: [B*GH*GW][ldg], columns = Cout */
  const void* src; /* conv input, NHWC [B,SH,SW,SC], pixel stride lda */
  float* dw;       /* [Cout][KH*KW][SC] fp32, accumulated with atomicAdd: caller zeroes it first */
  int32_t B, GH, GW, Cout;
  int32_t SH, SW, SC;
  int32_t KH, KW, stride, pad;
  int32_t ldg, lda;
  int32_t pro; /* FR_PRO_* applied to src */
  int32_t nsplit; /* pixel slices (gridDim.y) / strip groups */
  const float* pro_a;
  const float* pro_b;
  float* slab;     /* [nsplit][Cout][taps][SC] fp32 partial gradients: required by fr_conv_wgrad_strip; optional for
                      fr_conv_wgrad (NULL: pixel slices are combined with fp32 atomics onto a zeroed dw; non-NULL: each
                      slice stores its slab and a second launch adds them in a fixed order -- reproducible; dw is then
                      OVERWRITTEN with the sum of the slabs, whatever it held) */
  /* Deferred slab sum (fr_conv_wgrad_strip only; fr_conv_wgrad ignores these fields).  defer != 0:
   * this launch only writes its slabs; the caller owes them a sum -- either as the prev_* of a later deferring launch
   * on the same stream (whose workgroups add them while their first tiles are in flight: no launch of their own) or
   * through fr_reduce_slabs.  prev_n != 0: before its own work the launch writes
   * prev_dw[i] = sum_{g < prev_groups} prev_slab[g * prev_n + i] in the library's fixed order (bit-identical to
   * fr_reduce_slabs).  prev_slab must not be this launch's slab. */
  const float* prev_slab;
  float* prev_dw;
  int64_t prev_n;
  int32_t prev_groups;
  int32_t defer;
} FrWgradArgs;

/* Weight gradient  dw[co][tap][ci] += sum_p g[p][co] * pro(src[pixel(p,tap)][ci]).
 * Replaces the autograd weight-gradient of every Conv2d / Linear above. */
int fr_conv_wgrad(const FrWgradArgs* args, int dtype, void* stream);

/* Weight gradient of 3x3 convolutions (bf16) with both operand strips resident in LDS; partial results per strip
 * group go to `slab`, a second launch adds them into dw (overwrites; deterministic, no atomics).  Stride 1 (GH == SH):
 * fr_conv_wgrad_strip_supported tells whether a shape is served (else use fr_conv_wgrad).  Stride 2 (SH == 2*GH,
 * GW in {56, 28, 14, 7}, channels multiples of 64): the input tile holds the four parity planes of the strip. */
int fr_conv_wgrad_strip(const FrWgradArgs* args, void* stream);
int fr_conv_wgrad_strip_supported(int Cout, int Cin, int W);
/* 1 when fr_conv_wgrad_strip serves these arguments (every served shape honours defer / prev_*).  fr_reduce_slabs: out[i] = sum over the slabs g = 0 .. groups-1
 * of slab[g*n + i] in the library's fixed order (chunks of 16 slabs, csrc/slab_sum.h; n % 4 == 0, groups <= 256): the
 * sum a deferring launch left to its caller. */
int fr_conv_wgrad_strip_defers(const FrWgradArgs* args);
/* Host queries on the family's instance table (select_wgrad, csrc/conv_wgrad_strip.hip): pure arithmetic, no HIP call.
 * fr_conv_wgrad_strip_groups: the strip groups (nsplit) for a launch that may use `wgs` workgroups -- the work items of
 * the shape's strip geometry, capped at wgs / dW tiles, at least 1; 0: the family does not serve the problem.  Ignores
 * args->nsplit and args->slab.  fr_conv_wgrad_strip_kernel: which kernel fr_conv_wgrad_strip would launch for exactly
 * these arguments (nsplit included) under the current switches, one of the ids below; FR_WGRAD_NONE also where the entry
 * rejects ldg / lda / slab / nsplit.  It does not look at prev_*, which do not choose the kernel. */
enum {
  FR_WGRAD_NONE = 0,      /* not served */
  FR_WGRAD_STRIP = 1,     /* conv_wgrad_strip_kernel, stride 1 */
  FR_WGRAD_STRIP_S2 = 2,  /* conv_wgrad_strip_kernel on the four parity planes, stride 2 */
  FR_WGRAD_ROLL = 3,      /* conv_wgrad_roll_kernel (warp-specialised; 7x7, 14x14, 28x28) */
  FR_WGRAD_VR = 4,        /* conv_wgrad_vr_kernel (warp-specialised; 56x56, 112x112) */
  FR_WGRAD_S2ROLL = 5     /* conv_wgrad_s2roll_kernel (warp-specialised, stride 2) */
};
int fr_conv_wgrad_strip_groups(const FrWgradArgs* args, int wgs);
int fr_conv_wgrad_strip_kernel(const FrWgradArgs* args);
int fr_reduce_slabs(const float* slab, int groups, long long n, float* out, void* stream);

/* ---- stem: NCHW fp32 images (+ optional constant avg image, restyle_psp.py:445-447) -> im2col rows
 * out[(b,h,w)][(kh*3+kw)*C + c] in the compute dtype, K padded with zeros to ldk (32 or 64).
 * Replaces the unfold half of input_layer Conv2d(3|6,64,3,1,1) (model_irse.py:140, restyle_psp.py:137). */
int fr_stem_im2col(const float* x, const float* avg, void* out, int B, int H, int W, int C, int Cavg, int ldk,
                   int dtype, void* stream);

/* The stem GEMMs over those rows (bf16, K = ldk = 32 or 64, 64 output channels), shaped for 3.2 M rows x 64 columns:
 * fr_stem_gemm : out[M][64] = X[M][K] * Wp[64][K]^T, part[nblocks][2][64] = column sums / sums of squares of out
 *                (the EPI_STATS contract of fr_conv_igemm with nblocks partial rows);
 * fr_stem_wgrad: slab[nblocks][64][K] = per-workgroup partial of g[M][64]^T * X[M][K] (add them with fr_reduce_parts,
 *                K = 1, C = 64*K).
 * Replace the GEMM half of input_layer Conv2d(3|6,64,3,1,1) (model_irse.py:140) forward and its weight gradient. */
int fr_stem_gemm(const void* X, const void* Wp, void* out, float* part, long long M, int K, int nblocks, void* stream);
/* Round 4: the stem forward as TWO passes over the rows instead of GEMM + a BN-apply pass over its 411-MB output:
 * fr_stem_gemm(out = NULL) leaves only the statistics of y = X * Wp^T (nothing stored), and after fr_bn_finalize
 * fr_stem_gemm_bn_prelu recomputes y, stores z = PReLU(BN(y)) -- fr_bn_apply(slope) on the rounded y, element for element -- and
 * y itself (y may be NULL when nothing reads it) and leaves the statistics of the rounded z in part (for the BatchNorm of the
 * first residual unit).  Replaces input_layer = Conv2d -> BatchNorm2d -> PReLU (backbone/model_irse.py:140-142). */
int fr_stem_gemm_bn_prelu(const void* X, const void* Wp, const float* scale, const float* shift, const float* slope, void* y,
                          void* z, float* part, long long M, int K, int nblocks, void* stream);
/* ... and its backward WITHOUT the stored y (y = NULL above: 411 MB less memory and traffic at batch 256): both kernels
 * recompute y = X * Wp^T from the rows, rounded as the forward pass rounded it.
 * fr_stem_bwd_sums  : part[nblocks][3][64] = the rows of fr_bn_bwd_reduce(slope) over (G, y) -- sum g', sum g'*xhat, sum g*u*[u<=0];
 * fr_stem_wgrad_bn_r: fr_stem_wgrad_bn with y recomputed per 64-row trip (bit-identical slabs).
 * Replace the autograd of Conv2d -> BatchNorm2d -> PReLU of input_layer (backbone/model_irse.py:140-142). */
int fr_stem_bwd_sums(const void* X, const void* Wp, const void* G, const float* mean, const float* invstd, const float* scale,
                     const float* shift, const float* slope, float* part, long long M, int K, int nblocks, void* stream);
int fr_stem_wgrad_bn_r(const void* G, const void* X, const void* Wp, const float* mean, const float* invstd,
                       const float* scale, const float* shift, const float* slope, const float* gamma, const float* s0,
                       const float* s1, float inv_count, float* slab, long long M, int K, int nblocks, void* stream);
int fr_stem_wgrad(const void* G, const void* X, float* slab, long long M, int K, int nblocks, void* stream);
/* As fr_stem_wgrad, with the backward of BatchNorm2d(64) -> PReLU(64) (model_irse.py:141-142) applied to the rows of G
 * while they are staged: G = gradient at the PReLU output, Y = BN input (the stem GEMM output), s0/s1 = the reduced
 * sums of fr_bn_bwd_reduce; equals fr_bn_bwd_apply followed by fr_stem_wgrad bit for bit without the 3-pass round trip. */
int fr_stem_wgrad_bn(const void* G, const void* Y, const void* X, const float* mean, const float* invstd,
                     const float* scale, const float* shift, const float* slope, const float* gamma, const float* s0,
                     const float* s1, float inv_count, float* slab, long long M, int K, int nblocks, void* stream);
/* The data gradient of the same stem, for gradients with respect to the input images: G = dL/dz0 [M][64] (M = B*H*W rows of
 * the im2col layout above, Ct = C + Cavg channels per tap), the BatchNorm / PReLU coefficients and s0 / s1 with the meaning
 * they have for fr_stem_wgrad_bn_r (s0 = s1 = 0 in eval mode) ->
 *   gx[b][c][h][w] = sum over (kh, kw) of (g_y * Wp)[(b, h-kh+1, w-kw+1)][(kh*3+kw)*Ct + c],  c < C only (the average-image
 *   channels get none), taps outside the image dropped; written, not accumulated; fp32 NCHW [B][C][H][W].
 * dtype FR_BF16: y = X * Wp^T recomputed from the rows (rounded as the forward pass rounded it) when Y is NULL, else read
 * from Y; dtype FR_F32: Y (the stored stem output) is required.  Deterministic (no atomics).
 * Replaces the autograd of input_layer = Conv2d -> BatchNorm2d -> PReLU (backbone/model_irse.py:140-142) with respect to
 * its input. */
int fr_stem_dgrad(const void* G, const void* X, const void* Y, const void* Wp, const float* mean, const float* invstd,
                  const float* scale, const float* shift, const float* slope, const float* gamma, const float* s0,
                  const float* s1, float inv_count, float* gx, int B, int H, int W, int C, int Ct, int K, int dtype,
                  void* stream);

/* ---- BatchNorm statistics (train mode; torch defaults eps 1e-5, momentum 0.1 -- SURVEY App. B 13)
 * part: [nparts][2][C] partial (sum, sum of squares) rows; count = elements per channel.
 * Writes mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; updates running stats (unbiased var)
 * and num_batches_tracked when those pointers are non-NULL.  Replaces nn.BatchNorm2d/1d statistics
 * (model_irse.py:57,60,141,144,148). */
int fr_bn_finalize(const float* part, int nparts, int C, double count, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var, int64_t* nbt,
                   float* mean, float* invstd, float* scale, float* shift, void* stream);

/* Statistics of a residual sum without a pass over it (round 4): part = [nparts][3][C] rows of a FR_EPI_STATS_X launch
 * (sum y, sum y^2, sum y*o over the conv2 output y and the unit's input o).  One launch finalises `bn` (the BatchNorm behind
 * conv2: exactly what fr_bn_finalize(part rows 0..1) writes; bn->count = elements per channel) AND `next`, the BatchNorm that
 * normalises the unit's output o' = scale*y + shift + o:  mean' = scale*my + shift + mo,  var' = scale^2*vy + vo +
 * 2*scale*cov(y, o), with (mo, vo) from in_mean / in_invstd / in_eps -- the statistics the unit's own BN1 used for o.
 * next == NULL: only `bn` is finalised (rows of three vectors; squeeze-excite units, whose output statistics need the
 * gates: fr_se_pool_parts_mlp_fwd_res).
 * Replaces the statistics pass behind `res + shortcut` of bottleneck_IR (backbone/model_irse.py:64-66) for identity units. */
int fr_bn_finalize_res(const float* part, int nparts, int C, const FrBnFinArgs* bn, const float* in_mean,
                       const float* in_invstd, float in_eps, const FrBnFinArgs* next, void* stream);

/* per-channel (sum, sumsq) partials of an NHWC tensor: part[blk][2][C], blk < nblocks (= grid size) */
int fr_channel_stats(const void* x, long long rows, int C, float* part, int nblocks, int dtype, void* stream);

/* out = [prelu]( x*scale+shift [* se[b][c]] ) [+ res]  with (sum,sumsq) partials of `out` for the next BN.
 *   res_kind 0 none | 1 identity shortcut x_in[b, h*stride, w*stride, c] (MaxPool2d(1,s), model_irse.py:53)
 *            | 2 BN'd conv shortcut: res*rscale+rshift (model_irse.py:55-56)
 * Replaces BN apply + PReLU of the stem (:141-142) and BN + SE excite + residual add of a unit (:60-66). */
typedef struct FrApplyArgs {
  const void* x;       /* [B*H*W][C] */
  void* out;           /* [B*H*W][C] */
  const float* scale;  /* [C] */
  const float* shift;  /* [C] */
  const float* slope;  /* PReLU [C] or NULL */
  const float* se;     /* [B][C] or NULL */
  const void* res;     /* residual source or NULL */
  const float* rscale; /* [C] for res_kind 2 */
  const float* rshift;
  float* part;         /* [nblocks][2][C] or NULL */
  int32_t B, H, W, C;
  int32_t res_kind, res_stride; /* identity: res has geometry [B, H*res_stride, W*res_stride, C] */
  int32_t nblocks;     /* grid size == number of partial rows */
} FrApplyArgs;
int fr_bn_apply(const FrApplyArgs* args, int dtype, void* stream);

/* ---- BatchNorm backward.  g' is the gradient at the BN output:
 *   g' = g                                    plain
 *      = g * prelu'(u),  u = x*scale+shift    slope != NULL  (stem: BN -> PReLU, model_irse.py:141-142)
 *      = g * se[b][c] + gse[b][c]             se != NULL     (IR-SE: BN -> SE excite, model_irse.py:86-87)
 * fr_bn_bwd_reduce: part[blk][3][C]: k=0 sum g', k=1 sum g'*xhat, k=2 sum g*u*[u<=0] (PReLU slope gradient)
 * fr_bn_bwd_apply : gx = gamma*invstd*(g' - s0/n - xhat*s1/n) [+ add]
 *   add_kind 0 none | 1 tensor of the same geometry (conv-shortcut data gradient)
 *            | 2 identity shortcut MaxPool2d(1,s): add[b, h/s, w/s, c] where h%s==0 and w%s==0 */
typedef struct FrBnBwdArgs {
  const void* g;       /* upstream gradient [rows][C] */
  const void* x;       /* BN input [rows][C] */
  void* gx;            /* apply: output gradient [rows][C] */
  const float* mean;
  const float* invstd;
  const float* scale;  /* gamma*invstd, shift: only read when slope != NULL */
  const float* shift;
  const float* slope;
  const float* se;     /* [B][C] */
  const float* gse;    /* [B][C] gradient wrt the pooled BN output, already divided by H*W */
  const float* gamma;  /* apply */
  const float* s0;     /* apply: reduced sums [C] */
  const float* s1;
  const void* add;     /* apply */
  float* part;         /* reduce: [nblocks][3][C] */
  long long rows;
  float inv_count;     /* 1 / rows */
  int32_t C;
  int32_t rows_per_image; /* H*W (se indexing, identity scatter) */
  int32_t add_kind;
  int32_t H, W, add_stride; /* geometry of gx for add_kind 2 */
  int32_t nblocks;
  /* fr_bn_bwd_apply, round 6 (ABI v6), nx != NULL: the launch ALSO leaves the rows of fr_bn_bwd_reduce for the BatchNorm whose
   * output gradient it has just formed -- part rows npart[nblocks][2][C] = (sum gx, sum gx * xhat_n) over this workgroup's rows,
   * xhat_n = (nx - nmean) * ninvstd, gx as rounded and stored: on tensors that only stream through HBM (56x56 x 64 channels at
   * batch 256: 103 MB) the separate reduce pass re-read gx right behind this one.  bf16, no gate; fr_reduce_parts(npart,
   * nblocks, 2, C, ...) adds the rows. */
  const void* nx;
  const float* nmean;
  const float* ninvstd;
  float* npart;
} FrBnBwdArgs;
int fr_bn_bwd_reduce(const FrBnBwdArgs* args, int dtype, void* stream);
int fr_bn_bwd_apply(const FrBnBwdArgs* args, int dtype, void* stream);

/* Round 6 (ABI v6): the sums of fr_stem_bwd_sums when G is the LAST tensor the first residual unit would write -- gx of its BN1 backward
 * (bottleneck_IR: BatchNorm2d(in_channel) at the head of res_layer, backbone/model_irse.py:57, + the shortcut gradient of
 * MaxPool2d(1, stride) / the residual stream, :52-54, :64-66).  `unit` holds exactly the arguments of the fr_bn_bwd_apply
 * call this replaces (g, x, gx, mean, invstd, gamma, s0, s1, inv_count, add, add_kind 0 | 1 | 2, H, W, add_stride = 2,
 * rows_per_image; C = 64, rows = M; no slope, no gate): the kernel forms gx element for element as that call does, stores it
 * (the weight-gradient kernel reads it next) and feeds the rounded values to the sums -- gx and part are bit-identical to
 * fr_bn_bwd_apply followed by fr_stem_bwd_sums, and the 411-MB tensor (batch 256) is read once less.  unit->x == NULL: the
 * unit's input IS the stem's output z = PReLU(BN(X Wp^T)) of this step (fr_stem_gemm_bn_prelu with the same X, Wp, scale, shift,
 * slope): it is recomputed from the y tile the sums need anyway, bit for bit, instead of read (another 411 MB less). */
int fr_stem_bwd_sums_from(const FrBnBwdArgs* unit, const void* X, const void* Wp, const float* mean, const float* invstd,
                          const float* scale, const float* shift, const float* slope, float* part, long long M, int K,
                          int nblocks, void* stream);

/* add partial rows in double: o_k[c] = sum_blk part[blk][k][c], k < K <= 3; NULL outputs are skipped.
 * Used for d gamma (k=1), d beta (k=0), d PReLU slope (k=2) and for the conv-epilogue partials. */
int fr_reduce_parts(const float* part, int nparts, int K, int C, float* o0, float* o1, float* o2, void* stream);

/* eval-mode BatchNorm coefficients from the running statistics */
int fr_bn_eval_coeffs(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                      float eps, int C, float* mean, float* invstd, float* scale, float* shift, void* stream);
/* the same for every BatchNorm of a network in one launch (inference: util/utils.py:254-307 evaluates the backbone in
 * eval mode once per epoch on ~50 k images; 53 separate coefficient launches per forward were most of its launches) */
typedef struct FrBnEvalEntry {
  const float* rm;
  const float* rv;
  const float* gamma;
  const float* beta;
  float* mean;
  float* invstd;
  float* scale;
  float* shift;
  int32_t C;
  float eps;
} FrBnEvalEntry;
int fr_bn_eval_coeffs_multi(const FrBnEvalEntry* table_dev, int n, void* stream);

/* ---- SE block (model_irse.py:23-46 / restyle_psp_helpers.py:67-83) */
/* pooled[b][c] = mean_hw (x*scale+shift)  */
int fr_se_pool(const void* x, const float* scale, const float* shift, float* pooled, int B, int HW, int C,
               int dtype, void* stream);
/* the same from the per-strip column sums of a strip convolution's STATS epilogue (part[strip][2][C], the strips of
 * image b at rows b*rows_per_image ..): pooled[b][c] = scale[c] * (sum of those rows' [0][c]) / HW + shift[c] */
int fr_se_pool_parts(const float* part, int rows_per_image, const float* scale, const float* shift, float* pooled,
                     int B, int HW, int C, void* stream);
/* s = sigmoid(W2 relu(W1 pooled)); W1 [R][C], W2 [C][R]; saves hidden [B][R] */
int fr_se_mlp_fwd(const float* pooled, const float* w1, const float* w2, float* hidden, float* s, int B, int C,
                  int R, void* stream);
/* fr_se_pool_parts followed by fr_se_mlp_fwd in one launch (same arithmetic, same order; pooled [B][C] is written for the
 * weight gradient): the squeeze-excite branch of bottleneck_IR_SE (model_irse.py:23-46) behind a strip convolution */
int fr_se_pool_parts_mlp_fwd(const float* part, int rows_per_image, const float* scale, const float* shift,
                             const float* w1, const float* w2, float* pooled, float* hidden, float* s, int B, int HW,
                             int C, int R, void* stream);
/* fr_se_pool_parts_mlp_fwd on rows of `nv` vectors (3: FR_EPI_STATS_X rows -- sum y, sum y^2, sum y*x per strip) that also
 * derives, per IMAGE, the moments of the unit's output  o = (scale*y + shift)*s[b][c] + x  without a pass over it:
 *   om[b][0][c] = sum_hw o = s*(scale*Sy + shift*HW) + Sx
 *   om[b][1][c] = sum_hw o^2 = s^2*(scale^2*Syy + 2*scale*shift*Sy + shift^2*HW) + 2*s*(scale*Syx + shift*Sx) + Sxx
 * with (Sx, Sxx) = xm[b][0..1][c], the same per-image moments of the unit's INPUT (the om of the unit in front, or
 * fr_image_moments at the head of a chain).  fr_bn_finalize(om, B, C, B*HW, ..) then gives the next unit's BN1.
 * Replaces the statistics pass behind `res + shortcut` of bottleneck_IR_SE (backbone/model_irse.py:84-91). */
int fr_se_pool_parts_mlp_fwd_res(const float* part, int rows_per_image, int nv, const float* scale, const float* shift,
                                 const float* w1, const float* w2, float* pooled, float* hidden, float* s, int B, int HW,
                                 int C, int R, const float* xm, float* om, void* stream);
/* out[b][0][c] = sum_hw x, out[b][1][c] = sum_hw x^2 of an NHWC bf16 tensor [B][HW][C] (C / 8 a divisor of 256) */
int fr_image_moments(const void* x, int B, int HW, int C, float* out, void* stream);
/* gs[b][c] = sum_hw g * (x*scale+shift)  (gradient wrt the excite scale) */
int fr_se_gscale(const void* g, const void* x, const float* scale, const float* shift, float* gs, int B, int HW,
                 int C, int dtype, void* stream);
/* backward of the MLP: gpooled [B][C] (already divided by HW); dW1 [R][C], dW2 [C][R] OVERWRITTEN with the sums over
 * the batch in image order (reproducible, no atomics); gz [B][C], gh [B][R]: scratch the two launches hand over */
int fr_se_mlp_bwd(const float* gs, const float* s, const float* hidden, const float* pooled, const float* w1,
                  const float* w2, float* gpooled, float* dw1, float* dw2, float* gz, float* gh, int B, int C, int R,
                  int HW, void* stream);
/* fr_se_gscale followed by fr_se_mlp_bwd: the backward of the squeeze-excite branch of bottleneck_IR_SE (model_irse.py:23-46);
 * g = gradient at the unit output branch, x = y2.  gs_part == NULL: one 1024-thread workgroup per image, gs stays in LDS (same
 * arithmetic and order as the two calls).  gs_part != NULL (round 5; scratch [B][fr_se_gscale_slices(B, HW)][C] floats): the
 * squeeze runs over row slices of an image in 256-thread workgroups (B x slices of them: every CU has work at batch 128, and
 * they fit beside resident weight-gradient workgroups), the slices are added in order in front of the MLP part. */
int fr_se_gscale_mlp_bwd(const void* g, const void* x, const float* scale, const float* shift, const float* s,
                         const float* hidden, const float* pooled, const float* w1, const float* w2, float* gpooled,
                         float* dw1, float* dw2, float* gz, float* gh, float* gs_part, int B, int C, int R, int HW, int dtype,
                         void* stream);
/* Round 6 (ABI v6): dw1 = dw2 = NULL in fr_se_gscale_mlp_bwd leaves out its last launch, the weight gradients of the two
 * 1x1 convolutions of SEModule (fc1 / fc2, backbone/model_irse.py:28-35) -- sums over the batch in image order that feed
 * nothing downstream in the backward pass -- and fr_se_mlp_wgrad is that launch on its own, so that the caller can put it on
 * the weight-gradient stream (6-13 us per squeeze-excite unit off the main stream's chain).  gz [B][C], gh [B][R]: what
 * fr_se_gscale_mlp_bwd left; dw1 [R][C], dw2 [C][R] OVERWRITTEN. */
int fr_se_mlp_wgrad(const float* gz, const float* gh, const float* hidden, const float* pooled, float* dw1, float* dw2, int B,
                    int C, int R, void* stream);
/* Round 6 (ABI v6): fr_se_gscale_mlp_bwd (sliced squeeze, no weight-gradient launch) that ALSO leaves the rows of BN2's
 * backward sums, so that the fr_bn_bwd_reduce(se, gse) pass behind it -- a third read of (g, x) -- is not needed: behind the
 * excite gate BatchNorm2d(depth) of res_layer (backbone/model_irse.py:76-80, 86-87) sees g' = g * s[b][c] + gse[b][c], constant
 * over an image, so sum g' and sum g' * xhat follow from per-image sums of g, g * xhat and xhat taken in the squeeze pass:
 *   bn_part[b][0][c] = s * sum g + HW * gse,   bn_part[b][1][c] = s * sum g * xhat + gse * sum xhat   (xhat = (x - mean) * invstd)
 * fr_reduce_parts(bn_part, B, 2, C, dbeta, dgamma) adds the images.  gs_part: scratch [B][fr_se_gscale_slices(B, HW)][4][C]. */
int fr_se_gscale_mlp_bwd_sums(const void* g, const void* x, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* s, const float* hidden, const float* w1, const float* w2,
                              float* gpooled, float* gz, float* gh, float* gs_part, float* bn_part, int B, int C, int R, int HW,
                              int dtype, void* stream);
int fr_se_gscale_slices(int B, int HW);

/* ---- output layer pieces (model_irse.py:144-148) */
/* a[b][(h*7+w)*C + c] = dropout(x*scale+shift): mask from a counter hash of (seed, element index in the
 * reference's C-major flatten order), keep prob 1-p, scaled 1/(1-p); p = 0 disables. */
int fr_bn_dropout(const void* x, void* out, const float* scale, const float* shift, long long rows, int C, int HW,
                  float p, uint64_t seed, int dtype, void* stream);
int fr_dropout_bwd(void* g, long long rows, int C, int HW, float p, uint64_t seed, int dtype, void* stream);

/* The same pair with the Linear layer's activation in the reference's own Flatten order (round 4):
 *   fr_bn_dropout_cm : out[b][c*HW + hw] = dropout(x[b][hw][c]*scale[c] + shift[c])     (x NHWC, out = Flatten of NCHW)
 *   fr_dropout_bwd_cm: out[b][hw][c] = mask * g_cm[b][c*HW + hw] / (1 - p)              (out of place, back to NHWC)
 * same counter-hash mask as above.  C % 64 == 0.  With it Linear(512*7*7, 512) (model_irse.py:146-147) runs on the fp32
 * master weight in its own layout: */
int fr_bn_dropout_cm(const void* x, void* out, const float* scale, const float* shift, int B, int C, int HW, float p,
                     uint64_t seed, int dtype, void* stream);
int fr_dropout_bwd_cm(const void* g_cm, void* out, int B, int C, int HW, float p, uint64_t seed, int dtype, void* stream);
/* Linear(K, O) as weight-streaming GEMMs on the fp32 master W [O][K] (csrc/linear_gemm.hip; bf16 activations, the weight
 * rounded to bf16 in registers, fp32 accumulation):
 *   fr_linear_fwd  : slab[s][b][o] = sum_{k in K-slice s} a[b][k]*W[o][k] (+ bias[o] in slice 0), s < slices; add the slabs
 *                    with fr_reduce_parts(slab, slices, 1, B*O, out, ..) -- a fixed order, reproducible.  fr_linear_slices
 *                    returns the slice count the library recommends for (O, K) (0: shape not served); O % 64 == 0, K % 32 == 0
 *   fr_linear_dgrad: ga[b][k] = sum_o g[b][o]*W[o][k], ga in the compute dtype; O % 128 == 0, K % 128 == 0
 * The weight gradient dW[o][k] = sum_b g[b][o] a[b][k] is fr_conv_wgrad (taps = 1) on the same a.
 * Replace nn.Linear(512*7*7, 512) of output_layer (backbone/model_irse.py:147) forward and its autograd data gradient. */
int fr_linear_slices(int O, int K);
int fr_linear_fwd(const void* a, const float* W, const float* bias, float* slab, int B, int O, int K, int slices,
                  void* stream);
int fr_linear_dgrad(const void* g, const float* W, void* ga, int B, int O, int K, void* stream);

/* ---- weight packing: fp32 master [Cout][taps][Cin] (channels-last storage of the OIHW Parameter)
 *   wp [Cout][taps][Cin] compute dtype (NULL to skip), wt [Cin][taps][Cout] compute dtype (NULL to skip) */
int fr_pack_weight(const float* w, void* wp, void* wt, int Cout, int taps, int Cin, int dtype, void* stream);
/* the same for every convolution of the network in one launch: table_dev = device array of records, chunks_dev =
 * device array of (tensor index, tile index) pairs, tile index over taps x ceil(Cout/32) x ceil(Cin/32); bf16 tensors with
 * Cout % 64 == 0 and Cin % 64 == 0 may use 64 x 64 tiles instead (16-byte accesses): tile index -(1 + index over taps x
 * Cout/64 x Cin/64); one tensor's chunks are all of one kind */
typedef struct FrPackTensor {
  const float* w;
  void* wp; /* may be NULL */
  void* wt; /* may be NULL */
  int32_t Cout, taps, Cin;
  int32_t frag; /* ABI v7, bit 0: wp in MFMA-fragment order (FrConvArgs.w_frag; N = Cout, K = Cin), bit 1: wt (N = Cin, K = Cout);
                   bf16, Cout % 64 == 0 and Cin % 64 == 0 (the 64 x 64 tile chunks) */
  const float* oscale; /* [Cout] or NULL: wp = w * oscale[co] (BatchNorm scale folded into the output channels) */
} FrPackTensor;
int fr_pack_weights_multi(const FrPackTensor* table_dev, const int32_t* chunks_dev, int nchunks, int dtype,
                          void* stream);
/* Linear(25088,512): torch layout [O][C*HW] (c-major) <-> NHWC-flatten [O][HW*C]; dir 0: torch->packed
 * (dtype out, optional transposed copy wt [HW*C][O]), dir 1: packed fp32 grad -> torch fp32 grad */
int fr_permute_linear(const float* in, void* out, void* wt, int O, int C, int HW, int dir, int dtype,
                      void* stream);
/* stem weight: torch [64][C][3][3] fp32 (any strides given) <-> packed [64][ldk] with k=(kh*3+kw)*C+c */
int fr_pack_stem(const float* w, long long s_o, long long s_c, long long s_h, long long s_w, void* wp, int Cout,
                 int C, int ldk, int dtype, void* stream);
int fr_unpack_stem_grad(const float* gp, float* gw, long long s_o, long long s_c, long long s_h, long long s_w,
                        int Cout, int C, int ldk, void* stream);
/* generic cast fp32 -> compute dtype (n elements) and back */
int fr_cast(const void* in, void* out, long long n, int dtype_in, int dtype_out, void* stream);

/* ---- margin head (head/metrics.py:97-140 ArcFace, :164-191 CosFace) */
/* row L2 normalise (F.normalize, eps 1e-12): xn [rows][ldn] compute dtype (rows..rows_pad zero filled),
 * optional transposed copy xt [D][ldt], inv [rows] = 1/max(||x||,eps) */
int fr_row_normalize(const float* x, void* xn, void* xt, float* inv, int rows, int rows_pad, int D, int ldt,
                     int dtype, void* stream);
/* gcos[m][n] = scale * g[m][n] * (n==label[m] ? dphi(cos_t[m]) : 1), zero padded to ldg columns */
int fr_margin_bwd(const float* g, const int64_t* label, const float* cos_t, void* gcos, int rows, int N, int ldg,
                  int kind, int easy, float cos_m, float sin_m, float th, float scale, int dtype, void* stream);
/* backward through F.normalize: gx = (G - xhat*(xhat.G)) * inv, xhat = x*inv, rows of D */
int fr_normalize_bwd(const float* G, const float* x, const float* inv, float* gx, int rows, int D, void* stream);

/* ---- SphereFace / Am_softmax heads (head/metrics.py:200-277, :280-333), fp32.  The cosines come raw from fr_conv_igemm
 *      (FR_EPI_STORE, out_f32) in [rows][ld] (ld a multiple of 4 >= N); the margin is applied by these row kernels, and the
 *      backward pass reads the same raw cosines for its clamp mask.  kind 2 = SphereFace, 3 = Am_softmax; any other kind
 *      returns FR_UNSUPPORTED.  c = clamp(cos, -1, 1) (NaN passes), lab = label[m]:
 *   kind 2 (:236-268): out = ||x_m|| * (n == lab ? (phi - c) / p0 + c : c), phi = (-1)^k T_mi(c) - 2k,
 *                      k = floor(mi * acos(c) / 3.14159265) in fp32, T_mi the Chebyshev polynomial of mlambda (:227-234),
 *                      mi in 0..5, p0 = 1 + lambda, ||x_m|| = 1 / inv_x[m] of fr_row_normalize
 *   kind 3 (:310-331): out = p1 * (n == lab ? c - p0 : c), p0 = m, p1 = s (inv_x unused)
 * Columns N..ld of out are written as 0. */
int fr_margin_apply(const float* cos, const int64_t* label, const float* inv_x, float* out, int rows, int N, int ld,
                    int kind, int mi, float p0, float p1, void* stream);
/* gcos[m][n] = g[m][n] * d out / d cos, 0 where the clamp saturated (the closed interval passes, as torch.clamp does) and
 * in the padding columns N..ldg (the layout of fr_margin_bwd).  g is [rows][N] contiguous.  kind 2 also writes
 * r_part[m][p] = sum over the p-th column chunk of g * out / ||x_m||, p < fr_margin_apply_parts(ldg) (NULL for kind 3). */
int fr_margin_apply_bwd(const float* g, const float* cos, const int64_t* label, const float* inv_x, float* gcos,
                        float* r_part, int rows, int N, int ld, int ldg, int kind, int mi, float p0, float p1, void* stream);
/* number of column chunks of fr_margin_apply_bwd: r_part has [rows][fr_margin_apply_parts(ldg)] entries */
int fr_margin_apply_parts(int ldg);
/* fr_normalize_bwd plus the radial term of SphereFace's row scale ||x|| (torch.norm(input, 2, 1), :255,268):
 * gx = (G - xhat*(xhat.G)) * inv + r * xhat, r = r_part[m][0] + ... + r_part[m][nparts-1] in that order */
int fr_normalize_bwd_radial(const float* G, const float* x, const float* inv, const float* r_part, int nparts, float* gx,
                            int rows, int D, void* stream);
/* Am_softmax's l2_norm(kernel, axis=0) (:280-284, no eps: a zero column gives inf / NaN as in the reference) of
 * K [D][N]: kt [D][Np] = K / ||K[:, j]|| (columns N..Np zero), kn [Np][D] = kt^T (the GEMM's B operand, rows N..Np zero),
 * inv [N] = 1 / ||K[:, j]|| */
int fr_col_normalize(const float* K, float* kn, float* kt, float* inv, int D, int N, int Np, void* stream);
/* backward of fr_col_normalize: gK[d][j] = (GW[j][d] - kn[j][d] * (kn[j].GW[j])) * inv[j], GW [>= N][D] (the weight
 * gradient GEMM's rows), gK in K's [D][N] layout */
int fr_col_normalize_bwd(const float* GW, const float* kn, const float* inv, float* gK, int D, int N, void* stream);

/* ---- CurricularFace (head/metrics.py:475-510) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_col_normalize'd [D][N] kernel; c = clamp(cos, -1, 1) (NaN passes).
 *      t is a one-float DEVICE buffer (the module's EMA buffer): no entry point reads it on the host. */
/* per-row values (:497-502), rowv [4][rows]: tl = c[label], ctm = tl*cos_m - sqrt(1 - tl^2)*sin_m,
 * final = tl > th ? ctm : tl - mm, flag = tl > th (1.0 / 0.0).  A label outside [0, N) has no target: tl = 0.
 * mean[0] = the batch mean of tl, added in a fixed order in double by one workgroup (bit-reproducible).  train = 1 also
 * updates t[0] <- 0.01*mean + 0.99*t[0] (:505-506; the reference does so on every forward call); train = 0 leaves t alone,
 * for a caller that averages mean over the ranks first and then calls fr_curricular_ema. */
int fr_curricular_rows(const float* cos, const int64_t* label, float* rowv, float* mean, float* t, int rows, int N, int ld,
                       float cos_m, float sin_m, float th, float mm, int train, void* stream);
/* fr_curricular_rows from given target cosines tl [rows] (:497-506 after the gather of :496): the same rowv, mean and
 * update of t, bit for bit, for the same tl.  The class-sharded head passes the target cosines of the GLOBAL batch
 * (fr_shard_target_cos summed over the ranks), so every rank holds the rowv and t of one head over that batch. */
int fr_curricular_rows_from(const float* tl, float* rowv, float* mean, float* t, int rows, float cos_m, float sin_m,
                            float th, float mm, int train, void* stream);
/* t[0] <- 0.01*(scale*mean[0]) + 0.99*t[0]: the update above from a mean summed over `1 / scale` ranks */
int fr_curricular_ema(float* t, const float* mean, float scale, void* stream);
/* out[m][n] = s * (n == label[m] ? final[m] : (c > ctm[m] ? c*(t + c) : c))  (:501-509); ld a multiple of 4, columns N..ld of
 * out are written as 0.  A label outside [0, N) selects nothing. */
int fr_curricular_apply(const float* cos, const int64_t* label, const float* rowv, const float* t, float* out, int rows,
                        int N, int ld, float s, void* stream);
/* gcos[m][n] = g[m][n] * d out / d cos with t, the hard mask and the branch flag constant: s*(t + 2c) on hard negatives, s on
 * easy ones, on the label column s*(cos_m + sin_m*tl/sqrt(1 - tl^2)) where flag is set and s where it is not; 0 where the
 * clamp saturated (the closed interval passes) and in the padding columns N..ldg.  g is [rows][N] contiguous. */
int fr_curricular_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, const float* t, float* gcos,
                      int rows, int N, int ld, int ldg, float cos_m, float sin_m, float s, void* stream);

/* ---- MagFace (head/metrics.py:512-553) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_col_normalize'd [D][N] weight; c = clamp(cos, -1, 1) (NaN passes). */
/* per-row values (:533-536, :545), rowv [6][rows], from the embeddings' norms ||x_m||, RECOMPUTED from x [rows][D] (summed
 * in double in a fixed order, then rounded; not 1 / inv_x of fr_row_normalize, whose two reciprocals would cost the
 * difference 1/u_a^2 - 1/a^2 of the backward pass three digits near u_a):  a = clamp(||x||, l_a, u_a);  cos_m = cos(m(a)), sin_m = sin(m(a)) with
 * m(a) = (u_margin - l_margin) / (u_a - l_a) * (a - l_a) + l_margin;  min_cos = cos(pi - m(a));
 * loss_g = lamda * (a / u_a^2 + 1 / a);  inside = 1.0 if l_a <= ||x|| <= u_a else 0.0 (the mask of torch.clamp's
 * backward).  0 < l_a < u_a. */
int fr_magface_rows(const float* x, float* rowv, int rows, int D, float l_a, float u_a, float l_margin, float u_margin,
                    float lamda, void* stream);
/* out[m][n] = s * (n == label[m] ? (c > min_cos[m] ? c*cos_m[m] - sqrt(1 - c^2)*sin_m[m] : c - margin_am) : c)  (:540-552);
 * ld a multiple of 4, columns N..ld of out are written as 0.  A label outside [0, N) selects nothing. */
int fr_magface_apply(const float* cos, const int64_t* label, const float* rowv, float* out, int rows, int N, int ld, float s,
                     float margin_am, void* stream);
/* backward of :533-552.  g is [rows][N] contiguous, glossg [rows] the upstream gradient of loss_g (NULL: zeros).
 * gcos[m][n] = g[m][n] * d out / d cos: s off the label column, s*(cos_m + sin_m*c/sqrt(1 - c^2)) on it in the margin branch
 * (c > min_cos) and s in the other; 0 where the clamp saturated (the closed interval passes) and in the padding columns
 * N..ldg.  r[m] = d loss / d ||x_m|| = inside[m] * (g[m][label]*s*(-(sqrt(1 - c^2)*cos_m + c*sin_m))*(u_margin - l_margin)
 * / (u_a - l_a) [margin branch only; 0 where the label selects nothing] + glossg[m]*lamda*(1/u_a^2 - 1/a^2)): one writer per
 * row, no sum; it goes through fr_normalize_bwd_radial with nparts = 1. */
int fr_magface_bwd(const float* g, const float* glossg, const float* cos, const int64_t* label, const float* rowv,
                   float* gcos, float* r, int rows, int N, int ld, int ldg, float s, float l_a, float u_a, float l_margin,
                   float u_margin, float lamda, void* stream);

/* ---- AdaCos (head/metrics.py:336-369) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_row_normalize'd [N][D] weight.  scale is the head's one-float device buffer:
 *      read by fr_adacos_rows, moved by fr_adacos_scale (its only writer), read by fr_adacos_apply; never by the host. */
/* per-row values (:363, :366), rowv [2][rows]:  rowv[0][m] = sum over n < N, n != label[m] of expf(scale[0] * cos[m][n]), the
 * raw cosine without a clamp, added in a fixed order (per-thread sums in double over ascending columns, the wave's xor
 * butterfly, the sixteen waves of the row's workgroup in order);  rowv[1][m] = cos[m][label[m]], the raw target cosine.
 * A row whose label lies outside [0, N) has no target: all N columns enter its sum and rowv[1][m] is the marker 2.0f.
 * ld a multiple of 4. */
int fr_adacos_rows(const float* cos, const int64_t* label, const float* scale, float* rowv, int rows, int N, int ld,
                   void* stream);
/* scale[0] <- log(B_avg) / cos(min(pi/4, theta_med))  (:364-367), one workgroup, one writer:  B_avg = sum(rowv[0]) / rows,
 * added in double in a fixed order;  theta_med = torch.median of acos(clamp(rowv[1], -1 + 1e-7, 1 - 1e-7)) over the rows
 * that have a target, i.e. the LOWER median, the angle of the cosine at descending rank (n - 1) / 2 (ties by row index).
 * Any rows >= 0 (a rank-counting select through fixed-size LDS tiles: rows^2 / 256 compares per thread); rowv may be the
 * all-gathered rows of every rank.  rows == 0, or no row with a target: scale is left as it is.  A NaN target cosine
 * makes it NaN. */
int fr_adacos_scale(const float* rowv, int rows, float* scale, void* stream);
/* out[m][n] = scale[0] * src[m][n] for n < N and 0 for N <= n < ld_out; src has the pitch ld_src >= N, out the pitch
 * ld_out >= N, a multiple of 4.  Forward (:368): src = the raw cosines (pitch ld), out = the logits store (pitch ld): the
 * NEW scale times the unclamped cosine.  Backward: src = g [rows][N] contiguous, out = gcos (pitch Np), the scale this
 * forward call used: it is a constant of the graph (:362 no_grad), so d out / d cos = scale everywhere. */
int fr_adacos_apply(const float* src, const float* scale, float* out, int rows, int N, int ld_src, int ld_out, void* stream);

/* ---- NPCFace (head/metrics.py:592-636) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_col_normalize'd kernel.  The head has no state besides its kernel. */
/* per-row values (:616-632), rowv [6][rows]:  gt = clamp(cos[m][label[m]], -1, 1);  ctm = gt*cos_m - sqrt(1 - gt^2)*sin_m;
 * final = gt > 0 ? gt*cos(newm) - sqrt(1 - gt^2)*sin(newm) : gt with newm = m0 + m1*avg;  d final / d gt =
 * cos(newm) + sin(newm)*gt/sqrt(1 - gt^2) where gt > 0, else 1;  avg = (sum of the clamped cosines c[m][n] > ctm over
 * n < N, n != label[m]) / max(count, 1);  count = the number of those columns, as a float (exact up to 2^24).  The sum is
 * added in a fixed order (per-thread sums in double over ascending columns, the wave's xor butterfly, the sixteen waves of
 * the row's workgroup in order), no atomics.  A row whose label lies outside [0, N) has no target: gt = 0, ctm = +inf, so
 * count = 0 and nothing in it is hard.  ld a multiple of 4. */
int fr_npcface_rows(const float* cos, const int64_t* label, float* rowv, int rows, int N, int ld, float cos_m, float sin_m,
                    float m0, float m1, void* stream);
/* out[m][n] = s * (n == label[m] ? final[m] : (c > ctm[m] ? t*c + a : c)), c the clamped cosine  (:632-635); ld a multiple
 * of 4, columns N..ld of out are written as 0.  A label outside [0, N) selects nothing. */
int fr_npcface_apply(const float* cos, const int64_t* label, const float* rowv, float* out, int rows, int N, int ld, float t,
                     float a, float s, void* stream);
/* gcos[m][n] = g[m][n] * d out / d cos with newm, the hard mask and the branch constant (:621 no_grad): s*t on hard
 * negatives, s on easy ones, s * (d final / d gt)[m] on the label column; 0 where the clamp saturated (the closed interval
 * passes) and in the padding columns N..ldg.  g is [rows][N] contiguous. */
int fr_npcface_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos, int rows, int N,
                   int ld, int ldg, float t, float s, void* stream);

/* ---- MV_Softmax (head/metrics.py:555-590) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_col_normalize'd weight.  The head never clamps its cosines (a raw cosine of
 *      1 + 2^-23 keeps its value and its gradient) and has no state besides its weight. */
/* replaces :576-589.  Per row (every wave derives them from one load of the target cosine; the wave of column chunk 0
 * stores them), rowv [4][rows]:  gt = cos[m][label[m]];  is_am != 0 (:578-579, p0 = margin, p1 unused): thr = gt - p0,
 * final = gt > p0 ? gt - p0 : gt, d final / d gt = 1;  is_am == 0 (:581-584, p0 = cos_m, p1 = sin_m): thr = gt*p0 -
 * sqrt(1 - gt^2)*p1, final = gt > 0 ? thr : gt, d final / d gt = gt > 0 ? p0 + p1*gt/sqrt(1 - gt^2) : 1, unguarded: |gt| > 1
 * makes thr NaN and no column of the row hard.  out[m][n] = s * (n == label[m] ? final[m] : (c > thr[m] ? w*c + w - 1 : c))
 * with c the raw cosine (:586-589); ld a multiple of 4, columns N..ld of out are written as 0.  A row whose label lies
 * outside [0, N) has no target: rowv = 0, +inf, 0, 0, nothing in it is hard and no column is selected. */
int fr_mv_softmax_apply(const float* cos, const int64_t* label, float* rowv, float* out, int rows, int N, int ld, int is_am,
                        float p0, float p1, float w, float s, void* stream);
/* the backward of :576-589 with the hard mask and the branch constant (comparisons take no gradient): gcos[m][n] = g[m][n] *
 * (s*w on hard negatives, s on easy ones, s * (d final / d gt)[m] on the label column), whatever the raw cosine (no clamp,
 * no pass mask); 0 in the padding columns N..ldg.  g is [rows][N] contiguous, rowv as fr_mv_softmax_apply left it. */
int fr_mv_softmax_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos, int rows, int N,
                      int ld, int ldg, float w, float s, void* stream);

/* ---- CircleLoss (head/metrics.py:435-473), the classification form, on the raw cosines cos [rows][ld] of the FR_EPI_STORE
 *      GEMM between fr_row_normalize'd embeddings and the fr_col_normalize'd weight.  Element-wise after the clamp: no row
 *      values, no state besides the weight.  (The FaceX-Zoo AM_Softmax, :371-392, needs no entry of its own: it is
 *      fr_margin_apply / fr_margin_apply_bwd with kind 3 on the cosines of normalised embeddings.) */
/* replaces :455-472.  c = clamp(cos, -1, 1);  out[m][n] = gamma * (n == label[m] ? max(o_p - c, 0) * (c - delta_p)
 * : max(c - o_n, 0) * (c - delta_n)), every operation rounded to fp32 on its own and in this order, so out has the bits of
 * the reference's fp32 expression on the same cosines; the clamps are comparisons: NaN passes (torch.clamp, torch.clamp_min).
 * A negative with c <= o_n comes out as 0.  ld a multiple of 4, columns N..ld of out are written as 0.  A row whose label
 * lies outside [0, N) has no label column: all its columns are negatives. */
int fr_circle_apply(const float* cos, const int64_t* label, float* out, int rows, int N, int ld, float o_p, float o_n,
                    float delta_p, float delta_n, float gamma, void* stream);
/* the backward of :455-472 with alpha detached (:463-464): gcos[m][n] = (g[m][n] * gamma) * alpha, alpha = max(o_p - c, 0)
 * on the label column and max(c - o_n, 0) off it, recomputed from the raw cosine, where -1 <= cos[m][n] <= 1 (torch.clamp
 * passes gradient on the closed interval), else 0 (a NaN cosine too); 0 in the padding columns N..ldg.  g is [rows][N]
 * contiguous. */
int fr_circle_bwd(const float* g, const float* cos, const int64_t* label, float* gcos, int rows, int N, int ld, int ldg,
                  float o_p, float o_n, float gamma, void* stream);

/* ---- SST_Prototype (head/metrics.py:638-708, "Semi-Siamese Training for Shallow Face Learning").  The head has no weight:
 *      its class matrix is a queue of gallery embeddings, kept on the device in both GEMM layouts, q [D][Q] (the reference's
 *      buffer `queue`, the data gradient's operand) and qt [Q][D] (the cosine GEMM's operand), already normalised.  A call
 *      works on rows = B or 2 B probe rows (the two views stacked); row m has the label index + m % B and belongs to block
 *      blk = m / B.  The cosines come from two FR_EPI_STORE GEMMs: cos [rows][ld] against the whole of qt, whose window
 *      columns [index, index + B) are don't-care, and cw [rows][ldw] against the stacked gallery rows [g2n; g1n] that stand in
 *      the window: row m reads cw[m][blk * B + j] for the window column index + j (rows = B: the compact block cw[m][j]). */
/* replaces update_queue, :675-680, without its host reads.  gn [B][D]: the chosen gallery view, rows already normalised by
 * fr_row_normalize; ids [B].  Writes qt[index + b][d] = q[d][index + b] = gn[b][d] (the same bits in both copies) and
 * labels[index + b] = ids[b], for b < B, d < D.  It writes nothing else of q, qt and labels, reads nothing on the host and
 * does not synchronise.  index + B <= Q (the reference's slice assignment raises otherwise); it does not advance index. */
int fr_sst_enqueue(const float* gn, const int64_t* ids, float* qt, float* q, int64_t* labels, int index, int B, int D, int Q,
                   void* stream);
/* replaces compute_theta / add_margin and forward's * scale, :654-673, :701-702, without the clone of the queue.  A column
 * inside the window takes its cosine from cw, every other column from cos;  c = clamp(., -1, 1), the clamps comparisons: NaN
 * passes;  on the label column, kind 0 ('softmax' and any other string): c;  kind 1 ('am_softmax'): c - p0, p0 = margin;
 * kind 2 ('arc_softmax'): c * p0 - sqrt(1 - c * c) * p1, p0 = cos(margin), p1 = sin(margin) rounded to fp32 (no threshold
 * fallback, no mm);  out[m][n] = that * s.  Every operation is rounded to fp32 on its own, in the reference's order, with no
 * FMA contraction: on the same cosines out has the bits of the reference's fp32 expression (as fr_circle_apply).  ld a
 * multiple of 4, ldw >= rows; columns Q..ld of out are written as 0.  cos, cw and the queue are left alone. */
int fr_sst_apply(const float* cos, const float* cw, float* out, int rows, int B, int Q, int ld, int ldw, int index, int kind,
                 float p0, float p1, float s, void* stream);
/* the backward of :654-673, :701-702.  g is [rows][Q] contiguous.  gcos [rows][ldg] (ldg >= ld, a multiple of 4):
 * (g[m][n] * s) where -1 <= cos[m][n] <= 1 (torch.clamp passes gradient on the closed interval; a NaN cosine gets 0), and
 * exactly 0 in the window columns and in the padding Q..ldg: the label column lies in the window, so d out / d c = s
 * everywhere else.  gwin [rows][ldw], every column written, in cw's layout: gwin[m][blk * B + j] = (g[m][index + j] * s) * d
 * under the pass mask of cw[m][blk * B + j], d = 1 off the label column (j = m % B) and on it for kinds 0 and 1, d = p0 +
 * (c / sqrt(1 - c * c)) * p1 for kind 2; 0 outside the row's block.  So gwin is the K operand of one GEMM against the
 * stacked gallery rows, and the live queue's window enters neither direction.  A target cosine of exactly +-1 makes the
 * reference's own gradient infinite under kind 2 (sqrt(1 - c^2) = 0); nothing is done about that here either. */
int fr_sst_bwd(const float* g, const float* cos, const float* cw, float* gcos, float* gwin, int rows, int B, int Q, int ld,
               int ldg, int ldw, int index, int kind, float p0, float p1, float s, void* stream);

/* ---- ArcNegFace (head/metrics.py:394-433) on the raw cosines cos [rows][ld] of the FR_EPI_STORE GEMM between
 *      fr_row_normalize'd embeddings and the fr_row_normalize'd [N][D] weight.  The head never clamps its cosines and has
 *      no state besides its weight. */
/* replaces :418-433, the reference's loop over the rows with its two host reads per row.  Per row (every wave derives them
 * from one load of the target cosine; the wave of column chunk 0 stores them), rowv [3][rows]:  gt = cos[m][label[m]];
 * gt > thresh (:427-428; thresh is the largest float not above the reference's double cos(pi - margin), so that the
 * comparison decides as the reference's does for every float gt): a = cos(acos(gt) + margin), d a / d gt =
 * sin(acos(gt) + margin) / sqrt(1 - gt^2);  otherwise (:430, mm = sin(pi - margin) * margin): a = gt - mm, d a / d gt = 1.
 * out[m][n] = s * (n == label[m] ? a[m] : t*c + t - 1), t = alpha * exp(-(c - a[m])^2 / sigma), c the raw cosine
 * (:431-433); ld a multiple of 4, columns N..ld of out are written as 0.  Nothing is guarded: a raw target cosine above 1
 * (1 + 2^-23 by rounding) makes acos, a and every t of the row NaN, and so the whole row of out, as in the reference; a raw
 * negative beyond +-1 keeps its value.  A row whose label lies outside [0, N) has no target: rowv = 0, 0, 0, its t is
 * exactly 1 (the reference's initial a = 0 and t_scale = 1) and out = s * c with the bits of c. */
int fr_arcneg_apply(const float* cos, const int64_t* label, float* rowv, float* out, int rows, int N, int ld, float thresh,
                    float margin, float mm, float alpha, float sigma, float s, void* stream);
/* the backward of :418-433 with t and the branch constant (:431 .item(), :432 detach): gcos[m][n] = g[m][n] * s *
 * (n == label[m] ? (d a / d gt)[m] : t), t recomputed from the raw cosine and rowv's a (no [rows][N] buffer of t is kept),
 * whatever the raw cosine (no clamp, no pass mask); 0 in the padding columns N..ldg.  A row whose a is NaN is NaN in all
 * its columns; a row without a target gets g * s with these bits.  g is [rows][N] contiguous, rowv as fr_arcneg_apply left
 * it. */
int fr_arcneg_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos, int rows, int N,
                  int ld, int ldg, float alpha, float sigma, float s, void* stream);

/* ---- focal loss on the batch-mean cross entropy (loss/focal.py:17-21) + top-k (util/utils.py:343-358) */
/* per row of logits [rows][ld] (columns N..ld are not read): lse[m]; ce[m] = lse - z[label], formed as log(S) - (z[label] -
 * max) with S = sum exp(z - max) added in double for it (lse itself is max + logf of the fp32 sum), so that a confident
 * row (ce of 1e-3 under logits of 64) keeps a relative error of a few 1e-7; rank[m] = #{n < N: !(z[n] <= z[label])}: on finite data the columns strictly above the label (a tie
 * does not count against it); a NaN column counts as above it (torch.topk's order), and a NaN label logit or a label outside
 * [0, N) gives rank N, never a hit.  The ce of a label outside [0, N) is lse, bit for bit.  rows > 0, ld >= N > 0 and every
 * pointer are required (FR_UNSUPPORTED before any launch), as for the entries below down to fr_focal_bwd. */
int fr_ce_rows(const float* logits, const int64_t* label, float* lse, float* ce, int32_t* rank, int rows, int N,
               int ld, void* stream);
/* rank[m] only, by the same rule (accuracy on arbitrary logits, util/utils.py:343-358) */
int fr_rank_rows(const float* logits, const int64_t* label, int32_t* rank, int rows, int N, int ld, void* stream);
/* out[j] = scale * #{m < rows: rank[m] < k_j}, j < nk <= 4: precision@k in percent with scale = 100 / rows rounded to float,
 * the value correct_k.mul_(100.0 / batch_size) of util/utils.py:343-358 gives (counts are exact in fp32) */
int fr_topk_precision(const int32_t* rank, int rows, int nk, int k0, int k1, int k2, int k3, float scale, float* out,
                      void* stream);
/* scalars[0]=loss, [1]=dloss/dmeanCE, [2]=prec@1, [3]=prec@5, [4]=mean CE */
int fr_focal_finalize(const float* ce, const int32_t* rank, int rows, float gamma, float* scalars, void* stream);
/* grad[m][n] = gup[0]*scalars[1]/rows * (exp(z-lse[m]) - [n==label[m]]) */
int fr_focal_bwd(const float* logits, const int64_t* label, const float* lse, const float* scalars,
                 const float* gup, float* grad, int rows, int N, int ld, void* stream);
/* replaces nn.CrossEntropyLoss() on the logits (train.py:237-238, :300-302; LOSS_NAME 'Softmax'): fr_focal_finalize
 * without the modulation.  One workgroup; the batch mean l of ce is added as there (double, the same fixed order), so
 * scalars[4] has the bits fr_focal_finalize leaves on the same ce.  scalars[0] = scalars[4] = l, scalars[1] = 1.0f exactly
 * (fr_focal_finalize at gamma = 0 gives 0 * inf = NaN there when l is 0), [2] / [3] = prec@1 / @5 as there; slots 5..7 are
 * not written.  With this layout fr_focal_bwd is the backward kernel.  rows > 0. */
int fr_ce_finalize(const float* ce, const int32_t* rank, int rows, float* scalars, void* stream);

/* ---- Softmax head (head/metrics.py:12-63): logits = F.linear(x, weight, bias), :33.  The GEMM is fr_conv_igemm (1x1,
 *      FR_EPI_STORE with bias: the bias is added once, to the accumulated dot product) on the operands fr_pack_rows leaves,
 *      run over N = pad(N, 4) columns so that the padding columns of the logit store are written as 0. */
/* replaces nothing of the reference's arithmetic: lays out its operands.  w [rows][D] -> wp [rows_pad][D] (the rows from
 * `rows` on zero) and wt [D][ldt], wt[d][r] = wp[r][d] for r < rows_pad (fr_row_normalize's two layouts without the normalisation,
 * one launch); bias [rows] -> biasp [rows_pad] with zeros behind it (both may be NULL).  ldt >= rows_pad >= rows > 0, ldt
 * a multiple of 4. */
int fr_pack_rows(const float* w, const float* bias, float* wp, float* wt, float* biasp, int rows, int rows_pad, int D,
                 int ldt, void* stream);
/* out[m][n] = n < N ? g[m][n] : 0 for n < ldo: the upstream gradient g [rows][ldg] at the pitch the gradient GEMMs of
 * F.linear's backward read (gx = g W, gW = g^T x), padding zero.  ldg >= N > 0, ldo >= N, ldo a multiple of 4. */
int fr_pad_cols(const float* g, float* out, int rows, int N, int ldg, int ldo, void* stream);
/* replaces the bias gradient of F.linear's backward (g.sum(0)): out[n] = ((g[0][n] + g[1][n]) + g[2][n]) + ... in fp32,
 * the rows in order, every sum rounded: bit-defined, so a class shard gets the bits of its columns of the whole matrix.
 * One thread per column.  g is [rows][ldg], ldg >= N > 0. */
int fr_col_sums(const float* g, int rows, int N, int ldg, float* out, void* stream);

/* ---- class-sharded softmax (the process-per-GPU form of the class-dimension split of
 *      head/metrics.py:104-113,170-179): every rank holds the logits of a contiguous class range [lo, hi) for ALL rows of
 *      the global batch; label_local = label - lo, or any value outside [0, N) where another rank owns the label.
 *   fr_shard_row_stats : stats[0][m] = max_n z[m][n], stats[1][m] = sum_n exp(z - max), stats[2][m] = z[m][label_local]
 *                        (0 if not owned); stats is [3][rows] fp32
 *   fr_shard_combine   : stats_all = the ranks' stats in rank order, [world][3][rows]; lse[m] = log sum_n exp z over all
 *                        classes, tlogit[m] = the label's logit, ce[m] = lse - tlogit (fixed summation order: every
 *                        rank gets identical bits)
 *   fr_shard_rank_rows : rank[m] = #{n in this shard: z[m][n] > tlogit[m]} (sum over ranks = top-k rank of the label) */
int fr_shard_row_stats(const float* logits, const int64_t* label_local, float* stats, int rows, int N, int ld,
                       void* stream);
int fr_shard_combine(const float* stats_all, int world, int rows, float* lse, float* ce, float* tlogit, void* stream);
int fr_shard_rank_rows(const float* logits, const float* tlogit, int32_t* rank, int rows, int N, int ld, void* stream);
/* what the SphereFace and CurricularFace heads exchange besides the statistics, both [rows]-sized:
 *   fr_shard_target_cos : tl[m] = clamp(cos[m][label_local], -1, 1) (head/metrics.py:494-496: the clamp, then the gather)
 *                         where 0 <= label_local < N, else exactly +0: one rank owns each label, so the SUM of the ranks'
 *                         tl is exact and independent of order; cos is [rows][ld], ld >= N
 *   fr_shard_sum_parts  : r[m] = r_part[m][0] + ... + r_part[m][nparts-1] in that order (fr_normalize_bwd_radial's): the
 *                         radial term of SphereFace's row scale (head/metrics.py:255, :268) is a sum over all classes,
 *                         so over ranks; shards of different width have different nparts, the summed r goes through
 *                         fr_normalize_bwd_radial with nparts = 1 */
int fr_shard_target_cos(const float* cos, const int64_t* label_local, float* tl, int rows, int N, int ld, void* stream);
int fr_shard_sum_parts(const float* r_part, int nparts, float* r, int rows, void* stream);

/* ---- class sampling for the class-sharded head (Partial-FC, An et al. 2021/22; no counterpart in the reference, whose
 *      head/metrics.py:104-113 splits the classes and runs all of them): every step a rank runs its head on n_s of the n
 *      classes of its shard, the classes of the global batch among them.  All integer arithmetic is mod 2^32:
 *   fmix32(h)  : h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16      (a bijection on uint32)
 *   key(c)     = fmix32((class0 + c) ^ salt), c = 0 .. n - 1, class0 the shard's first global class; class0 + n <= 2^32, so
 *                the keys of a shard are distinct and the selection has no ties
 *   pos[c]     = some row's label_local is c (values outside [0, n), the -1 of rows owned elsewhere among them, mark nothing)
 *   S          = every positive + the n_s - P non-positive classes with the smallest keys (P positives): |S| = n_s exactly
 *   idx [n_s]  = S in ascending class order;  inv [n] = position in idx, or -1;
 *   label_s [rows] = inv[label_local] where 0 <= label_local < n, else -1
 * 1 <= n_s <= n and n_s >= min(n, rows), so that P <= n_s holds without reading the device.  Writes every element of idx,
 * inv and label_s and nothing outside them; reads nothing on the host, does not synchronise the stream, allocates nothing.
 * A three-pass radix descent (11 / 11 / 10 key bits; LDS histograms with integer atomics, added into one histogram per
 * pass with integer atomics, narrowed by one workgroup) finds the (n_s - P)-th smallest key, a count + ordered-write pair
 * compacts: integer arithmetic and integer atomics only, whose sums do not depend on their order, so the result is
 * bit-defined and the same from run to run.  work: fr_class_sample_work(n) uint32 words. */
int fr_class_sample_work(int n);
int fr_class_sample(const int64_t* label_local, int rows, int n, int n_s, uint32_t salt, uint32_t class0, int32_t* idx,
                    int32_t* inv, int64_t* label_s, uint32_t* work, void* stream);
/* out[j][:] = w[idx[j]][:], j < n_s: the selected rows of a [n][D] fp32 parameter (D = 1: a bias), D >= 1 */
int fr_gather_rows(const float* w, const int32_t* idx, float* out, int n_s, int D, void* stream);
/* out[c][:] = inv[c] >= 0 ? g[inv[c]][:] : 0, c < n: the dense [n][D] gradient from the gathered one.  Every element of
 * out is written exactly once: no memset, no atomics. */
int fr_scatter_rows(const float* g, const int32_t* inv, float* out, int n, int D, void* stream);

/* ---- GPU-side training-input transform (replaces the per-sample host transform of train.py:108-116
 *      applied in dataset.py:85-88): Resize(Hr x Wr, Pillow 8-bit bilinear, bit-exact) -> crop S x S at crop[b] = (x0, y0)
 *      -> horizontal flip where flip[b] -> ToTensor -> Normalize, for a batch of staged uint8 images.
 *   src  uint8 [B][Hin][Win][3] (HWC, as decoded)          out  float32 [B][3][S][S] (NCHW, what the reference collates)
 *   xtab int32 [Wr][kx+2], ytab int32 [Hr][ky+2]: per resized column / row (first input index, tap count, kx / ky integer
 *        weights with 22 fractional bits) -- Pillow's precompute_coeffs + normalize_coeffs_8bpc (frhip/input_pipeline.py)
 *   lut  float32 [256][3]: ((v / 255) - mean[c]) / std[c], every step rounded to float32
 *   crop offsets must satisfy 0 <= x0 <= Wr - S, 0 <= y0 <= Hr - S (checked by the caller: they live in device memory) */
int fr_augment_u8(const uint8_t* src, const int32_t* xtab, const int32_t* ytab, const int32_t* crop, const uint8_t* flip,
                  const float* lut, float* out, int B, int Hin, int Win, int Hr, int Wr, int S, int kx, int ky,
                  void* stream);
/* The same transform on a batch drawn from a device-resident store (frhip/resident.py): image b of the batch is
 * store[idx[b]], transformed exactly as fr_augment_u8 transforms image b of a staged batch (same tables, crop, flip, lut),
 * and label_out[b] = labels[idx[b]] is written by the same launch.  One launch, the grid of fr_augment_u8.
 *   store uint8 [M][Hin][Win][3]    labels int64 [M]    idx int32 [B], 0 <= idx[b] < M (checked by the caller: the indices
 *   live in device memory), may repeat, in any order    label_out int64 [B]    labels / label_out may both be null
 * The slot offset idx[b] * Hin * Win * 3 is formed in 64 bits: stores beyond 4 GiB are the normal case.  B <= 0 returns 0;
 * M <= 0, the size conditions of fr_augment_u8, B > 65535 and a null store / idx / out are refused before any launch. */
int fr_augment_u8_gather(const uint8_t* store, const int64_t* labels, const int32_t* idx, const int32_t* xtab,
                         const int32_t* ytab, const int32_t* crop, const uint8_t* flip, const float* lut, float* out,
                         int64_t* label_out, int M, int B, int Hin, int Win, int Hr, int Wr, int S, int kx, int ky,
                         void* stream);
/* RandAugment on the decoded images (data_processing/randaugment.py, the served set): image b of the batch is
 * src[idx ? idx[b] : b], taken through the K operations (op[b][k], par[b][k]), k = 0 .. K-1 in order, every step rounded
 * to uint8 as Pillow rounds between operations; the bytes are Pillow's (tests/randaug_ref.py).  One workgroup per image:
 * one read from HBM, the whole chain in LDS, one write.  Integer statistics only: the same bytes from run to run.
 *   src uint8 [idx ? M : B][H][W][3]    dst uint8 [B][H][W][3]    op uint8 [B][K]    par float32 [B][K]
 *   idx int32 [B] or null, 0 <= idx[b] < M (checked by the caller: device memory), may repeat, in any order; the slot
 *   offset is formed in 64 bits    labels int64 [M] / label_out int64 [B]: label_out[b] = labels[slot] when both are given
 *   op  0 identity (equalize, which the reference leaves undone; padding; any code above 9)
 *       1 autocontrast                          6 brightness, par = factor
 *       2 solarize, par = threshold             7 translateX, par = integer shift sx: out[y][x] = in[y][x + sx], else black
 *       3 color, par = factor                   8 translateY, par = integer shift sy: out[y][x] = in[y + sy][x], else black
 *       4 posterize, par = bits kept (0..8)     9 invert
 *       5 contrast, par = factor (the mean is that of the image as the step finds it)
 * B <= 0 returns 0.  Refused before any launch: B > 65535, K outside 1..16, a null src / op / par / dst, M <= 0 with idx,
 * H or W <= 0, and an image beyond the LDS budget H * W * 3 + 3 * 256 * 4 <= 65536 (128x128 fits, 148x148 does not). */
int fr_randaug_u8(const uint8_t* src, const int64_t* labels, const int32_t* idx, const uint8_t* op, const float* par,
                  uint8_t* dst, int64_t* label_out, int M, int B, int K, int H, int W, void* stream);
/* F.interpolate(x, size, mode='bilinear') of pSp.forward (backbone/restyle_psp.py:440-443: align_corners = False, no
 * antialias) on fp32 NCHW planes: in [planes][Hin][Win] -> out [planes][Hout][Wout]; planes = B * C <= 65535. */
int fr_resize_bilinear(const float* in, float* out, int planes, int Hin, int Win, int Hout, int Wout, void* stream);
/* Its adjoint: gin [planes][Hin][Win] = the gradient of fr_resize_bilinear's input for gout [planes][Hout][Wout]; a gather
 * over the outputs each input pixel entered (no atomics).  Same argument checks as the forward.  Replaces the autograd of
 * F.interpolate(..., mode='bilinear') in pSp.forward (backbone/restyle_psp.py:440-443). */
int fr_resize_bilinear_bwd(const float* gout, float* gin, int planes, int Hin, int Win, int Hout, int Wout, void* stream);

/* ---- RB-WebFace pair tallies (rb-webface/scripts/test_RB_Webface.py:153-233: calc_FNMR, calc_FMR), fp32.  E [M][ldE] holds
 *      M L2-normalised rows of D floats (fr_row_normalize), thr [T] the thresholds on the device, T <= 32:
 *   mode 0: counts[t] = #{ i < j                         : E_i . E_j > thr[t] }   (all pairs; `group` ignored)
 *   mode 1: counts[t] = #{ i < j, i / group == j / group : E_i . E_j < thr[t] }   (group consecutive rows = one person,
 *                                                                                  2 <= group <= 16; a short last group counts the pairs it has)
 * Both comparisons are strict and a NaN score is in no tally.  The M x M scores are never stored: one workgroup per
 * 128 x 128 tile of the upper triangle (mode 1: the diagonal tiles and the right neighbour wherever a tile edge cuts a group)
 * forms its scores with the f32-input MFMA, tallies them and writes one row of partials [fr_pair_counts_parts()][T] uint32;
 * a second kernel of the same call sums the rows into counts [T] int64.  Integer sums: bit-identical from run to run.
 * M >= 2, D % 4 == 0, 4 <= D <= 2048, ldE % 4 == 0, E 16-byte aligned.  Allocates nothing. */
int fr_pair_counts(const float* E, int ldE, int M, int D, const float* thr, int T, int mode, int group, uint32_t* partials,
                   int64_t* counts, void* stream);
/* rows of `partials` a call with (M, mode, group) writes (host arithmetic only); < 0: unsupported argument */
int fr_pair_counts_parts(int M, int mode, int group);

/* ---- Histogram of the same pair scores over a window of their integer keys: one pass of the radix select that finds the
 *      exact threshold at a chosen FPR (the np.interp lines of rb-webface/scripts/test_RB_Webface.py:153-233 interpolate
 *      between twenty hand-placed thresholds instead).  E, ldE, M, D, mode and group as for fr_pair_counts, and the scores
 *      are bit for bit the ones fr_pair_counts compares (one main loop, csrc/pair_tile.h).  The key of a score s keeps
 *      the order of the scores and has no NaN:
 *   u = bits(s == 0 ? +0.0f : s);   key = (u & 0x80000000) ? ~u : (u | 0x80000000)
 *   hist[0]      = #{ pairs : key <  key_lo }
 *   hist[1 + b]  = #{ pairs : key_lo + (b << shift) <= key < key_lo + ((b + 1) << shift) },   0 <= b < NB
 *   hist[NB + 1] = #{ pairs : key >= key_lo + (NB << shift) }
 * A NaN score (a zero row) is in no slot.  1 <= NB <= 2048, 0 <= shift <= 21, key_lo + (NB << shift) <= 2^32.  Persistent
 * workgroups bin into LDS and write one row each of partials [fr_pair_hist_parts()][NB + 2] uint32; a second kernel of the
 * same call sums the rows into hist [NB + 2] int64.  No global atomics: bit-identical from run to run.  Allocates nothing. */
int fr_pair_hist(const float* E, int ldE, int M, int D, uint32_t key_lo, int shift, int NB, int mode, int group,
                 uint32_t* partials, int64_t* hist, void* stream);
/* rows of `partials` a call with (M, mode, group) writes (host arithmetic only); < 0: unsupported argument, among them an
 * M so large that one workgroup would see 2^32 pairs */
int fr_pair_hist_parts(int M, int mode, int group);

/* ---- multi-tensor SGD with momentum (torch.optim.SGD defaults; train.py:196)
 *   d = g + wd*p ; buf = momentum*buf + d ; p -= lr*buf      (buf starts at 0, so the first step gives buf = d)
 * table_dev: device array of tensor records; chunks_dev: device array of (tensor index, chunk index) pairs,
 * one thread block per chunk of fr_sgd_chunk_elems() elements. */
typedef struct FrSgdTensor {
  float* p;
  const float* g;
  float* buf;
  long long n;
  float wd;
  int32_t pad_;
} FrSgdTensor;
int fr_sgd_chunk_elems(void);
int fr_sgd_step(const FrSgdTensor* table_dev, const int32_t* chunks_dev, int nchunks, float lr, float momentum,
                void* stream);
/* The same update on the rows idx[0 .. n_s) of ONE dense fp32 parameter p [n][D] and its momentum buffer buf [n][D], with
 * the gradient given as the gathered rows g_rows [n_s][D] (contiguous) -- the lazy update of Partial-FC v1 for the sampled
 * class-sharded head (frhip/sharded_head.py, sparse_update):
 *   r = idx[j], j < n_s:   d = g_rows[j] + wd*p[r] ; buf[r] = momentum*buf[r] + d ; p[r] -= lr*buf[r]
 * element for element the expression of fr_sgd_step with the same roundings (one device function serves both kernels).
 * Rows not in idx are neither read nor written: no weight decay and no momentum step while a row is unselected.  idx is
 * ascending and distinct with every entry in [0, n), as fr_class_sample leaves it (n does not cross the ABI and nothing
 * checks the entries): one writer per element, plain stores, no atomics.  D >= 1 (D = 1: a bias); 16-byte accesses where
 * D % 4 == 0 and p, buf and g_rows are 16-byte aligned, 4-byte accesses otherwise.  One launch whose grid follows n_s * D,
 * 20 bytes of memory traffic per element of the selected rows.  n_s <= 0 launches nothing and returns 0; with n_s > 0 all
 * four pointers are required. */
int fr_sgd_rows(float* p, float* buf, const float* g_rows, const int32_t* idx, int n_s, int D, float lr, float momentum,
                float wd, void* stream);

/* ---- multi-tensor Adam (torch.optim.Adam defaults: no weight decay, no amsgrad; the reference's OPTIMIZER_NAME ==
 *      'Adam' branch, train.py:197-198), same table / chunk scheme as fr_sgd_step:
 *   m += (g - m) * w1 ; v = v * beta2 + (w2 * g) * g ; p += (-step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 * with the scalars torch derives in double precision on the host and rounds to float: w1 = 1 - beta1, w2 = 1 - beta2,
 * step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step).  Operation order = ATen's kernels (lerp, mul +
 * addcmul, sqrt / bc2_sqrt + eps, addcdiv), every operation rounded to fp32 on its own (no FMA contraction, correctly
 * rounded sqrt and division): bit for bit the np.float32 restatement of tests/loss_optim_ref.py.  torch's own kernels fuse
 * the multiply-adds of lerp and addcmul, so they agree with this to the last bit or two, not bit for bit.
 * nchunks <= 0 launches nothing and returns 0 (fr_sgd_step alike); with nchunks > 0 both tables are required. */
typedef struct FrAdamTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
} FrAdamTensor;
int fr_adam_step(const FrAdamTensor* table_dev, const int32_t* chunks_dev, int nchunks, float step_size, float w1,
                 float beta2, float w2, float eps, float bc2_sqrt, void* stream);

/* ---- multi-tensor moving average of parameters: the gallery network of SST_Prototype follows the probe network (head/
 *      metrics.py:638-708 takes both networks' embeddings; the reference has no driver that moves the gallery), same table /
 *      chunk scheme as fr_sgd_step:
 *   dst = a * dst + b * src
 * with a = float(alpha), b = float(1.0 - alpha), the subtraction done in double on the host.  Two multiplies and one add,
 * each rounded to fp32 on its own (no FMA contraction): bit for bit the np.float32 restatement.  src is left alone.
 * nchunks <= 0 launches nothing and returns 0; with nchunks > 0 both tables are required.  One thread block per chunk of
 * fr_ema_chunk_elems() elements. */
typedef struct FrEmaTensor {
  float* dst;
  const float* src;
  long long n;
} FrEmaTensor;
int fr_ema_chunk_elems(void);
int fr_ema_step(const FrEmaTensor* table_dev, const int32_t* chunks_dev, int nchunks, float a, float b, void* stream);

/* ---- device-side gradient guard: global L2 norm of a set of gradients, clip coefficient and non-finite step skip
 *      (torch.nn.utils.clip_grad_norm_(parameters, max_norm), norm type 2, plus the skip GradScaler does on inf / NaN),
 *      same table / chunk scheme as fr_sgd_step.  Two small launches before the optimizer step leave a control word on the
 *      device; the *_ctl step entries read it.  Nothing crosses to the host and no gradient is written.
 *
 * fr_grad_sumsq: one workgroup of 256 threads per (tensor index, chunk index) pair; parts[c] is the sum of
 * (double)g[i] * (double)g[i] over the L <= fr_sgd_chunk_elems() elements of chunk c, x[0 .. L), added in double in this
 * order, which depends on L alone:
 *   thread t (0 .. 255):  a[t] = ((x[t]^2 + x[t + 256]^2) + x[t + 512]^2) + ...   over t + 256 j < L, j ascending; no
 *                         element: a[t] = +0.0   (a square of an fp32 value is exact in double, fused or not)
 *   wave w (0 .. 3):      its 64 values v[0 .. 64) = a[64 w ..] fold in halves, v[l] += v[l + h] for l < h, h = 32, 16, 8,
 *                         4, 2, 1 (the xor butterfly of wave_sum_d); the wave's sum is v[0]
 *   parts[c] = ((s[0] + s[1]) + s[2]) + s[3]   over the four waves' sums.
 * Every access to g is 4 bytes wide, so a tensor at any 4-byte offset is read inside [g, g + n) and in that order.  Plain
 * stores, no atomics: bit-identical from run to run, whatever the grid and the order of the chunk list.  nchunks <= 0
 * launches nothing and returns 0; with nchunks > 0 table_dev, chunks_dev and parts are required. */
typedef struct FrGradTensor {
  const float* g;
  long long n;
} FrGradTensor;
int fr_grad_sumsq(const FrGradTensor* table_dev, const int32_t* chunks_dev, int nchunks, double* parts, void* stream);
/* fr_grad_guard: ONE workgroup of 256 threads turns the partial sums into the control word ctl [4] (fp32, device):
 *   total:   thread t adds parts[t], parts[t + 256], ... in ascending index order in double (no part: +0.0); the 256 values
 *            are then summed by the tree of fr_grad_sumsq (halving folds per wave, the four waves in order).  The tree
 *            depends on nparts alone.
 *   ctl[0] = (float)sqrt(total)                           the global L2 norm (double square root, rounded once more to fp32)
 *   ctl[1] = the clip coefficient, torch's expression with every operation rounded to fp32 on its own:
 *            c = max_norm / (ctl[0] + 1e-6f);  ctl[1] = c > 1 ? 1 : c      -- a NaN passes through, an infinite norm gives 0;
 *            max_norm <= 0 is "measure only": ctl[1] = 1 exactly
 *   ctl[2] = the go flag: 0.0f when skip_nonfinite != 0 and total is not finite, else 1.0f
 *   ctl[3] = 0
 * skipped (int32 [2], device) may be NULL; otherwise thread 0 does skipped[0] += 1 when the go flag is 0 and skipped[1] += 1
 * always, with plain loads and stores (calls on one stream are ordered).  nparts == 0 is allowed, parts may then be NULL:
 * norm 0, coefficient 1 (or max_norm / 1e-6f clamped, which is 1 for every max_norm >= 1e-6f), go 1.  nparts < 0, a NaN
 * max_norm, a missing ctl and missing parts with nparts > 0 are refused. */
int fr_grad_guard(const double* parts, int nparts, float max_norm, int skip_nonfinite, float* ctl, int32_t* skipped,
                  void* stream);
/* The step entries under the control word.  ctl[2] == 0: every workgroup returns before it touches p, buf, m or v (the
 * gradients are not read either).  Otherwise the update of the entry without _ctl, by the same device functions, on
 *   g' = g * ctl[1]  when use_coef != 0 (a multiply of its own, rounded to fp32, never contracted into the wd * p FMA),
 *   g' = g           when use_coef == 0;
 * g is never written.  Bit for bit "scale the gradients in place in fp32, then fr_sgd_step / fr_adam_step"; with ctl =
 * {x, 1, 1, 0} bit for bit the entry without _ctl.  fr_sgd_rows_ctl honours the go flag alone (the head is not clipped:
 * the norm is the backbone's, frhip/optim.py).  ctl is required whenever the entry would launch. */
int fr_sgd_step_ctl(const FrSgdTensor* table_dev, const int32_t* chunks_dev, int nchunks, float lr, float momentum,
                    const float* ctl, int use_coef, void* stream);
int fr_adam_step_ctl(const FrAdamTensor* table_dev, const int32_t* chunks_dev, int nchunks, float step_size, float w1,
                     float beta2, float w2, float eps, float bc2_sqrt, const float* ctl, int use_coef, void* stream);
int fr_sgd_rows_ctl(float* p, float* buf, const float* g_rows, const int32_t* idx, int n_s, int D, float lr, float momentum,
                    float wd, const float* ctl, void* stream);

/* out[r][c] = bias ? bias[c] : 0  (fp32 [rows][C]); seeds the split-K accumulation of Linear(25088,512) */
int fr_fill_rows(float* out, const float* bias, long long rows, int C, void* stream);

/* ---- misc */
/* Capability queries.  SURVEY.md 8(b)-ii sketched ONE `fr_supported(op, dtype, Cin, Cout, H, W, stride)`; the build answers
 * the same question per kernel family instead, because the answer doubles as the launch geometry the caller must size
 * buffers for: fr_conv3x3_strip_parts / fr_conv3x3_s2_strip_parts return the number of partial-sum rows a launch will
 * write (0 = shape not served: the caller uses fr_conv_igemm, which serves every shape), fr_conv_wgrad_strip_supported
 * answers yes / no, fr_conv_wgrad_strip_groups returns the strip groups to launch with (0 = shape not served: the caller
 * uses fr_conv_wgrad) and fr_conv_wgrad_strip_kernel names the kernel a launch reaches.  Every entry point additionally
 * returns < 0 for an unsupported argument (text in fr_last_error_string()), never silently computing something else. */
int fr_abi_version(void);
/* Run-time switches (kernel-family A/B switches, test hooks; README "Switches"): an int per name, first read from the
 * environment variable of that name, then cached for the life of the process.  fr_set_option overrides the cached value
 * (returns the previous one); fr_get_option reads it (dflt when neither set nor in the environment). */
int fr_set_option(const char* name, int value);
int fr_get_option(const char* name, int dflt);
/* Completion event of a kernel (ABI v6).  The backward pass hands its weight gradients to a second stream behind dependency
 * edges (the reference runs them inside autograd's single stream: loss.backward(), train.py:314); an edge set with
 * hipEventRecord costs the producing stream a marker packet the next kernel waits for (+3.0 ... 5.1 us per edge, three edges
 * per residual unit; tools/edge_probe.hip).  fr_arm_stop_event(event) makes the NEXT kernel this thread launches through one
 * of fr_conv3x3_strip / fr_conv3x3_s2_strip / fr_conv_igemm / fr_conv1x1_stream / fr_reduce_parts carry `event` (a
 * hipEvent_t) as its own completion signal instead (+0.0 ... 1.6 us).  fr_finish_stop_event(stream) ends the bracket: it
 * returns the number of kernels launched since the event was armed and, unless that is exactly one, records the event on
 * `stream` the ordinary way (entry points that launch no such kernel, or several), so the event is ALWAYS behind the whole
 * call.  Per-thread state, like the error string.  < 0: no event armed / hipEventRecord failed. */
int fr_arm_stop_event(void* event);
int fr_finish_stop_event(void* stream);
/* sizeof() of the argument structs as compiled, for binding self-checks: 0 FrConvArgs, 1 FrWgradArgs,
 * 2 FrApplyArgs, 3 FrBnBwdArgs, 4 FrSgdTensor, 5 FrPackTensor, 6 FrAdamTensor, 7 FrBnEvalEntry, 8 FrBnFinArgs,
 * 9 FrEmaTensor, 10 FrGradTensor */
int fr_struct_size(int which);
const char* fr_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif
