// frhip -- margin-head row kernels, focal loss on the batch-mean cross entropy, top-k rank, multi-tensor SGD.
//
// Reference arithmetic replaced (paths under /root/reference):
//   F.normalize(x), F.normalize(W) (eps 1e-12) + their autograd      head/metrics.py:103, :167
//   d phi / d cos of the ArcFace / CosFace margin, label select       head/metrics.py:115-138, :181-189
//   SphereFace margin (clamp, k, Chebyshev phi, lambda blend, *||x||)  head/metrics.py:236-268
//   Am_softmax l2_norm(kernel, axis=0), clamp, label margin, *s         head/metrics.py:280-284, :302-331
//   CurricularFace per-row margin, EMA of t, hard-negative re-weighting head/metrics.py:494-509
//   MagFace magnitude-dependent margin, loss_g, label-column margin      head/metrics.py:533-552
//   AdaCos row sums of exp(s cos), median target angle, the scale moved  head/metrics.py:359-368
//   Softmax head: the operands of F.linear(x, W, b), the bias gradient  head/metrics.py:12-63
//   nn.CrossEntropyLoss() on the rows of the cross entropy            train.py:237-238, :300-302
//   FocalLoss on mean CE                                              loss/focal.py:17-21
//   accuracy top-1/5                                                  util/utils.py:343-358
//   optim.SGD(momentum, coupled weight decay on group 0)              train.py:196, :313-316
//   the gallery network of SST_Prototype as a moving average of the probe network (head/metrics.py:638-708; the
//   reference has no driver for it: dst = a dst + b src over the parameters)
#include <stdio.h>

#include "common.h"
#include "frhip_internal.h"

namespace {

// ------------------------------------------------------------------------------------------ row normalise
template <typename T>
__global__ void row_normalize_kernel(const float* __restrict__ x, T* __restrict__ xn, T* __restrict__ xt,
                                     float* __restrict__ inv, int rows, int rows_pad, int D, int ldt) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows_pad) return;
  if (row >= rows) {
    for (int d = lane; d < D; d += 64) {
      Elt<T>::st(xn + (size_t)row * D + d, 0.f);
      if (xt) Elt<T>::st(xt + (size_t)d * ldt + row, 0.f);
    }
    return;
  }
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = x[(size_t)row * D + d];
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  const float iv = 1.0f / fmaxf(nrm, 1e-12f);
  if (lane == 0) inv[row] = iv;
  for (int d = lane; d < D; d += 64) {
    const float v = x[(size_t)row * D + d] * iv;
    Elt<T>::st(xn + (size_t)row * D + d, v);
    if (xt) Elt<T>::st(xt + (size_t)d * ldt + row, v);
  }
}

// xt[d][r] = xn[r][d] through 64 x 64 LDS tiles (both sides coalesced).  The per-row kernel above writes the transposed
// copy as 4-byte stores with a stride of a whole row per lane; for the head weight (N x 512) this second pass is 3x cheaper.
template <typename T>
__global__ __launch_bounds__(256) void transpose_rows_kernel(const T* __restrict__ in, T* __restrict__ out, int R, int D,
                                                             int ldt) {
  __shared__ T tt[64][66];
  const int d0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int j = ty; j < 64; j += 4)
    if (r0 + j < R && d0 + tx < D) tt[j][tx] = in[(size_t)(r0 + j) * D + d0 + tx];
  __syncthreads();
  for (int j = ty; j < 64; j += 4)
    if (d0 + j < D && r0 + tx < R) out[(size_t)(d0 + j) * ldt + r0 + tx] = tt[tx][j];
}

__global__ void normalize_bwd_kernel(const float* __restrict__ G, const float* __restrict__ x,
                                     const float* __restrict__ inv, float* __restrict__ gx, int rows, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float iv = inv[row];
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot = fmaf(x[(size_t)row * D + d] * iv, G[(size_t)row * D + d], dot);
  dot = wave_sum(dot);
  for (int d = lane; d < D; d += 64) {
    const float xh = x[(size_t)row * D + d] * iv;
    gx[(size_t)row * D + d] = (G[(size_t)row * D + d] - xh * dot) * iv;
  }
}

// ------------------------------------------------------------------------------------------ margin backward
template <typename T>
__global__ void margin_bwd_kernel(const float* __restrict__ g, const long long* __restrict__ label,
                                  const float* __restrict__ cos_t, T* __restrict__ gcos, int rows, int N, int ldg,
                                  int kind, int easy, float cos_m, float sin_m, float th, float scale) {
  const int m = blockIdx.y;
  if (m >= rows) return;
  const long long lab = label[m];
  float dphi = 1.f;
  if (kind == 0) {
    const float c = cos_t[m];
    const bool use_phi = easy ? (c > 0.f) : (c > th);
    if (use_phi) {
      const float t = 1.0f - c * c;
      const bool inside = t > 1e-10f && t < 1.0f - 1e-10f;  // clamp passes gradient only strictly inside
      dphi = cos_m + (inside ? sin_m * c / sqrtf(t) : 0.f);
    }
  }
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < ldg; n += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (n < N) v = scale * g[(size_t)m * N + n] * (n == lab ? dphi : 1.f);
    Elt<T>::st(gcos + (size_t)m * ldg + n, v);
  }
}

// ------------------------------------------------------------------------------------------ SphereFace / Am_softmax
// Margin on the raw cosines the GEMM stored (FR_EPI_STORE): the GEMM epilogue, shared with the backbone, stays as it is,
// and the saved raw cosines give the backward pass its clamp mask.  Block = 4 waves = 4 rows, one f32x4 per lane, 1024
// columns per block (blockIdx.x); ld and ldg are multiples of 4.
constexpr int MARGIN_COLS = 1024;

// torch.clamp(c, -1, 1): NaN passes through (fminf / fmaxf would turn it into a bound)
__device__ __forceinline__ float clamp1(float c) { return c > 1.f ? 1.f : (c < -1.f ? -1.f : c); }

// SphereFace on the label column (head/metrics.py:227-268): phi = (-1)^k T_m(c) - 2k, k = floor(m acos(c) / 3.14159265)
// in fp32, detached; returns (phi - c) / div + c and d/dc of it
__device__ __forceinline__ float sphere_label(float c, int mi, float div, float* dout) {
  const float c2 = c * c;
  float t, dt;
  switch (mi) {
    case 0: t = 1.f; dt = 0.f; break;
    case 1: t = c; dt = 1.f; break;
    case 2: t = 2.f * c2 - 1.f; dt = 4.f * c; break;
    case 3: t = 4.f * c2 * c - 3.f * c; dt = 12.f * c2 - 3.f; break;
    case 4: t = 8.f * (c2 * c2) - 8.f * c2 + 1.f; dt = 32.f * c2 * c - 16.f * c; break;
    default: t = 16.f * (c2 * c2 * c) - 20.f * (c2 * c) + 5.f * c; dt = 80.f * (c2 * c2) - 60.f * c2 + 5.f; break;
  }
  const float k = floorf((float)mi * acosf(c) / 3.14159265f);
  const float sg = ((int)k & 1) ? -1.f : 1.f;
  const float phi = sg * t - 2.f * k;
  *dout = 1.f + (sg * dt - 1.f) / div;
  return (phi - c) / div + c;
}

// Forward walker of one row: out[n] = body(n, raw cosine) for n < N, 0 in the padding columns [N, ld)
template <typename Body>
__device__ __forceinline__ void margin_cols_fwd(const float* __restrict__ cos, float* __restrict__ out, int row, int N,
                                                int ld, Body body) {
  const int lane = threadIdx.x & 63;
  const int end = min(ld, (int)(blockIdx.x + 1) * MARGIN_COLS);
  for (int n = blockIdx.x * MARGIN_COLS + lane * 4; n < end; n += 256) {
    const f32x4 ch = *reinterpret_cast<const f32x4*>(cos + (size_t)row * ld + n);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = body(n + j, ch[j]);
      o[j] = n + j < N ? v : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)row * ld + n) = o;
  }
}

// Backward walker of one row: gcos[n] = body(n, raw cosine, g[n]) where the clamp passes gradient (torch.clamp: the closed
// interval), 0 where it saturated and in the padding columns [N, ldg).  cos has the pitch ld <= ldg.  kPassMask = false is
// for a head that never clamps (MV_Softmax): every column n < N gets body's value, whatever its raw cosine.
template <bool kPassMask = true, typename Body>
__device__ __forceinline__ void margin_cols_bwd(const float* __restrict__ g, const float* __restrict__ cos,
                                                float* __restrict__ gcos, int row, int N, int ld, int ldg, Body body) {
  const int lane = threadIdx.x & 63;
  const float* crow = cos + (size_t)row * ld;
  const float* grow = g + (size_t)row * N;
  float* orow = gcos + (size_t)row * ldg;
  const int end = min(ldg, (int)(blockIdx.x + 1) * MARGIN_COLS);
  for (int n = blockIdx.x * MARGIN_COLS + lane * 4; n < end; n += 256) {
    f32x4 ch = {0.f, 0.f, 0.f, 0.f};
    if (n < ld) ch = *reinterpret_cast<const f32x4*>(crow + n);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      if (n + j < N) {
        const float gg = grow[n + j];
        const bool pass = !kPassMask || (ch[j] >= -1.f && ch[j] <= 1.f);
        const float d = body(n + j, ch[j], gg);
        v = pass ? d : 0.f;
      }
      o[j] = v;
    }
    *reinterpret_cast<f32x4*>(orow + n) = o;
  }
}

// The opening of every walker kernel: wave w of block y has row 4 y + w; the waves past the last row leave at once, the
// others run body(row, its label, has: the label selects a column of the row).
template <typename Body>
__device__ __forceinline__ void walk_row(const long long* __restrict__ label, int rows, int N, Body body) {
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long lab = label[row];
  body(row, lab, lab >= 0 && lab < N);
}

// Every wave of a row derives the same K row values; the wave of column chunk 0 leaves them in rowv [K][rows].
template <int K>
__device__ __forceinline__ void chunk0_store(float* __restrict__ rowv, int rows, int row, const float (&v)[K]) {
  if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) rowv[k * rows + row] = v[k];
  }
}

// kind 2: out = nrm * (label ? sphere : c), nrm = ||x_m|| (p0 = 1 + lambda);  kind 3: out = p1 * (label ? c - p0 : c)
__global__ __launch_bounds__(256) void margin_apply_kernel(const float* __restrict__ cos, const long long* __restrict__ label,
                                                           const float* __restrict__ inv_x, float* __restrict__ out,
                                                           int rows, int N, int ld, int kind, int mi, float p0, float p1) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float scale = kind == 2 ? 1.f / inv_x[row] : p1;
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float raw) {
      const float c = clamp1(raw);
      float v = c;
      if (n == lab) {
        float unused;
        v = kind == 2 ? sphere_label(c, mi, p0, &unused) : c - p0;
      }
      return v * scale;
    });
  });
}

// gcos = g * d out / d cos.  kind 2 also leaves r_part[row][blockIdx.x] = sum over the block's columns of g * out / nrm.
__global__ __launch_bounds__(256) void margin_apply_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                               const long long* __restrict__ label,
                                                               const float* __restrict__ inv_x, float* __restrict__ gcos,
                                                               float* __restrict__ r_part, int rows, int N, int ld, int ldg,
                                                               int kind, int mi, float p0, float p1) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float scale = kind == 2 ? 1.f / inv_x[row] : p1;
    float r = 0.f;
    margin_cols_bwd(g, cos, gcos, row, N, ld, ldg, [&](int n, float raw, float gg) {
      const float c = clamp1(raw);
      float a = c, d = 1.f;
      if (kind == 2 && n == lab) a = sphere_label(c, mi, p0, &d);
      if (kind == 2) r = fmaf(gg, a, r);
      return gg * scale * d;
    });
    if (kind == 2) {
      r = wave_sum(r);
      if ((threadIdx.x & 63) == 0) r_part[(size_t)row * gridDim.x + blockIdx.x] = r;
    }
  });
}

// normalise backward plus the radial term of a row scale ||x|| (SphereFace's NormOfFeature, head/metrics.py:255,268):
// gx = (G - xh (xh . G)) inv + r xh, r = the row's r_part added in order
__global__ void normalize_bwd_radial_kernel(const float* __restrict__ G, const float* __restrict__ x,
                                            const float* __restrict__ inv, const float* __restrict__ r_part, int nparts,
                                            float* __restrict__ gx, int rows, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float iv = inv[row];
  float r = 0.f;
  for (int p = 0; p < nparts; ++p) r += r_part[(size_t)row * nparts + p];
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot = fmaf(x[(size_t)row * D + d] * iv, G[(size_t)row * D + d], dot);
  dot = wave_sum(dot);
  for (int d = lane; d < D; d += 64) {
    const float xh = x[(size_t)row * D + d] * iv;
    gx[(size_t)row * D + d] = (G[(size_t)row * D + d] - xh * dot) * iv + r * xh;
  }
}

// r[row] = r_part[row][0] + ... + r_part[row][nparts - 1], in the order normalize_bwd_radial_kernel adds them.  The
// class-sharded SphereFace head sums r over the ranks (shards of different width have different nparts) and then calls
// that kernel with nparts = 1.
__global__ __launch_bounds__(256) void sum_row_parts_kernel(const float* __restrict__ r_part, int nparts,
                                                            float* __restrict__ r, int rows) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float acc = 0.f;
  for (int p = 0; p < nparts; ++p) acc += r_part[(size_t)row * nparts + p];
  r[row] = acc;
}

// Am_softmax's l2_norm(kernel, axis=0) (head/metrics.py:280-284, no eps): kt[d][j] = K[d][j] / ||K[:, j]|| in the [D][Np]
// layout of K (columns N..Np zero), inv[j] = 1 / ||K[:, j]||.  Block = 64 columns x 4 slices of D, slices added in order.
__global__ __launch_bounds__(256) void col_normalize_kernel(const float* __restrict__ K, float* __restrict__ kt,
                                                            float* __restrict__ inv, int D, int N, int Np) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + tx;
  float ss = 0.f;
  if (j < N)
    for (int d = ty; d < D; d += 4) {
      const float v = K[(size_t)d * N + j];
      ss = fmaf(v, v, ss);
    }
  part[ty][tx] = ss;
  __syncthreads();
  if (j >= Np) return;
  const float nrm = sqrtf(part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx]);
  if (j < N && ty == 0) inv[j] = 1.f / nrm;
  for (int d = ty; d < D; d += 4) kt[(size_t)d * Np + j] = j < N ? K[(size_t)d * N + j] / nrm : 0.f;
}

// gK[d][j] = (GW[j][d] - kn[j][d] (kn[j] . GW[j])) inv[j]: the backward of the column normalisation, written back in K's
// [D][N] layout through 64 x 64 LDS tiles.  Block = 64 columns.
__global__ __launch_bounds__(256) void col_normalize_bwd_kernel(const float* __restrict__ GW, const float* __restrict__ kn,
                                                                const float* __restrict__ inv, float* __restrict__ gK,
                                                                int D, int N) {
  __shared__ float dot[64];
  __shared__ float tile[64][65];
  const int j0 = blockIdx.x * 64, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int q = 0; q < 16; ++q) {
    const int j = j0 + w * 16 + q;
    float s = 0.f;
    if (j < N)
      for (int d = lane; d < D; d += 64) s = fmaf(kn[(size_t)j * D + d], GW[(size_t)j * D + d], s);
    s = wave_sum(s);
    if (lane == 0) dot[w * 16 + q] = s;
  }
  __syncthreads();
  for (int d0 = 0; d0 < D; d0 += 64) {
    for (int jj = w; jj < 64; jj += 4) {
      const int j = j0 + jj, d = d0 + lane;
      float v = 0.f;
      if (j < N && d < D) v = (GW[(size_t)j * D + d] - kn[(size_t)j * D + d] * dot[jj]) * inv[j];
      tile[jj][lane] = v;
    }
    __syncthreads();
    for (int dd = w; dd < 64; dd += 4) {
      const int d = d0 + dd, j = j0 + lane;
      if (d < D && j < N) gK[(size_t)d * N + j] = tile[lane][dd];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ CurricularFace
// head/metrics.py:494-509 on the raw cosines of the FR_EPI_STORE GEMM.  rowv is [4][rows]: tl = clamp(cos[label]),
// ctm = cos(theta_tl + m), final (the label column's value) and flag (1: the ctm branch, 0: tl - mm).  A row whose label
// lies outside [0, N) has no target: tl counts as 0.
constexpr float CURR_MOMENTUM = 0.01f;  // t <- 0.01 mean(tl) + (1 - 0.01) t  (:506)

// the row values of one target cosine, shared by the two row kernels below
__device__ __forceinline__ void curricular_row_values(float tl, int i, int rows, float* __restrict__ rowv, float cos_m,
                                                      float sin_m, float th, float mm) {
  const float ctm = tl * cos_m - sqrtf(1.0f - tl * tl) * sin_m;
  const bool first = tl > th;
  rowv[i] = tl;
  rowv[rows + i] = ctm;
  rowv[2 * rows + i] = first ? ctm : tl - mm;
  rowv[3 * rows + i] = first ? 1.f : 0.f;
}

// batch mean of tl from the threads' double sums (256 threads, fixed order) and the update of t; both row kernels end here
__device__ __forceinline__ void curricular_mean_update(double s, double* dred, float* __restrict__ mean,
                                                       float* __restrict__ t, int rows, int train) {
  block_put(dred, wave_sum_d(s));
  if (threadIdx.x == 0) {
    const float mu = (float)(waves_sum<4>(dred) / rows);
    mean[0] = mu;
    if (train) t[0] = __fadd_rn(__fmul_rn(mu, CURR_MOMENTUM), __fmul_rn(1.0f - CURR_MOMENTUM, t[0]));
  }
}

// one workgroup: the batch mean of tl is added in a fixed order in double (as focal_finalize_kernel), so t is reproducible
__global__ __launch_bounds__(256) void curricular_rows_kernel(const float* __restrict__ cos,
                                                              const long long* __restrict__ label,
                                                              float* __restrict__ rowv, float* __restrict__ mean,
                                                              float* __restrict__ t, int rows, int N, int ld, float cos_m,
                                                              float sin_m, float th, float mm, int train) {
  __shared__ double dred[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const long long lab = label[i];
    const float tl = (lab >= 0 && lab < N) ? clamp1(cos[(size_t)i * ld + lab]) : 0.f;
    curricular_row_values(tl, i, rows, rowv, cos_m, sin_m, th, mm);
    s += (double)tl;
  }
  curricular_mean_update(s, dred, mean, t, rows, train);
}

// the same from given target cosines: the class-sharded head gathers them per shard (shard_target_cos_kernel) and sums
// them over the ranks, so every rank runs this over the global batch and ends with the same rowv and t
__global__ __launch_bounds__(256) void curricular_rows_from_kernel(const float* __restrict__ tlv, float* __restrict__ rowv,
                                                                   float* __restrict__ mean, float* __restrict__ t,
                                                                   int rows, float cos_m, float sin_m, float th, float mm,
                                                                   int train) {
  __shared__ double dred[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const float tl = tlv[i];
    curricular_row_values(tl, i, rows, rowv, cos_m, sin_m, th, mm);
    s += (double)tl;
  }
  curricular_mean_update(s, dred, mean, t, rows, train);
}

// tl[i] = clamp(cos[i][label_local[i]]) where this shard owns the label, +0 elsewhere: one rank owns each label, so the sum
// of the ranks' tl is exact in any order
__global__ __launch_bounds__(256) void shard_target_cos_kernel(const float* __restrict__ cos,
                                                               const long long* __restrict__ label,
                                                               float* __restrict__ tl, int rows, int N, int ld) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const long long lab = label[i];
  tl[i] = (lab >= 0 && lab < N) ? clamp1(cos[(size_t)i * ld + lab]) : 0.f;
}

// t <- 0.01 (scale * mean) + 0.99 t: the update of curricular_rows_kernel from a mean summed over the ranks
__global__ void curricular_ema_kernel(float* __restrict__ t, const float* __restrict__ mean, float scale) {
  if (threadIdx.x == 0)
    t[0] = __fadd_rn(__fmul_rn(__fmul_rn(mean[0], scale), CURR_MOMENTUM), __fmul_rn(1.0f - CURR_MOMENTUM, t[0]));
}

// out = s * (label ? final : (c > ctm ? c (t + c) : c)), c = clamp(cos)
__global__ __launch_bounds__(256) void curricular_apply_kernel(const float* __restrict__ cos,
                                                               const long long* __restrict__ label,
                                                               const float* __restrict__ rowv, const float* __restrict__ t,
                                                               float* __restrict__ out, int rows, int N, int ld, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float ctm = rowv[rows + row], fin = rowv[2 * rows + row], tt = t[0];
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float raw) {
      const float c = clamp1(raw);
      float v = c > ctm ? c * (tt + c) : c;
      if (n == lab) v = fin;
      return v * s;
    });
  });
}

// gcos = g * d out / d cos with t, the hard mask and the branch flags constant: s (t + 2c) on hard negatives, s on easy
// ones, s (cos_m + sin_m tl / sqrt(1 - tl^2)) or s on the label column
__global__ __launch_bounds__(256) void curricular_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                             const long long* __restrict__ label,
                                                             const float* __restrict__ rowv, const float* __restrict__ t,
                                                             float* __restrict__ gcos, int rows, int N, int ld, int ldg,
                                                             float cos_m, float sin_m, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float tl = rowv[row], ctm = rowv[rows + row], tt = t[0];
    const float dlab = rowv[3 * rows + row] != 0.f ? cos_m + sin_m * tl / sqrtf(1.0f - tl * tl) : 1.f;
    margin_cols_bwd(g, cos, gcos, row, N, ld, ldg, [&](int n, float raw, float gg) {
      const float c = clamp1(raw);
      float d = c > ctm ? tt + 2.f * c : 1.f;
      if (n == lab) d = dlab;
      return gg * s * d;
    });
  });
}

// ------------------------------------------------------------------------------------------ MagFace
// head/metrics.py:533-552 on the raw cosines of the FR_EPI_STORE GEMM.  rowv is [6][rows]: a = clamp(||x||, l_a, u_a),
// cos_m = cos(m(a)), sin_m = sin(m(a)), min_cos = cos(pi - m(a)), loss_g = lamda (a / u_a^2 + 1 / a) and inside (1: the
// clamp passes gradient, l_a <= ||x|| <= u_a).  ||x|| is recomputed from x, one wave per row, summed in double in a fixed
// order: a is the correctly rounded norm, and 1 / u_a^2 - 1 / a^2 of the backward pass cancels up to 3x near u_a.
__global__ __launch_bounds__(256) void magface_rows_kernel(const float* __restrict__ x, float* __restrict__ rowv, int rows,
                                                           int D, float l_a, float u_a, float l_margin, float u_margin,
                                                           float lamda) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= rows) return;
  const float* xr = x + (size_t)i * D;
  double ss = 0.0;
  if (D % 4 == 0) {
    for (int d = lane * 4; d < D; d += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + d);
#pragma unroll
      for (int j = 0; j < 4; ++j) ss += (double)v[j] * (double)v[j];
    }
  } else {
    for (int d = lane; d < D; d += 64) ss += (double)xr[d] * (double)xr[d];
  }
  ss = wave_sum_d(ss);
  if (lane != 0) return;
  const float nrm = (float)sqrt(ss);
  const float a = nrm < l_a ? l_a : (nrm > u_a ? u_a : nrm);  // torch.clamp: NaN passes
  const float m = (u_margin - l_margin) / (u_a - l_a) * (a - l_a) + l_margin;
  rowv[i] = a;
  rowv[rows + i] = cosf(m);
  rowv[2 * rows + i] = sinf(m);
  rowv[3 * rows + i] = cosf(3.14159265358979323846f - m);
  rowv[4 * rows + i] = lamda * (float)((double)a / ((double)u_a * u_a) + 1.0 / (double)a);
  rowv[5 * rows + i] = (nrm >= l_a && nrm <= u_a) ? 1.f : 0.f;
}

// out = s * (label ? (c > min_cos ? c cos_m - sqrt(1 - c^2) sin_m : c - margin_am) : c), c = clamp(cos)
__global__ __launch_bounds__(256) void magface_apply_kernel(const float* __restrict__ cos,
                                                            const long long* __restrict__ label,
                                                            const float* __restrict__ rowv, float* __restrict__ out,
                                                            int rows, int N, int ld, float s, float margin_am) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float cos_m = rowv[rows + row], sin_m = rowv[2 * rows + row], min_cos = rowv[3 * rows + row];
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float raw) {
      const float c = clamp1(raw);
      float v = c;
      if (n == lab) v = c > min_cos ? c * cos_m - sqrtf(1.0f - c * c) * sin_m : c - margin_am;
      return v * s;
    });
  });
}

// gcos = g * d out / d cos: s, and s (cos_m + sin_m c / sqrt(1 - c^2)) on the label column in the margin branch.  The wave
// whose column chunk holds the label (chunk 0 when no column is selected) also writes the row's radial scalar
// r = inside (g[label] s (-(sqrt(1 - c^2) cos_m + c sin_m)) dm/da [margin branch] + glossg lamda (1 / u_a^2 - 1 / a^2)):
// d loss / d ||x|| through the margin and through loss_g, one writer per row, no sum.
__global__ __launch_bounds__(256) void magface_bwd_kernel(const float* __restrict__ g, const float* __restrict__ glossg,
                                                          const float* __restrict__ cos, const long long* __restrict__ label,
                                                          const float* __restrict__ rowv, float* __restrict__ gcos,
                                                          float* __restrict__ r, int rows, int N, int ld, int ldg, float s,
                                                          float slope, double inv_ua2, float lamda) {
  walk_row(label, rows, N, [&](int row, long long lab, bool has) {
    const float cos_m = rowv[rows + row], sin_m = rowv[2 * rows + row], min_cos = rowv[3 * rows + row];
    margin_cols_bwd(g, cos, gcos, row, N, ld, ldg, [&](int n, float raw, float gg) {
      const float c = clamp1(raw);
      float d = 1.f;
      if (n == lab && c > min_cos) d = cos_m + sin_m * c / sqrtf(1.0f - c * c);
      return gg * s * d;
    });
    const int owner = has ? (int)((unsigned)lab / MARGIN_COLS) : 0;  // has: 0 <= lab < N, an int
    if ((int)blockIdx.x == owner && (threadIdx.x & 63) == 0) {
      const float a = rowv[row];
      float v = 0.f;
      if (has) {
        const float c = clamp1(cos[(size_t)row * ld + lab]);
        if (c > min_cos) v = g[(size_t)row * N + lab] * s * (-(sqrtf(1.0f - c * c) * cos_m + c * sin_m)) * slope;
      }
      if (glossg) v += glossg[row] * lamda * (float)(inv_ua2 - 1.0 / ((double)a * a));
      r[row] = rowv[5 * rows + row] != 0.f ? v : 0.f;
    }
  });
}

// ------------------------------------------------------------------------------------------ AdaCos
// head/metrics.py:359-368 on the raw cosines of the FR_EPI_STORE GEMM.  The scale is a one-float device buffer: the row
// kernel reads the old value inside exp, one workgroup turns the row values into the new one and writes it (the only
// writer), and the apply kernel reads that.  rowv is [2][rows]: the row's sum of exp(scale * cos) over the columns that
// are not its label, and its raw target cosine, ADACOS_NO_TARGET where the label lies outside [0, N).
constexpr float ADACOS_NO_TARGET = 2.0f;  // no cosine reaches it

// One workgroup of 1024 threads per row (a whole-row reduction: one wave per row would leave 256 waves on the chip at batch
// 256; sixteen per row keep enough loads in flight).  Order of the sum, fixed: thread t adds its columns 4t .. 4t+3,
// 4t+4096 .. in ascending order in double, the 64 lanes of a wave go through wave_sum_d's xor butterfly, and thread 0 adds
// the sixteen waves' sums in wave order.
constexpr int ADACOS_ROW_THREADS = 1024;

__global__ __launch_bounds__(ADACOS_ROW_THREADS) void adacos_rows_kernel(const float* __restrict__ cos, const long long* __restrict__ label,
                                                          const float* __restrict__ scale, float* __restrict__ rowv,
                                                          int rows, int N, int ld) {
  __shared__ double dred[ADACOS_ROW_THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long lab = label[row];
  const float s = scale[0];
  const float* crow = cos + (size_t)row * ld;
  double acc = 0.0;
  for (int n = tid * 4; n < N; n += 4 * ADACOS_ROW_THREADS) {  // n + 3 < ld: n < N <= ld, both multiples of 4
    const f32x4 ch = *reinterpret_cast<const f32x4*>(crow + n);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (n + j < N && n + j != lab) acc += (double)expf(s * ch[j]);  // the raw cosine, no clamp (:363)
  }
  block_put(dred, wave_sum_d(acc));
  if (tid == 0) {
    rowv[row] = (float)waves_sum<ADACOS_ROW_THREADS / 64>(dred);
    rowv[rows + row] = (lab >= 0 && lab < N) ? crow[lab] : ADACOS_NO_TARGET;
  }
}

// One workgroup: B_avg = sum(rowv[0]) / rows in double in a fixed order (thread t adds rows t, t + 256, .., then as
// above), and the lower median of the target angles = the angle of the target cosine at descending rank (n - 1) / 2 among
// the n rows that have one (acos falls, so the order statistic is taken on the cosines).  Rank of row i: the number of rows j with c_j > c_i, or c_j == c_i and j < i -- a permutation
// of 0 .. n-1, so exactly one row has the wanted rank; found by counting through 256-float LDS tiles, no sort and no
// storage that grows with rows.  A NaN target cosine makes the scale NaN (torch.median propagates it).  rows without a
// target enter B_avg (their whole row is in rowv[0]) and not the median; with none that has one the scale stays.
__global__ __launch_bounds__(256) void adacos_scale_kernel(const float* __restrict__ rowv, int rows,
                                                           float* __restrict__ scale) {
  __shared__ double dred[4];
  __shared__ float tile[256];
  __shared__ int nred[4], bad[4];
  __shared__ float sel;
  const int tid = threadIdx.x;
  const float* tc = rowv + rows;
  double acc = 0.0;
  int cnt = 0, isn = 0;
  for (int i = tid; i < rows; i += 256) {
    acc += (double)rowv[i];
    const float c = tc[i];
    cnt += c != ADACOS_NO_TARGET;
    isn |= c != c;
  }
  acc = wave_sum_d(acc);
  const int wcnt = (int)wave_sum((float)cnt);  // cnt <= rows / 256 + 1 per thread: exact in fp32 below 2^24 rows
  const int wnan = __any(isn);
  block_put(dred, acc, nred, wcnt, bad, wnan);
  const int n = waves_sum<4>(nred);
  if (n == 0) return;  // no row has a target: the scale stays (uniform over the workgroup)
  const int want = (n - 1) / 2;
  for (int base = 0; base < rows; base += 256) {
    const int i = base + tid;
    const float ci = i < rows ? tc[i] : ADACOS_NO_TARGET;
    int rank = 0;
    for (int jb = 0; jb < rows; jb += 256) {
      __syncthreads();
      tile[tid] = jb + tid < rows ? tc[jb + tid] : ADACOS_NO_TARGET;
      __syncthreads();
      const int jn = min(256, rows - jb);
      for (int jj = 0; jj < jn; ++jj) {
        const float cj = tile[jj];
        rank += cj != ADACOS_NO_TARGET && (cj > ci || (cj == ci && jb + jj < i));
      }
    }
    if (ci != ADACOS_NO_TARGET && rank == want) sel = ci;
  }
  __syncthreads();
  if (tid == 0) {
    const double b_avg = waves_sum<4>(dred) / rows;
    const float lo = (float)(-1.0 + 1e-7), hi = (float)(1.0 - 1e-7);  // the clamp of :359 on fp32 cosines
    const float c = sel < lo ? lo : (sel > hi ? hi : sel);
    // cos(min(pi/4, acos(c))) = max(cos(pi/4), c): cos falls on [0, pi], so neither the angle nor its cosine is formed
    float v = (float)(log(b_avg) / fmax(0.70710678118654752440, (double)c));
    if (bad[0] | bad[1] | bad[2] | bad[3]) v = __builtin_nanf("");
    scale[0] = v;
  }
}

// out[m][n] = scale[0] * src[m][n] for n < N, 0 in the padding columns [N, ld_out): the logits from the raw cosines
// (:368, the NEW scale times the unclamped cosine) and gcos from g (the scale is a constant of the graph).  One wave per
// row, four rows per workgroup, 1024 columns per block as the margin walkers; src is read as f32x4 where its pitch allows.
__global__ __launch_bounds__(256) void adacos_apply_kernel(const float* __restrict__ src, const float* __restrict__ scale,
                                                           float* __restrict__ out, int rows, int N, int ld_src,
                                                           int ld_out) {
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float s = scale[0];
  const float* srow = src + (size_t)row * ld_src;
  float* orow = out + (size_t)row * ld_out;
  const bool vec = ld_src % 4 == 0;
  const int end = min(ld_out, (int)(blockIdx.x + 1) * MARGIN_COLS);
  for (int n = blockIdx.x * MARGIN_COLS + lane * 4; n < end; n += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      if (n < ld_src) v = *reinterpret_cast<const f32x4*>(srow + n);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (n + j < N) v[j] = srow[n + j];
    }
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = n + j < N ? __fmul_rn(s, v[j]) : 0.f;
    *reinterpret_cast<f32x4*>(orow + n) = o;
  }
}

// ------------------------------------------------------------------------------------------ NPCFace
// head/metrics.py:616-635 on the raw cosines of the FR_EPI_STORE GEMM.  rowv is [6][rows]: gt = clamp(cos[label]),
// ctm = cos(theta_gt + margin), final (the label column's value), d final / d gt, avg (the mean of the row's hard
// negatives) and their count as a float (exact up to 2^24).  A row whose label lies outside [0, N) has no target: gt counts
// as 0 and ctm is +inf, so nothing in it is hard.

// One workgroup of 1024 threads per row, as adacos_rows_kernel (a whole-row reduction).  Order of the sum, fixed: thread t
// adds the hard cosines among its columns 4t .. 4t+3, 4t+4096 .. in ascending order in double, the 64 lanes of a wave go
// through wave_sum_d's xor butterfly, and thread 0 adds the sixteen waves' sums in wave order.  The count is an integer.
constexpr int NPCFACE_ROW_THREADS = 1024;

__global__ __launch_bounds__(NPCFACE_ROW_THREADS) void npcface_rows_kernel(const float* __restrict__ cos,
                                                                           const long long* __restrict__ label,
                                                                           float* __restrict__ rowv, int rows, int N, int ld,
                                                                           float cos_m, float sin_m, float m0, float m1) {
  __shared__ double dred[NPCFACE_ROW_THREADS / 64];
  __shared__ int nred[NPCFACE_ROW_THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long lab = label[row];
  const bool has = lab >= 0 && lab < N;
  const float* crow = cos + (size_t)row * ld;
  const float gt = has ? clamp1(crow[lab]) : 0.f;
  const float sn = sqrtf(1.0f - gt * gt);
  const float ctm = has ? gt * cos_m - sn * sin_m : __builtin_inff();
  double acc = 0.0;
  int cnt = 0;
  for (int n = tid * 4; n < N; n += 4 * NPCFACE_ROW_THREADS) {  // n + 3 < ld: n < N <= ld, both multiples of 4
    const f32x4 ch = *reinterpret_cast<const f32x4*>(crow + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c = clamp1(ch[j]);
      if (n + j < N && n + j != lab && c > ctm) {  // the label column is taken out of the mask (:623)
        acc += (double)c;
        ++cnt;
      }
    }
  }
  acc = wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  block_put(dred, acc, nred, cnt);
  if (tid == 0) {
    const double sum = waves_sum<NPCFACE_ROW_THREADS / 64>(dred);
    const int count = waves_sum<NPCFACE_ROW_THREADS / 64>(nred);
    const float avg = (float)(sum / (double)max(count, 1));  // clamp(count, 1, num_class) (:627): count <= N - 1
    const float newm = m0 + m1 * avg;
    const float cn = cosf(newm), sm = sinf(newm);
    const bool pos = gt > 0.f;
    rowv[row] = gt;
    rowv[rows + row] = ctm;
    rowv[2 * rows + row] = pos ? gt * cn - sn * sm : gt;
    rowv[3 * rows + row] = pos ? cn + sm * gt / sn : 1.f;
    rowv[4 * rows + row] = avg;
    rowv[5 * rows + row] = (float)count;
  }
}

// out = s * (label ? final : (c > ctm ? t c + a : c)), c = clamp(cos)
__global__ __launch_bounds__(256) void npcface_apply_kernel(const float* __restrict__ cos,
                                                            const long long* __restrict__ label,
                                                            const float* __restrict__ rowv, float* __restrict__ out,
                                                            int rows, int N, int ld, float t, float a, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float ctm = rowv[rows + row], fin = rowv[2 * rows + row];
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float raw) {
      const float c = clamp1(raw);
      float v = c > ctm ? t * c + a : c;
      if (n == lab) v = fin;
      return v * s;
    });
  });
}

// gcos = g * d out / d cos with newm, the hard mask and the branch constant: s t on hard negatives, s on easy ones,
// s * rowv[3] (cos(newm) + sin(newm) gt / sqrt(1 - gt^2), or 1) on the label column
__global__ __launch_bounds__(256) void npcface_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                          const long long* __restrict__ label,
                                                          const float* __restrict__ rowv, float* __restrict__ gcos, int rows,
                                                          int N, int ld, int ldg, float t, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float ctm = rowv[rows + row], dlab = rowv[3 * rows + row];
    margin_cols_bwd(g, cos, gcos, row, N, ld, ldg, [&](int n, float raw, float gg) {
      const float c = clamp1(raw);
      float d = c > ctm ? t : 1.f;
      if (n == lab) d = dlab;
      return gg * s * d;
    });
  });
}

// ------------------------------------------------------------------------------------------ MV_Softmax
// head/metrics.py:571-590 on the raw cosines of the FR_EPI_STORE GEMM; the head never clamps.  Its per-row values depend on
// the target cosine alone, so there is no rows launch: every wave of mv_softmax_apply_kernel loads its row's target cosine
// (one address per wave) and derives the same bits, and the wave of column chunk 0 leaves them in rowv [4][rows] for the
// backward pass: gt, thr, final, d final / d gt.  is_am: thr = gt - p0 (p0 = margin), final = gt > p0 ? thr : gt, slope 1.
// Otherwise (p0, p1) = (cos_m, sin_m): thr = gt p0 - sqrt(1 - gt^2) p1, final = gt > 0 ? thr : gt, slope p0 + p1 gt / sqrt(..)
// or 1; |gt| > 1 makes thr NaN, unguarded as in the reference (no column is hard then).  A row whose label lies outside
// [0, N) has no target: 0, +inf, 0, 0.
struct MvRow {
  float gt, thr, fin, dfin;
};

__device__ __forceinline__ MvRow mv_softmax_row(const float* __restrict__ crow, long long lab, bool has, int is_am, float p0,
                                                float p1) {
  MvRow r = {0.f, __builtin_inff(), 0.f, 0.f};
  if (!has) return r;
  const float gt = crow[lab];
  r.gt = gt;
  if (is_am) {
    r.thr = gt - p0;
    r.fin = gt > p0 ? r.thr : gt;
    r.dfin = 1.f;
  } else {
    const float sn = sqrtf(1.0f - gt * gt);
    r.thr = gt * p0 - sn * p1;
    r.fin = gt > 0.f ? r.thr : gt;
    r.dfin = gt > 0.f ? p0 + p1 * gt / sn : 1.f;
  }
  return r;
}

// out = s * (label ? final : (c > thr ? w c + w - 1 : c)), c the raw cosine
__global__ __launch_bounds__(256) void mv_softmax_apply_kernel(const float* __restrict__ cos,
                                                               const long long* __restrict__ label,
                                                               float* __restrict__ rowv, float* __restrict__ out, int rows,
                                                               int N, int ld, int is_am, float p0, float p1, float w,
                                                               float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool has) {
    const MvRow r = mv_softmax_row(cos + (size_t)row * ld, lab, has, is_am, p0, p1);
    chunk0_store(rowv, rows, row, {r.gt, r.thr, r.fin, r.dfin});
    const float thr = r.thr, fin = r.fin, w1 = w - 1.0f;
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float c) {
      float v = c > thr ? w * c + w1 : c;
      if (n == lab) v = fin;
      return v * s;
    });
  });
}

// gcos = g * d out / d cos with the hard mask and the branch constant: s w on hard negatives, s on easy ones,
// s * rowv[3] on the label column; no clamp, so no pass mask
__global__ __launch_bounds__(256) void mv_softmax_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                             const long long* __restrict__ label,
                                                             const float* __restrict__ rowv, float* __restrict__ gcos,
                                                             int rows, int N, int ld, int ldg, float w, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    const float thr = rowv[rows + row], dlab = rowv[3 * rows + row];
    margin_cols_bwd<false>(g, cos, gcos, row, N, ld, ldg, [&](int n, float c, float gg) {
      float d = c > thr ? w : 1.f;
      if (n == lab) d = dlab;
      return gg * s * d;
    });
  });
}

// ------------------------------------------------------------------------------------------ ArcNegFace
// head/metrics.py:413-433 on the raw cosines of the FR_EPI_STORE GEMM; the head never clamps.  The reference fills its
// logits in a loop over the rows with two host reads per row; each row's values depend on its target cosine alone, so, as
// for MV_Softmax, there is no rows launch: every wave of arcneg_apply_kernel loads its row's target cosine (one address per
// wave) and derives the same bits, and the wave of column chunk 0 leaves them in rowv [3][rows] for the backward pass: gt,
// a, d a / d gt.  gt > thresh: a = cos(acos(gt) + margin), slope sin(acos(gt) + margin) / sqrt(1 - gt^2); otherwise a =
// gt - mm, slope 1.  Unguarded as in the reference: gt > 1 makes acos, a and with them every t of the row NaN.  A row whose
// label lies outside [0, N) has no target: 0, 0, 0, and its t is exactly 1 (the reference's initial a and t_scale).
struct ArcNegRow {
  float gt, a, da;
};

__device__ __forceinline__ ArcNegRow arcneg_row(const float* __restrict__ crow, long long lab, bool has, float thresh,
                                                float margin, float mm) {
  ArcNegRow r = {0.f, 0.f, 0.f};
  if (!has) return r;
  const float gt = crow[lab];
  r.gt = gt;
  if (gt > thresh) {
    const float th = acosf(gt) + margin;
    r.a = cosf(th);
    r.da = sinf(th) / sqrtf(1.0f - gt * gt);
  } else {
    r.a = gt - mm;
    r.da = 1.f;
  }
  return r;
}

// t of a raw cosine, detached in the reference (:431-432): alpha * exp(-(c - a)^2 / sigma), nis = -1 / sigma.  At B = 256,
// N = 28 000 the apply kernel runs at about 5 TB/s, so the arithmetic per element shows in its time: with expf and an fp32
// division it took 13.4 us against mv_softmax_apply's 10.9 us; one multiply in place of the division (the same bits for
// sigma = 2) and __expf (the hardware exp2; its argument lies in about [-2.5, 0] for cosines within +-1) bring it to 11.3 us
// with the same measured errors (profiles/arcnegface_head_b256_n28000.txt).
__device__ __forceinline__ float arcneg_t(float c, float a, float alpha, float nis) {
  const float d = c - a;
  return alpha * __expf(d * d * nis);
}

// out = s * (label ? a : t c + t - 1), c the raw cosine; a row without a target: out = s * c
__global__ __launch_bounds__(256) void arcneg_apply_kernel(const float* __restrict__ cos, const long long* __restrict__ label,
                                                           float* __restrict__ rowv, float* __restrict__ out, int rows,
                                                           int N, int ld, float thresh, float margin, float mm,
                                                           float alpha, float sigma, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool has) {
    const ArcNegRow r = arcneg_row(cos + (size_t)row * ld, lab, has, thresh, margin, mm);
    chunk0_store(rowv, rows, row, {r.gt, r.a, r.da});
    const float a = r.a, nis = -1.0f / sigma;
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float c) {
      float v = c;
      if (has) {
        const float t = arcneg_t(c, a, alpha, nis);
        v = n == lab ? a : t * c + t - 1.0f;
      }
      return v * s;
    });
  });
}

// gcos = g * s * (label ? d a / d gt : t), t recomputed from the raw cosine and rowv[1] (no [B, N] buffer of t is kept); t
// and the branch are constants of the graph; no clamp, so no pass mask.  A row without a target: gcos = g * s
__global__ __launch_bounds__(256) void arcneg_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                         const long long* __restrict__ label,
                                                         const float* __restrict__ rowv, float* __restrict__ gcos, int rows,
                                                         int N, int ld, int ldg, float alpha, float sigma, float s) {
  walk_row(label, rows, N, [&](int row, long long lab, bool has) {
    const float a = rowv[rows + row], dlab = rowv[2 * rows + row], nis = -1.0f / sigma;
    margin_cols_bwd<false>(g, cos, gcos, row, N, ld, ldg, [&](int n, float c, float gg) {
      float d = 1.f;
      if (has) d = n == lab ? dlab : arcneg_t(c, a, alpha, nis);
      return gg * s * d;
    });
  });
}

// ------------------------------------------------------------------------------------------ CircleLoss
// head/metrics.py:451-473 on the raw cosines of the FR_EPI_STORE GEMM.  Element-wise after the clamp: no row values, no
// rows launch.  The operations keep the reference's fp32 order, each rounded on its own (O_p - c, the clamp at 0, c - delta_p,
// the product, then * gamma), so the result has the bits of the torch expression on the same cosines; the clamps are
// comparisons and let NaN through, as torch.clamp and torch.clamp_min do (fmaxf would not).
__device__ __forceinline__ float clamp_min0(float a) { return a < 0.f ? 0.f : a; }

// alpha of a clamped cosine, detached in the reference: clamp_min(O_p - c, 0) on the label column, clamp_min(c - O_n, 0) off it
__device__ __forceinline__ float circle_alpha(float c, bool lab, float o_p, float o_n) {
  return clamp_min0(lab ? __fsub_rn(o_p, c) : __fsub_rn(c, o_n));
}

// out = gamma * (label ? alpha_p (c - delta_p) : alpha_n (c - delta_n)), c the clamped cosine; a label outside [0, N)
// matches no column: every column of its row is a negative
__global__ __launch_bounds__(256) void circle_apply_kernel(const float* __restrict__ cos, const long long* __restrict__ label,
                                                           float* __restrict__ out, int rows, int N, int ld, float o_p,
                                                           float o_n, float delta_p, float delta_n, float gamma) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    margin_cols_fwd(cos, out, row, N, ld, [&](int n, float raw) {
      const float c = clamp1(raw);
      const bool pos = n == lab;
      const float alpha = circle_alpha(c, pos, o_p, o_n);
      return __fmul_rn(__fmul_rn(alpha, __fsub_rn(c, pos ? delta_p : delta_n)), gamma);
    });
  });
}

// gcos = (g gamma) alpha where the clamp at +-1 passes (the walker's mask), alpha recomputed from the raw cosine: autograd's
// order, since alpha is a constant of the graph and d (alpha (c - delta)) / dc = alpha
__global__ __launch_bounds__(256) void circle_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                         const long long* __restrict__ label, float* __restrict__ gcos,
                                                         int rows, int N, int ld, int ldg, float o_p, float o_n,
                                                         float gamma) {
  walk_row(label, rows, N, [&](int row, long long lab, bool) {
    margin_cols_bwd(g, cos, gcos, row, N, ld, ldg, [&](int n, float raw, float gg) {
      return __fmul_rn(__fmul_rn(gg, gamma), circle_alpha(clamp1(raw), n == lab, o_p, o_n));
    });
  });
}

// ------------------------------------------------------------------------------------------ cross entropy rows
// The label's rank, shared by ce_rows_kernel, rank_rows_kernel and shard_rank_rows_kernel: a column counts unless it is
// <= the label's logit.  On finite data that is z[n] > z[label] (a tie does not count against the label).  A NaN counts as
// above the label wherever it stands, as torch.topk orders it, and a NaN label logit is below every column: rank N.  A
// label outside [0, N) is given a NaN logit, so its row is never a hit (the reference's pred.eq(target) finds no match).
__device__ __forceinline__ int ranks_above(float v, float zl) { return !(v <= zl) ? 1 : 0; }

// ce = lse - z[label] as log(S) - (z[label] - mx): with a confident label (z[label] = mx, or near it) the second term is
// exact or small and ce keeps the relative error of log(S); (mx + logf(S)) - z[label] rounds the sum to an ulp of mx
// first, which is an absolute error of 2e-6 at mx = 64 on a ce of 1e-3 (profiles/ce_rows_error.txt).  There S = 1 + ce, so
// an ulp of S is a relative error of 1e-7 / ce in ce: for ce, S is added a second time in double in a fixed order (thread t
// adds its columns t, t + 256, .. in ascending order, the xor butterfly, the four waves in order; the fp32 sum carries the 1
// of the leading column through nine roundings), and log(S) = logf(Sf) + (S - Sf) / S takes the rounding of S to fp32 back
// out.  lse = mx + logf(the fp32 sum) keeps the bits it always had: focal_bwd_kernel forms the gradient from it, and a
// training run in bf16 amplifies a changed last bit of a gradient within tens of steps.  A label outside [0, N): ce = lse.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ z, const long long* __restrict__ label,
                                                      float* __restrict__ lse, float* __restrict__ ce,
                                                      int* __restrict__ rank, int N, int ld) {
  __shared__ float sred[4];
  __shared__ double dred[4];
  __shared__ int ired[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* row = z + (size_t)m * ld;
  const long long lab = label[m];
  const bool has = lab >= 0 && lab < N;
  const float zl = has ? row[lab] : __builtin_nanf("");
  float mx = -INFINITY;
  int cnt = 0;
  for (int n = tid; n < N; n += 256) {
    const float v = row[n];
    mx = fmaxf(mx, v);
    cnt += ranks_above(v, zl);
  }
  block_put(sred, wave_max(mx));
  mx = waves_max4(sred);
  __syncthreads();
  float se = 0.f;
  double sd = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float e = __expf(row[n] - mx);
    se += e;
    sd += (double)e;
  }
  se = wave_sum(se);
  sd = wave_sum_d(sd);
  float fc = wave_sum((float)cnt);
  block_put(sred, se, dred, sd, ired, (int)fc);
  if (tid == 0) {
    const float l = mx + logf(waves_sum<4>(sred));
    const double S = waves_sum<4>(dred);
    const float Sf = (float)S;
    const float ls = logf(Sf) + (float)((S - (double)Sf) / S);
    lse[m] = l;
    ce[m] = has ? ls - (zl - mx) : l;
    rank[m] = waves_sum<4>(ired);
  }
}

// What the two finalize kernels share (one workgroup of 256 threads): l = the batch mean of ce, added in double in a fixed
// order (thread t adds rows t, t + 256, .., the xor butterfly, the four waves in order), and the top-1 / top-5 counts.
// Thread 0 calls head(l), which writes scalars[0..1] (the loss and the slope focal_bwd_kernel multiplies by), and leaves
// precision@1, precision@5 and l in scalars[2..4].
template <typename Head>
__device__ __forceinline__ void loss_finalize(const float* __restrict__ ce, const int* __restrict__ rank, int rows,
                                              float* __restrict__ scalars, Head head) {
  __shared__ double dred[4];
  __shared__ int r1[4], r5[4];
  const int tid = threadIdx.x;
  double s = 0.0;
  int c1 = 0, c5 = 0;
  for (int i = tid; i < rows; i += 256) {
    s += (double)ce[i];
    c1 += rank[i] < 1;
    c5 += rank[i] < 5;
  }
  s = wave_sum_d(s);
  const float f1 = wave_sum((float)c1), f5 = wave_sum((float)c5);
  block_put(dred, s, r1, (int)f1, r5, (int)f5);
  if (tid == 0) {
    const float l = (float)(waves_sum<4>(dred) / rows);
    head(l);
    scalars[2] = 100.0f * (float)waves_sum<4>(r1) / rows;
    scalars[3] = 100.0f * (float)waves_sum<4>(r5) / rows;
    scalars[4] = l;
  }
}

__global__ void focal_finalize_kernel(const float* __restrict__ ce, const int* __restrict__ rank, int rows,
                                      float gamma, float* __restrict__ scalars) {
  loss_finalize(ce, rank, rows, scalars, [&](float l) {
    const float p = expf(-l);
    const float omp = 1.0f - p;
    const float w = powf(omp, gamma);
    scalars[0] = w * l;
    // d/dl [(1-p)^g * l] = g (1-p)^(g-1) p l + (1-p)^g          
    scalars[1] = gamma * powf(omp, gamma - 1.0f) * p * l + w;
  });
}

__global__ void focal_bwd_kernel(const float* __restrict__ z, const long long* __restrict__ label,
                                 const float* __restrict__ lse, const float* __restrict__ scalars,
                                 const float* __restrict__ gup, float* __restrict__ grad, int rows, int N, int ld) {
  const int m = blockIdx.y;
  const float k = gup[0] * scalars[1] / (float)rows;
  const float l = lse[m];
  const long long lab = label[m];
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    const float sm = __expf(z[(size_t)m * ld + n] - l);
    grad[(size_t)m * ld + n] = k * (sm - (n == lab ? 1.f : 0.f));
  }
}

// nn.CrossEntropyLoss() on the rows of ce_rows_kernel (train.py:237-238, :300-302): focal_finalize_kernel without the
// modulation, so scalars[4] has the same bits on the same ce; scalars[1], the slope focal_bwd_kernel multiplies by, is
// exactly 1 (focal_finalize_kernel at gamma = 0 computes 0 * powf(0, -1) = NaN there when the mean is 0).
__global__ void ce_finalize_kernel(const float* __restrict__ ce, const int* __restrict__ rank, int rows,
                                   float* __restrict__ scalars) {
  loss_finalize(ce, rank, rows, scalars, [&](float l) {
    scalars[0] = l;
    scalars[1] = 1.0f;
  });
}

// ------------------------------------------------------------------------------------------ Softmax head (linear + bias)
// head/metrics.py:12-63.  The GEMM operands of an [N][D] weight that is NOT normalised: wp [rows_pad][D] (rows >= N zero)
// and its transpose wt [D][ldt] (columns >= N zero), both written coalesced from one 64 x 64 LDS tile; biasp [rows_pad] is
// the bias with zeros behind it, so that the GEMM's bias epilogue may run over the padding columns of the logit store.
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ wp, float* __restrict__ wt,
                                                        float* __restrict__ biasp, int rows, int rows_pad, int D, int ldt) {
  __shared__ float tt[64][65];
  const int d0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int j = ty; j < 64; j += 4) {
    const int r = r0 + j, d = d0 + tx;
    const float v = (r < rows && d < D) ? w[(size_t)r * D + d] : 0.f;
    tt[j][tx] = v;
    if (r < rows_pad && d < D) wp[(size_t)r * D + d] = v;
  }
  __syncthreads();
  for (int j = ty; j < 64; j += 4) {
    const int d = d0 + j, r = r0 + tx;
    if (d < D && r < rows_pad) wt[(size_t)d * ldt + r] = tt[tx][j];
  }
  if (biasp && blockIdx.x == 0 && ty == 0 && r0 + tx < rows_pad)
    biasp[r0 + tx] = (bias && r0 + tx < rows) ? bias[r0 + tx] : 0.f;
}

// out[m][n] = n < N ? g[m][n] : 0 for n < ldo: the upstream gradient at the pitch the two gradient GEMMs read
__global__ __launch_bounds__(256) void pad_cols_kernel(const float* __restrict__ g, float* __restrict__ out, int N, int ldg,
                                                       int ldo) {
  const int m = blockIdx.y;
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < ldo; n += gridDim.x * blockDim.x)
    out[(size_t)m * ldo + n] = n < N ? g[(size_t)m * ldg + n] : 0.f;
}

// out[n] = ((g[0][n] + g[1][n]) + g[2][n]) + ...: one thread per column, the rows in order, each sum rounded to fp32 (the
// bias gradient; bit-defined, so a shard of the columns gets the bits the whole matrix gives).  Neighbouring threads read
// neighbouring columns; four loads are in flight per thread before their four additions.
__global__ __launch_bounds__(256) void col_sums_kernel(const float* __restrict__ g, int rows, int N, int ldg,
                                                       float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* p = g + n;
  float acc = p[0];
  int m = 1;
  for (; m + 4 <= rows; m += 4) {
    const float a = p[(size_t)m * ldg], b = p[(size_t)(m + 1) * ldg], c = p[(size_t)(m + 2) * ldg],
                d = p[(size_t)(m + 3) * ldg];
    acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, a), b), c), d);
  }
  for (; m < rows; ++m) acc = __fadd_rn(acc, p[(size_t)m * ldg]);
  out[n] = acc;
}

// rank-only (accuracy on arbitrary logits)
__global__ __launch_bounds__(256) void rank_rows_kernel(const float* __restrict__ z, const long long* __restrict__ label,
                                                        int* __restrict__ rank, int N, int ld) {
  __shared__ int ired[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* row = z + (size_t)m * ld;
  const long long lab = label[m];
  const float zl = (lab >= 0 && lab < N) ? row[lab] : __builtin_nanf("");
  int cnt = 0;
  for (int n = tid; n < N; n += 256) cnt += ranks_above(row[n], zl);
  block_put(ired, (int)wave_sum((float)cnt));
  if (tid == 0) rank[m] = waves_sum<4>(ired);
}

// out[j] = scale * #{m: rank[m] < k_j}: precision@k of util/utils.py:343-358 from the label ranks, one launch instead of
// four small torch kernels per k
__global__ __launch_bounds__(256) void topk_precision_kernel(const int* __restrict__ rank, int rows, int nk, int4 ks,
                                                             float scale, float* __restrict__ out) {
  __shared__ int ired[4][4];
  const int tid = threadIdx.x;
  const int kk[4] = {ks.x, ks.y, ks.z, ks.w};
  int cnt[4] = {0, 0, 0, 0};
  for (int m = tid; m < rows; m += 256) {
    const int r = rank[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] += (j < nk && r < kk[j]) ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) cnt[j] = (int)wave_sum((float)cnt[j]);  // exact: counts below 2^24
  block_put(ired[0], cnt[0], ired[1], cnt[1], ired[2], cnt[2], ired[3], cnt[3]);
  if (tid < nk) out[tid] = (float)waves_sum<4>(ired[tid]) * scale;
}

// ------------------------------------------------------------------------------------------ class-sharded softmax
// One rank holds the logits of its own contiguous class range only.  Per row it contributes (max, sum exp(z - max),
// label logit or 0); the ranks' triples are gathered and combined in rank order (shard_combine_kernel), which gives every
// rank the same log-sum-exp / cross entropy bit for bit.
__global__ __launch_bounds__(256) void shard_row_stats_kernel(const float* __restrict__ z,
                                                              const long long* __restrict__ label,
                                                              float* __restrict__ stats, int rows, int N, int ld) {
  __shared__ float sred[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* row = z + (size_t)m * ld;
  float mx = -INFINITY;
  for (int n = tid; n < N; n += 256) mx = fmaxf(mx, row[n]);
  block_put(sred, wave_max(mx));
  mx = waves_max4(sred);
  __syncthreads();
  float se = 0.f;
  for (int n = tid; n < N; n += 256) se += __expf(row[n] - mx);
  block_put(sred, wave_sum(se));
  if (tid == 0) {
    const long long lab = label[m];
    stats[m] = mx;
    stats[rows + m] = waves_sum<4>(sred);
    stats[2 * rows + m] = (lab >= 0 && lab < N) ? row[lab] : 0.f;
  }
}

__global__ void shard_combine_kernel(const float* __restrict__ stats_all, int world, int rows, float* __restrict__ lse,
                                     float* __restrict__ ce, float* __restrict__ tlogit) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= rows) return;
  float gmax = -INFINITY;
  for (int w = 0; w < world; ++w) gmax = fmaxf(gmax, stats_all[(size_t)w * 3 * rows + m]);
  float sum = 0.f, t = 0.f;
  for (int w = 0; w < world; ++w) {
    const float* s = stats_all + (size_t)w * 3 * rows;
    sum += s[rows + m] * expf(s[m] - gmax);
    t += s[2 * rows + m];  // exactly one rank owns the label, the others contribute 0
  }
  const float ls = logf(sum);
  lse[m] = gmax + ls;
  ce[m] = ls - (t - gmax);  // the order of ce_rows_kernel, on the fp32 sums the ranks sent (no double residual of S here)
  tlogit[m] = t;
}

// rank[m] = #{n in this shard: !(z[m][n] <= t[m])} (ranks_above); the ranks' counts add up to the global rank of the label
__global__ __launch_bounds__(256) void shard_rank_rows_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                              int* __restrict__ rank, int N, int ld) {
  __shared__ int ired[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* row = z + (size_t)m * ld;
  const float zl = t[m];
  int cnt = 0;
  for (int n = tid; n < N; n += 256) cnt += ranks_above(row[n], zl);
  block_put(ired, (int)wave_sum((float)cnt));
  if (tid == 0) rank[m] = waves_sum<4>(ired);
}

// ------------------------------------------------------------------------------------------ SGD
constexpr int SGD_CHUNK = 4096;

// One element of the update, shared by the dense and the row-sparse kernel so that both round alike: returns the new
// parameter and leaves the new momentum in *bv.
__device__ __forceinline__ float sgd_element(float pv, float g, float* bv, float wd, float momentum, float lr) {
  const float d = fmaf(wd, pv, g);
  const float b = fmaf(momentum, *bv, d);
  *bv = b;
  return pv - lr * b;
}

// The gradient an element's update takes under the guard's control word (fr_grad_guard): g * coef as a multiply of its own,
// rounded to fp32 -- what scaling the gradient in place would have stored -- so that no compiler folds it into the FMA
// that follows.
__device__ __forceinline__ float guard_scaled(float g, float coef) {
#pragma clang fp contract(off)
  const float s = g * coef;
  return s;
}

// One chunk of the dense step, shared by sgd_kernel and sgd_ctl_kernel so that both round alike.  SCALE is a compile-time
// false in sgd_kernel, which therefore keeps the instructions it had.
template <bool SCALE>
__device__ __forceinline__ void sgd_chunk(const FrSgdTensor* __restrict__ table, const int2* __restrict__ chunks, float lr,
                                          float momentum, float coef) {
  const int2 ch = chunks[blockIdx.x];
  const FrSgdTensor t = table[ch.x];
  const long long base = (long long)ch.y * SGD_CHUNK;
  long long end = base + SGD_CHUNK;
  if (end > t.n) end = t.n;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    const float pv = t.p[i];
    const float g = SCALE ? guard_scaled(t.g[i], coef) : t.g[i];
    float b = t.buf[i];
    const float pn = sgd_element(pv, g, &b, t.wd, momentum, lr);
    t.buf[i] = b;
    t.p[i] = pn;
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(const FrSgdTensor* __restrict__ table,
                                                  const int2* __restrict__ chunks, float lr, float momentum) {
  sgd_chunk<false>(table, chunks, lr, momentum, 1.0f);
}

// fr_sgd_step_ctl: the go flag and the coefficient come from the control word; both are uniform over the grid.
__global__ __launch_bounds__(256) void sgd_ctl_kernel(const FrSgdTensor* __restrict__ table,
                                                      const int2* __restrict__ chunks, float lr, float momentum,
                                                      const float* __restrict__ ctl, int use_coef) {
  if (ctl[2] == 0.0f) return;
  if (use_coef)
    sgd_chunk<true>(table, chunks, lr, momentum, ctl[1]);
  else
    sgd_chunk<false>(table, chunks, lr, momentum, 1.0f);
}

// The lazy update of Partial-FC v1 on the rows idx[0 .. n_s) of a dense [n][D] parameter and its momentum buffer: element
// (idx[j], d) takes sgd_element with the gradient g_rows[j][d]; no other row is read or written.  idx is ascending and
// distinct, so every element has one writer: plain stores, no atomics.  Flat over the n_s * D / V elements of the selected
// rows as cs_gather_kernel (class_sample.hip); V floats per thread and access (4: D % 4 == 0 and 16-byte aligned pointers).
// 20 bytes of HBM traffic per element (p, buf, g read; p, buf written), whatever n is.
// CTL (fr_sgd_rows_ctl): the same rows under the go flag of the gradient guard's control word -- every workgroup returns
// before it touches p or buf when ctl[2] == 0; the head's rows are not clipped.  Without CTL the argument is not read.
template <int V, bool CTL>
__global__ __launch_bounds__(256) void sgd_rows_kernel(float* __restrict__ p, float* __restrict__ buf,
                                                       const float* __restrict__ g_rows, const int32_t* __restrict__ idx,
                                                       long long total, int dv, float lr, float momentum, float wd,
                                                       const float* __restrict__ ctl) {
  if (CTL && ctl[2] == 0.0f) return;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long j = e / dv;
    const int q = (int)(e - j * dv);
    const long long at = ((long long)idx[j] * dv + q) * V;
    if (V == 4) {
      const float4 pv = *reinterpret_cast<const float4*>(p + at);
      const float4 gv = *reinterpret_cast<const float4*>(g_rows + e * 4);
      float4 bv = *reinterpret_cast<const float4*>(buf + at);
      float4 o;
      o.x = sgd_element(pv.x, gv.x, &bv.x, wd, momentum, lr);
      o.y = sgd_element(pv.y, gv.y, &bv.y, wd, momentum, lr);
      o.z = sgd_element(pv.z, gv.z, &bv.z, wd, momentum, lr);
      o.w = sgd_element(pv.w, gv.w, &bv.w, wd, momentum, lr);
      *reinterpret_cast<float4*>(buf + at) = bv;
      *reinterpret_cast<float4*>(p + at) = o;
    } else {
      float b = buf[at];
      const float o = sgd_element(p[at], g_rows[e], &b, wd, momentum, lr);
      buf[at] = b;
      p[at] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------ Adam
// Operation order of torch.optim.Adam's single-tensor path (lerp, mul + addcmul, sqrt / sqrt(bc2) + eps, addcdiv), every
// operation rounded to fp32 on its own.  Plain operators under "fp contract(off)", and sqrtf: without
// OCML_BASIC_ROUNDED_OPERATIONS the __fmul_rn / __fadd_rn of the HIP headers are plain operators that the compiler may
// still contract into an FMA, and __fsqrt_rn is the native square root, which is not correctly rounded (it was 1 ulp off in
// about 1 element of 100; tests/test_gpu_loss_optim.py holds the kernel to the np.float32 restatement bit for bit).
// One chunk, shared by adam_kernel and adam_ctl_kernel (SCALE: the gradient times the guard's coefficient first).
template <bool SCALE>
__device__ __forceinline__ void adam_chunk(const FrAdamTensor* __restrict__ table, const int2* __restrict__ chunks,
                                           float step_size, float w1, float beta2, float w2, float eps, float bc2_sqrt,
                                           float coef) {
#pragma clang fp contract(off)
  const int2 ch = chunks[blockIdx.x];
  const FrAdamTensor t = table[ch.x];
  const long long base = (long long)ch.y * SGD_CHUNK;
  long long end = base + SGD_CHUNK;
  if (end > t.n) end = t.n;
  const float neg_step = -step_size;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    const float g = SCALE ? guard_scaled(t.g[i], coef) : t.g[i];
    const float m0 = t.m[i];
    const float m = m0 + w1 * (g - m0);
    const float v = t.v[i] * beta2 + (w2 * g) * g;
    t.m[i] = m;
    t.v[i] = v;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    t.p[i] = t.p[i] + (neg_step * m) / denom;  // addcdiv: self + (value * t1) / t2
  }
}

__global__ __launch_bounds__(256) void adam_kernel(const FrAdamTensor* __restrict__ table,
                                                   const int2* __restrict__ chunks, float step_size, float w1,
                                                   float beta2, float w2, float eps, float bc2_sqrt) {
  adam_chunk<false>(table, chunks, step_size, w1, beta2, w2, eps, bc2_sqrt, 1.0f);
}

__global__ __launch_bounds__(256) void adam_ctl_kernel(const FrAdamTensor* __restrict__ table,
                                                       const int2* __restrict__ chunks, float step_size, float w1,
                                                       float beta2, float w2, float eps, float bc2_sqrt,
                                                       const float* __restrict__ ctl, int use_coef) {
  if (ctl[2] == 0.0f) return;
  if (use_coef)
    adam_chunk<true>(table, chunks, step_size, w1, beta2, w2, eps, bc2_sqrt, ctl[1]);
  else
    adam_chunk<false>(table, chunks, step_size, w1, beta2, w2, eps, bc2_sqrt, 1.0f);
}

// ------------------------------------------------------------------------------------------ gradient guard
// The sum of 256 threads' doubles in the fixed tree both guard kernels document (include/frhip.h): wave_sum_d's xor
// butterfly -- lane 0 holds the halving folds v[l] += v[l + h], h = 32 .. 1 -- then the four waves' sums in wave order.
// Valid in thread 0.
__device__ __forceinline__ double guard_block_sum(double a, double* dred) {
  block_put(dred, wave_sum_d(a));
  return waves_sum<4>(dred);
}

// parts[chunk] = sum of (double)g^2 over the chunk.  Thread t takes the elements t, t + 256, ... of the chunk in ascending
// order; 4-byte loads only, so the order and the bounds hold at any alignment.  A full chunk issues its 16 loads together.
// 4 bytes of HBM traffic per element.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const FrGradTensor* __restrict__ table,
                                                         const int2* __restrict__ chunks, double* __restrict__ parts) {
  __shared__ double dred[4];
  const int2 ch = chunks[blockIdx.x];
  const FrGradTensor t = table[ch.x];
  const long long base = (long long)ch.y * SGD_CHUNK;
  long long end = base + SGD_CHUNK;
  if (end > t.n) end = t.n;
  const float* __restrict__ g = t.g + base;
  const int len = end > base ? (int)(end - base) : 0;
  double a = 0.0;
  if (len == SGD_CHUNK) {
    float x[SGD_CHUNK / 256];
#pragma unroll
    for (int j = 0; j < SGD_CHUNK / 256; ++j) x[j] = g[j * 256 + threadIdx.x];
#pragma unroll
    for (int j = 0; j < SGD_CHUNK / 256; ++j) a += (double)x[j] * (double)x[j];
  } else {
    for (int i = threadIdx.x; i < len; i += 256) a += (double)g[i] * (double)g[i];
  }
  const double s = guard_block_sum(a, dred);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// One workgroup: total of the parts (thread t: parts[t], parts[t + 256], ... ascending, then the tree above), and thread 0
// writes the control word and the counters.
__global__ __launch_bounds__(256) void grad_guard_kernel(const double* __restrict__ parts, int nparts, float max_norm,
                                                         int skip_nonfinite, float* __restrict__ ctl,
                                                         int32_t* __restrict__ skipped) {
#pragma clang fp contract(off)
  __shared__ double dred[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += parts[i];
  const double total = guard_block_sum(a, dred);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(total);
  float coef = 1.0f;
  if (max_norm > 0.0f) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  const bool go = !(skip_nonfinite && !isfinite(total));
  ctl[0] = norm;
  ctl[1] = coef;
  ctl[2] = go ? 1.0f : 0.0f;
  ctl[3] = 0.0f;
  if (skipped) {
    if (!go) skipped[0] = skipped[0] + 1;
    skipped[1] = skipped[1] + 1;
  }
}

// ------------------------------------------------------------------------------------------ parameter moving average
// dst = a * dst + b * src: two multiplies and one add, each rounded to fp32 on its own (plain operators under "fp
// contract(off)", as adam_kernel), so the result has the bits of the np.float32 restatement.
__global__ __launch_bounds__(256) void ema_kernel(const FrEmaTensor* __restrict__ table, const int2* __restrict__ chunks,
                                                  float a, float b) {
#pragma clang fp contract(off)
  const int2 ch = chunks[blockIdx.x];
  const FrEmaTensor t = table[ch.x];
  const long long base = (long long)ch.y * SGD_CHUNK;
  long long end = base + SGD_CHUNK;
  if (end > t.n) end = t.n;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    const float keep = a * t.dst[i];
    const float take = b * t.src[i];
    t.dst[i] = keep + take;
  }
}

}  // namespace

extern "C" int fr_row_normalize(const float* x, void* xn, void* xt, float* inv, int rows, int rows_pad, int D,
                                int ldt, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int grid = (rows_pad + 3) / 4;
  const bool tiled = xt && rows_pad >= 256;  // transposed copy by a second, coalesced pass
  const dim3 tgrid((D + 63) / 64, (rows_pad + 63) / 64);
  if (dtype == FR_F32) {
    hipLaunchKernelGGL(row_normalize_kernel<float>, dim3(grid), dim3(256), 0, st, x, (float*)xn,
                       tiled ? (float*)nullptr : (float*)xt, inv, rows, rows_pad, D, ldt);
    if (tiled)
      hipLaunchKernelGGL(transpose_rows_kernel<float>, tgrid, dim3(256), 0, st, (const float*)xn, (float*)xt, rows_pad, D,
                         ldt);
  } else if (dtype == FR_BF16) {
    hipLaunchKernelGGL(row_normalize_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, x, (bf16_t*)xn,
                       tiled ? (bf16_t*)nullptr : (bf16_t*)xt, inv, rows, rows_pad, D, ldt);
    if (tiled)
      hipLaunchKernelGGL(transpose_rows_kernel<bf16_t>, tgrid, dim3(256), 0, st, (const bf16_t*)xn, (bf16_t*)xt, rows_pad,
                         D, ldt);
  } else {
    FR_UNSUPPORTED("fr_row_normalize: dtype");
  }
  FR_LAUNCH_CHECK();
}

extern "C" int fr_normalize_bwd(const float* G, const float* x, const float* inv, float* gx, int rows, int D,
                                void* stream) {
  hipLaunchKernelGGL(normalize_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, G, x, inv, gx,
                     rows, D);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_margin_bwd(const float* g, const int64_t* label, const float* cos_t, void* gcos, int rows, int N,
                             int ldg, int kind, int easy, float cos_m, float sin_m, float th, float scale, int dtype,
                             void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((ldg + 1023) / 1024, rows);
  if (dtype == FR_F32)
    hipLaunchKernelGGL(margin_bwd_kernel<float>, grid, dim3(256), 0, st, g, (const long long*)label, cos_t,
                       (float*)gcos, rows, N, ldg, kind, easy, cos_m, sin_m, th, scale);
  else if (dtype == FR_BF16)
    hipLaunchKernelGGL(margin_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, g, (const long long*)label, cos_t,
                       (bf16_t*)gcos, rows, N, ldg, kind, easy, cos_m, sin_m, th, scale);
  else
    FR_UNSUPPORTED("fr_margin_bwd: dtype");
  FR_LAUNCH_CHECK();
}

extern "C" int fr_margin_apply_parts(int ldg) { return (ldg + MARGIN_COLS - 1) / MARGIN_COLS; }

// Shape check and launch of a walker kernel for the entry point `entry` (its name opens the error text): four rows per
// workgroup, MARGIN_COLS columns per blockIdx.x of the pitch `walk` the kernel walks: gcos's ldg >= ld for a backward
// kernel; an apply kernel walks the cosines' own pitch and passes ld twice.
template <typename... P, typename... A>
static int launch_walker(const char* entry, void (*kern)(P...), void* stream, int rows, int N, int ld, int walk, A... args) {
  if (rows <= 0 || N <= 0 || ld < N || ld % 4 || walk < ld || walk % 4) {
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: shape (rows > 0, ld >= N > 0, ldg >= ld if there is one, multiples of 4)", entry);
    FR_UNSUPPORTED(msg);
  }
  hipLaunchKernelGGL(kern, dim3(fr_margin_apply_parts(walk), (rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, args...);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_margin_apply(const float* cos, const int64_t* label, const float* inv_x, float* out, int rows, int N,
                               int ld, int kind, int mi, float p0, float p1, void* stream) {
  if (kind != 2 && kind != 3) FR_UNSUPPORTED("fr_margin_apply: kind 2 (SphereFace) or 3 (Am_softmax)");
  if (kind == 2 && (mi < 0 || mi > 5)) FR_UNSUPPORTED("fr_margin_apply: SphereFace m in 0..5");
  return launch_walker("fr_margin_apply", margin_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label, inv_x,
                       out, rows, N, ld, kind, mi, p0, p1);
}

extern "C" int fr_margin_apply_bwd(const float* g, const float* cos, const int64_t* label, const float* inv_x, float* gcos,
                                   float* r_part, int rows, int N, int ld, int ldg, int kind, int mi, float p0, float p1,
                                   void* stream) {
  if (kind != 2 && kind != 3) FR_UNSUPPORTED("fr_margin_apply_bwd: kind 2 (SphereFace) or 3 (Am_softmax)");
  if (kind == 2 && (mi < 0 || mi > 5)) FR_UNSUPPORTED("fr_margin_apply_bwd: SphereFace m in 0..5");
  return launch_walker("fr_margin_apply_bwd", margin_apply_bwd_kernel, stream, rows, N, ld, ldg, g, cos,
                       (const long long*)label, inv_x, gcos, r_part, rows, N, ld, ldg, kind, mi, p0, p1);
}

extern "C" int fr_normalize_bwd_radial(const float* G, const float* x, const float* inv, const float* r_part, int nparts,
                                       float* gx, int rows, int D, void* stream) {
  if (rows <= 0 || nparts <= 0) FR_UNSUPPORTED("fr_normalize_bwd_radial: empty");
  hipLaunchKernelGGL(normalize_bwd_radial_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, G, x, inv,
                     r_part, nparts, gx, rows, D);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_col_normalize(const float* K, float* kn, float* kt, float* inv, int D, int N, int Np, void* stream) {
  if (D <= 0 || N <= 0 || Np < N) FR_UNSUPPORTED("fr_col_normalize: shape (Np >= N)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(col_normalize_kernel, dim3((Np + 63) / 64), dim3(256), 0, st, K, kt, inv, D, N, Np);
  // kn [Np][D] = kt^T: the GEMM's B operand, rows >= N zero
  hipLaunchKernelGGL(transpose_rows_kernel<float>, dim3((Np + 63) / 64, (D + 63) / 64), dim3(256), 0, st,
                     (const float*)kt, kn, D, Np, D);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_col_normalize_bwd(const float* GW, const float* kn, const float* inv, float* gK, int D, int N,
                                    void* stream) {
  if (D <= 0 || N <= 0) FR_UNSUPPORTED("fr_col_normalize_bwd: empty");
  hipLaunchKernelGGL(col_normalize_bwd_kernel, dim3((N + 63) / 64), dim3(256), 0, (hipStream_t)stream, GW, kn, inv, gK,
                     D, N);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_curricular_rows(const float* cos, const int64_t* label, float* rowv, float* mean, float* t, int rows,
                                  int N, int ld, float cos_m, float sin_m, float th, float mm, int train, void* stream) {
  if (rows <= 0 || N <= 0 || ld < N) FR_UNSUPPORTED("fr_curricular_rows: shape (rows > 0, ld >= N > 0)");
  if (train != 0 && train != 1) FR_UNSUPPORTED("fr_curricular_rows: train is 0 or 1");
  hipLaunchKernelGGL(curricular_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cos, (const long long*)label,
                     rowv, mean, t, rows, N, ld, cos_m, sin_m, th, mm, train);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_curricular_rows_from(const float* tl, float* rowv, float* mean, float* t, int rows, float cos_m,
                                       float sin_m, float th, float mm, int train, void* stream) {
  if (rows <= 0) FR_UNSUPPORTED("fr_curricular_rows_from: shape (rows > 0)");
  if (train != 0 && train != 1) FR_UNSUPPORTED("fr_curricular_rows_from: train is 0 or 1");
  hipLaunchKernelGGL(curricular_rows_from_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tl, rowv, mean, t, rows,
                     cos_m, sin_m, th, mm, train);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_curricular_ema(float* t, const float* mean, float scale, void* stream) {
  if (!(scale > 0.f)) FR_UNSUPPORTED("fr_curricular_ema: scale > 0 (1 / world size)");
  hipLaunchKernelGGL(curricular_ema_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t, mean, scale);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_curricular_apply(const float* cos, const int64_t* label, const float* rowv, const float* t, float* out,
                                   int rows, int N, int ld, float s, void* stream) {
  return launch_walker("fr_curricular_apply", curricular_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label,
                       rowv, t, out, rows, N, ld, s);
}

extern "C" int fr_curricular_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, const float* t,
                                 float* gcos, int rows, int N, int ld, int ldg, float cos_m, float sin_m, float s,
                                 void* stream) {
  return launch_walker("fr_curricular_bwd", curricular_bwd_kernel, stream, rows, N, ld, ldg, g, cos, (const long long*)label,
                       rowv, t, gcos, rows, N, ld, ldg, cos_m, sin_m, s);
}

extern "C" int fr_magface_rows(const float* x, float* rowv, int rows, int D, float l_a, float u_a, float l_margin,
                               float u_margin, float lamda, void* stream) {
  if (rows <= 0 || D <= 0) FR_UNSUPPORTED("fr_magface_rows: shape (rows > 0, D > 0)");
  if (!(l_a > 0.f && u_a > l_a)) FR_UNSUPPORTED("fr_magface_rows: 0 < l_a < u_a");
  hipLaunchKernelGGL(magface_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, rowv, rows, D, l_a,
                     u_a, l_margin, u_margin, lamda);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_magface_apply(const float* cos, const int64_t* label, const float* rowv, float* out, int rows, int N,
                                int ld, float s, float margin_am, void* stream) {
  return launch_walker("fr_magface_apply", magface_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label, rowv,
                       out, rows, N, ld, s, margin_am);
}

extern "C" int fr_magface_bwd(const float* g, const float* glossg, const float* cos, const int64_t* label,
                              const float* rowv, float* gcos, float* r, int rows, int N, int ld, int ldg, float s, float l_a,
                              float u_a, float l_margin, float u_margin, float lamda, void* stream) {
  if (!(l_a > 0.f && u_a > l_a)) FR_UNSUPPORTED("fr_magface_bwd: 0 < l_a < u_a");
  return launch_walker("fr_magface_bwd", magface_bwd_kernel, stream, rows, N, ld, ldg, g, glossg, cos,
                       (const long long*)label, rowv, gcos, r, rows, N, ld, ldg, s, (u_margin - l_margin) / (u_a - l_a),
                       1.0 / ((double)u_a * u_a), lamda);
}

extern "C" int fr_adacos_rows(const float* cos, const int64_t* label, const float* scale, float* rowv, int rows, int N,
                              int ld, void* stream) {
  if (rows <= 0 || N <= 0 || ld < N || ld % 4) FR_UNSUPPORTED("fr_adacos_rows: shape (rows > 0, ld >= N > 0, ld a multiple of 4)");
  hipLaunchKernelGGL(adacos_rows_kernel, dim3(rows), dim3(ADACOS_ROW_THREADS), 0, (hipStream_t)stream, cos, (const long long*)label, scale,
                     rowv, rows, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_adacos_scale(const float* rowv, int rows, float* scale, void* stream) {
  if (rows < 0) FR_UNSUPPORTED("fr_adacos_scale: rows >= 0");
  if (rows == 0) return 0;  // no rows: the scale stays, nothing to launch
  hipLaunchKernelGGL(adacos_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rowv, rows, scale);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_adacos_apply(const float* src, const float* scale, float* out, int rows, int N, int ld_src, int ld_out,
                               void* stream) {
  if (rows <= 0 || N <= 0 || ld_src < N || ld_out < N || ld_out % 4)
    FR_UNSUPPORTED("fr_adacos_apply: shape (ld_src >= N, ld_out >= N and a multiple of 4)");
  hipLaunchKernelGGL(adacos_apply_kernel, dim3(fr_margin_apply_parts(ld_out), (rows + 3) / 4), dim3(256), 0,
                     (hipStream_t)stream, src, scale, out, rows, N, ld_src, ld_out);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_npcface_rows(const float* cos, const int64_t* label, float* rowv, int rows, int N, int ld, float cos_m,
                               float sin_m, float m0, float m1, void* stream) {
  if (rows <= 0 || N <= 0 || ld < N || ld % 4) FR_UNSUPPORTED("fr_npcface_rows: shape (rows > 0, ld >= N > 0, ld a multiple of 4)");
  hipLaunchKernelGGL(npcface_rows_kernel, dim3(rows), dim3(NPCFACE_ROW_THREADS), 0, (hipStream_t)stream, cos,
                     (const long long*)label, rowv, rows, N, ld, cos_m, sin_m, m0, m1);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_npcface_apply(const float* cos, const int64_t* label, const float* rowv, float* out, int rows, int N,
                                int ld, float t, float a, float s, void* stream) {
  return launch_walker("fr_npcface_apply", npcface_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label, rowv,
                       out, rows, N, ld, t, a, s);
}

extern "C" int fr_npcface_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos,
                              int rows, int N, int ld, int ldg, float t, float s, void* stream) {
  return launch_walker("fr_npcface_bwd", npcface_bwd_kernel, stream, rows, N, ld, ldg, g, cos, (const long long*)label, rowv,
                       gcos, rows, N, ld, ldg, t, s);
}

extern "C" int fr_mv_softmax_apply(const float* cos, const int64_t* label, float* rowv, float* out, int rows, int N, int ld,
                                   int is_am, float p0, float p1, float w, float s, void* stream) {
  return launch_walker("fr_mv_softmax_apply", mv_softmax_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label,
                       rowv, out, rows, N, ld, is_am, p0, p1, w, s);
}

extern "C" int fr_mv_softmax_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos,
                                 int rows, int N, int ld, int ldg, float w, float s, void* stream) {
  return launch_walker("fr_mv_softmax_bwd", mv_softmax_bwd_kernel, stream, rows, N, ld, ldg, g, cos, (const long long*)label,
                       rowv, gcos, rows, N, ld, ldg, w, s);
}

extern "C" int fr_arcneg_apply(const float* cos, const int64_t* label, float* rowv, float* out, int rows, int N, int ld,
                               float thresh, float margin, float mm, float alpha, float sigma, float s, void* stream) {
  return launch_walker("fr_arcneg_apply", arcneg_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label, rowv,
                       out, rows, N, ld, thresh, margin, mm, alpha, sigma, s);
}

extern "C" int fr_arcneg_bwd(const float* g, const float* cos, const int64_t* label, const float* rowv, float* gcos,
                             int rows, int N, int ld, int ldg, float alpha, float sigma, float s, void* stream) {
  return launch_walker("fr_arcneg_bwd", arcneg_bwd_kernel, stream, rows, N, ld, ldg, g, cos, (const long long*)label, rowv,
                       gcos, rows, N, ld, ldg, alpha, sigma, s);
}

extern "C" int fr_circle_apply(const float* cos, const int64_t* label, float* out, int rows, int N, int ld, float o_p,
                               float o_n, float delta_p, float delta_n, float gamma, void* stream) {
  return launch_walker("fr_circle_apply", circle_apply_kernel, stream, rows, N, ld, ld, cos, (const long long*)label, out,
                       rows, N, ld, o_p, o_n, delta_p, delta_n, gamma);
}

extern "C" int fr_circle_bwd(const float* g, const float* cos, const int64_t* label, float* gcos, int rows, int N, int ld,
                             int ldg, float o_p, float o_n, float gamma, void* stream) {
  return launch_walker("fr_circle_bwd", circle_bwd_kernel, stream, rows, N, ld, ldg, g, cos, (const long long*)label, gcos,
                       rows, N, ld, ldg, o_p, o_n, gamma);
}

extern "C" int fr_ce_rows(const float* logits, const int64_t* label, float* lse, float* ce, int32_t* rank, int rows,
                          int N, int ld, void* stream) {
  if (rows <= 0 || N <= 0 || ld < N) FR_UNSUPPORTED("fr_ce_rows: shape (rows > 0, ld >= N > 0)");
  if (!logits || !label || !lse || !ce || !rank) FR_UNSUPPORTED("fr_ce_rows: logits, label, lse, ce and rank are required");
  hipLaunchKernelGGL(ce_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (const long long*)label,
                     lse, ce, rank, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_rank_rows(const float* logits, const int64_t* label, int32_t* rank, int rows, int N, int ld,
                            void* stream) {
  if (rows <= 0 || N <= 0 || ld < N) FR_UNSUPPORTED("fr_rank_rows: shape (rows > 0, ld >= N > 0)");
  if (!logits || !label || !rank) FR_UNSUPPORTED("fr_rank_rows: logits, label and rank are required");
  hipLaunchKernelGGL(rank_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits,
                     (const long long*)label, rank, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_topk_precision(const int32_t* rank, int rows, int nk, int k0, int k1, int k2, int k3, float scale,
                                 float* out, void* stream) {
  if (nk < 1 || nk > 4 || rows < 0) FR_UNSUPPORTED("fr_topk_precision: 1..4 values of k");
  hipLaunchKernelGGL(topk_precision_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rank, rows, nk,
                     make_int4(k0, k1, k2, k3), scale, out);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_focal_finalize(const float* ce, const int32_t* rank, int rows, float gamma, float* scalars,
                                 void* stream) {
  if (rows <= 0 || !ce || !rank || !scalars) FR_UNSUPPORTED("fr_focal_finalize: ce, rank, scalars and rows > 0 are required");
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ce, rank, rows, gamma,
                     scalars);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_focal_bwd(const float* logits, const int64_t* label, const float* lse, const float* scalars,
                            const float* gup, float* grad, int rows, int N, int ld, void* stream) {
  if (rows <= 0 || N <= 0 || ld < N) FR_UNSUPPORTED("fr_focal_bwd: shape (rows > 0, ld >= N > 0)");
  if (!logits || !label || !lse || !scalars || !gup || !grad)
    FR_UNSUPPORTED("fr_focal_bwd: logits, label, lse, scalars, gup and grad are required");
  dim3 grid((N + 1023) / 1024, rows);
  hipLaunchKernelGGL(focal_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits, (const long long*)label,
                     lse, scalars, gup, grad, rows, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_ce_finalize(const float* ce, const int32_t* rank, int rows, float* scalars, void* stream) {
  if (rows <= 0 || !ce || !rank || !scalars) FR_UNSUPPORTED("fr_ce_finalize: ce, rank, scalars and rows > 0 are required");
  hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ce, rank, rows, scalars);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_pack_rows(const float* w, const float* bias, float* wp, float* wt, float* biasp, int rows, int rows_pad,
                            int D, int ldt, void* stream) {
  if (rows <= 0 || D <= 0 || rows_pad < rows || ldt < rows_pad || ldt % 4)
    FR_UNSUPPORTED("fr_pack_rows: shape (D > 0, ldt >= rows_pad >= rows > 0, ldt a multiple of 4)");
  if (!w || !wp || !wt) FR_UNSUPPORTED("fr_pack_rows: w, wp and wt are required");
  hipLaunchKernelGGL(pack_rows_kernel, dim3((D + 63) / 64, (rows_pad + 63) / 64), dim3(256), 0, (hipStream_t)stream, w,
                     bias, wp, wt, biasp, rows, rows_pad, D, ldt);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_pad_cols(const float* g, float* out, int rows, int N, int ldg, int ldo, void* stream) {
  if (rows <= 0 || N <= 0 || ldg < N || ldo < N || ldo % 4)
    FR_UNSUPPORTED("fr_pad_cols: shape (rows > 0, ldg >= N > 0, ldo >= N, ldo a multiple of 4)");
  if (!g || !out) FR_UNSUPPORTED("fr_pad_cols: g and out are required");
  hipLaunchKernelGGL(pad_cols_kernel, dim3((ldo + 1023) / 1024, rows), dim3(256), 0, (hipStream_t)stream, g, out, N, ldg,
                     ldo);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_col_sums(const float* g, int rows, int N, int ldg, float* out, void* stream) {
  if (rows <= 0 || N <= 0 || ldg < N) FR_UNSUPPORTED("fr_col_sums: shape (rows > 0, ldg >= N > 0)");
  if (!g || !out) FR_UNSUPPORTED("fr_col_sums: g and out are required");
  hipLaunchKernelGGL(col_sums_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, rows, N, ldg, out);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_shard_row_stats(const float* logits, const int64_t* label_local, float* stats, int rows, int N, int ld,
                                  void* stream) {
  if (rows <= 0 || N <= 0) FR_UNSUPPORTED("fr_shard_row_stats: empty shard");
  hipLaunchKernelGGL(shard_row_stats_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits,
                     (const long long*)label_local, stats, rows, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_shard_combine(const float* stats_all, int world, int rows, float* lse, float* ce, float* tlogit,
                                void* stream) {
  if (rows <= 0 || world <= 0) FR_UNSUPPORTED("fr_shard_combine: empty");
  hipLaunchKernelGGL(shard_combine_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats_all,
                     world, rows, lse, ce, tlogit);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_shard_rank_rows(const float* logits, const float* tlogit, int32_t* rank, int rows, int N, int ld,
                                  void* stream) {
  if (rows <= 0 || N <= 0) FR_UNSUPPORTED("fr_shard_rank_rows: empty shard");
  hipLaunchKernelGGL(shard_rank_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, tlogit, rank, N,
                     ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_shard_target_cos(const float* cos, const int64_t* label_local, float* tl, int rows, int N, int ld,
                                   void* stream) {
  if (rows <= 0 || N <= 0 || ld < N) FR_UNSUPPORTED("fr_shard_target_cos: shape (rows > 0, ld >= N > 0)");
  hipLaunchKernelGGL(shard_target_cos_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, cos,
                     (const long long*)label_local, tl, rows, N, ld);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_shard_sum_parts(const float* r_part, int nparts, float* r, int rows, void* stream) {
  if (rows <= 0 || nparts <= 0) FR_UNSUPPORTED("fr_shard_sum_parts: shape (rows > 0, nparts > 0)");
  hipLaunchKernelGGL(sum_row_parts_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, r_part, nparts, r,
                     rows);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_adam_step(const FrAdamTensor* table_dev, const int32_t* chunks_dev, int nchunks, float step_size,
                            float w1, float beta2, float w2, float eps, float bc2_sqrt, void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev) FR_UNSUPPORTED("fr_adam_step: table_dev and chunks_dev are required when nchunks > 0");
  hipLaunchKernelGGL(adam_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev, (const int2*)chunks_dev,
                     step_size, w1, beta2, w2, eps, bc2_sqrt);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sgd_chunk_elems(void) { return SGD_CHUNK; }

extern "C" int fr_sgd_step(const FrSgdTensor* table_dev, const int32_t* chunks_dev, int nchunks, float lr,
                           float momentum, void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev) FR_UNSUPPORTED("fr_sgd_step: table_dev and chunks_dev are required when nchunks > 0");
  hipLaunchKernelGGL(sgd_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     (const int2*)chunks_dev, lr, momentum);
  FR_LAUNCH_CHECK();
}

// The row-sparse step with or without the guard's control word: vector width and grid follow the selected rows.
template <bool CTL>
static int launch_sgd_rows(float* p, float* buf, const float* g_rows, const int32_t* idx, int n_s, int D, float lr,
                           float momentum, float wd, const float* ctl, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool vec = D % 4 == 0 && (uintptr_t)p % 16 == 0 && (uintptr_t)buf % 16 == 0 && (uintptr_t)g_rows % 16 == 0;
  const int dv = vec ? D / 4 : D;
  const long long total = (long long)n_s * dv;  // the grid follows the selected rows, not the parameter
  const long long want = (total + 255) / 256;
  const dim3 grid((unsigned)(want > 4096 ? 4096 : want));  // 16 workgroups per CU, grid-stride beyond
  if (vec)
    hipLaunchKernelGGL((sgd_rows_kernel<4, CTL>), grid, dim3(256), 0, st, p, buf, g_rows, idx, total, dv, lr, momentum, wd,
                       ctl);
  else
    hipLaunchKernelGGL((sgd_rows_kernel<1, CTL>), grid, dim3(256), 0, st, p, buf, g_rows, idx, total, dv, lr, momentum, wd,
                       ctl);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sgd_rows(float* p, float* buf, const float* g_rows, const int32_t* idx, int n_s, int D, float lr,
                           float momentum, float wd, void* stream) {
  if (n_s <= 0) return 0;
  if (!p || !buf || !g_rows || !idx) FR_UNSUPPORTED("fr_sgd_rows: p, buf, g_rows and idx are required when n_s > 0");
  if (D < 1) FR_UNSUPPORTED("fr_sgd_rows: D >= 1");
  return launch_sgd_rows<false>(p, buf, g_rows, idx, n_s, D, lr, momentum, wd, nullptr, stream);
}

extern "C" int fr_grad_sumsq(const FrGradTensor* table_dev, const int32_t* chunks_dev, int nchunks, double* parts,
                             void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev || !parts)
    FR_UNSUPPORTED("fr_grad_sumsq: table_dev, chunks_dev and parts are required when nchunks > 0");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     (const int2*)chunks_dev, parts);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_grad_guard(const double* parts, int nparts, float max_norm, int skip_nonfinite, float* ctl,
                             int32_t* skipped, void* stream) {
  if (nparts < 0) FR_UNSUPPORTED("fr_grad_guard: nparts >= 0");
  if (nparts > 0 && !parts) FR_UNSUPPORTED("fr_grad_guard: parts is required when nparts > 0");
  if (!ctl) FR_UNSUPPORTED("fr_grad_guard: ctl is required");
  if (max_norm != max_norm) FR_UNSUPPORTED("fr_grad_guard: max_norm is NaN (max_norm <= 0 measures without clipping)");
  hipLaunchKernelGGL(grad_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, parts, nparts, max_norm,
                     skip_nonfinite, ctl, skipped);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sgd_step_ctl(const FrSgdTensor* table_dev, const int32_t* chunks_dev, int nchunks, float lr,
                               float momentum, const float* ctl, int use_coef, void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev || !ctl)
    FR_UNSUPPORTED("fr_sgd_step_ctl: table_dev, chunks_dev and ctl are required when nchunks > 0");
  hipLaunchKernelGGL(sgd_ctl_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     (const int2*)chunks_dev, lr, momentum, ctl, use_coef);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_adam_step_ctl(const FrAdamTensor* table_dev, const int32_t* chunks_dev, int nchunks, float step_size,
                                float w1, float beta2, float w2, float eps, float bc2_sqrt, const float* ctl,
                                int use_coef, void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev || !ctl)
    FR_UNSUPPORTED("fr_adam_step_ctl: table_dev, chunks_dev and ctl are required when nchunks > 0");
  hipLaunchKernelGGL(adam_ctl_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev,
                     (const int2*)chunks_dev, step_size, w1, beta2, w2, eps, bc2_sqrt, ctl, use_coef);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sgd_rows_ctl(float* p, float* buf, const float* g_rows, const int32_t* idx, int n_s, int D, float lr,
                               float momentum, float wd, const float* ctl, void* stream) {
  if (n_s <= 0) return 0;
  if (!p || !buf || !g_rows || !idx || !ctl)
    FR_UNSUPPORTED("fr_sgd_rows_ctl: p, buf, g_rows, idx and ctl are required when n_s > 0");
  if (D < 1) FR_UNSUPPORTED("fr_sgd_rows_ctl: D >= 1");
  return launch_sgd_rows<true>(p, buf, g_rows, idx, n_s, D, lr, momentum, wd, ctl, stream);
}

extern "C" int fr_ema_chunk_elems(void) { return SGD_CHUNK; }

extern "C" int fr_ema_step(const FrEmaTensor* table_dev, const int32_t* chunks_dev, int nchunks, float a, float b,
                           void* stream) {
  if (nchunks <= 0) return 0;
  if (!table_dev || !chunks_dev) FR_UNSUPPORTED("fr_ema_step: table_dev and chunks_dev are required when nchunks > 0");
  hipLaunchKernelGGL(ema_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev, (const int2*)chunks_dev, a,
                     b);
  FR_LAUNCH_CHECK();
}
