// frhip -- SST_Prototype ("Semi-Siamese Training for Shallow Face Learning"): the gallery queue and the head's row kernels.
//
// Reference arithmetic replaced (paths in the reference checkout):
//   update_queue: the window of the queue and of label_list takes the chosen gallery view   head/metrics.py:675-680
//   compute_theta's queue.clone() with the window substituted (never materialised here)       head/metrics.py:669-671
//   add_margin: clamp, the label column's margin; forward's * scale                          head/metrics.py:654-666, :701-702
//
// The queue lives on the device in both GEMM layouts: q [D][Q] (the reference's buffer, the data gradient's operand) and
// qt [Q][D] (the cosine GEMM's operand).  A step replaces B of the Q columns; nothing else of either copy is touched, and
// the cosines against the substituted window come from a small GEMM against the gallery rows themselves (cw), so neither
// direction ever reads the live queue's window.
#include <stdio.h>

#include "common.h"
#include "frhip_internal.h"

namespace {

constexpr int SST_COLS = 1024;  // columns per blockIdx.x of the row kernels: 4 waves = 4 rows, one f32x4 per lane and pass

// torch.clamp(c, -1, 1): NaN passes through (fminf / fmaxf would turn it into a bound)
__device__ __forceinline__ float clamp1(float c) { return c > 1.f ? 1.f : (c < -1.f ? -1.f : c); }

// qt[index + b][d] = gn[b][d], q[d][index + b] = gn[b][d], labels[index + b] = ids[b].  One 64 x 64 tile of gn per block
// through LDS: the read of gn and the write of qt run along d, the write of q along b (B contiguous floats per d row), so
// all three are coalesced.  The blocks of d tile 0 also carry the labels.
__global__ __launch_bounds__(256) void sst_enqueue_kernel(const float* __restrict__ gn, const long long* __restrict__ ids,
                                                          float* __restrict__ qt, float* __restrict__ q,
                                                          long long* __restrict__ labels, int index, int B, int D, int Q) {
  __shared__ float tt[64][65];
  const int d0 = blockIdx.x * 64, b0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int j = ty; j < 64; j += 4) {
    if (b0 + j < B && d0 + tx < D) {
      const float v = gn[(size_t)(b0 + j) * D + d0 + tx];
      tt[j][tx] = v;
      qt[(size_t)(index + b0 + j) * D + d0 + tx] = v;
    }
  }
  __syncthreads();
  for (int j = ty; j < 64; j += 4)
    if (d0 + j < D && b0 + tx < B) q[(size_t)(d0 + j) * Q + index + b0 + tx] = tt[tx][j];
  if (blockIdx.x == 0 && ty == 0 && b0 + tx < B) labels[index + b0 + tx] = ids[b0 + tx];
}

// The label column's value from its clamped cosine.  Plain operators under "fp contract(off)" and sqrtf: every operation
// is rounded to fp32 on its own, in the reference's order (gt * cos(m) - sqrt(1.0 - gt^2) * sin(m), :663-664).
__device__ __forceinline__ float sst_label(float c, int kind, float p0, float p1) {
#pragma clang fp contract(off)
  if (kind == 1) return c - p0;
  if (kind == 2) {
    const float t1 = c * p0;
    const float sr = sqrtf(1.0f - c * c);
    const float t2 = sr * p1;
    return t1 - t2;
  }
  return c;
}

// d label value / d c
__device__ __forceinline__ float sst_dlabel(float c, int kind, float p0, float p1) {
#pragma clang fp contract(off)
  if (kind == 2) {
    const float r = c / sqrtf(1.0f - c * c);
    const float t = r * p1;
    return p0 + t;
  }
  return 1.f;
}

// out[m][n] = s * (n == label ? margin(c) : c), c = clamp(n in the window ? cw[m][blk * B + n - index] : cos[m][n]);
// label = index + m % B, blk = m / B; 0 in the padding columns [Q, ld)
__global__ __launch_bounds__(256) void sst_apply_kernel(const float* __restrict__ cos, const float* __restrict__ cw,
                                                        float* __restrict__ out, int rows, int B, int Q, int ld, int ldw,
                                                        int index, int kind, float p0, float p1, float s) {
#pragma clang fp contract(off)
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int blk = row / B;
  const int lab = index + (row - blk * B);
  const float* wrow = cw + (size_t)row * ldw + (size_t)blk * B;
  const int end = min(ld, (int)(blockIdx.x + 1) * SST_COLS);
  for (int n = blockIdx.x * SST_COLS + lane * 4; n < end; n += 256) {
    const f32x4 ch = *reinterpret_cast<const f32x4*>(cos + (size_t)row * ld + n);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = n + j;
      float v = 0.f;
      if (c < Q) {
        const bool win = c >= index && c < index + B;
        const float cl = clamp1(win ? wrow[c - index] : ch[j]);
        v = (c == lab ? sst_label(cl, kind, p0, p1) : cl) * s;
      }
      o[j] = v;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)row * ld + n) = o;
  }
}

// gcos[m][n] = (g[m][n] * s) where the clamp passes, 0 in the window, where it saturated (a NaN cosine too) and in the
// padding [Q, ldg): the label column lies in the window, so every column outside it has d out / d c = s.
// gwin[m][j], j in [0, ldw): the window column index + j - blk * B of row m for j in the row's block [blk * B, blk * B + B),
// (g * s) * d label / d c on the label column, under the pass mask of the cosine cw[m][j]; 0 outside the block.  The waves of
// blockIdx.x == 0 write gwin.
__global__ __launch_bounds__(256) void sst_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cos,
                                                      const float* __restrict__ cw, float* __restrict__ gcos,
                                                      float* __restrict__ gwin, int rows, int B, int Q, int ld, int ldg,
                                                      int ldw, int index, int kind, float p0, float p1, float s) {
#pragma clang fp contract(off)
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int blk = row / B;
  const int j0 = blk * B;
  const float* grow = g + (size_t)row * Q;
  const float* crow = cos + (size_t)row * ld;
  float* orow = gcos + (size_t)row * ldg;
  const int end = min(ldg, (int)(blockIdx.x + 1) * SST_COLS);
  for (int n = blockIdx.x * SST_COLS + lane * 4; n < end; n += 256) {
    f32x4 ch = {0.f, 0.f, 0.f, 0.f};
    if (n < ld) ch = *reinterpret_cast<const f32x4*>(crow + n);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = n + j;
      float v = 0.f;
      if (c < Q && !(c >= index && c < index + B)) {
        const bool pass = ch[j] >= -1.f && ch[j] <= 1.f;
        const float gs = grow[c] * s;
        v = pass ? gs : 0.f;
      }
      o[j] = v;
    }
    *reinterpret_cast<f32x4*>(orow + n) = o;
  }
  if (blockIdx.x != 0) return;
  const float* wrow = cw + (size_t)row * ldw;
  float* wout = gwin + (size_t)row * ldw;
  for (int j = lane; j < ldw; j += 64) {
    float v = 0.f;
    if (j >= j0 && j < j0 + B) {
      const float raw = wrow[j];
      const bool pass = raw >= -1.f && raw <= 1.f;
      const float gs = grow[index + j - j0] * s;
      const float d = j == row ? sst_dlabel(raw, kind, p0, p1) : 1.f;  // block layout: row m's label column is j = m
      v = pass ? gs * d : 0.f;
    }
    wout[j] = v;
  }
}

// the shape both row kernels take; `what` opens the error text
int sst_shape(const char* what, int rows, int B, int Q, int ld, int ldw, int index, int kind) {
  if (B <= 0 || (rows != B && rows != 2 * B) || Q <= 0 || ld < Q || ld % 4 || ldw < rows || index < 0 ||
      (long long)index + B > Q || kind < 0 || kind > 2) {
    char msg[200];
    snprintf(msg, sizeof(msg),
             "%s: shape (B > 0, rows = B or 2 B, ld >= Q > 0, ld a multiple of 4, ldw >= rows, 0 <= index, index + B <= Q, "
             "kind 0..2)", what);
    fr_set_error(msg);
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" int fr_sst_enqueue(const float* gn, const int64_t* ids, float* qt, float* q, int64_t* labels, int index, int B,
                              int D, int Q, void* stream) {
  if (B <= 0 || D <= 0 || Q <= 0 || index < 0 || (long long)index + B > Q)
    FR_UNSUPPORTED("fr_sst_enqueue: shape (B > 0, D > 0, 0 <= index, index + B <= Q)");
  if (!gn || !ids || !qt || !q || !labels) FR_UNSUPPORTED("fr_sst_enqueue: gn, ids, qt, q and labels are required");
  hipLaunchKernelGGL(sst_enqueue_kernel, dim3((D + 63) / 64, (B + 63) / 64), dim3(256), 0, (hipStream_t)stream, gn,
                     (const long long*)ids, qt, q, (long long*)labels, index, B, D, Q);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sst_apply(const float* cos, const float* cw, float* out, int rows, int B, int Q, int ld, int ldw,
                            int index, int kind, float p0, float p1, float s, void* stream) {
  if (sst_shape("fr_sst_apply", rows, B, Q, ld, ldw, index, kind)) return -1;
  if (!cos || !cw || !out) FR_UNSUPPORTED("fr_sst_apply: cos, cw and out are required");
  hipLaunchKernelGGL(sst_apply_kernel, dim3((ld + SST_COLS - 1) / SST_COLS, (rows + 3) / 4), dim3(256), 0,
                     (hipStream_t)stream, cos, cw, out, rows, B, Q, ld, ldw, index, kind, p0, p1, s);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_sst_bwd(const float* g, const float* cos, const float* cw, float* gcos, float* gwin, int rows, int B,
                          int Q, int ld, int ldg, int ldw, int index, int kind, float p0, float p1, float s, void* stream) {
  if (sst_shape("fr_sst_bwd", rows, B, Q, ld, ldw, index, kind)) return -1;
  if (ldg < ld || ldg % 4) FR_UNSUPPORTED("fr_sst_bwd: ldg >= ld, a multiple of 4");
  if (!g || !cos || !cw || !gcos || !gwin) FR_UNSUPPORTED("fr_sst_bwd: g, cos, cw, gcos and gwin are required");
  hipLaunchKernelGGL(sst_bwd_kernel, dim3((ldg + SST_COLS - 1) / SST_COLS, (rows + 3) / 4), dim3(256), 0,
                     (hipStream_t)stream, g, cos, cw, gcos, gwin, rows, B, Q, ld, ldg, ldw, index, kind, p0, p1, s);
  FR_LAUNCH_CHECK();
}
