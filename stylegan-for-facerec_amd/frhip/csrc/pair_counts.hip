// frhip -- threshold tallies over the pairwise cosine scores of one embedding matrix (RB-WebFace FMR / FNMR,
// rb-webface/scripts/test_RB_Webface.py:153-233 of the reference), without ever writing the M x M scores.
//
//   mode 0: count[t] = #{ i < j           : E_i . E_j > thr[t] }      (impostor pairs, calc_FMR)
//   mode 1: count[t] = #{ i < j, i/g==j/g : E_i . E_j < thr[t] }      (genuine pairs, calc_FNMR; g rows = one person)
//
// One workgroup owns one 128 x 128 tile (ti, tj >= ti) of the Gram matrix: both operands are row blocks of E, staged
// through LDS in k-chunks of 32 and fed to v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fmaf chain, so the error
// bound of the scores is the textbook one).  The epilogue turns every accumulator that is not a pair (i >= j, j >= M,
// another person) into NaN, which fails both strict comparisons exactly like the NaN score of a zero row does, then
// compares each accumulator with each threshold: v_cmp into a lane mask, popcount and add on the scalar unit.  The
// per-wave tallies go through LDS; the workgroup writes one row of uint32 partials [n_workgroups][T] (a tile has
// 16 384 pairs) and a second launch sums the rows into int64.  Integer sums: the result does not depend on the order
// the workgroups ran in.
#include "common.h"
#include "frhip_internal.h"
#include "pair_tile.h"  // the tiles of the triangle, the Gram main loop and the pair mask, shared with pair_hist.hip

namespace {

constexpr int PC_MAX_T = 32;
constexpr const char* PC_MODES = "0 (impostor pairs, score > thr) or 1 (genuine pairs, score < thr)";

__global__ __launch_bounds__(256, 2) void pair_counts_kernel(const float* __restrict__ E, int ldE, int M, int D,
                                                             const float* __restrict__ thr, int T, int mode, int group,
                                                             int nt, int q, uint32_t* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sA[PC_TILE * PC_LD];
  __shared__ __attribute__((aligned(16))) float sB[PC_TILE * PC_LD];
  __shared__ uint32_t sCnt[4][PC_MAX_T];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t p = (uint32_t)xcd_remap((int)blockIdx.x, (int)gridDim.x);
  int ti, tj;
  if (mode == 0)
    pc_tile_mode0(p, nt, ti, tj);
  else
    pc_tile_mode1(p, nt, q, ti, tj);
  const int row0 = ti * PC_TILE, col0 = tj * PC_TILE;

  f32x16 acc[2][2];
  pc_gram_tile(E, ldE, M, D, row0, col0, sA, sB, acc);
  pc_mask_pairs(acc, mode, group, ti, tj, row0, col0, M);  // NaN wherever the accumulator is not a pair
  // mode 1 counts score < thr: the same comparison on the negated score and threshold
  const float sgn = mode == 0 ? 1.f : -1.f;
  if (mode != 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][n][r] = -acc[m][n][r];
  }

  for (int t = 0; t < T; ++t) {
    const float th = thr[t] * sgn;
    uint32_t c = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) c += (uint32_t)__builtin_popcountll(__ballot(acc[m][n][r] > th));
    if (lane == 0) sCnt[wave][t] = c;
  }
  __syncthreads();
  if (tid < T) partials[(size_t)blockIdx.x * T + tid] = sCnt[0][tid] + sCnt[1][tid] + sCnt[2][tid] + sCnt[3][tid];
}

// counts[t] = sum over the workgroups' rows; one block per threshold
__global__ __launch_bounds__(256) void pair_counts_sum_kernel(const uint32_t* __restrict__ partials, long long parts, int T,
                                                              long long* __restrict__ counts) {
  __shared__ unsigned long long sh[4];
  const int t = blockIdx.x;
  unsigned long long s = 0;
  for (long long w = threadIdx.x; w < parts; w += blockDim.x) s += partials[(size_t)w * T + t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) counts[t] = (long long)(sh[0] + sh[1] + sh[2] + sh[3]);
}

}  // namespace

extern "C" int fr_pair_counts_parts(int M, int mode, int group) {
  if (pc_check_shape(M, mode, group, "fr_pair_counts", PC_MODES)) return -1;
  return (int)pc_geom(M, mode, group).parts;
}

extern "C" int fr_pair_counts(const float* E, int ldE, int M, int D, const float* thr, int T, int mode, int group,
                              uint32_t* partials, int64_t* counts, void* stream) {
  if (pc_check_shape(M, mode, group, "fr_pair_counts", PC_MODES)) return -1;
  if (T < 1 || T > PC_MAX_T) FR_UNSUPPORTED("fr_pair_counts: 1 <= T <= 32 thresholds per launch");
  if (D < 4 || D > PC_MAX_D || D % 4) FR_UNSUPPORTED("fr_pair_counts: D must be a multiple of 4, 4 <= D <= 2048");
  if (ldE < D || ldE % 4) FR_UNSUPPORTED("fr_pair_counts: ldE >= D and ldE % 4 == 0 (16-byte row pitch)");
  if (!E || !thr || !partials || !counts) FR_UNSUPPORTED("fr_pair_counts: E, thr, partials and counts are required");
  if ((uintptr_t)E % 16) FR_UNSUPPORTED("fr_pair_counts: E must be 16-byte aligned");
  const PcGeom s = pc_geom(M, mode, group);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_counts_kernel, dim3((unsigned)s.parts), dim3(256), 0, st, E, ldE, M, D, thr, T, mode,
                     mode == 0 ? 1 : group, s.nt, s.q, partials);
  hipLaunchKernelGGL(pair_counts_sum_kernel, dim3(T), dim3(256), 0, st, (const uint32_t*)partials, s.parts, T,
                     reinterpret_cast<long long*>(counts));
  FR_LAUNCH_CHECK();
}
