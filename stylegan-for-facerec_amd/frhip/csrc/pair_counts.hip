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

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int PC_TILE = 128;          // rows and columns of the Gram matrix per workgroup
constexpr int PC_BK = 32;             // k per LDS stage
constexpr int PC_LD = PC_BK + 4;      // LDS row pitch in floats: 16 consecutive rows hit 16 distinct 16-byte slots
constexpr int PC_BAND = 8;            // mode 0 walks the triangle in bands of 8 tile columns (L2 reuse of both operands)
constexpr int PC_MAX_T = 32;
constexpr int PC_MAX_D = 2048;

struct PcGeom {
  int nt;          // tiles per side
  long long parts; // workgroups = rows of partials
  int q;           // mode 1: every q-th tile edge falls between two groups (q = odd part of g; 1: all of them do)
};

__host__ __device__ inline int pc_odd_part(int g) {
  while ((g & 1) == 0) g >>= 1;
  return g;
}

inline PcGeom pc_geom(int M, int mode, int group) {
  PcGeom s;
  s.nt = (M + PC_TILE - 1) / PC_TILE;
  s.q = 1;
  if (mode == 0) {
    s.parts = (long long)s.nt * (s.nt + 1) / 2;
  } else {
    // tile edge k * 128 (k = 1 .. nt - 1) cuts a group in two unless it is a multiple of g, i.e. unless k % q == 0
    s.q = pc_odd_part(group);
    const int edges = s.nt - 1;
    s.parts = s.nt + (s.q == 1 ? 0 : edges - edges / s.q);
  }
  return s;
}

// Linear index -> tile (ti, tj), tj >= ti.  The triangle is cut into bands of PC_BAND tile columns; a band is walked row
// by row, so the workgroups in flight at one time share a few row blocks and a few column blocks.  Before band b lie the
// c (c + 1) / 2 tiles of its c = b * PC_BAND columns.
__device__ __forceinline__ void pc_tile_mode0(uint32_t p, int nt, int& ti, int& tj) {
  int c = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);  // largest c with c (c + 1) / 2 <= p, after the fix-up
  while ((unsigned long long)c * (c + 1) / 2 > p) --c;
  while ((unsigned long long)(c + 1) * (c + 2) / 2 <= p) ++c;
  const int c0 = c / PC_BAND * PC_BAND;
  const int w = min(PC_BAND, nt - c0);
  uint32_t r = p - (uint32_t)c0 * (uint32_t)(c0 + 1) / 2;
  if (r < (uint32_t)c0 * (uint32_t)w) {  // the rectangle above the band's diagonal block
    ti = (int)(r / (uint32_t)w);
    tj = c0 + (int)(r % (uint32_t)w);
    return;
  }
  r -= (uint32_t)c0 * (uint32_t)w;
  int row = 0;  // the diagonal block: row `row` has w - row tiles
  while (r >= (uint32_t)(w - row)) {
    r -= (uint32_t)(w - row);
    ++row;
  }
  ti = c0 + row;
  tj = c0 + row + (int)r;
}

// mode 1: the nt diagonal tiles, then (k - 1, k) for every tile edge k that cuts a group
__device__ __forceinline__ void pc_tile_mode1(uint32_t p, int nt, int q, int& ti, int& tj) {
  if (p < (uint32_t)nt) {
    ti = tj = (int)p;
    return;
  }
  const int idx = (int)p - nt;
  const int k = idx + idx / (q - 1) + 1;  // skips every q-th edge
  ti = k - 1;
  tj = k;
}

__global__ __launch_bounds__(256, 2) void pair_counts_kernel(const float* __restrict__ E, int ldE, int M, int D,
                                                             const float* __restrict__ thr, int T, int mode, int group,
                                                             int nt, int q, uint32_t* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sA[PC_TILE * PC_LD];
  __shared__ __attribute__((aligned(16))) float sB[PC_TILE * PC_LD];
  __shared__ uint32_t sCnt[4][PC_MAX_T];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // this wave's 64 x 64 quarter of the tile
  const uint32_t p = (uint32_t)xcd_remap((int)blockIdx.x, (int)gridDim.x);
  int ti, tj;
  if (mode == 0)
    pc_tile_mode0(p, nt, ti, tj);
  else
    pc_tile_mode1(p, nt, q, ti, tj);
  const int row0 = ti * PC_TILE, col0 = tj * PC_TILE;

  // loader: 8 threads take the 32 floats of one row, 32 rows per pass, 4 passes per operand
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  f32x4 ra[4], rb[4];
  auto load = [&](int k0) {
    const bool kin = k0 + lk < D;  // D % 4 == 0: a 16-byte chunk is inside or outside as a whole
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int r = lr + 32 * s;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      ra[s] = (kin && row0 + r < M) ? *reinterpret_cast<const f32x4*>(E + (size_t)(row0 + r) * ldE + k0 + lk) : z;
      rb[s] = (kin && col0 + r < M) ? *reinterpret_cast<const f32x4*>(E + (size_t)(col0 + r) * ldE + k0 + lk) : z;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // fragment base: lane l feeds row (l & 31) of a 32-row block; lane half h = l >> 5 takes k = 8 kk + 4 h + j for the
  // j-th MFMA of chunk kk -- the same permutation of k for both operands, hence the same dot product
  const float* fa = sA + (wm * 64 + (lane & 31)) * PC_LD + (lane >> 5) * 4;
  const float* fb = sB + (wn * 64 + (lane & 31)) * PC_LD + (lane >> 5) * 4;

  load(0);
  for (int k0 = 0; k0 < D; k0 += PC_BK) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      *reinterpret_cast<f32x4*>(sA + (lr + 32 * s) * PC_LD + lk) = ra[s];
      *reinterpret_cast<f32x4*>(sB + (lr + 32 * s) * PC_LD + lk) = rb[s];
    }
    __syncthreads();
    if (k0 + PC_BK < D) load(k0 + PC_BK);  // in flight while the MFMAs of this stage run
#pragma unroll
    for (int kk = 0; kk < PC_BK / 8; ++kk) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const f32x4*>(fa + m * 32 * PC_LD + kk * 8);
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const f32x4*>(fb + n * 32 * PC_LD + kk * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][j], b[n][j], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- which accumulators are pairs.  C/D of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
  // An off-diagonal tile that lies inside the matrix holds pairs only (mode 0): no pass over it.
  const bool all_pairs = mode == 0 && ti != tj && col0 + PC_TILE <= M;
  if (!all_pairs) {
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int j = col0 + wn * 64 + n * 32 + (lane & 31);
      // same person <=> first row of j's group <= i (given i < j)
      const int lo = mode == 0 ? 0 : j / group * group;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = row0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const bool pair = i < j && j < M && i >= lo;
          acc[m][n][r] = pair ? acc[m][n][r] : nan;
        }
    }
  }
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

// argument checks shared by the two entry points; 0 = fine
int pc_check_shape(int M, int mode, int group, const char** why) {
  if (M < 2) {
    *why = "fr_pair_counts: M >= 2 is required (one pair at least)";
    return -1;
  }
  if (mode != 0 && mode != 1) {
    *why = "fr_pair_counts: mode must be 0 (impostor pairs, score > thr) or 1 (genuine pairs, score < thr)";
    return -1;
  }
  if (mode == 1 && (group < 2 || group > 16)) {
    *why = "fr_pair_counts: mode 1 needs 2 <= group <= 16 rows per person";
    return -1;
  }
  if (pc_geom(M, mode, group).parts > 0x7fffffffLL) {
    *why = "fr_pair_counts: M is too large for one launch (more than 2^31 - 1 tiles)";
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" int fr_pair_counts_parts(int M, int mode, int group) {
  const char* why = nullptr;
  if (pc_check_shape(M, mode, group, &why)) FR_UNSUPPORTED(why);
  return (int)pc_geom(M, mode, group).parts;
}

extern "C" int fr_pair_counts(const float* E, int ldE, int M, int D, const float* thr, int T, int mode, int group,
                              uint32_t* partials, int64_t* counts, void* stream) {
  const char* why = nullptr;
  if (pc_check_shape(M, mode, group, &why)) FR_UNSUPPORTED(why);
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
