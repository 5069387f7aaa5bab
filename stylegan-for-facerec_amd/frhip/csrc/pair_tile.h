// frhip -- the Gram tile of the pairwise-score kernels (pair_counts.hip: threshold tallies; pair_hist.hip: histograms of
// the score keys), written once: which 128 x 128 tiles of the upper triangle a call covers and in which order, the LDS
// staging / MFMA main loop that forms the 64 x 64 scores of a wave, and the mask that turns every accumulator that is not a
// pair into NaN.  Both kernels therefore see the same fp32 scores bit for bit; what they do with them stays with the kernel.
#pragma once
#include <string>
#include "common.h"

namespace {  // included by the two pair kernels only; nothing here has a name outside their translation units

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int PC_TILE = 128;          // rows and columns of the Gram matrix per workgroup
constexpr int PC_BK = 32;             // k per LDS stage
constexpr int PC_LD = PC_BK + 4;      // LDS row pitch in floats: 16 consecutive rows hit 16 distinct 16-byte slots
constexpr int PC_BAND = 8;            // mode 0 walks the triangle in bands of 8 tile columns (L2 reuse of both operands)
constexpr int PC_MAX_D = 2048;

struct PcGeom {
  int nt;          // tiles per side
  long long parts; // tiles of the call (fr_pair_counts: one workgroup and one row of partials each)
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

// acc = E[row0 .. row0 + 127] . E[col0 .. col0 + 127]^T, this wave's 64 x 64 quarter (wm, wn) as 2 x 2 MFMA tiles.  Both
// operands are row blocks of E, staged through sA / sB (PC_TILE * PC_LD floats each) in k-chunks of 32 and fed to
// v_mfma_f32_32x32x2_f32: an exact f32, k-ordered fmaf chain.  All 256 threads of the workgroup call it together; it
// ends on a barrier, so sA / sB are free again when it returns.
__device__ __forceinline__ void pc_gram_tile(const float* __restrict__ E, int ldE, int M, int D, int row0, int col0,
                                             float* sA, float* sB, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // this wave's 64 x 64 quarter of the tile

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
}

// Which accumulators are pairs: everything else (i >= j, j >= M, another person in mode 1) becomes NaN.  C/D of the 32x32
// MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  An off-diagonal tile that lies inside the
// matrix holds pairs only (mode 0): no pass over it.
__device__ __forceinline__ void pc_mask_pairs(f32x16 (&acc)[2][2], int mode, int group, int ti, int tj, int row0, int col0,
                                              int M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
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
}

// The shape checks of the entry points that take (M, mode, group).  `who` is the caller's name and `modes` what modes 0 and 1
// mean to it; on a refusal the message is set (fr_set_error copies it) and -1 returned, else 0.
inline int pc_check_shape(int M, int mode, int group, const char* who, const char* modes) {
  const char* why = nullptr;
  std::string mode_why;
  if (M < 2) {
    why = "M >= 2 is required (one pair at least)";
  } else if (mode != 0 && mode != 1) {
    mode_why = std::string("mode must be ") + modes;
    why = mode_why.c_str();
  } else if (mode == 1 && (group < 2 || group > 16)) {
    why = "mode 1 needs 2 <= group <= 16 rows per person";
  } else if (pc_geom(M, mode, group).parts > 0x7fffffffLL) {
    why = "M is too large for one launch (more than 2^31 - 1 tiles)";
  }
  if (!why) return 0;
  fr_set_error((std::string(who) + ": " + why).c_str());
  return -1;
}

}  // namespace
