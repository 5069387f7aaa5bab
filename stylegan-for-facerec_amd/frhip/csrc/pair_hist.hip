// frhip -- histogram of the pairwise cosine scores of one embedding matrix over a window of their order-preserving
// integer keys: one pass of the radix select behind "the exact threshold at a chosen FPR" (frhip/pairwise.py:
// score_at_rank; the np.interp lines of rb-webface/scripts/test_RB_Webface.py:153-233 of the reference, made exact).
//
//   u   = bits(s == 0 ? +0.0f : s)
//   key = (u & 0x80000000) ? ~u : (u | 0x80000000)          s1 < s2  <=>  key1 < key2; a NaN score has no key
//   hist[0]       = #{ pairs : key <  key_lo }
//   hist[1 + b]   = #{ pairs : key_lo + (b << shift) <= key < key_lo + ((b + 1) << shift) },   b = 0 .. NB - 1
//   hist[NB + 1]  = #{ pairs : key >= key_lo + (NB << shift) }
//
// Tiles, modes, main loop and pair mask are those of fr_pair_counts (pair_tile.h), so the scores are the same fp32 bits.
// The workgroups are persistent: about as many as the chip holds at once, each walks the banded tile order with a stride
// of the grid, bins its scores into one LDS histogram with LDS atomic adds and flushes it once, with vector stores, into
// its row of uint32 partials [workgroups][NB + 2]; a second kernel sums the rows into int64.  No global atomics, integer
// sums: the result does not depend on scheduling.
#include "common.h"
#include "frhip_internal.h"
#include "pair_tile.h"

namespace {

constexpr int PH_MAX_NB = 2048;
constexpr int PH_MAX_SHIFT = 21;   // 11 + 11 + 10 key bits: the first pass of the select bins on the top 11
constexpr int PH_GRID = 768;       // 256 CUs x 3 resident workgroups (44.0 KB LDS, 164 VGPRs)
constexpr const char* PH_MODES = "0 (impostor pairs: all i < j) or 1 (genuine pairs: i < j inside a group)";

__device__ __forceinline__ uint32_t ph_key(float s) {
  const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);  // -0 and +0 share a key
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256, 2) void pair_hist_kernel(const float* __restrict__ E, int ldE, int M, int D, uint32_t key_lo,
                                                           int shift, int NB, int mode, int group, int nt, int q,
                                                           uint32_t tiles, uint32_t* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sA[PC_TILE * PC_LD];
  __shared__ __attribute__((aligned(16))) float sB[PC_TILE * PC_LD];
  __shared__ uint32_t sH[PH_MAX_NB + 2];

  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < NB + 2; i += 256) sH[i] = 0;
  __syncthreads();

  // workgroups on one XCD take neighbouring tiles of every round (xcd_remap), as in fr_pair_counts
  const uint32_t w = (uint32_t)xcd_remap((int)blockIdx.x, (int)gridDim.x);
  for (uint32_t p = w; p < tiles; p += gridDim.x) {
    int ti, tj;
    if (mode == 0)
      pc_tile_mode0(p, nt, ti, tj);
    else
      pc_tile_mode1(p, nt, q, ti, tj);
    const int row0 = ti * PC_TILE, col0 = tj * PC_TILE;

    f32x16 acc[2][2];
    pc_gram_tile(E, ldE, M, D, row0, col0, sA, sB, acc);
    pc_mask_pairs(acc, mode, group, ti, tj, row0, col0, M);  // NaN wherever the accumulator is not a pair

#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[m][n][r];
          const uint32_t key = ph_key(s);
          const uint32_t b = (key - key_lo) >> shift;
          const uint32_t slot = key < key_lo ? 0u : min(b, (uint32_t)NB) + 1u;  // slot <= NB + 1 < PH_MAX_NB + 2
          const bool scored = s == s;  // a NaN score goes nowhere
          // Same-slot adds of one wave instruction serialise in the LDS, and in passes 2 and 3 of the select nearly every
          // score lies outside the window: all 64 lanes add to the slot below or above it.  So the wave takes the slot of
          // its first scored lane, counts the lanes that share it (ballot + popcount on the scalar unit) and lets that one
          // lane add the count; one LDS atomic then serves the lanes left.  One such round, by measurement:
          // none costs passes 2 and 3 a quarter more time, two or four slow pass 1 down.
          const unsigned long long any = __ballot(scored);
          if (any == 0) continue;
          const int first = __builtin_ctzll(any);
          const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, first);
          const bool same = scored && slot == s0;
          const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(same));
          if (lane == first) atomicAdd(&sH[s0], cnt);
          if (scored && !same) atomicAdd(&sH[slot], 1u);
        }
  }
  __syncthreads();
  uint32_t* row = partials + (size_t)blockIdx.x * (size_t)(NB + 2);
  for (int i = tid; i < NB + 2; i += 256) row[i] = sH[i];
}

// hist[i] = sum over the workgroups' rows; one thread per slot, the rows read coalesced
__global__ __launch_bounds__(256) void pair_hist_sum_kernel(const uint32_t* __restrict__ partials, int rows, int slots,
                                                            long long* __restrict__ hist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= slots) return;
  unsigned long long s = 0;
  for (int w = 0; w < rows; ++w) s += partials[(size_t)w * slots + i];
  hist[i] = (long long)s;
}

int ph_check_shape(int M, int mode, int group) {
  if (pc_check_shape(M, mode, group, "fr_pair_hist", PH_MODES)) return -1;
  // a row of partials is uint32: one workgroup must see fewer than 2^32 pairs (16 384 per tile)
  const long long tiles = pc_geom(M, mode, group).parts;
  const long long grid = tiles < PH_GRID ? tiles : PH_GRID;
  if ((tiles + grid - 1) / grid >= (1LL << 32) / (PC_TILE * PC_TILE)) {
    FR_UNSUPPORTED("fr_pair_hist: M is too large (one workgroup would see 2^32 pairs or more)");
  }
  return 0;
}

}  // namespace

extern "C" int fr_pair_hist_parts(int M, int mode, int group) {
  if (ph_check_shape(M, mode, group)) return -1;
  const long long tiles = pc_geom(M, mode, group).parts;
  return (int)(tiles < PH_GRID ? tiles : PH_GRID);
}

extern "C" int fr_pair_hist(const float* E, int ldE, int M, int D, uint32_t key_lo, int shift, int NB, int mode, int group,
                            uint32_t* partials, int64_t* hist, void* stream) {
  if (ph_check_shape(M, mode, group)) return -1;
  if (NB < 1 || NB > PH_MAX_NB) FR_UNSUPPORTED("fr_pair_hist: 1 <= NB <= 2048 bins per launch");
  if (shift < 0 || shift > PH_MAX_SHIFT) FR_UNSUPPORTED("fr_pair_hist: 0 <= shift <= 21");
  if ((unsigned long long)key_lo + ((unsigned long long)NB << shift) > (1ULL << 32))
    FR_UNSUPPORTED("fr_pair_hist: the window key_lo + (NB << shift) must not pass 2^32");
  if (D < 4 || D > PC_MAX_D || D % 4) FR_UNSUPPORTED("fr_pair_hist: D must be a multiple of 4, 4 <= D <= 2048");
  if (ldE < D || ldE % 4) FR_UNSUPPORTED("fr_pair_hist: ldE >= D and ldE % 4 == 0 (16-byte row pitch)");
  if (!E || !partials || !hist) FR_UNSUPPORTED("fr_pair_hist: E, partials and hist are required");
  if ((uintptr_t)E % 16) FR_UNSUPPORTED("fr_pair_hist: E must be 16-byte aligned");
  const PcGeom s = pc_geom(M, mode, group);
  const int grid = (int)(s.parts < PH_GRID ? s.parts : PH_GRID);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_hist_kernel, dim3((unsigned)grid), dim3(256), 0, st, E, ldE, M, D, key_lo, shift, NB, mode,
                     mode == 0 ? 1 : group, s.nt, s.q, (uint32_t)s.parts, partials);
  hipLaunchKernelGGL(pair_hist_sum_kernel, dim3((unsigned)((NB + 2 + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)partials, grid, NB + 2, reinterpret_cast<long long*>(hist));
  FR_LAUNCH_CHECK();
}
