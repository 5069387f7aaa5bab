// frhip -- the epilogue arithmetic of the bf16 MFMA-tile kernels (LDS strips, stride-2 strips, rolling windows, the
// warp-specialised stride-2 kernel, the 1x1 stream and the stem GEMM): what each FR_EPI_* kind computes, written once.
//
// The kernels run their MFMAs with the weights as the A operand, so a lane holds, per 16x16 tile, FOUR CONSECUTIVE
// CHANNELS (fq*4 + r) of ONE pixel (fr = lane & 15): a "cell", 8 bytes of bf16 in the output tile.  The helpers below
// take plain values; where the coefficients and the aux cell come from, and the order of the loops, stay with the kernel.
#pragma once
#include <type_traits>
#include "common.h"
#include "frhip.h"

// ---------------------------------------------------------------------------------------------------------------- kinds
__host__ __device__ constexpr bool fr_epi_reads_aux(int e) {  // the cell holds aux (PReLU / BN input, shortcut) first
  return e == FR_EPI_PRELU_BWD || e == FR_EPI_BNBWD || e == FR_EPI_BIAS_RES || e == FR_EPI_STATS_X;
}
__host__ __device__ constexpr bool fr_epi_uses_a(int e) {
  return e == FR_EPI_PRELU_BWD || e == FR_EPI_BNBWD || e == FR_EPI_BIAS_RES;
}
__host__ __device__ constexpr bool fr_epi_uses_b(int e) { return e == FR_EPI_BNBWD || e == FR_EPI_BIAS_RES; }
__host__ __device__ constexpr bool fr_epi_has_sums(int e) {  // leaves part rows
  return e == FR_EPI_STATS || e == FR_EPI_PRELU_BWD || e == FR_EPI_BNBWD || e == FR_EPI_STATS_X;
}
__host__ __device__ constexpr int fr_epi_nsums(int e) { return e == FR_EPI_STATS_X ? 3 : 2; }  // part rows per kind

// The epilogue kind is a run-time argument, but inside the per-element loops it must be a compile-time constant: with
// `epi` tested per element the compiler emitted a scalar branch per accumulator (8000 instructions, ~10 us).  Calls
// f(std::integral_constant<int, E>{}) for the first listed kind E equal to epi; the LAST listed kind takes every other value.
template <int E, int... Es, class F>
__device__ __forceinline__ void fr_epi_dispatch(int epi, F&& f) {
  if constexpr (sizeof...(Es) == 0) {
    f(std::integral_constant<int, E>{});
  } else {
    if (epi == E) f(std::integral_constant<int, E>{});
    else fr_epi_dispatch<Es...>(epi, f);
  }
}

// ---------------------------------------------------------------------------------------------------------------- cells
__device__ __forceinline__ void fr_cell_unpack(uint2 u, float (&x)[4]) {
  x[0] = __uint_as_float(u.x << 16);
  x[1] = __uint_as_float(u.x & 0xFFFF0000u);
  x[2] = __uint_as_float(u.y << 16);
  x[3] = __uint_as_float(u.y & 0xFFFF0000u);
}
__device__ __forceinline__ uint2 fr_cell_pack(const float (&v)[4]) {
  uint2 o;
  o.x = pack2bf(v[0], v[1]);
  o.y = pack2bf(v[2], v[3]);
  return o;
}

// One cell of kind E: v = the fp32 accumulators (rewritten to the value stored), x = the aux cell (fr_epi_reads_aux),
// ea / eb = epi_a / epi_b of the four channels (fr_epi_uses_a / _b); adds the cell to the per-channel sums s0 .. s2 (s2:
// FR_EPI_STATS_X only).  Arguments a kind does not read may be null.  The FR_EPI_* comments of frhip.h define the kinds.
template <int E>
__device__ __forceinline__ void fr_epi_cell(float (&v)[4], const float* x, const float* ea, const float* eb, float* s0,
                                            float* s1, float* s2 = nullptr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (E == FR_EPI_STATS) {
      s0[r] += v[r];
      s1[r] = fmaf(v[r], v[r], s1[r]);
    } else if (E == FR_EPI_STATS_X) {  // + the cross moment with the residual input (fr_bn_finalize_res)
      s0[r] += v[r];
      s1[r] = fmaf(v[r], v[r], s1[r]);
      s2[r] = fmaf(v[r], x[r], s2[r]);
    } else if (E == FR_EPI_PRELU_BWD) {
      const bool pos = x[r] > 0.f;
      s0[r] += pos ? 0.f : v[r] * x[r];
      v[r] = pos ? v[r] : v[r] * ea[r];
    } else if (E == FR_EPI_BNBWD) {
      s0[r] += v[r];
      s1[r] = fmaf(v[r], (x[r] - ea[r]) * eb[r], s1[r]);
    } else if (E == FR_EPI_BIAS_RES) {
      v[r] += ea[r] + eb[r] + x[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- sums
// folds NV per-channel sums over the 16 pixel lanes of a tile (lane bits 0..3), side by side; every lane gets the totals
template <int NV>
__device__ __forceinline__ void fr_fold16(float (&s)[NV]) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1)
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] += __shfl_xor(s[k], o, 64);
}

// folds the NV sums of column col and parks them, from lane fr == 0, in the LDS rows red[wm][k][ld] (k < NV), which the
// kernel then adds over its row groups wm into one part row
template <int NV>
__device__ __forceinline__ void fr_fold16_park(float* red, int ld, int wm, int col, int fr, float s0, float s1,
                                               float s2 = 0.f) {
  float s[NV];
  s[0] = s0;
  s[1] = s1;
  if constexpr (NV == 3) s[2] = s2;
  fr_fold16(s);
  if (fr == 0) {
    red[(wm * NV + 0) * ld + col] = s[0];
    red[(wm * NV + 1) * ld + col] = s[1];
    if constexpr (NV == 3) red[(wm * NV + 2) * ld + col] = s[2];
  }
}
