// frhip -- what the stride-2 3x3 kernels share on the device: the tap table of a parity plane / class (FrTaps) and the
// tap loop of the LDS-resident kernels (fr_mma_taps).  conv3x3_s2_strip.hip and conv3x3_s2_ws.hip run the loop with their
// own ring depths; conv3x3_s2_roll64.hip takes the gradient's taps from the table.
#pragma once
#include "common.h"

// Tap list of plane / class P = 2*ph + pw on the LOW-resolution grid (conv3x3_s2_strip.hip): NT = (ph ? 2 : 1) * (pw ? 2 : 1)
// taps; tap t -> (kernel tap index, LDS row and column offset).  Forward (KIND 0): kernel row kh reads high-res row
// 2i+kh-1 = plane row i-1 (kh = 0, ph = 1), i (kh = 1, ph = 0) or i (kh = 2, ph = 1); the image holds rows
// row0-1 .. row0+ROWS-1, so the LDS row offset is 0 or 1.  Data gradient (KIND 1): dx row 2i+ph collects g rows i+1 (kh = 0)
// and i (kh = 2) for ph = 1, g row i (kh = 1) for ph = 0; the image holds rows row0 .. row0+ROWS.  Columns alike.
template <int KIND, int P>
struct FrTaps {
  static constexpr int PH = P >> 1, PW = P & 1;
  static constexpr int NWD = PW ? 2 : 1, NT = (PH ? 2 : 1) * NWD;
  static constexpr int kh(int t) { return PH ? 2 * (t / NWD) : 1; }
  static constexpr int kw(int t) { return PW ? 2 * (t % NWD) : 1; }
  static constexpr int ktap(int t) { return kh(t) * 3 + kw(t); }
  static constexpr int roff(int t) { return KIND == 0 ? (PH ? t / NWD : 1) : (PH ? 1 - t / NWD : 0); }
  static constexpr int coff(int t) { return KIND == 0 ? (PW ? t % NWD : 1) : (PW ? 1 - t % NWD : 0); }
};

// acc += sum over the taps of T = FrTaps<KIND, P> and the CRES resident input channels of a layer with CIN of them: A
// fragments are single ds_read_b128 out of the LDS image `buf` (geometry C: TM x TN tiles per wave, RSTR / PSTR strides,
// abase0 = this lane's address for tap offset (0, 0), chunk 0), B fragments (weights) stream from global / L2 through wrow.
// A tap-step = one (tap, 32-channel chunk) = TM x TN MFMAs.  The caller's policy:
//   DB  weight ring depth == request distance in tap-steps;
//   D   A-fragment ring depth in (tap-step, M tile) steps of LDS-read lead (divides the steps of a body);
//   UC  32-channel chunks per unrolled body (a body holds a multiple of DB tap-steps).
template <class C, class T, int CIN, int CRES, int DB, int D, int UC>
__device__ __forceinline__ void fr_mma_taps(const char* buf, const int (&abase0)[C::TM], f32x4 (&acc)[C::TM][C::TN],
                                            const bf16_t* const (&wrow)[C::TN], const int wsh) {
  constexpr int NT = T::NT;
  constexpr int QB = UC * NT;  // tap-steps per body
  constexpr int NSTEP = QB * C::TM;
  static_assert((CRES / 32) % UC == 0 && QB % DB == 0 && DB <= QB && NSTEP % D == 0, "bad body shape");
  int abase[C::TM];
#pragma unroll
  for (int i = 0; i < C::TM; ++i) abase[i] = abase0[i];
  s16x8 bq[DB][C::TN];
  s16x8 ring[D];
  auto load_b = [&](int slot, int c0, int q) {
    const int t = q % NT, u = q / NT;
#pragma unroll
    for (int j = 0; j < C::TN; ++j)
      bq[slot][j] = *reinterpret_cast<const s16x8*>(wrow[j] + ((T::ktap(t) * CIN + c0 + u * 32) << wsh));
  };
  auto a_addr = [&](int step) -> const s16x8* {  // step in [0, 2*NSTEP): second half = next body
    const int wrap = step >= NSTEP ? 1 : 0;
    const int st = wrap ? step - NSTEP : step;
    const int q = st / C::TM, i = st - q * C::TM;
    const int t = q % NT, u = q / NT;
    return reinterpret_cast<const s16x8*>(buf + abase[i] + T::roff(t) * C::RSTR + T::coff(t) * C::PSTR + u * 64 +
                                          wrap * UC * 64);
  };
#pragma unroll
  for (int d = 0; d < DB; ++d) load_b(d, 0, d);
#pragma unroll
  for (int d = 0; d < D; ++d) ring[d] = *a_addr(d);
  for (int c0 = 0; c0 < CRES; c0 += 32 * UC) {
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
      const int q = st / C::TM, i = st - q * C::TM;
      const int slot = q % DB;
      const s16x8 a = ring[st % D];
#pragma unroll
      for (int j = 0; j < C::TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[slot][j], a, acc[i][j], 0, 0, 0);  // = (W X^T) tile
      ring[st % D] = *a_addr(st + D);  // past the last chunk this reads (never used) bytes inside the image's LDS slack
      if (i == C::TM - 1) {
        int nq = q + DB, nc = c0;
        if (nq >= QB) {
          nq -= QB;
          nc += 32 * UC;
        }
        nc = nc < CRES ? nc : CRES - 32 * UC;  // clamp instead of branching: the count of loads in flight stays static
        load_b(slot, nc, nq);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, C::TN, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
      if (i == C::TM - 1) __builtin_amdgcn_sched_barrier(0);  // keep the weight requests DB tap-steps ahead
    }
#pragma unroll
    for (int i = 0; i < C::TM; ++i) abase[i] += 64 * UC;
  }
}
