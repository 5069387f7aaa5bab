// internal view of the public C ABI (include/frhip.h is on the include path)
#pragma once
#include "frhip.h"

#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"  // U128 (pro8), FR_UNSUPPORTED (fr_by_pro)

// run-time switch `name` (api.hip): pointer to its cached value (environment variable of that name, else dflt)
int* fr_option_slot(const char* name, int dflt);
// FRHIP_XCD_ORDER=0: the strip kernels' workgroups take strips in dispatch order (A/B switch for tools/kbench.py); else 1
int fr_xcd_order();

// What a convolution family's shape table (select_strip, conv3x3_strip.hip; select_s2, conv3x3_s2_strip.hip) answers for a
// problem: the host queries report these fields and the entry point calls `launch`, so the two cannot disagree.
struct FrConvInstance {
  int parts;   // partial-sum rows the launch writes into FrConvArgs.part; 0: the family does not serve the problem
  bool frag;   // reads fragment-order weights (FrConvArgs.w_frag)
  bool resbn;  // serves the two-source prologues (FR_PRO_RESBN[_SE]) and FR_EPI_STATS_X
  int (*launch)(const FrConvArgs&, hipStream_t);
};
// strips of a batch for a strip geometry C (SC / S2) with NIMG images per workgroup: the partial-sum rows of a forward
// launch.  A table line computes `parts` from it and the launch its grid (x NSPL), so the two cannot differ.
template <class C, int NIMG>
constexpr int fr_strips_of(int B) {
  return B * C::NS / NIMG;
}

// Row segments per walk of a rolling-window kernel: `forced` when it is a candidate (option slot, test hook), else the first
// of the n ascending candidates that gives one workgroup per CU on 256 CUs (per_seg = work items at one segment), else the last
inline int fr_pick_nseg(const int* cand, int n, int forced, long long per_seg) {
  for (int k = 0; k < n; ++k)
    if (forced == cand[k]) return cand[k];
  for (int k = 0; k < n; ++k)
    if (per_seg * cand[k] >= 256) return cand[k];
  return cand[n - 1];
}

// out[i] = sum_g slab[g][i] in the fixed order g = 0, 1, ... (n elements, n % 4 == 0); conv_wgrad_strip.hip
int fr_launch_reduce_slabs(const float* slab, int groups, long long n, float* out, hipStream_t st);

// 64 -> 64 stride-1 3x3 layers on the rolling-window kernel (conv3x3_roll64.hip); a line of select_strip
bool fr_roll64_enabled();
int fr_roll64_parts(int B, int W);
int fr_roll64_launch(const FrConvArgs& a, hipStream_t st);

// 64-channel stride-2 3x3 layer (112 -> 56) and its data gradient on the rolling-window kernel (conv3x3_s2_roll64.hip);
// a line of select_s2
bool fr_s2roll_serves(const FrConvArgs& a);
int fr_s2roll_parts(int B);
int fr_s2roll_launch(const FrConvArgs& a, hipStream_t st);
bool fr_s2roll_enabled();

// What the table of the 3x3 weight-gradient family (select_wgrad, conv_wgrad_strip.hip) answers for a problem: the host
// queries report these fields and fr_conv_wgrad_strip calls `launch`, so the two cannot disagree.
struct FrWgradInstance {
  int fills;   // work items of the line's strip geometry: what fr_conv_wgrad_strip_groups caps the group count at
  int kernel;  // FR_WGRAD_*; FR_WGRAD_NONE: the family does not serve the problem
  int (*launch)(const FrWgradArgs&, hipStream_t);
};
// The warp-specialised kernels (conv_wgrad_roll.hip) as lines of select_wgrad: KERNEL = FR_WGRAD_ROLL / _VR / _S2ROLL at
// gradient width W.  fr_wgrad_ws_limit: the most groups (nsplit) a launch over B images takes -- one image, phase or
// virtual row each.  Instantiated in conv_wgrad_roll.hip for the widths each kernel has.
bool fr_wgrad_roll_enabled();
template <int KERNEL, int W>
int fr_wgrad_ws_limit(int B);
template <int KERNEL, int W>
int fr_wgrad_ws_launch(const FrWgradArgs& a, hipStream_t st);

// stride-2 3x3 forward at 128 / 256 / 512 channels on the warp-specialised kernel (conv3x3_s2_ws.hip); a line of
// select_s2.  fr_s2ws_strips: partial-sum rows of a served (B, C, low-res width), 0 = not served.
bool fr_s2ws_serves(const FrConvArgs& a);
int fr_s2ws_strips(int B, int C, int WL);
int fr_s2ws_launch(const FrConvArgs& a, hipStream_t st);

#if defined(__HIPCC__)
// prologue on one dword (two bf16): BN apply or PReLU, fp32 arithmetic, one rounding back to bf16
// Written as instructions: from the equivalent C the compiler rebuilds 16-bit compares + v_cndmask + v_perm (49 vector
// instructions per 16-byte chunk instead of 28) -- and these run on the SIMDs whose issue slots the MFMA waves need.
template <int PRO>
__device__ __forceinline__ uint32_t pro2(uint32_t u, float a0, float b0, float a1, float b1) {
  uint32_t lo, hi, r;
  if (PRO == FR_PRO_BN) {
    asm("v_lshlrev_b32 %0, 16, %3\n\t"
        "v_and_b32 %1, 0xffff0000, %3\n\t"
        "v_fma_f32 %0, %0, %4, %5\n\t"
        "v_fma_f32 %1, %1, %6, %7\n\t"
        "v_cvt_pk_bf16_f32 %2, %0, %1"
        : "=&v"(lo), "=&v"(hi), "=v"(r)
        : "v"(u), "v"(a0), "v"(b0), "v"(a1), "v"(b1));
    return r;
  }
  // PReLU: x > 0 ? x : a x.  Both halves scaled and packed; v_pk_ashrrev_i16 spreads the two sign bits into a mask and
  // v_bfi_b32 takes the scaled half where the sign is set, the input half elsewhere.  Same values as the compare form:
  // -0 and negative NaNs go through a x (x > 0 is false for them too), a x of a positive x is never selected.
  uint32_t m;
  asm("v_lshlrev_b32 %0, 16, %4\n\t"
      "v_and_b32 %1, 0xffff0000, %4\n\t"
      "v_mul_f32 %0, %0, %5\n\t"
      "v_mul_f32 %1, %1, %6\n\t"
      "v_cvt_pk_bf16_f32 %0, %0, %1\n\t"
      "v_pk_ashrrev_i16 %2, 15, %4 op_sel_hi:[0,1]\n\t"
      "v_bfi_b32 %3, %2, %0, %4"
      : "=&v"(lo), "=&v"(hi), "=&v"(m), "=v"(r)
      : "v"(u), "v"(a0), "v"(a1));
  return r;
}
// ... on one 16-byte chunk: eight channels with their coefficients a[j] (scale / slope) and b[j] (BN shift)
template <int PRO>
__device__ __forceinline__ U128 pro8(U128 x, const float (&a)[8], const float (&b)[8]) {
  x.x = pro2<PRO>(x.x, a[0], b[0], a[1], b[1]);
  x.y = pro2<PRO>(x.y, a[2], b[2], a[3], b[3]);
  x.z = pro2<PRO>(x.z, a[4], b[4], a[5], b[5]);
  x.w = pro2<PRO>(x.w, a[6], b[6], a[7], b[7]);
  return x;
}
// keep (all ones) or zero (0) a chunk without a branch: padding stays zero behind a prologue (BN would turn it into the shift)
__device__ __forceinline__ void fr_keep16(U128& x, unsigned keep) {
  x.x &= keep;
  x.y &= keep;
  x.z &= keep;
  x.w &= keep;
}
// Pins the uses of a loaded chunk behind this point of the program.  The instruction scheduler otherwise hoists the unpacking
// of the OTHER register set's chunks (committed after the next barrier) in front of the barrier, and with it their
// s_waitcnt: the wait then covers loads that were meant to stay in flight for another iteration.
__device__ __forceinline__ void pin(U128& a) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w)); }
// f(std::integral_constant<int, S>) ... f(std::integral_constant<int, N - 1>): a loop whose index is a constant expression
template <int S, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (S < N) {
    f(std::integral_constant<int, S>{});
    static_for<S + 1, N>(f);
  }
}
// the 64-channel rolling-window kernels: per-channel coefficients into LDS, by threads 0..63 -- coef = [pro_a | pro_b | epi_a]
// x 64 (0 where PRO / EA has no use for one)
template <int PRO, bool EA>
__device__ __forceinline__ void fr_roll_stage_coef(float* coef, const FrConvArgs& p, int tid) {
  coef[tid] = PRO != FR_PRO_NONE ? p.pro_a[tid] : 0.f;
  coef[64 + tid] = PRO == FR_PRO_BN ? p.pro_b[tid] : 0.f;
  coef[2 * 64 + tid] = EA ? p.epi_a[tid] : 0.f;
}
// staged chunk index -> (image, halo row, halo column) of NIMG stacked [GH][GW] halo images with CH 16-byte chunks per pixel
template <int NIMG, int GH, int GW, int CH>
__device__ __forceinline__ void fr_chunk_pixel(int idx, int& img, int& gh, int& gw) {
  int pc = idx / CH;
  img = NIMG > 1 ? pc / (GH * GW) : 0;
  pc -= img * (GH * GW);
  gh = pc / GW;
  gw = pc - gh * GW;
}

constexpr int FR_WGRAD_CT = 64;  // co and ci tile of every weight-gradient slab kernel

// Launch of one weight-gradient slab kernel instance (CT co x CT ci dW tiles x nsplit groups, `lds` bytes of dynamic LDS):
// attribute once per device, launch, error check, then the slab sum unless the caller defers it (prev_* of a later launch,
// or fr_reduce_slabs).  A plain launch on purpose, not FR_LAUNCH_KERNEL: an armed stop event (fr_arm_stop_event) must
// not attach to this kernel and complete before the slab sum behind it.
template <auto Kern>
int fr_launch_slab_kernel(const FrWgradArgs& a, hipStream_t st, int threads, int lds) {
  static unsigned long long attr_done = 0;  // one bit per device
  if (fr_attr_needed(attr_done)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    fr_attr_done(attr_done);
  }
  const int tiles = (a.Cout / FR_WGRAD_CT) * (a.SC / FR_WGRAD_CT);
  hipLaunchKernelGGL(Kern, dim3(tiles * a.nsplit), dim3(threads), lds, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fr_set_error(hipGetErrorString(e));
    return (int)e;
  }
  if (a.defer) return 0;
  return fr_launch_reduce_slabs(a.slab, a.nsplit, (long long)a.Cout * 9 * a.SC, a.dw, st);
}
// f(std::integral_constant<int, PRO>) for the one-source prologue of a launch; `unknown`: the calling family's message for
// any other value (default: the weight-gradient family's)
template <class F>
int fr_by_pro(int pro, F f, const char* unknown = "fr_conv_wgrad_strip: unknown prologue") {
  switch (pro) {
    case FR_PRO_NONE: return f(std::integral_constant<int, FR_PRO_NONE>{});
    case FR_PRO_BN: return f(std::integral_constant<int, FR_PRO_BN>{});
    case FR_PRO_PRELU: return f(std::integral_constant<int, FR_PRO_PRELU>{});
  }
  FR_UNSUPPORTED(unknown);
}
#endif
