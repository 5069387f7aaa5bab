// frhip -- the stride-2 3x3 convolution of the first unit of every stage (bottleneck_IR conv2 with stride 2,
// backbone/model_irse.py:57-59) and its data gradient, as LDS-resident strips (bf16, gfx950).
//
// Both directions are written on the LOW-resolution grid (HL x WL = the output of the forward convolution).  A
// stride-2 window touches the four parity planes x[2i+ph][2j+pw] of the high-resolution image with 1, 2, 2 and 4 of
// its 9 taps, and inside one plane those taps are plain neighbour offsets (0 / -1 rows and columns).  So
//   forward (KIND 0):   y[i][j] = sum over the 4 planes of a small stride-1 "convolution" of that plane -- a workgroup
//                       owning ROWS low-res rows of one image stages one plane at a time in LDS (prologue applied once)
//                       and accumulates all four into the same MFMA accumulators;
//   data gradient (KIND 1): dx[2i+ph][2j+pw] = the same kind of sum over the low-res gradient g (offsets 0 / +1) with
//                       the taps of class (ph, pw) -- the g strip is staged once and the four output classes are
//                       produced one after the other, each with its own fused epilogue (PReLU backward of
//                       model_irse.py:58 / BN-backward sums) and 9/4 taps per pixel instead of 9.
// Everything else follows conv3x3_strip.hip: A fragments are single ds_read_b128 at (row register + immediate tap
// offset) out of a conflict-free padded [pixel][channel] image, weights stream L2 -> registers (2-deep ring, requested
// two tap-steps ahead), no barrier inside a tap list, bf16 results leave through an LDS tile as row-contiguous
// 16-byte stores.  Same contracts as fr_conv_igemm (mode 0 stride 2 / mode 2): bit-compatible layouts of src, w,
// out, aux and the column partial sums.
// Shared with the other 3x3 kernels: the tap table and the tap loop (conv_taps.h: FrTaps, fr_mma_taps; the ring depths are
// this file's), the epilogue cells (conv_epilogue.h), the prologue pro8, fr_chunk_pixel and the prologue switch fr_by_pro
// (frhip_internal.h), the launch fr_launch_lds (common.h).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "conv_epilogue.h"
#include "conv_taps.h"
#include "frhip_internal.h"

#ifdef FRHIP_STAMPS
// Diagnostic build only (make stamps -> libfrhip_stamps.so; never the product library): wave 0 of every workgroup writes
// s_memrealtime (100 MHz) at its phase boundaries to a buffer of its own (16 slots per workgroup), read by tools/stamps_s2.py.
__device__ unsigned long long* fr_stamp_buf_s2 = nullptr;
extern "C" int fr_debug_set_stamp_buffer_s2(unsigned long long* dev_ptr) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(fr_stamp_buf_s2), &dev_ptr, sizeof(dev_ptr));
}
#define S2_STAMP(k)                                                                                          \
  do {                                                                                                       \
    if (threadIdx.x == 0 && fr_stamp_buf_s2) fr_stamp_buf_s2[(size_t)blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define S2_STAMP(k)
#endif

namespace {

// COUT is the width ONE workgroup computes (NSPL workgroups share a strip, conv3x3_strip.hip); NIMG > 1: a workgroup owns
// NIMG whole images (ROWS == WL) stacked in LDS, so that a weight fragment feeds NIMG x ROWS x WL pixels.
template <int CIN, int COUT, int WL, int ROWS, int WN, int NW, int KIND, int NIMG = 1>
struct S2 {
  static constexpr int NTH = NW * 64;
  static constexpr int HL = WL;
  static constexpr int GW = WL + 1;                        // one halo column (left: forward, right: gradient)
  static constexpr int GH = ROWS + 1;                      // one halo row
  static constexpr int CH = CIN / 8;
  static constexpr int PPAD = CIN == 64 ? 16 : 32;         // see conv3x3_strip.hip: conflict-free pixel stride
  static constexpr int PSTR = CIN * 2 + PPAD;
  // row stride: the 16-byte slot index keeps counting across a row wrap of an M tile (slot(h+1, 0) == slot(h, WL) mod 16)
  // (multi-image instances: the same residue with the next row starting INSIDE the last pixel's 32 padding bytes -- 256 B
  // less per row, which is what lets two 512-channel gradient images sit beside the output tile)
  static constexpr bool TIGHT = NIMG > 1 && PSTR % 256 <= PPAD;
  static constexpr int RSTR = TIGHT ? GW * PSTR - PSTR % 256 : GW * PSTR + (256 - PSTR % 256) % 256;
  static constexpr int ISTR = GH * RSTR;                   // one image (NIMG > 1)
  static constexpr int IMG_BYTES = NIMG * ISTR + 512;      // + slack for ring reads past the last channel chunk
  static constexpr int M = NIMG * ROWS * WL;
  static constexpr int MT = (M + 15) / 16;
  static constexpr int WM = NW / WN;
  static constexpr int TN = COUT / 16 / WN;
  static constexpr int TM = (MT + WM - 1) / WM;
  static constexpr int OSTR = COUT * 2 + 16;
  static constexpr int OUT_BYTES = (M * OSTR + 15) / 16 * 16;
  static constexpr int RED_BYTES = WM * 2 * COUT * 4;
  // forward: the output tile reuses the (dead) plane image; gradient: the g strip stays live across the four classes
  static constexpr int OUT_OFF = KIND == 0 ? 0 : (IMG_BYTES + 15) / 16 * 16;
  static constexpr int SYNC_OFF = OUT_OFF + OUT_BYTES + RED_BYTES;  // gradient: counters of the half-workgroup barriers
  static constexpr int LDS = KIND == 0 ? (IMG_BYTES > OUT_BYTES + RED_BYTES ? IMG_BYTES : OUT_BYTES + RED_BYTES)
                                       : SYNC_OFF + 64;
  static constexpr int NS = HL / ROWS;
  static_assert(HL % ROWS == 0, "strip rows must divide the low-res image");
  static_assert(NIMG == 1 || ROWS == WL, "multi-image workgroups own whole images");
  static_assert(NTH % CH == 0, "threads must be a multiple of the chunks per pixel");
  static_assert(COUT % (16 * WN) == 0 && NW % WN == 0, "bad wave split");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

// acc += sum over the taps of (KIND, P) and all CIN channels, A from the LDS image, B from global/L2: the shared tap loop
// (conv_taps.h) with the strip instances' ring depths
template <class C, int CIN, int KIND, int P>
__device__ __forceinline__ void mma_taps(const char* smem, const int (&abase0)[C::TM], f32x4 (&acc)[C::TM][C::TN],
                                         const bf16_t* const (&wrow)[C::TN], const int wsh) {
  using T = FrTaps<KIND, P>;
  constexpr int UC = T::NT == 1 ? 2 : 1;  // 32-channel chunks per unrolled body (so that a body holds >= 2 tap-steps: 2, 2, 2, 4)
  constexpr int DB = 2;                   // weight ring depth == request distance in tap-steps
  // A ring depth (divides the steps of a body): one slot per M tile; 2 in the whole-image 256-channel instance (13 slots:
  // 8-76 bytes of scratch, same time)
  constexpr int D = (C::TM == 13 && CIN >= 256) ? 2 : C::TM;
  static_assert(D * 4 + C::TM * C::TN * 4 <= 140, "fragment ring + accumulators: register budget");
  fr_mma_taps<C, T, CIN, CIN, DB, D, UC>(smem, abase0, acc, wrow, wsh);
}

template <int CIN, int COUT, int WL, int ROWS, int WN, int NW, int KIND, int PRO, int NSPL = 1, int NIMG = 1>
__global__ __launch_bounds__(NW * 64, 2) void conv3x3_s2_kernel(const FrConvArgs p, const int xcd) {
  using C = S2<CIN, COUT, WL, ROWS, WN, NW, KIND, NIMG>;
  constexpr int NTH = C::NTH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const otile = smem + C::OUT_OFF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const bf16_t* __restrict__ src = reinterpret_cast<const bf16_t*>(p.src);
  const bf16_t* __restrict__ wgt = reinterpret_cast<const bf16_t*>(p.w);
  bf16_t* __restrict__ out = reinterpret_cast<bf16_t*>(p.out);

  const int lb = (xcd & 1) ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;  // halo-sharing strips (and the NSPL parts of one
                                                                         // strip) meet in one XCD's L2
  const int nh = NSPL > 1 ? lb % NSPL : 0;
  const int ncol0 = nh * COUT;                                           // first output channel of this workgroup
  const int sblk = NSPL > 1 ? lb / NSPL : lb;
  const int nstrips = gridDim.x / NSPL;
  const int b = NIMG > 1 ? sblk * NIMG : sblk / C::NS;                   // (first) image of the strip
  const int row0 = NIMG > 1 ? 0 : (sblk - b * C::NS) * ROWS;
  constexpr int PLANE = C::GH * C::GW;                                   // staged pixels per image

  // ------------------------------------------------------------------ image loader (prologue applied once)
  constexpr int TOTAL = NIMG * C::GH * C::GW * C::CH;
  const int ch = tid % C::CH;
  float pa[8], pb[8];
  if (PRO != FR_PRO_NONE) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pa[j] = p.pro_a[ch * 8 + j];
      pb[j] = PRO == FR_PRO_BN ? p.pro_b[ch * 8 + j] : 0.f;
    }
  }
  auto load_image = [&](int ph, int pw) {
    // one batch when it is at most 16 loads per thread: a second trip of this loop costs a second HBM round trip, and the
    // compiler answered the two-trip form with kilobytes of scratch in the whole-image 256-channel instance
    constexpr int PER = (TOTAL + NTH - 1) / NTH;
    constexpr int UNR = PER <= 16 ? PER : 8;
    for (int base = 0; base < TOTAL; base += NTH * UNR) {
      U128 v[UNR];
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = base + u * NTH + tid;
        int img, gh, gw;
        fr_chunk_pixel<NIMG, C::GH, C::GW, C::CH>(idx, img, gh, gw);
        size_t pix;
        if (KIND == 0) {  // plane (ph, pw) of the high-res input: low-res rows row0-1 .. row0+ROWS-1, columns -1 .. WL-1
          const int i = row0 + gh - 1, j = gw - 1;
          ok[u] = idx < TOTAL && i >= 0 && j >= 0;
          pix = ((size_t)((b + img) * 2 * C::HL + 2 * i + ph) * (2 * WL) + 2 * j + pw);
        } else {          // low-res gradient rows row0 .. row0+ROWS, columns 0 .. WL
          const int i = row0 + gh, j = gw;
          ok[u] = idx < TOTAL && i < C::HL && j < WL;
          pix = ((size_t)((b + img) * C::HL + i) * WL + j);
        }
        v[u] = ok[u] ? ld16(src + pix * (size_t)p.lda + ch * 8) : zero16();
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = base + u * NTH + tid;
        if (idx < TOTAL) {
          int img, gh, gw;
          fr_chunk_pixel<NIMG, C::GH, C::GW, C::CH>(idx, img, gh, gw);
          U128 x = v[u];
          if (PRO != FR_PRO_NONE && ok[u]) {  // pro2 (frhip_internal.h): the prologue on packed pairs
            x = pro8<PRO>(x, pa, pb);
          }
          st16(smem + img * C::ISTR + gh * C::RSTR + gw * C::PSTR + ch * 16, x);
        }
      }
    }
  };

  // Forward: the NEXT plane is requested into registers before the taps of the current one run and committed after them
  // (one workgroup per CU at 256 / 512 channels: nothing else hides the load latency of the four phases).
  // Only where the register budget is spent anyway: at 64 / 128 channels the 20-32 extra registers cost a resident workgroup
  // (128 -> 128 @28: 0.166 -> 0.196 ms with the prefetch).
  // Round 3, measured again with 7-row strips (tools/ab_libs.sh, one box): the prefetch at 128 channels 0.1355 -> 0.1372 ms;
  // two plane buffers (commit into the buffer the taps are not reading, one barrier per plane instead of two)
  // 128 ch 0.1355 -> 0.137, 256 ch 0.1066 -> 0.118 (costs the second resident workgroup), 512 ch 0.148 -> 0.147: the plane
  // loads are not what these kernels wait for.  4-wave workgroups at 128 channels (13 M tiles per wave, half the weight
  // stream): 170-3000 bytes of scratch per lane in every instance.
  constexpr int NPF = (TOTAL + NTH - 1) / NTH;
#ifndef FRHIP_S2_PFP_BUDGET
#define FRHIP_S2_PFP_BUDGET 150
#endif
  // ... and only where prefetch registers + accumulators + fragment ring fit (the whole-image 256-channel instance: 15
  // prefetch registers x 4 + 52 + 52 -> 370-520 bytes of scratch with it)
  constexpr bool PFP = KIND == 0 && CIN >= 256 && NPF * 4 + C::TM * C::TN * 4 + C::TM * 4 <= FRHIP_S2_PFP_BUDGET;
  U128 pf[PFP ? NPF : 1];
  unsigned pfok = 0;
  auto issue_plane = [&](int ph, int pw) {
    pfok = 0;
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int idx = u * NTH + tid;
      int pc = idx / C::CH;  // (not fr_chunk_pixel: through the helper the prefetching 512-channel kernels change)
      const int img = NIMG > 1 ? pc / PLANE : 0;
      pc -= img * PLANE;
      const int gh = pc / C::GW, gw = pc - gh * C::GW;
      const int i = row0 + gh - 1, j = gw - 1;
      const bool ok = idx < TOTAL && i >= 0 && j >= 0;
      const size_t pix = ((size_t)((b + img) * 2 * C::HL + 2 * i + ph) * (2 * WL) + 2 * j + pw);
      pf[PFP ? u : 0] = ok ? ld16(src + pix * (size_t)p.lda + ch * 8) : zero16();
      pfok |= ok ? (1u << u) : 0u;
    }
  };
  auto commit_plane = [&]() {
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int idx = u * NTH + tid;
      if (idx < TOTAL) {
        int img, gh, gw;
        fr_chunk_pixel<NIMG, C::GH, C::GW, C::CH>(idx, img, gh, gw);
        U128 x = pf[PFP ? u : 0];
        if (PRO != FR_PRO_NONE && ((pfok >> u) & 1u)) {
          x = pro8<PRO>(x, pa, pb);
        }
        st16(smem + img * C::ISTR + gh * C::RSTR + gw * C::PSTR + ch * 16, x);
      }
    }
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = wn * C::TN * 16;
  const bf16_t* wrow[C::TN];
#pragma unroll
  for (int j = 0; j < C::TN; ++j) wrow[j] = wgt + (size_t)(ncol0 + n0 + j * 16 + fr) * 9 * CIN + fq * 8;
  const int wsh = p.w_frag ? 4 : 0;  // weights in MFMA-fragment order (FrConvArgs.w_frag; conv3x3_strip.hip): 1024 contiguous bytes per load
  if (wsh) {
#pragma unroll
    for (int j = 0; j < C::TN; ++j) wrow[j] = wgt + (size_t)((ncol0 + n0) / 16 + j) * 16 * 9 * CIN + lane * 8;
  }
  int abase[C::TM];
#pragma unroll
  for (int i = 0; i < C::TM; ++i) {
    int m = (wm * C::TM + i) * 16 + fr;
    m = m < C::M ? m : 0;
    const int img = NIMG > 1 ? m / (ROWS * WL) : 0;
    m -= img * (ROWS * WL);
    const int h = m / WL, w = m - h * WL;
    abase[i] = img * C::ISTR + h * C::RSTR + w * C::PSTR + fq * 16;
  }
  const int epi = p.epi;
  const bool stats = epi == FR_EPI_STATS || epi == FR_EPI_PRELU_BWD || epi == FR_EPI_BNBWD;
  constexpr int OCH = COUT / 8;
  // Round 6, data gradient: the two HALVES of the workgroup run half a class out of step.  A wave owns 16 (or 32) output
  // channels of every pixel, waves w and w + 4 share a SIMD; with all eight in lock-step the SIMD's matrix pipe idles through
  // every epilogue (aux tile -> LDS, PReLU-backward cells, tile -> global: 5.2 of the 9.5 us a class takes, tools/stamps_s2.py)
  // and its vector pipe through every tap list.  The halves touch disjoint columns of the output tile and of the reduction
  // scratch, so each gets barriers of its own (an LDS counter, 4 waves) and waves 4-7 start their first tap list when waves
  // 0-3 have finished theirs: from then on one wave of a SIMD issues MFMAs while the other runs its epilogue.  Same
  // arithmetic, same order: bit-identical.
  constexpr bool STG = KIND == 1 && NW == 8 && WN == 8;
  const int half = STG ? wave >> 2 : 0;
  const int htid = STG ? (tid & 255) : tid;
  const int hnth = STG ? 256 : NTH;
  const int hoch = STG ? OCH / 2 : OCH;       // 16-byte chunks of a tile row this half moves
  const int hc0 = half * hoch;
  volatile unsigned* hctr = reinterpret_cast<volatile unsigned*>(smem + C::SYNC_OFF) + half;  // [0], [1]: barrier counters; [2]: start flag
  unsigned hgen = 0;
  auto hsync = [&]() {
    if constexpr (!STG) {
      __syncthreads();
      return;
    }
    hgen += 4;  // four waves arrive per barrier; the counter only grows
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_fetch_add(const_cast<unsigned*>(hctr), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (*hctr < hgen) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  f32x4 acc[C::TM][C::TN];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < C::TM; ++i)
#pragma unroll
      for (int j = 0; j < C::TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };

  // ------------------------------------------------------------------ epilogue of one output class
  // cls < 0: forward (output pixel = low-res pixel); cls = 2*ph + pw: gradient class (output pixel (2i+ph, 2j+pw))
  // aux cells of one output class: requested before the taps of that class run (data gradient), written into the output
  // tile behind them
  constexpr int NAX = (C::M * OCH + NTH - 1) / NTH;
  U128 axr[KIND == 1 ? NAX : 1];  // forward (inference epilogue only): loaded inside the epilogue, no registers held across the taps
  const bool has_aux = epi == FR_EPI_PRELU_BWD || epi == FR_EPI_BNBWD || epi == FR_EPI_BIAS_RES;
  auto out_pix = [&](int cls, int r) -> size_t {
    const int ph = cls < 0 ? 0 : cls >> 1, pw = cls < 0 ? 0 : cls & 1;
    const int img = NIMG > 1 ? r / (ROWS * WL) : 0;
    r -= img * (ROWS * WL);
    const int h = r / WL, w = r - h * WL;
    if (KIND == 0) return (size_t)((b + img) * C::HL + row0 + h) * WL + w;
    return (size_t)((b + img) * 2 * C::HL + 2 * (row0 + h) + ph) * (2 * WL) + 2 * w + pw;
  };
  auto issue_aux = [&](int cls) {
    if (KIND == 1 && has_aux) {
      const bf16_t* __restrict__ aux = reinterpret_cast<const bf16_t*>(p.aux);
#pragma unroll
      for (int u = 0; u < NAX; ++u) {
        int idx = u * hnth + htid;
        idx = idx < C::M * hoch ? idx : C::M * hoch - 1;
        const int r = idx / hoch, c8 = hc0 + idx - r * hoch;
        axr[KIND == 1 ? u : 0] = ld16(aux + out_pix(cls, r) * (size_t)p.ldaux + ncol0 + c8 * 8);
      }
    }
  };
  auto epilogue = [&](int cls) {
    auto dst_pix = [&](int r) -> size_t { return out_pix(cls, r); };
    if (has_aux) {
      if (KIND == 1) {
#pragma unroll
        for (int u = 0; u < NAX; ++u) {
          const int idx = u * hnth + htid;
          if (idx < C::M * hoch) {
            const int r = idx / hoch, c8 = hc0 + idx - r * hoch;
            st16(otile + r * C::OSTR + c8 * 16, axr[KIND == 1 ? u : 0]);
          }
        }
      } else {
        const bf16_t* __restrict__ aux = reinterpret_cast<const bf16_t*>(p.aux);
        for (int idx = tid; idx < C::M * OCH; idx += NTH) {
          const int r = idx / OCH, c8 = idx - r * OCH;
          st16(otile + r * C::OSTR + c8 * 16, ld16(aux + dst_pix(r) * (size_t)p.ldaux + ncol0 + c8 * 8));
        }
      }
      hsync();
    }
    // weights were the MFMA A operand: a lane holds four consecutive channels (fq*4 + r) of one pixel (fr) per tile
    float* red = reinterpret_cast<float*>(otile + C::OUT_BYTES);  // [WM][2][COUT] column sums, behind the output tile
    auto cells = [&](auto tag) {
      constexpr int E = decltype(tag)::value;
      float ea[C::TN][4], eb[C::TN][4], s0[C::TN][4], s1[C::TN][4];
  #pragma unroll
      for (int j = 0; j < C::TN; ++j)
  #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = ncol0 + n0 + j * 16 + fq * 4 + r;
          ea[j][r] = fr_epi_uses_a(E) ? p.epi_a[n] : 0.f;
          eb[j][r] = fr_epi_uses_b(E) ? p.epi_b[n] : 0.f;
          s0[j][r] = s1[j][r] = 0.f;
        }
  #pragma unroll
      for (int i = 0; i < C::TM; ++i) {
        const int m = (wm * C::TM + i) * 16 + fr;
        if (wm * C::TM + i >= C::MT || m >= C::M) continue;
  #pragma unroll
        for (int j = 0; j < C::TN; ++j) {
          uint2* cell = reinterpret_cast<uint2*>(otile + m * C::OSTR + (n0 + j * 16 + fq * 4) * 2);
          float v[4], x[4];
  #pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
          if (fr_epi_reads_aux(E)) fr_cell_unpack(*cell, x);
          fr_epi_cell<E>(v, x, ea[j], eb[j], s0[j], s1[j]);
          *cell = fr_cell_pack(v);
        }
      }
      if (fr_epi_has_sums(E)) {
  #pragma unroll
        for (int j = 0; j < C::TN; ++j)
  #pragma unroll
          for (int r = 0; r < 4; ++r) fr_fold16_park<2>(red, COUT, wm, n0 + j * 16 + fq * 4 + r, fr, s0[j][r], s1[j][r]);
      }
    };
    fr_epi_dispatch<FR_EPI_STATS, FR_EPI_PRELU_BWD, FR_EPI_BNBWD, FR_EPI_BIAS_RES, FR_EPI_STORE>(epi, cells);
    hsync();
    for (int idx = htid; idx < C::M * hoch; idx += hnth) {
      const int r = idx / hoch, c8 = hc0 + idx - r * hoch;
      st16(out + dst_pix(r) * (size_t)p.ldc + ncol0 + c8 * 8, ld16(otile + r * C::OSTR + c8 * 16));
    }
    if (stats) {
      const size_t prow = (size_t)(cls < 0 ? 0 : cls) * nstrips + sblk;  // gradient: rows ordered [class][strip]
      const int hcout = STG ? COUT / 2 : COUT;
      for (int c = htid; c < 2 * hcout; c += hnth) {
        const int k = c / hcout, n = half * hcout + c - k * hcout;
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < C::WM; ++g) t += red[(g * 2 + k) * COUT + n];
        st_part(p.part + (prow * 2 + k) * (COUT * NSPL) + ncol0 + n, t);
      }
    }
    hsync();  // the tile and the reduction scratch (this half's columns) are free again
  };

  if (KIND == 0 && !PFP) {
    zero_acc();
    S2_STAMP(0);
    load_image(0, 0);
    S2_STAMP(1);
    __syncthreads();
    S2_STAMP(2);
    mma_taps<C, CIN, 0, 0>(smem, abase, acc, wrow, wsh);
    S2_STAMP(3);
    __syncthreads();  // every wave is done reading the plane
    S2_STAMP(4);
    load_image(0, 1);
    __syncthreads();
    S2_STAMP(5);
    mma_taps<C, CIN, 0, 1>(smem, abase, acc, wrow, wsh);
    __syncthreads();
    S2_STAMP(6);
    load_image(1, 0);
    __syncthreads();
    S2_STAMP(7);
    mma_taps<C, CIN, 0, 2>(smem, abase, acc, wrow, wsh);
    __syncthreads();
    S2_STAMP(8);
    load_image(1, 1);
    S2_STAMP(9);
    __syncthreads();
    S2_STAMP(10);
    issue_aux(-1);
    mma_taps<C, CIN, 0, 3>(smem, abase, acc, wrow, wsh);
    S2_STAMP(11);
    __syncthreads();  // LDS is now the output tile
    S2_STAMP(12);
    epilogue(-1);
    S2_STAMP(13);
  } else if (KIND == 0) {
    zero_acc();
    issue_plane(0, 0);
    commit_plane();
    __syncthreads();
    issue_plane(0, 1);
    mma_taps<C, CIN, 0, 0>(smem, abase, acc, wrow, wsh);
    __syncthreads();  // every wave is done reading the plane
    commit_plane();
    __syncthreads();
    issue_plane(1, 0);
    mma_taps<C, CIN, 0, 1>(smem, abase, acc, wrow, wsh);
    __syncthreads();
    commit_plane();
    __syncthreads();
    issue_plane(1, 1);
    mma_taps<C, CIN, 0, 2>(smem, abase, acc, wrow, wsh);
    __syncthreads();
    commit_plane();
    __syncthreads();
    issue_aux(-1);
    mma_taps<C, CIN, 0, 3>(smem, abase, acc, wrow, wsh);
    __syncthreads();  // LDS is now the output tile
    epilogue(-1);
  } else {
    S2_STAMP(0);
    if (STG && tid < 4) reinterpret_cast<unsigned*>(smem + C::SYNC_OFF)[tid] = 0u;
    load_image(0, 0);
    S2_STAMP(1);
    __syncthreads();
    S2_STAMP(2);
    zero_acc();
    issue_aux(0);
    if constexpr (STG) {
      volatile unsigned* start = reinterpret_cast<volatile unsigned*>(smem + C::SYNC_OFF) + 2;
      if (half == 1) {  // half a class behind: wait for waves 0-3 to finish their first tap list
        while (*start < 4u) __builtin_amdgcn_s_sleep(2);
      }
      mma_taps<C, CIN, 1, 0>(smem, abase, acc, wrow, wsh);
      if (half == 0 && lane == 0)
        __hip_atomic_fetch_add(const_cast<unsigned*>(start), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      mma_taps<C, CIN, 1, 0>(smem, abase, acc, wrow, wsh);
    }
    S2_STAMP(3);
    epilogue(0);
    S2_STAMP(4);
    zero_acc();
    issue_aux(1);
    mma_taps<C, CIN, 1, 1>(smem, abase, acc, wrow, wsh);
    S2_STAMP(5);
    epilogue(1);
    S2_STAMP(6);
    zero_acc();
    issue_aux(2);
    mma_taps<C, CIN, 1, 2>(smem, abase, acc, wrow, wsh);
    S2_STAMP(7);
    epilogue(2);
    S2_STAMP(8);
    zero_acc();
    issue_aux(3);
    mma_taps<C, CIN, 1, 3>(smem, abase, acc, wrow, wsh);
    S2_STAMP(9);
    epilogue(3);
    S2_STAMP(10);
  }
}

template <int CIN, int COUT, int WL, int ROWS, int WN, int NW, int KIND, int PRO, int NSPL, int NIMG>
int launch(const FrConvArgs& a, hipStream_t st) {
  using C = S2<CIN, COUT, WL, ROWS, WN, NW, KIND, NIMG>;
  return fr_launch_lds<&conv3x3_s2_kernel<CIN, COUT, WL, ROWS, WN, NW, KIND, PRO, NSPL, NIMG>>(
      fr_strips_of<C, NIMG>(a.B) * NSPL, C::NTH, C::LDS, st, a, fr_xcd_order());
}

template <int CIN, int COUT, int WL, int ROWS, int WN, int NW, int KIND, int NSPL = 1, int NIMG = 1>
int by_pro(const FrConvArgs& a, hipStream_t st) {
  return fr_by_pro(
      a.pro, [&](auto pro) { return launch<CIN, COUT, WL, ROWS, WN, NW, KIND, decltype(pro)::value, NSPL, NIMG>(a, st); },
      "fr_conv3x3_s2_strip: unknown prologue");
}

// One line of the table: an LDS-strip instance of one KIND (0: forward, one partial-sum row per strip; 1: data gradient,
// 4 parity classes x strips, ordered [class][strip]).  Fragment-order weights but at 64 channels.
template <int KIND, int CIN, int COUT, int WL, int ROWS, int WN, int NW, int NSPL = 1, int NIMG = 1>
FrConvInstance s2(int B) {
  return {(KIND ? 4 : 1) * fr_strips_of<S2<CIN, COUT, WL, ROWS, WN, NW, KIND, NIMG>, NIMG>(B), CIN != 64, false,
          &by_pro<CIN, COUT, WL, ROWS, WN, NW, KIND, NSPL, NIMG>};
}
// ... of both kinds
template <int CIN, int COUT, int WL, int ROWS, int WN, int NW, int NSPL = 1, int NIMG = 1>
FrConvInstance s2(int B, int mode) {
  return mode == 0 ? s2<0, CIN, COUT, WL, ROWS, WN, NW, NSPL, NIMG>(B) : s2<1, CIN, COUT, WL, ROWS, WN, NW, NSPL, NIMG>(B);
}

// The shape table of the stride-2 family (the four IR stage transitions, C -> C): the instance that serves (batch, channels,
// low-res width, mode) under the current switches, parts == 0 when none does.  fr_conv3x3_s2_strip_parts / _takes_frag
// report it, fr_conv3x3_s2_strip launches it -- nothing else decides.  `a`: the launch's arguments; nullptr for the queries,
// which have no epilogue argument and answer with the kernel that serves the training step's epilogues.
// The LDS-strip lines (round 3; their round-2 predecessors behind FRHIP_S2_VARIANT=0 were removed in round 4): instances in
// which ONE weight fragment feeds as many M tiles as the registers allow -- a wave's cost per MFMA is its private weight
// stream from L2 (conv3x3_strip.hip):
//   128 @28: 8 waves x (13 tiles x 1 column) instead of 4 x 2 waves x (7 x 2): 0.139 -> 0.116 ms forward, 0.193 -> 0.168 gradient
//   256 @14 forward: the whole image (13 tiles) x 1 column, output channels over two workgroups (123 KB plane);
//            the gradient keeps 7-row strips: its g strip stays resident beside the output tile (178 KB otherwise)
//   512 @7:  two images per workgroup (7 tiles x 1 column), output channels over four workgroups; odd batches keep the
//            one-image instance
FrConvInstance select_s2(int B, int C, int WL, int mode, const FrConvArgs* a) {
  const auto is = [&](int c, int wl) { return C == c && WL == wl; };
  // 64 channels: the rolling-window kernel (conv3x3_s2_roll64.hip; one row per work item in either mode, weights resident:
  // plain layout), for the epilogues it serves -- forward STORE / STATS, gradient PReLU backward
  if (is(64, 56) && fr_s2roll_enabled() && (!a || fr_s2roll_serves(*a))) return {fr_s2roll_parts(B), false, false, &fr_s2roll_launch};
  // forward at 128 / 256 / 512 channels: the warp-specialised kernel (conv3x3_s2_ws.hip, round 6), which has its own strip
  // count at 7x7 (four images per workgroup)
  if (const int ws = mode == 0 ? fr_s2ws_strips(B, C, WL) : 0; ws && (!a || fr_s2ws_serves(*a))) return {ws, true, false, &fr_s2ws_launch};
  if (is(64, 56)) return s2<64, 64, 56, 2, 2, 4>(B, mode);  // 2 low-res rows per workgroup
  // 128 -> 128: 7-row strips (196 pixels per weight pass) although only one workgroup then fits a CU: 0.166 -> 0.140 ms
  // forward, 0.221 -> 0.206 ms gradient against the 4-row strips (the kernel is bound by the weight stream)
  if (is(128, 28)) return s2<128, 128, 28, 7, 8, 8>(B, mode);
  if (is(256, 14) && mode == 0) return s2<0, 256, 128, 14, 14, 8, 8, 2, 1>(B);
  if (is(512, 7) && B % 2 == 0) return s2<512, 128, 7, 7, 8, 8, 4, 2>(B, mode);
  if (is(256, 14)) return s2<256, 256, 14, 7, 8, 8>(B, mode);  // (reached by the gradient only)
  if (is(512, 7)) return s2<512, 512, 7, 7, 8, 8>(B, mode);
  return {};
}

}  // namespace

// Partial-sum rows the kernel writes for a supported (B, C -> C, low-res width) problem; 0 when not served.
// mode 0: forward (one row per workgroup); mode 2: data gradient (4 classes x workgroups, ordered [class][workgroup]).
extern "C" int fr_conv3x3_s2_strip_parts(int B, int Cin, int Cout, int WL, int mode) {
  return Cin == Cout ? select_s2(B, Cin, WL, mode, nullptr).parts : 0;
}

// 1 when the launch reads fragment-order weights (FrConvArgs.w_frag): every served shape but the 64-channel layer
extern "C" int fr_conv3x3_s2_strip_takes_frag(int B, int C, int WL, int mode) { return select_s2(B, C, WL, mode, nullptr).frag; }

extern "C" int fr_conv3x3_s2_strip(const FrConvArgs* args, void* stream) {
  const FrConvArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.KH != 3 || a.KW != 3 || a.stride != 2 || a.pad != 1 || a.out_f32 || a.splitk > 1 || a.bias ||
      a.epi == FR_EPI_MARGIN || a.epi == FR_EPI_ATOMIC || (a.mode != 0 && a.mode != 2))
    FR_UNSUPPORTED("fr_conv3x3_s2_strip: stride-2 3x3 pad-1 bf16 convolution (mode 0) or its data gradient (mode 2)");
  if (a.mode == 2 && (a.par_h >= 0 || a.par_w >= 0))
    FR_UNSUPPORTED("fr_conv3x3_s2_strip: the data gradient produces all four parity classes (par_h = par_w = -1)");
  if (a.lda % 8 || a.ldc % 8 || (a.aux && a.ldaux % 8)) FR_UNSUPPORTED("fr_conv3x3_s2_strip: strides must be 16-byte multiples");
  // low-res grid: forward output / gradient input
  const int WLo = a.mode == 0 ? a.RW : a.SW, HLo = a.mode == 0 ? a.RH : a.SH;
  const int WHi = a.mode == 0 ? a.SW : a.RW, HHi = a.mode == 0 ? a.SH : a.RH;
  if (WLo != HLo || WHi != 2 * WLo || HHi != 2 * HLo || a.SC != a.N)
    FR_UNSUPPORTED("fr_conv3x3_s2_strip: square images, high-res side = 2 x low-res side, Cin == Cout");
  const FrConvInstance inst = select_s2(a.B, a.SC, WLo, a.mode, &a);
  if (!inst.parts) FR_UNSUPPORTED("fr_conv3x3_s2_strip: shape not in the table");
  if (a.w_frag && inst.launch == &fr_s2roll_launch)
    FR_UNSUPPORTED("fr_conv3x3_s2_strip: the 64-channel rolling-window kernel takes the plain weight layout (w_frag)");
  // fr_conv3x3_s2_strip_parts() has no epilogue argument: `part` was sized for the instance it selected.  If this launch's
  // prologue / epilogue needs another one, its summing epilogue would write that instance's rows (a DIFFERENT number, in
  // general) into the buffer -- refuse instead of overrunning it.
  if (a.part && (a.epi == FR_EPI_STATS || a.epi == FR_EPI_PRELU_BWD || a.epi == FR_EPI_BNBWD) &&
      inst.launch != select_s2(a.B, a.SC, WLo, a.mode, nullptr).launch)
    FR_UNSUPPORTED("fr_conv3x3_s2_strip: this prologue / epilogue combination writes the partial rows of another instance "
                   "than the one fr_conv3x3_s2_strip_parts() reports (switch that kernel off -- FRHIP_ROLL64=0, "
                   "FRHIP_S2_WS=0 -- or use fr_conv_igemm)");
  return inst.launch(a, st);
}
