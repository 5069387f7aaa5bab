// GPU-side training-input transform: staged uint8 HWC images -> the float32 NCHW batch the reference's
// host transform produces (train.py:108-116: Resize(128*S/112) -> RandomCrop(S) -> RandomHorizontalFlip -> ToTensor ->
// Normalize), one launch per batch.
//
// The resize is Pillow's 8-bit bilinear resample restated exactly (src/libImaging/Resample.c: integer weights with 22
// fractional bits, horizontal pass rounded to uint8, then the vertical pass), so the result is bit-identical to the host
// path; the weights and windows come precomputed per axis (frhip/input_pipeline.py, the same table Pillow builds).  Only
// the S x S crop is ever computed: every output pixel evaluates its <= ky rows of <= kx horizontal taps straight from the
// staged image (uint8 reads served by L2; 9.6 MB in, 38.5 MB out at B = 256), ToTensor + Normalize are a 256-entry
// table per channel built on the host in float32, so there is no device-side division to disagree about.
//
// HBM-bound byte work: one thread per output pixel, x fastest -> each of the three channel planes is written with
// fully coalesced 256-byte wave stores.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// xtab / ytab rows: [first input index, tap count, k_0 .. k_{K-1}]
// One output pixel `pix` of one image: `img` is that image's [Hin][Win][3] bytes, `o` its [3][S][S] floats.  Shared by the
// staged-batch kernel and the resident-store gather, which differ in where `img` comes from and in nothing else.
__device__ __forceinline__ void augment_pixel(const unsigned char* __restrict__ img, const int* __restrict__ xtab,
                                              const int* __restrict__ ytab, int x0, int y0, bool flipped,
                                              const float* slut, float* __restrict__ o, int pix, int Win, int S, int kx,
                                              int ky) {
  const int y = pix / S, x = pix - y * S;
  const int rx = x0 + (flipped ? S - 1 - x : x), ry = y0 + y;  // position in the resized image
  const int* xr = xtab + (size_t)rx * (kx + 2);
  const int* yr = ytab + (size_t)ry * (ky + 2);
  const int xmin = xr[0], xn = xr[1], ymin = yr[0], yn = yr[1];
  int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
  for (int t = 0; t < yn; ++t) {
    const unsigned char* row = img + ((size_t)(ymin + t) * Win + xmin) * 3;
    int h[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
    for (int j = 0; j < xn; ++j) {
      const int k = xr[2 + j];
      h[0] += row[3 * j] * k;
      h[1] += row[3 * j + 1] * k;
      h[2] += row[3 * j + 2] * k;
    }
    const int kv = yr[2 + t];
    acc[0] += clip8(h[0]) * kv;  // the horizontal pass is rounded to uint8 before the vertical pass reads it
    acc[1] += clip8(h[1]) * kv;
    acc[2] += clip8(h[2]) * kv;
  }
  const size_t plane = (size_t)S * S;
  o[pix] = slut[clip8(acc[0]) * 3];
  o[plane + pix] = slut[clip8(acc[1]) * 3 + 1];
  o[2 * plane + pix] = slut[clip8(acc[2]) * 3 + 2];
}

__global__ __launch_bounds__(256) void augment_u8_kernel(const unsigned char* __restrict__ src,
                                                         const int* __restrict__ xtab, const int* __restrict__ ytab,
                                                         const int* __restrict__ crop,
                                                         const unsigned char* __restrict__ flip,
                                                         const float* __restrict__ lut, float* __restrict__ out,
                                                         int Hin, int Win, int S, int kx, int ky) {
  __shared__ float slut[768];
  for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
  __syncthreads();
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= S * S) return;
  augment_pixel(src + (size_t)b * Hin * Win * 3, xtab, ytab, crop[2 * b], crop[2 * b + 1], flip[b] != 0, slut,
                out + (size_t)b * 3 * S * S, pix, Win, S, kx, ky);
}

// The same batch drawn from a resident store [M][Hin][Win][3]: image b is store[idx[b]] (idx may repeat, in any order;
// 0 <= idx[b] < M is the caller's to guarantee, the indices live in device memory).  The slot offset is formed in size_t: a
// store of 1.3 M 112x112 images is 49 GB.  The label of image b travels with it, written by one thread of its first
// workgroup.
__global__ __launch_bounds__(256) void augment_u8_gather_kernel(
    const unsigned char* __restrict__ store, const long long* __restrict__ labels, const int* __restrict__ idx,
    const int* __restrict__ xtab, const int* __restrict__ ytab, const int* __restrict__ crop,
    const unsigned char* __restrict__ flip, const float* __restrict__ lut, float* __restrict__ out,
    long long* __restrict__ label_out, int Hin, int Win, int S, int kx, int ky) {
  __shared__ float slut[768];
  for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
  __syncthreads();
  const int b = blockIdx.y;
  const size_t slot = (size_t)idx[b];
  if (label_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) label_out[b] = labels[slot];
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= S * S) return;
  augment_pixel(store + slot * ((size_t)Hin * Win * 3), xtab, ytab, crop[2 * b], crop[2 * b + 1], flip[b] != 0, slut,
                out + (size_t)b * 3 * S * S, pix, Win, S, kx, ky);
}

}  // namespace

extern "C" int fr_augment_u8(const uint8_t* src, const int32_t* xtab, const int32_t* ytab, const int32_t* crop,
                             const uint8_t* flip, const float* lut, float* out, int B, int Hin, int Win, int Hr, int Wr,
                             int S, int kx, int ky, void* stream) {
  if (B <= 0) return 0;
  if (Hin <= 0 || Win <= 0 || S <= 0 || S > Hr || S > Wr || kx <= 0 || ky <= 0)
    FR_UNSUPPORTED("fr_augment_u8: sizes (need 0 < S <= resized size, at least one tap per axis)");
  if (B > 65535) FR_UNSUPPORTED("fr_augment_u8: more than 65535 images per launch");
  dim3 grid((S * S + 255) / 256, B);
  hipLaunchKernelGGL(augment_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, xtab, ytab, crop, flip, lut, out,
                     Hin, Win, S, kx, ky);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_augment_u8_gather(const uint8_t* store, const int64_t* labels, const int32_t* idx, const int32_t* xtab,
                                    const int32_t* ytab, const int32_t* crop, const uint8_t* flip, const float* lut,
                                    float* out, int64_t* label_out, int M, int B, int Hin, int Win, int Hr, int Wr, int S,
                                    int kx, int ky, void* stream) {
  if (B <= 0) return 0;
  if (M <= 0) FR_UNSUPPORTED("fr_augment_u8_gather: the store holds no image (M <= 0)");
  if (Hin <= 0 || Win <= 0 || S <= 0 || S > Hr || S > Wr || kx <= 0 || ky <= 0)
    FR_UNSUPPORTED("fr_augment_u8_gather: sizes (need 0 < S <= resized size, at least one tap per axis)");
  if (B > 65535) FR_UNSUPPORTED("fr_augment_u8_gather: more than 65535 images per launch");
  if (!store || !idx || !out) FR_UNSUPPORTED("fr_augment_u8_gather: store, idx and out are required");
  if (!labels) label_out = nullptr;  // the labels travel only when both ends exist
  dim3 grid((S * S + 255) / 256, B);
  hipLaunchKernelGGL(augment_u8_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, store,
                     (const long long*)labels, idx, xtab, ytab, crop, flip, lut, out, (long long*)label_out, Hin, Win, S,
                     kx, ky);
  FR_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------ RandAugment (served set)
// The reference's data_processing/randaugment.py applies a chain of Pillow operations to the decoded image.  Here one
// workgroup owns one image: it is read from HBM once into LDS, the K steps of its chain run there in order with a barrier
// between them -- every step rounds to uint8, as Pillow does between operations -- and it is written once.  The results
// are Pillow's bytes (tests/randaug_ref.py restates each operation, tests/test_randaug_host.py pins the restatement
// against the installed Pillow):
//   * ImageEnhance.{Brightness, Color, Contrast} are Image.blend(degenerate, image, factor) = d + a * (i - d) in float32,
//     product and sum rounded separately (no contraction, see ra_blend), <= 0 -> 0, >= 255 -> 255, else truncated
//     (inside 0 <= a <= 1 the clip never acts, so the one form serves both of Pillow's branches);
//   * the degenerate image is 0 (brightness), Pillow's L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 on the three
//     channels (color), or the constant int(mean(L) + 0.5) of the CURRENT image (contrast), formed as
//     (2 * sum + count) / (2 * count) in integers: sum / count + 0.5 lies at least 1 / (2 * count) from the next integer
//     unless it is one, far beyond a double's rounding, so the two forms agree;
//   * ImageOps.autocontrast is a 256-entry table per channel, int(i * scale + offset) in double, clipped;
//   * a translation by Image.transform(AFFINE, (1, 0, c, 0, 1, 0)) is nearest-neighbour, an integer shift, and what comes
//     in from outside is black (the reference's fill=128 is not Pillow's fillcolor).
// LDS layout: the image as it lies in memory, bytes [H][W][3], padded to whole units of 4 pixels = 12 bytes = 3 dwords.
// A lane owns whole units (unit u of lane t: u = t + i * 1024) and moves them as three ds_read_b32 / ds_write_b32 at a
// lane stride of 3 dwords, which is odd: conflict-free over the 32 banks.  Statistics are integer: a wave reduction, then
// one LDS atomic per wave (add / min / max on integers: the order cannot show), so the bytes are the same from run to run.
namespace {

constexpr int RA_THREADS = 1024;
constexpr int RA_LDS_BUDGET = 64 * 1024;             // the rule of the ABI: H * W * 3 + 3 * 256 dwords within 64 KB
constexpr int RA_MAX_PIXELS = (RA_LDS_BUDGET - 3 * 256 * 4) / 3;

enum { RA_IDENTITY = 0, RA_AUTOCONTRAST = 1, RA_SOLARIZE = 2, RA_COLOR = 3, RA_POSTERIZE = 4, RA_CONTRAST = 5,
       RA_BRIGHTNESS = 6, RA_TRANSLATE_X = 7, RA_TRANSLATE_Y = 8, RA_INVERT = 9 };

// Plain operators under `fp contract(off)`, not __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn: the HIP headers define those
// as the plain operators compiled under hipcc's default -ffp-contract=fast, so once inlined their product and sum fuse into
// one fma (seen in the listing, and as wrong table entries on the device).  The pragma governs the operators written here,
// and keeps the product and the sum rounded separately.
__device__ __forceinline__ int ra_blend(int d, int v, float a) {
#pragma clang fp contract(off)
  const float prod = a * (float)(v - d);
  const float t = (float)d + prod;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
// ImageOps.autocontrast's table entry, int(i * scale + offset) clipped, in double as Python forms it
__device__ __forceinline__ int ra_stretch(int i, int lo, int hi) {
#pragma clang fp contract(off)
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = -(double)lo * scale;
  const double prod = (double)i * scale;
  const double x = prod + offset;
  return x <= 0.0 ? 0 : (x >= 255.0 ? 255 : (int)x);
}
__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// the 12 bytes of a unit, v[3 * pixel + channel]
__device__ __forceinline__ void ra_unpack(const unsigned* w, int* v) {
#pragma unroll
  for (int j = 0; j < 12; ++j) v[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
}
__device__ __forceinline__ void ra_pack(const int* v, unsigned* w) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    w[k] = (unsigned)v[4 * k] | ((unsigned)v[4 * k + 1] << 8) | ((unsigned)v[4 * k + 2] << 16) | ((unsigned)v[4 * k + 3] << 24);
}

__device__ __forceinline__ int ra_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int ra_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int ra_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// Every byte of the image through f(value, channel), in place: a lane rewrites only the units it read.
template <class F>
__device__ __forceinline__ void ra_pointwise(unsigned* img, int units, F f) {
  for (int u = threadIdx.x; u < units; u += RA_THREADS) {
    unsigned w[3] = {img[3 * u], img[3 * u + 1], img[3 * u + 2]};
    int v[12];
    ra_unpack(w, v);
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = f(v[j], j % 3);
    ra_pack(v, w);
    img[3 * u] = w[0];
    img[3 * u + 1] = w[1];
    img[3 * u + 2] = w[2];
  }
}

// A translation in place: out[y][x] = in[y][x + s] (horizontal) or in[y + s][x], black where the source lies outside the
// image; |s| <= W or H.  In pixels that is p -> p + shift with shift = s or s * W, valid where the column x + s stays inside
// the row (horizontal) or p + shift inside the image (vertical).  A unit's 12 bytes lie 3 * shift bytes from their place, at
// any byte alignment: four aligned dwords are read and funnelled into three (word indices clamped into the image: what a
// clamped read brings belongs to pixels that are masked to black anyway).
// In place: the workgroup takes the units in batches of one per lane -- all lanes read, a barrier, all lanes write -- and
// takes the batches in the direction of the shift (upwards for shift > 0, downwards for shift < 0), so the bytes a batch
// uses are never ones an earlier batch wrote: one barrier per batch, three dwords held per lane.
__device__ __forceinline__ void ra_shift(unsigned* img, int units, int pixels, int W, int s, bool horizontal) {
  const int last = 3 * units - 1;
  const int shift = horizontal ? s : s * W;
  const int batches = (units + RA_THREADS - 1) / RA_THREADS;
  for (int j = 0; j < batches; ++j) {
    const int u = (shift >= 0 ? j : batches - 1 - j) * RA_THREADS + threadIdx.x;
    unsigned o0 = 0, o1 = 0, o2 = 0;
    if (u < units) {
      const int at = 12 * u + 3 * shift;  // byte address of the source, possibly outside the image
      const int word = at >> 2, rot = at & 3;
      unsigned w[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) w[t] = img[min(max(word + t, 0), last)];
      const int x0 = (4 * u) % W;
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = 4 * u + k;
        int x = x0 + k;  // < W + 3: at most three rows further on (W = 1)
#pragma unroll
        for (int t = 0; t < 3; ++t) x -= x >= W ? W : 0;
        const int q = horizontal ? x + s : p + shift;
        ok[k] = p < pixels && q >= 0 && q < (horizontal ? W : pixels);
      }
      o0 = __builtin_amdgcn_alignbyte(w[1], w[0], rot) & ((ok[0] ? 0x00FFFFFFu : 0u) | (ok[1] ? 0xFF000000u : 0u));
      o1 = __builtin_amdgcn_alignbyte(w[2], w[1], rot) & ((ok[1] ? 0x0000FFFFu : 0u) | (ok[2] ? 0xFFFF0000u : 0u));
      o2 = __builtin_amdgcn_alignbyte(w[3], w[2], rot) & ((ok[2] ? 0x000000FFu : 0u) | (ok[3] ? 0xFFFFFF00u : 0u));
    }
    __syncthreads();
    if (u < units) {
      img[3 * u] = o0;
      img[3 * u + 1] = o1;
      img[3 * u + 2] = o2;
    }
  }
}

__global__ __launch_bounds__(RA_THREADS) void randaug_u8_kernel(
    const unsigned char* __restrict__ src, const long long* __restrict__ labels, const int* __restrict__ idx,
    const unsigned char* __restrict__ op, const float* __restrict__ par, unsigned char* __restrict__ dst,
    long long* __restrict__ label_out, int K, int H, int W) {
  extern __shared__ uint4 ra_lds[];  // [image, padded to whole units and to 16 bytes][table 768 bytes][stats 8 ints]
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int pixels = H * W, n = pixels * 3, units = (pixels + 3) / 4;
  const int image_bytes = (units * 12 + 15) & ~15;
  unsigned* img = (unsigned*)ra_lds;
  unsigned char* img8 = (unsigned char*)ra_lds;
  unsigned char* table = img8 + image_bytes;
  int* stats = (int*)(table + 768);  // [0] sum of L, [1..3] min, [4..6] max per channel

  const size_t slot = idx != nullptr ? (size_t)idx[b] : (size_t)b;
  if (label_out != nullptr && tid == 0) label_out[b] = labels[slot];
  const unsigned char* in = src + slot * (size_t)n;
  unsigned char* out = dst + (size_t)b * (size_t)n;

  // HBM -> LDS: 16-byte loads where this image starts on a 16-byte boundary (112x112x3 and 128x128x3 are multiples of
  // 16, so every image of such a batch does), bytes otherwise; the padding is zeroed so no step reads undefined bytes
  const int vec = ((size_t)in & 15) == 0 ? n >> 4 : 0;
  for (int i = tid; i < vec; i += RA_THREADS) ra_lds[i] = ((const uint4*)in)[i];
  for (int i = vec * 16 + tid; i < image_bytes; i += RA_THREADS) img8[i] = i < n ? in[i] : (unsigned char)0;
  __syncthreads();

  for (int k = 0; k < K; ++k) {
    const int code = op[(size_t)b * K + k];  // uniform over the workgroup: the branches below do not diverge
    const float p = par[(size_t)b * K + k];
    if (code == RA_SOLARIZE) {
      ra_pointwise(img, units, [p](int v, int) { return (float)v < p ? v : 255 - v; });
    } else if (code == RA_POSTERIZE) {
      const int bits = p >= 8.f ? 8 : (p >= 0.f ? (int)p : 0);
      const int mask = (0xFF << (8 - bits)) & 0xFF;
      ra_pointwise(img, units, [mask](int v, int) { return v & mask; });
    } else if (code == RA_INVERT) {
      ra_pointwise(img, units, [](int v, int) { return 255 - v; });
    } else if (code == RA_BRIGHTNESS) {
      ra_pointwise(img, units, [p](int v, int) { return ra_blend(0, v, p); });
    } else if (code == RA_COLOR) {
      for (int u = tid; u < units; u += RA_THREADS) {
        unsigned w[3] = {img[3 * u], img[3 * u + 1], img[3 * u + 2]};
        int v[12];
        ra_unpack(w, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int l = ra_luma(v[3 * q], v[3 * q + 1], v[3 * q + 2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * q + c] = ra_blend(l, v[3 * q + c], p);
        }
        ra_pack(v, w);
        img[3 * u] = w[0];
        img[3 * u + 1] = w[1];
        img[3 * u + 2] = w[2];
      }
    } else if (code == RA_CONTRAST) {
      if (tid == 0) stats[0] = 0;
      __syncthreads();
      int sum = 0;
      for (int u = tid; u < units; u += RA_THREADS) {
        unsigned w[3] = {img[3 * u], img[3 * u + 1], img[3 * u + 2]};
        int v[12];
        ra_unpack(w, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * u + q < pixels) sum += ra_luma(v[3 * q], v[3 * q + 1], v[3 * q + 2]);
      }
      sum = ra_wave_sum(sum);
      if ((tid & 63) == 0) atomicAdd(&stats[0], sum);
      __syncthreads();
      const int mean = (2 * stats[0] + pixels) / (2 * pixels);  // int(sum / count + 0.5), see above
      ra_pointwise(img, units, [mean, p](int v, int) { return ra_blend(mean, v, p); });
    } else if (code == RA_AUTOCONTRAST) {
      if (tid < 3) {
        stats[1 + tid] = 255;
        stats[4 + tid] = 0;
      }
      __syncthreads();
      int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
      for (int u = tid; u < units; u += RA_THREADS) {
        unsigned w[3] = {img[3 * u], img[3 * u + 1], img[3 * u + 2]};
        int v[12];
        ra_unpack(w, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * u + q < pixels) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              lo[c] = min(lo[c], v[3 * q + c]);
              hi[c] = max(hi[c], v[3 * q + c]);
            }
          }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = ra_wave_min(lo[c]);
        hi[c] = ra_wave_max(hi[c]);
        if ((tid & 63) == 0) {
          atomicMin(&stats[1 + c], lo[c]);
          atomicMax(&stats[4 + c], hi[c]);
        }
      }
      __syncthreads();
      if (tid < 768) {  // one lane per table entry; the identity where hi <= lo
        const int c = tid >> 8, i = tid & 255;
        const int l = stats[1 + c], h = stats[4 + c];
        table[tid] = (unsigned char)(h > l ? ra_stretch(i, l, h) : i);
      }
      __syncthreads();
      ra_pointwise(img, units, [table](int v, int c) { return (int)table[c * 256 + v]; });
    } else if (code == RA_TRANSLATE_X || code == RA_TRANSLATE_Y) {
      const int span = code == RA_TRANSLATE_X ? W : H;
      const float pc = p >= (float)span ? (float)span : (p <= -(float)span ? -(float)span : p);
      const int s = pc == pc ? (int)pc : 0;  // |s| <= W or H: no index below overflows; a NaN shifts by nothing
      ra_shift(img, units, pixels, W, s, code == RA_TRANSLATE_X);
    }  // RA_IDENTITY and every code beyond the table: the image stays as it is
    __syncthreads();
  }

  // LDS -> HBM, the same two forms
  const int ovec = ((size_t)out & 15) == 0 ? n >> 4 : 0;
  for (int i = tid; i < ovec; i += RA_THREADS) ((uint4*)out)[i] = ra_lds[i];
  for (int i = ovec * 16 + tid; i < n; i += RA_THREADS) out[i] = img8[i];
}

}  // namespace

extern "C" int fr_randaug_u8(const uint8_t* src, const int64_t* labels, const int32_t* idx, const uint8_t* op,
                             const float* par, uint8_t* dst, int64_t* label_out, int M, int B, int K, int H, int W,
                             void* stream) {
  if (B <= 0) return 0;
  if (B > 65535) FR_UNSUPPORTED("fr_randaug_u8: more than 65535 images per launch");
  if (K < 1 || K > 16) FR_UNSUPPORTED("fr_randaug_u8: the chain holds 1..16 steps (K)");
  if (!src || !op || !par || !dst) FR_UNSUPPORTED("fr_randaug_u8: src, op, par and dst are required");
  if (idx && M <= 0) FR_UNSUPPORTED("fr_randaug_u8: the store holds no image (M <= 0 with idx)");
  if (H <= 0 || W <= 0 || (long long)H * W > RA_MAX_PIXELS)
    FR_UNSUPPORTED("fr_randaug_u8: the image and its 3 x 256 table words must fit 64 KB of LDS (H * W * 3 + 3072 <= 65536)");
  if (!labels) label_out = nullptr;  // the labels travel only when both ends exist
  const int units = (H * W + 3) / 4;
  const size_t lds = (size_t)((units * 12 + 15) & ~15) + 768 + 8 * sizeof(int);
  hipLaunchKernelGGL(randaug_u8_kernel, dim3(B), dim3(RA_THREADS), lds, (hipStream_t)stream, src,
                     (const long long*)labels, idx, op, par, dst, (long long*)label_out, K, H, W);
  FR_LAUNCH_CHECK();
}


// ------------------------------------------------------------------------------------------ bilinear resize (pSp)
// pSp.forward resizes a batch whose side differs from the encoder's input size with
// F.interpolate(x, size, mode='bilinear') (reference backbone/restyle_psp.py:440-443): align_corners = False, no
// antialiasing -- ATen's upsample_bilinear2d restated: src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out in
// float, the two taps weighted 1 - l and l in float32.  planes = B * C NCHW planes; one thread per output pixel.
namespace {
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              int Hin, int Win, int Hout, int Wout, float sh, float sw) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Hout * Wout) return;
  const int oy = pix / Wout, ox = pix - oy * Wout;
  float fy = sh * ((float)oy + 0.5f) - 0.5f, fx = sw * ((float)ox + 0.5f) - 0.5f;
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < Hin - 1 ? 1 : 0), x1 = x0 + (x0 < Win - 1 ? 1 : 0);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float* pl = in + (size_t)blockIdx.y * Hin * Win;
  const float v = hy * (hx * pl[(size_t)y0 * Win + x0] + lx * pl[(size_t)y0 * Win + x1]) +
                  ly * (hx * pl[(size_t)y1 * Win + x0] + lx * pl[(size_t)y1 * Win + x1]);
  out[(size_t)blockIdx.y * Hout * Wout + pix] = v;
}
}  // namespace

extern "C" int fr_resize_bilinear(const float* in, float* out, int planes, int Hin, int Win, int Hout, int Wout,
                                  void* stream) {
  if (planes < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || planes > 65535)
    FR_UNSUPPORTED("fr_resize_bilinear: planes in 1..65535 and positive sizes");
  const float sh = (float)Hin / (float)Hout, sw = (float)Win / (float)Wout;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((Hout * Wout + 255) / 256, planes), dim3(256), 0, (hipStream_t)stream, in,
                     out, Hin, Win, Hout, Wout, sh, sw);
  FR_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------ ... and its adjoint
// gin[plane][iy][ix] = sum over (oy, ox) of gout[plane][oy][ox] * wy(oy, iy) * wx(ox, ix), the weights with which input
// (iy, ix) entered output (oy, ox) above.  A gather, one thread per INPUT pixel: the outputs that read input index i along
// an axis are those whose first tap is i - 1 or i (the first tap is non-decreasing in the output index), found by stepping
// from a lower estimate; fixed summation order, no atomics.
namespace {
struct Taps {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ Taps bilinear_taps(int o, float s, int n) {  // resize_bilinear_kernel's expressions
  float f = s * ((float)o + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  const int i0 = (int)f;
  const float l = f - (float)i0;
  return {i0, i0 + (i0 < n - 1 ? 1 : 0), 1.f - l, l};
}
__device__ __forceinline__ float tap_weight(const Taps& t, int i) {
  return (t.i0 == i ? t.w0 : 0.f) + (t.i1 == i ? t.w1 : 0.f);
}
__device__ __forceinline__ int first_reader(int i, float s, int n_in, int n_out) {  // smallest o with first tap >= i - 1
  int o = (int)floorf(((float)i - 0.5f) / s - 0.5f) - 2;
  o = o < 0 ? 0 : o;
  while (o < n_out && bilinear_taps(o, s, n_in).i0 < i - 1) ++o;
  return o;
}

__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin,
                                                                  int Hin, int Win, int Hout, int Wout, float sh, float sw) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Hin * Win) return;
  const int iy = pix / Win, ix = pix - iy * Win;
  const float* pl = gout + (size_t)blockIdx.y * Hout * Wout;
  const int ox0 = first_reader(ix, sw, Win, Wout);
  float acc = 0.f;
  for (int oy = first_reader(iy, sh, Hin, Hout); oy < Hout; ++oy) {
    const Taps ty = bilinear_taps(oy, sh, Hin);
    if (ty.i0 > iy) break;
    const float wy = tap_weight(ty, iy);
    float row = 0.f;
    for (int ox = ox0; ox < Wout; ++ox) {
      const Taps tx = bilinear_taps(ox, sw, Win);
      if (tx.i0 > ix) break;
      row = fmaf(tap_weight(tx, ix), pl[(size_t)oy * Wout + ox], row);
    }
    acc = fmaf(wy, row, acc);
  }
  gin[(size_t)blockIdx.y * Hin * Win + pix] = acc;
}
}  // namespace

extern "C" int fr_resize_bilinear_bwd(const float* gout, float* gin, int planes, int Hin, int Win, int Hout, int Wout,
                                      void* stream) {
  if (planes < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || planes > 65535)
    FR_UNSUPPORTED("fr_resize_bilinear_bwd: planes in 1..65535 and positive sizes");
  if (!gout || !gin) FR_UNSUPPORTED("fr_resize_bilinear_bwd: gout and gin are required");
  const float sh = (float)Hin / (float)Hout, sw = (float)Win / (float)Wout;
  hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3((Hin * Win + 255) / 256, planes), dim3(256), 0, (hipStream_t)stream,
                     gout, gin, Hin, Win, Hout, Wout, sh, sw);
  FR_LAUNCH_CHECK();
}
