// frhip -- class sampling for the class-sharded head (Partial-FC, An et al. 2021/22): every step a rank keeps the classes
// of its shard that occur in the global batch (the positives) and the n_s - P other classes with the smallest hash keys,
// gathers their weight rows, runs the sharded step on them and scatters the gradient rows back (frhip/sharded_head.py).
// The reference has no counterpart (head/metrics.py:104-113 is a plain class split).
//
//   fmix32(h)  : h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16      (a bijection on uint32)
//   key(c)     = fmix32((class0 + c) ^ salt),  c = 0 .. n - 1: distinct inside a shard (class0 + n <= 2^32), so no ties
//   pos[c]     = some row's local label is c;  P = number of positives
//   S          = positives + the (n_s - P) non-positive classes with the smallest keys;  |S| = n_s exactly
//   idx [n_s]  = S ascending;   inv [n] = position in idx or -1;   label_s [rows] = inv[label] (0 <= label < n) or -1
//
// The selection is a radix descent on the keys of the non-positive classes, as in pair_hist.hip: three passes of 11 / 11 /
// 10 key bits, every workgroup bins the keys of its contiguous class range into an LDS histogram (integer LDS atomics) and
// adds its non-zero bins to the pass's histogram in the workspace with integer atomics (an integer sum does not depend on
// the order of its terms; rows of partials summed by the one workgroup that follows were measured first: at 256 rows
// that workgroup read 2 MB through one CU, 78 us a pass); a one-workgroup kernel finds the bin of the k-th smallest key
// (k = n_s - P; P is counted in the first pass) and narrows the prefix.  After three passes the prefix IS the k-th
// smallest key, and the distinct keys make `key <= it` select exactly k classes.  The keys are recomputed in every pass
// (five integer instructions) instead of stored.  Compaction: per-workgroup counts, then every workgroup adds the counts
// before it and writes idx / inv for its range in class order.  `inv` doubles as the positives flags until the compaction
// overwrites it (each class by the thread that read its flag).  Integer arithmetic and integer atomics only, no host
// state, nothing synchronises the stream: bit-defined and reproducible.
#include "common.h"
#include "frhip_internal.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_PER_WG = 1024;       // classes a workgroup takes before the grid stops growing
constexpr int CS_MAX_GRID = 256;      // one workgroup per CU
constexpr int CS_BINS = 2048;         // 11 bits; the third pass uses the lower 1024
constexpr int CS_ROW = CS_BINS + 1;   // a pass's histogram: the bins, then the positives (first pass)
constexpr int CS_STATE = 16;          // words of selection state at the head of the workspace
constexpr int CS_NARROW_THREADS = 1024;
// state words
constexpr int ST_PREFIX = 0;  // key bits fixed so far (after pass 3: the k-th smallest key itself)
constexpr int ST_K = 1;       // rank still looked for inside the prefix (1-based)
constexpr int ST_TAKE = 2;    // 1: negatives are drawn (k >= 1); 0: the positives fill n_s

__device__ __forceinline__ uint32_t cs_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

struct CsGeom {
  int grid;  // workgroups of the histogram and compaction kernels
  int per;   // classes per workgroup: workgroup g owns [g * per, min(n, (g + 1) * per))
};
__host__ __device__ inline CsGeom cs_geom(int n) {
  CsGeom s;
  const int want = (n + CS_PER_WG - 1) / CS_PER_WG;
  s.grid = want < 1 ? 1 : (want > CS_MAX_GRID ? CS_MAX_GRID : want);
  s.per = (int)(((long long)n + s.grid - 1) / s.grid);
  return s;
}

// inv[c] = 0 for every class: the flags before the labels mark them; and the three passes' histograms
__global__ __launch_bounds__(CS_THREADS) void cs_clear_kernel(int32_t* __restrict__ inv, int n, uint32_t* __restrict__ hists) {
  for (long long c = (long long)blockIdx.x * CS_THREADS + threadIdx.x; c < n; c += (long long)gridDim.x * CS_THREADS)
    inv[c] = 0;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < 3 * CS_ROW; i += CS_THREADS) hists[i] = 0;
}

// inv[label] = 1: plain stores of the same value, so rows that share a label need no ordering
__global__ __launch_bounds__(CS_THREADS) void cs_mark_kernel(const int64_t* __restrict__ label, int rows,
                                                             int32_t* __restrict__ inv, int n) {
  const int r = blockIdx.x * CS_THREADS + threadIdx.x;
  if (r >= rows) return;
  const long long l = label[r];
  if (l >= 0 && l < n) inv[l] = 1;
}

// One pass of the descent.  PASS 0: bins on key >> 21 and counts the positives; PASS 1: keys whose top 11 bits are the
// prefix, bins on bits 20..10; PASS 2: keys whose top 22 bits are the prefix, bins on bits 9..0.
template <int PASS>
__global__ __launch_bounds__(CS_THREADS) void cs_hist_kernel(const int32_t* __restrict__ flags, int n, int per, uint32_t salt,
                                                             uint32_t class0, const uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ hist) {
  __shared__ uint32_t sH[CS_ROW];
  const int tid = threadIdx.x;
  for (int i = tid; i < CS_ROW; i += CS_THREADS) sH[i] = 0;
  __syncthreads();
  const uint32_t prefix = PASS == 0 ? 0u : state[ST_PREFIX];
  const long long c0 = (long long)blockIdx.x * per;
  const long long c1 = c0 + per < n ? c0 + per : n;
  for (long long c = c0 + tid; c < c1; c += CS_THREADS) {
    if (flags[c]) {
      if (PASS == 0) atomicAdd(&sH[CS_BINS], 1u);
      continue;
    }
    const uint32_t key = cs_fmix32((class0 + (uint32_t)c) ^ salt);
    if (PASS == 0) {
      atomicAdd(&sH[key >> 21], 1u);
    } else if (PASS == 1) {
      if ((key >> 21) == prefix) atomicAdd(&sH[(key >> 10) & 2047u], 1u);
    } else {
      if ((key >> 10) == prefix) atomicAdd(&sH[key & 1023u], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < CS_ROW; i += CS_THREADS) {
    const uint32_t v = sH[i];
    if (v) atomicAdd(&hist[i], v);  // passes 2 and 3: nearly every bin is empty
  }
}

// One workgroup: finds the bin of the pass's histogram that holds the k-th smallest key and narrows the state.  Thread t
// owns the neighbouring bins 2t and 2t + 1; an inclusive scan of the pair sums gives the count below each bin.
template <int PASS>
__global__ __launch_bounds__(CS_NARROW_THREADS) void cs_narrow_kernel(const uint32_t* __restrict__ hist, int n_s,
                                                                      uint32_t* __restrict__ state) {
  __shared__ uint32_t sS[CS_NARROW_THREADS];
  const int t = threadIdx.x;
  uint32_t k, prefix, take;
  if (PASS == 0) {
    const uint32_t P = hist[CS_BINS];
    k = (uint32_t)n_s > P ? (uint32_t)n_s - P : 0u;
    prefix = 0;
    take = k > 0 ? 1u : 0u;
  } else {
    k = state[ST_K];
    prefix = state[ST_PREFIX];
    take = state[ST_TAKE];
  }
  const uint32_t h0 = hist[2 * t], h1 = hist[2 * t + 1];
  sS[t] = h0 + h1;
  __syncthreads();
  for (int off = 1; off < CS_NARROW_THREADS; off <<= 1) {
    const uint32_t v = t >= off ? sS[t - off] : 0u;
    __syncthreads();
    sS[t] += v;
    __syncthreads();
  }
  const uint32_t below0 = sS[t] - (h0 + h1), below1 = below0 + h0;
  constexpr int BITS = PASS == 2 ? 10 : 11;
  if (PASS == 0 && t == 0) state[ST_TAKE] = take;
  if (!take) {  // nothing is drawn: the later passes and the compaction look at ST_TAKE only
    if (t == 0) {
      state[ST_PREFIX] = 0;
      state[ST_K] = 0;
    }
    return;
  }
  // exactly one bin has below < k <= below + h (k <= the number of keys inside the prefix)
  if (h0 > 0 && below0 < k && k <= below0 + h0) {
    state[ST_PREFIX] = (prefix << BITS) | (uint32_t)(2 * t);
    state[ST_K] = k - below0;
  }
  if (h1 > 0 && below1 < k && k <= below1 + h1) {
    state[ST_PREFIX] = (prefix << BITS) | (uint32_t)(2 * t + 1);
    state[ST_K] = k - below1;
  }
}

__device__ __forceinline__ bool cs_selected(int32_t flag, long long c, uint32_t salt, uint32_t class0, uint32_t take,
                                            uint32_t kth) {
  return flag != 0 || (take && cs_fmix32((class0 + (uint32_t)c) ^ salt) <= kth);
}

// counts[g] = selected classes of workgroup g's range
__global__ __launch_bounds__(CS_THREADS) void cs_count_kernel(const int32_t* __restrict__ flags, int n, int per, uint32_t salt,
                                                              uint32_t class0, const uint32_t* __restrict__ state,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t sC;
  const int tid = threadIdx.x;
  if (tid == 0) sC = 0;
  __syncthreads();
  const uint32_t take = state[ST_TAKE], kth = state[ST_PREFIX];
  const long long c0 = (long long)blockIdx.x * per;
  const long long c1 = c0 + per < n ? c0 + per : n;
  uint32_t mine = 0;
  for (long long c = c0 + tid; c < c1; c += CS_THREADS) mine += cs_selected(flags[c], c, salt, class0, take, kth) ? 1u : 0u;
  if (mine) atomicAdd(&sC, mine);
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = sC;
}

// Workgroup g: base = counts[0] + ... + counts[g - 1]; then its range in tiles of 256 consecutive classes, every thread one
// class, positions by ballot inside a wave and a running base across waves and tiles: idx ascending by construction.
__global__ __launch_bounds__(CS_THREADS) void cs_write_kernel(int32_t* __restrict__ inv, int n, int n_s, int per, uint32_t salt,
                                                              uint32_t class0, const uint32_t* __restrict__ state,
                                                              const uint32_t* __restrict__ counts, int32_t* __restrict__ idx) {
  __shared__ uint32_t sBase;
  __shared__ uint32_t sWave[CS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) sBase = 0;
  __syncthreads();
  uint32_t before = 0;
  for (int g = tid; g < (int)blockIdx.x; g += CS_THREADS) before += counts[g];
  if (before) atomicAdd(&sBase, before);
  __syncthreads();
  uint32_t base = sBase;
  const uint32_t take = state[ST_TAKE], kth = state[ST_PREFIX];
  const long long c0 = (long long)blockIdx.x * per;
  const long long c1 = c0 + per < n ? c0 + per : n;
  for (long long t0 = c0; t0 < c1; t0 += CS_THREADS) {
    const long long c = t0 + tid;
    const bool in = c < c1;
    const bool sel = in && cs_selected(inv[c], c, salt, class0, take, kth);
    const unsigned long long m = __ballot(sel);
    if (lane == 0) sWave[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t off = base, total = 0;
    for (int w = 0; w < CS_THREADS / 64; ++w) {
      const uint32_t v = sWave[w];
      if (w < wave) off += v;
      total += v;
    }
    __syncthreads();  // sWave is rewritten by the next tile
    if (in) {
      const uint32_t p = off + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (sel && p < (uint32_t)n_s) {  // p < n_s always (P <= n_s is checked on the host side); the guard keeps idx in bounds
        idx[p] = (int32_t)c;
        inv[c] = (int32_t)p;
      } else {
        inv[c] = -1;
      }
    }
    base += total;
  }
}

__global__ __launch_bounds__(CS_THREADS) void cs_labels_kernel(const int64_t* __restrict__ label, int rows,
                                                               const int32_t* __restrict__ inv, int n,
                                                               int64_t* __restrict__ label_s) {
  const int r = blockIdx.x * CS_THREADS + threadIdx.x;
  if (r >= rows) return;
  const long long l = label[r];
  label_s[r] = (l >= 0 && l < n) ? (long long)inv[l] : -1ll;
}

// out[j][:] = w[idx[j]][:]; V floats per thread and access (4: D % 4 == 0 and 16-byte aligned pointers)
template <int V>
__global__ __launch_bounds__(CS_THREADS) void cs_gather_kernel(const float* __restrict__ w, const int32_t* __restrict__ idx,
                                                               float* __restrict__ out, long long total, int dv) {
  for (long long e = (long long)blockIdx.x * CS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CS_THREADS) {
    const long long j = e / dv;
    const int q = (int)(e - j * dv);
    const long long src = ((long long)idx[j] * dv + q) * V;
    if (V == 4)
      *reinterpret_cast<float4*>(out + e * 4) = *reinterpret_cast<const float4*>(w + src);
    else
      out[e] = w[src];
  }
}

// out[c][:] = inv[c] >= 0 ? g[inv[c]][:] : 0; every element of out written exactly once
template <int V>
__global__ __launch_bounds__(CS_THREADS) void cs_scatter_kernel(const float* __restrict__ g, const int32_t* __restrict__ inv,
                                                                float* __restrict__ out, long long total, int dv) {
  for (long long e = (long long)blockIdx.x * CS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CS_THREADS) {
    const long long c = e / dv;
    const int q = (int)(e - c * dv);
    const int32_t j = inv[c];
    if (V == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j >= 0) v = *reinterpret_cast<const float4*>(g + ((long long)j * dv + q) * 4);
      *reinterpret_cast<float4*>(out + e * 4) = v;
    } else {
      out[e] = j >= 0 ? g[(long long)j * dv + q] : 0.f;
    }
  }
}

inline unsigned cs_row_grid(long long total) {
  const long long want = (total + CS_THREADS - 1) / CS_THREADS;
  return (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));  // 16 workgroups per CU, grid-stride beyond
}

}  // namespace

extern "C" int fr_class_sample_work(int n) {
  if (n < 1) FR_UNSUPPORTED("fr_class_sample_work: n >= 1");
  const CsGeom s = cs_geom(n);
  return CS_STATE + 3 * CS_ROW + s.grid;
}

extern "C" int fr_class_sample(const int64_t* label_local, int rows, int n, int n_s, uint32_t salt, uint32_t class0,
                               int32_t* idx, int32_t* inv, int64_t* label_s, uint32_t* work, void* stream) {
  if (rows < 1 || n < 1) FR_UNSUPPORTED("fr_class_sample: rows >= 1 and n >= 1");
  if ((unsigned long long)class0 + (unsigned long long)n > (1ULL << 32))
    FR_UNSUPPORTED("fr_class_sample: class0 + n must not pass 2^32 (the keys of a shard are distinct below it)");
  if (n_s < 1 || n_s > n) FR_UNSUPPORTED("fr_class_sample: 1 <= n_s <= n");
  if (n_s < (n < rows ? n : rows))
    FR_UNSUPPORTED("fr_class_sample: n_s >= min(n, rows), so that every class of the batch fits (smallest rate: min(n, rows) / n)");
  if (!label_local || !idx || !inv || !label_s || !work)
    FR_UNSUPPORTED("fr_class_sample: label_local, idx, inv, label_s and work are required");
  const CsGeom s = cs_geom(n);
  uint32_t* state = work;
  uint32_t* hists = work + CS_STATE;  // one histogram per pass, cleared with the flags
  uint32_t* counts = hists + 3 * CS_ROW;
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg(CS_THREADS), grid((unsigned)s.grid), row_grid((unsigned)((rows + CS_THREADS - 1) / CS_THREADS));
  hipLaunchKernelGGL(cs_clear_kernel, dim3(cs_row_grid(n)), wg, 0, st, inv, n, hists);
  hipLaunchKernelGGL(cs_mark_kernel, row_grid, wg, 0, st, label_local, rows, inv, n);
  hipLaunchKernelGGL(cs_hist_kernel<0>, grid, wg, 0, st, (const int32_t*)inv, n, s.per, salt, class0, (const uint32_t*)state,
                     hists + 0 * CS_ROW);
  hipLaunchKernelGGL(cs_narrow_kernel<0>, dim3(1), dim3(CS_NARROW_THREADS), 0, st, (const uint32_t*)(hists + 0 * CS_ROW), n_s,
                     state);
  hipLaunchKernelGGL(cs_hist_kernel<1>, grid, wg, 0, st, (const int32_t*)inv, n, s.per, salt, class0, (const uint32_t*)state,
                     hists + 1 * CS_ROW);
  hipLaunchKernelGGL(cs_narrow_kernel<1>, dim3(1), dim3(CS_NARROW_THREADS), 0, st, (const uint32_t*)(hists + 1 * CS_ROW), n_s,
                     state);
  hipLaunchKernelGGL(cs_hist_kernel<2>, grid, wg, 0, st, (const int32_t*)inv, n, s.per, salt, class0, (const uint32_t*)state,
                     hists + 2 * CS_ROW);
  hipLaunchKernelGGL(cs_narrow_kernel<2>, dim3(1), dim3(CS_NARROW_THREADS), 0, st, (const uint32_t*)(hists + 2 * CS_ROW), n_s,
                     state);
  hipLaunchKernelGGL(cs_count_kernel, grid, wg, 0, st, (const int32_t*)inv, n, s.per, salt, class0, (const uint32_t*)state,
                     counts);
  hipLaunchKernelGGL(cs_write_kernel, grid, wg, 0, st, inv, n, n_s, s.per, salt, class0, (const uint32_t*)state,
                     (const uint32_t*)counts, idx);
  hipLaunchKernelGGL(cs_labels_kernel, row_grid, wg, 0, st, label_local, rows, (const int32_t*)inv, n, label_s);
  FR_LAUNCH_CHECK();
}

extern "C" int fr_gather_rows(const float* w, const int32_t* idx, float* out, int n_s, int D, void* stream) {
  if (n_s < 1 || D < 1) FR_UNSUPPORTED("fr_gather_rows: n_s >= 1 and D >= 1");
  if (!w || !idx || !out) FR_UNSUPPORTED("fr_gather_rows: w, idx and out are required");
  hipStream_t st = (hipStream_t)stream;
  if (D % 4 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0) {
    const long long total = (long long)n_s * (D / 4);
    hipLaunchKernelGGL(cs_gather_kernel<4>, dim3(cs_row_grid(total)), dim3(CS_THREADS), 0, st, w, idx, out, total, D / 4);
  } else {
    const long long total = (long long)n_s * D;
    hipLaunchKernelGGL(cs_gather_kernel<1>, dim3(cs_row_grid(total)), dim3(CS_THREADS), 0, st, w, idx, out, total, D);
  }
  FR_LAUNCH_CHECK();
}

extern "C" int fr_scatter_rows(const float* g, const int32_t* inv, float* out, int n, int D, void* stream) {
  if (n < 1 || D < 1) FR_UNSUPPORTED("fr_scatter_rows: n >= 1 and D >= 1");
  if (!g || !inv || !out) FR_UNSUPPORTED("fr_scatter_rows: g, inv and out are required");
  hipStream_t st = (hipStream_t)stream;
  if (D % 4 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)out % 16 == 0) {
    const long long total = (long long)n * (D / 4);
    hipLaunchKernelGGL(cs_scatter_kernel<4>, dim3(cs_row_grid(total)), dim3(CS_THREADS), 0, st, g, inv, out, total, D / 4);
  } else {
    const long long total = (long long)n * D;
    hipLaunchKernelGGL(cs_scatter_kernel<1>, dim3(cs_row_grid(total)), dim3(CS_THREADS), 0, st, g, inv, out, total, D);
  }
  FR_LAUNCH_CHECK();
}
