// Single-pulse search kernels (gfx950 / CDNA4): see psoup/singlepulse.hpp for
// the definition.  Three launches per chunk of DM trials (the DM is the
// grid's second dimension):
//
//   block_means_kernel : exact integer sum of every trend block -> its mean
//   sigma_kernel       : partial sums of x^2 in double over fixed ranges
//   search_kernel      : a workgroup owns kSpTile start samples plus a halo
//     of 2^K.  It reads the uint8 row once, subtracts the trend, scales by
//     1 / sigma and stages floats in LDS.  Every thread owns groups of four
//     consecutive samples (lanes on consecutive groups: 16-byte LDS accesses,
//     conflict-free at every stride).  Widths 1, 2, 4, 8 are formed in
//     registers from three 16-byte reads; wider levels by dyadic doubling,
//     B_2w[i] = B_w[i] + B_w[i + w], the thread's B_w[i] kept in registers
//     and B_w[i + w] read from LDS (one LDS round per level, no prefix-sum
//     cancellation).  The 16 lanes that share a 64-sample block reduce its
//     maximum and argmax with cross-lane exchanges; the wave's (up to 16)
//     above-threshold blocks of a level reserve their records with one
//     atomic.
#include "device_common.hpp"
#include "psoup/singlepulse.hpp"

#include <cfloat>

namespace psoup {
namespace kern {

namespace {

constexpr int kThreads = 512;
constexpr int kHaloMax = 1 << kSpMaxLog2;
constexpr int kLdsFloats = kSpTile + kHaloMax + 8;   // + 8: the register levels read 12 samples per group
constexpr int kGroups = (kSpTile + kHaloMax) / (4 * kThreads);  // 4-sample groups per thread (6)
constexpr int kOwnGroups = kSpTile / (4 * kThreads);            // of them, groups of start samples (4)
static_assert((kSpTile + kHaloMax) % (4 * kThreads) == 0 && kSpTile % (4 * kThreads) == 0, "tile / thread layout");
static_assert(kOwnGroups <= 16, "one holder lane per own group in a 16-lane row");
static_assert(kSpTile % kSpBlock == 0 && kSpBlock == 64, "64-sample blocks = 16 lanes x 4 samples");

// Trend at sample i: linear between block centres, flat beyond the first and
// last centre (ffa.hip detrend_kernel).  inv_w = 1 / w in double.
__device__ __forceinline__ float trend_at(uint64_t i, const float* __restrict__ means, int nblk, double half,
                                          double inv_w) {
  const double pos = (static_cast<double>(i) - half) * inv_w;  // in block-centre units
  if (pos <= 0.0 || nblk == 1) return means[0];
  if (pos >= nblk - 1) return means[nblk - 1];
  const int b = static_cast<int>(pos);
  const float fr = static_cast<float>(pos - b);
  const float m0 = means[b];
  return m0 + fr * (means[b + 1] - m0);
}

// grid (nblk, ndm): one workgroup sums one trend block of one DM.
__global__ void __launch_bounds__(256) block_means_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride,
                                                          uint64_t n, uint64_t w, int nblk,
                                                          float* __restrict__ means) {
  __shared__ unsigned long long scratch[4];
  const uint8_t* in = rows + static_cast<uint64_t>(blockIdx.y) * row_stride;
  const uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * w;
  const uint64_t b1 = b0 + w < n ? b0 + w : n;
  unsigned long long acc = 0;
  for (uint64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) acc += in[i];
  acc = dev::block_sum(acc, scratch);
  if (threadIdx.x == 0)
    means[static_cast<uint64_t>(blockIdx.y) * nblk + blockIdx.x] =
        static_cast<float>(static_cast<double>(acc) / static_cast<double>(b1 - b0));
}

// grid (kSpSigmaParts, ndm): part p sums x^2 over samples [p span, (p + 1) span).
__global__ void __launch_bounds__(256) sigma_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, uint64_t n,
                                                    uint64_t w, const float* __restrict__ means_all, int nblk,
                                                    uint64_t span, double* __restrict__ partials) {
  __shared__ double scratch[4];
  const uint8_t* in = rows + static_cast<uint64_t>(blockIdx.y) * row_stride;
  const float* means = means_all + static_cast<uint64_t>(blockIdx.y) * nblk;
  const double half = 0.5 * static_cast<double>(w), inv_w = 1.0 / static_cast<double>(w);
  const uint64_t a0 = static_cast<uint64_t>(blockIdx.x) * span;
  const uint64_t a1 = a0 + span < n ? a0 + span : n;
  double acc = 0.0;
  for (uint64_t i = a0 + threadIdx.x; i < a1; i += blockDim.x) {
    const float x = static_cast<float>(in[i]) - trend_at(i, means, nblk, half, inv_w);
    acc += static_cast<double>(x) * static_cast<double>(x);
  }
  acc = dev::block_sum(acc, scratch);
  if (threadIdx.x == 0) partials[static_cast<uint64_t>(blockIdx.y) * kSpSigmaParts + blockIdx.x] = acc;
}

// (v, idx) <- the larger of it and its partner `off` lanes away; the lower
// index on an exact tie.
__device__ __forceinline__ void row_max_step(float& v, uint32_t& idx, int off) {
  const float ov = __shfl_xor(v, off, 64);
  const uint32_t oi = __shfl_xor(idx, off, 64);
  if (ov > v || (ov == v && oi < idx)) {
    v = ov;
    idx = oi;
  }
}

struct SearchArgs {
  const uint8_t* rows;
  uint64_t row_stride;
  uint64_t n;
  uint64_t baseline;
  const float* means;
  int nblk;
  const double* partials;
  int kmax;
  float thresh;
  int dm_idx0;
  SpEvent* events;
  uint32_t* count;
  uint32_t capacity;
  float* best_snr;
  uint32_t* best_arg;
  uint32_t nblk64;
};

// S/N of the four boxcars of width 2^k a thread holds (starts g0 .. g0 + 3)
// -> maximum over the 64-sample block its 16-lane row covers; every lane of
// the row gets the result.  Starts past n - w are not evaluated.
__device__ __forceinline__ void block_max(const float (&b)[4], float scale, uint64_t g0, uint64_t last_start,
                                          bool has_last, float& v, uint32_t& idx) {
  v = -FLT_MAX;
  idx = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float s = b[j] * scale;
    const bool ok = has_last && g0 + j <= last_start;
    if (ok && s > v) {
      v = s;
      idx = static_cast<uint32_t>(g0 + j);
    }
  }
  row_max_step(v, idx, 1);
  row_max_step(v, idx, 2);
  row_max_step(v, idx, 4);
  row_max_step(v, idx, 8);
}

// The wave's block maxima of level k sit in the holder lanes (hold): dense
// output, and one atomic for all of the wave's records of this level.
__device__ __forceinline__ void emit_level(const SearchArgs& a, int k, bool hold, uint32_t blk, float v, uint32_t idx,
                                           bool live_row) {
  const int lane = threadIdx.x & 63;
  const bool in_range = hold && blk < a.nblk64;
  const bool found = in_range && idx != 0xffffffffu;
  if (a.best_snr && in_range) {
    const uint64_t o = (static_cast<uint64_t>(blockIdx.y) * (a.kmax + 1) + k) * a.nblk64 + blk;
    a.best_snr[o] = found ? v : 0.f;
    a.best_arg[o] = idx;
  }
  const bool pred = found && live_row && v >= a.thresh;
  const unsigned long long mask = __ballot(pred);
  if (mask == 0ull) return;  // the usual case
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(a.count, static_cast<uint32_t>(__popcll(mask)));
  base = __shfl(base, 0, 64);
  if (pred) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t pos = base + static_cast<uint32_t>(__popcll(mask & lt));
    if (pos < a.capacity) a.events[pos] = SpEvent{idx, k, v, a.dm_idx0 + static_cast<int32_t>(blockIdx.y)};
  }
}

// grid (ceil(n / kSpTile), ndm), kThreads threads.
__global__ void __launch_bounds__(kThreads) search_kernel(SearchArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ double s_sumsq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.kmax;
  const int H = 1 << K;
  const int L = kSpTile + H;  // LDS samples a boxcar can touch
  const uint64_t n = a.n;
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kSpTile;
  const uint8_t* row = a.rows + static_cast<uint64_t>(blockIdx.y) * a.row_stride;
  const float* means = a.means + static_cast<uint64_t>(blockIdx.y) * a.nblk;

  // sigma from the partial sums, the same fixed order in every workgroup
  if (wave == 0) {
    const double p = a.partials[static_cast<uint64_t>(blockIdx.y) * kSpSigmaParts + lane];
    const double tot = dev::wave_sum(p);
    if (lane == 0) s_sumsq = tot;
  }
  __syncthreads();
  const double sigma = sqrt(s_sumsq / static_cast<double>(n));
  const bool live_row = sigma > 0.0;
  const float inv_sigma = live_row ? static_cast<float>(1.0 / sigma) : 0.f;

  // stage (u - trend) / sigma; samples at or past n are zero (no evaluated boxcar covers them)
  {
    const double half = 0.5 * static_cast<double>(a.baseline), inv_w = 1.0 / static_cast<double>(a.baseline);
    for (int q = tid; q < (L + 8) / 4; q += kThreads) {
      const uint64_t g = t0 + 4u * static_cast<uint64_t>(q);
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g < n) {  // the dword lies inside the row: row_stride >= n and is a multiple of 4
        const uint32_t u = *reinterpret_cast<const uint32_t*>(row + g);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x = static_cast<float>((u >> (8 * j)) & 0xffu) - trend_at(g + j, means, a.nblk, half, inv_w);
          v[j] = g + j < n ? x * inv_sigma : 0.f;
        }
        y = make_float4(v[0], v[1], v[2], v[3]);
      }
      *reinterpret_cast<float4*>(&lds[4 * q]) = y;
    }
  }
  __syncthreads();

  const int row16 = lane >> 4, in_row = lane & 15;
  const bool hold = in_row < kOwnGroups;  // lane in_row of a row keeps the row's block of own group in_row
  // 64-sample block of this lane's row in own group g: t0 / 64 + g * (kThreads / 16) + wave * 4 + row16
  const uint32_t blk_base = static_cast<uint32_t>(t0 / kSpBlock) + static_cast<uint32_t>(wave * 4 + row16);
  const uint32_t my_blk = blk_base + static_cast<uint32_t>(in_row) * (kThreads / 16);

  // levels 0..3 (widths 1, 2, 4, 8) in registers; b[g] = B_8 of group g
  float b[kGroups][4];
  {
    float hv[4];
    uint32_t hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hv[k] = -FLT_MAX;
      hi[k] = 0xffffffffu;
    }
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int i = 4 * (g * kThreads + tid);
      float y[12];
      if (i + 4 <= L) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float4 r = *reinterpret_cast<const float4*>(&lds[i + 4 * c]);
          y[4 * c] = r.x, y[4 * c + 1] = r.y, y[4 * c + 2] = r.z, y[4 * c + 3] = r.w;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 12; ++c) y[c] = 0.f;
      }
      float b2[10], b4[8];
#pragma unroll
      for (int j = 0; j < 10; ++j) b2[j] = y[j] + y[j + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) b4[j] = b2[j] + b2[j + 2];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[g][j] = b4[j] + b4[j + 4];
      if (g < kOwnGroups) {
        const uint64_t g0 = t0 + static_cast<uint64_t>(i);
        const float lv[4][4] = {{y[0], y[1], y[2], y[3]},
                                {b2[0], b2[1], b2[2], b2[3]},
                                {b4[0], b4[1], b4[2], b4[3]},
                                {b[g][0], b[g][1], b[g][2], b[g][3]}};
        const float sc[4] = {1.f, 0.70710678118654752f, 0.5f, 0.35355339059327376f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k > K) continue;
          const uint64_t w = 1ull << k;
          float v;
          uint32_t idx;
          block_max(lv[k], sc[k], g0, n >= w ? n - w : 0, n >= w, v, idx);
          if (in_row == g) {
            hv[k] = v;
            hi[k] = idx;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k <= K) emit_level(a, k, hold, my_blk, hv[k], hi[k], live_row);
  }
  __syncthreads();  // every read of the staged samples is done
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const int i = 4 * (g * kThreads + tid);
    if (i + 4 <= L) *reinterpret_cast<float4*>(&lds[i]) = make_float4(b[g][0], b[g][1], b[g][2], b[g][3]);
  }
  __syncthreads();

  // levels 4..K: B_2w[i] = B_w[i] (registers) + B_w[i + w] (LDS).  A group
  // whose partner lies past L keeps a stale value; only starts at or past
  // kSpTile + H - 2w (not needed by any wider level) can depend on it.
  for (int k = 4; k <= K; ++k) {
    const int w = 1 << (k - 1);
    const float scale = (k & 1) ? 0.70710678118654752f / static_cast<float>(1 << (k >> 1))
                                : 1.f / static_cast<float>(1 << (k >> 1));
    const uint64_t w2 = 2ull * w;
    float hv = -FLT_MAX;
    uint32_t hi = 0xffffffffu;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int i = 4 * (g * kThreads + tid);
      if (i + w + 4 <= L) {
        const float4 r = *reinterpret_cast<const float4*>(&lds[i + w]);
        b[g][0] += r.x, b[g][1] += r.y, b[g][2] += r.z, b[g][3] += r.w;
      }
      if (g < kOwnGroups) {
        float v;
        uint32_t idx;
        block_max(b[g], scale, t0 + static_cast<uint64_t>(i), n >= w2 ? n - w2 : 0, n >= w2, v, idx);
        if (in_row == g) {
          hv = v;
          hi = idx;
        }
      }
    }
    emit_level(a, k, hold, my_blk, hv, hi, live_row);
    if (k == K) break;
    __syncthreads();  // every read of B_w is done
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int i = 4 * (g * kThreads + tid);
      if (i + w + 4 <= L) *reinterpret_cast<float4*>(&lds[i]) = make_float4(b[g][0], b[g][1], b[g][2], b[g][3]);
    }
    __syncthreads();
  }
}

void check_rows(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline) {
  PSOUP_CHECK(rows != nullptr && ndm > 0 && ndm < 65536, "single pulse: bad trial block");
  PSOUP_CHECK(n > 0 && n < (uint64_t(1) << 32), "single pulse: series length");
  PSOUP_CHECK(row_stride >= n && row_stride % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 4 == 0,
              "single pulse: rows must be 4-byte aligned with a stride >= nsamps");
  PSOUP_CHECK(baseline > 0 && baseline <= n, "single pulse: trend block length");
}

}  // namespace

void sp_block_means(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, float* means,
                    hipStream_t s) {
  check_rows(rows, row_stride, ndm, n, baseline);
  const uint64_t nblk = (n + baseline - 1) / baseline;
  block_means_kernel<<<dim3(static_cast<unsigned>(nblk), ndm), 256, 0, s>>>(rows, row_stride, n, baseline,
                                                                            static_cast<int>(nblk), means);
  post_launch_check("sp block_means_kernel", s);
}

void sp_sigma(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, const float* means,
              double* partials, hipStream_t s) {
  check_rows(rows, row_stride, ndm, n, baseline);
  const uint64_t nblk = (n + baseline - 1) / baseline;
  const uint64_t span = (n + kSpSigmaParts - 1) / kSpSigmaParts;
  sigma_kernel<<<dim3(kSpSigmaParts, ndm), 256, 0, s>>>(rows, row_stride, n, baseline, means, static_cast<int>(nblk),
                                                        span, partials);
  post_launch_check("sp sigma_kernel", s);
}

void sp_search(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, const float* means,
               const double* partials, int kmax, float thresh, int dm_idx0, SpEvent* events, uint32_t* count,
               uint32_t capacity, float* best_snr, uint32_t* best_arg, hipStream_t s) {
  check_rows(rows, row_stride, ndm, n, baseline);
  PSOUP_CHECK(kmax >= 2 && kmax <= kSpMaxLog2 && (uint64_t(1) << kmax) <= n, "single pulse: width ladder");
  PSOUP_CHECK((best_snr == nullptr) == (best_arg == nullptr), "single pulse: dense outputs come as a pair");
  PSOUP_CHECK(events != nullptr || capacity == 0, "single pulse: record buffer");
  SearchArgs a{};
  a.rows = rows;
  a.row_stride = row_stride;
  a.n = n;
  a.baseline = baseline;
  a.means = means;
  a.nblk = static_cast<int>((n + baseline - 1) / baseline);
  a.partials = partials;
  a.kmax = kmax;
  a.thresh = thresh;
  a.dm_idx0 = dm_idx0;
  a.events = events;
  a.count = count;
  a.capacity = capacity;
  a.best_snr = best_snr;
  a.best_arg = best_arg;
  a.nblk64 = static_cast<uint32_t>((n + kSpBlock - 1) / kSpBlock);
  const unsigned ntiles = static_cast<unsigned>((n + kSpTile - 1) / kSpTile);
  search_kernel<<<dim3(ntiles, ndm), kThreads, 0, s>>>(a);
  post_launch_check("sp search_kernel", s);
}

}  // namespace kern
}  // namespace psoup
