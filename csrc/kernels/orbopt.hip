// orbopt kernels (psoup/orbopt.hpp): the fused resample-and-fold of a
// dedispersed byte row at K circular-orbit templates, and the search of the
// fold planes over period drift and boxcar width.  Integer arithmetic
// throughout; every output is an integer sum or maximum, so it does not depend
// on the order of evaluation.
//
// orbopt_fold.  Grid (subint x slice, template, candidate); a workgroup copies
// the 16 KiB sine table into LDS once (as orbit.hip) and walks
// kOoptTilesPerGroup tiles of its slice of one subint.  Lanes run along time
// and a lane owns 16 adjacent samples on a 16-sample raster.  The template {W,
// F, Aq}, G and the row index are the same for the whole workgroup and come
// through scalar loads.  Where the lane's span lies inside the subint, holds no
// turning point of the sine and has equal shifts at its two ends, the shift is
// one value throughout (orbit.hpp's monotonicity argument) and the 16 source
// bytes are contiguous: five aligned dword loads and a byte alignment assemble
// them.  Every other lane -- a clamp, a turning point, a changing shift, the
// edges of the subint -- computes s per sample and loads bytes.  The resampled
// row is never written.  The phase histogram of the subint sits in LDS: a lane
// adds into a register while its bin does not change and issues an LDS atomic
// only at a bin change; what is left at the end of its span is reduced across
// the wave first when the whole wave sits in one bin (a slow pulsar), else
// added per lane.  One integer global atomic per (k, j, b) and workgroup then
// adds the histogram into fold, which is zeroed before the launch.
//
// orbopt_search.  cubeopt.hip's structure: one workgroup of four waves per
// (candidate, template), the plane d = fold - m hits in LDS, a wave per drift
// trial, a lane per bin (and every 64th after it), box sums by dyadic doubling
// through a per-wave LDS row, value and inverted flat index as one 64-bit key,
// one atomic maximum per wave and width; tcurve, centre and msum go by plain
// stores.
#include <algorithm>
#include <atomic>

#include "device_common.hpp"
#include "psoup/orbopt.hpp"

namespace psoup {
namespace kern {

namespace {

constexpr int kLane = kOoptLane;
constexpr int32_t kLowest = INT32_MIN;
static_assert(kOoptThreads == 256, "four waves per workgroup");
constexpr int kWaves = kOoptThreads / 64;

// the definition's S(th) on the table in LDS
__device__ __forceinline__ long long sine_of(const int32_t* tbl, uint64_t th) {
  const uint32_t j = static_cast<uint32_t>(th >> 52);
  const long long f = static_cast<long long>((th >> 32) & 0xFFFFFull);
  const long long t0 = tbl[j], t1 = tbl[j + 1];
  return t0 + (((t1 - t0) * f + (1ll << 19)) >> 20);
}

// the definition's s(i) from th_i
__device__ __forceinline__ long long shift_of(const int32_t* tbl, uint64_t th, long long aq, long long sf) {
  return (aq * (sine_of(tbl, th) - sf) + (1ll << 37)) >> 38;
}

__device__ __forceinline__ int bin_of(uint64_t phi, uint32_t nbins) {
  return static_cast<int>(((phi >> 32) * static_cast<uint64_t>(nbins)) >> 32);
}

__global__ __launch_bounds__(kOoptThreads) void orbopt_fold_kernel(
    const uint8_t* __restrict__ in, uint64_t row_stride, uint64_t in_bytes, int in_aligned,
    const int32_t* __restrict__ row_of, const uint64_t* __restrict__ Gs, const OrbitQuant* __restrict__ q, int K,
    uint64_t n, int nints, int nbins, int slices, const int32_t* __restrict__ table, uint32_t* __restrict__ fold) {
  __shared__ int32_t tbl[kOrbitTable];
  __shared__ uint32_t hist[kOoptMaxBins];
  const int tid = static_cast<int>(threadIdx.x);
  const int j = static_cast<int>(blockIdx.x) / slices;
  const int slice = static_cast<int>(blockIdx.x) - j * slices;
  // the subint's samples [lo, hi): j(i) = (i nints) / n == j
  const uint64_t lo = (static_cast<uint64_t>(j) * n + static_cast<uint64_t>(nints) - 1) / static_cast<uint64_t>(nints);
  const uint64_t hi =
      (static_cast<uint64_t>(j + 1) * n + static_cast<uint64_t>(nints) - 1) / static_cast<uint64_t>(nints);
  const uint64_t first = (lo & ~static_cast<uint64_t>(kLane - 1)) +
                         static_cast<uint64_t>(slice) * (static_cast<uint64_t>(kOoptTile) * kOoptTilesPerGroup);
  if (first >= hi) return;  // uniform: nothing of this subint in this slice (before any barrier)
  for (int e = tid; e < kOrbitTable; e += kOoptThreads) tbl[e] = table[e];
  for (int e = tid; e < nbins; e += kOoptThreads) hist[e] = 0u;
  __syncthreads();
  const int k = static_cast<int>(blockIdx.y);
  const uint64_t c = blockIdx.z;
  const OrbitQuant* qc = q + c * static_cast<uint64_t>(K) + static_cast<uint64_t>(k);
  const uint64_t W = qc->W, F = qc->F;
  const long long aq = qc->Aq;
  const uint64_t G = Gs[c];
  const uint64_t rbase = static_cast<uint64_t>(row_of[c]) * row_stride;  // byte offset of the row in `in`
  const uint8_t* x = in + rbase;
  const long long sf = sine_of(tbl, F);
  const long long N = static_cast<long long>(n);
  const uint32_t nb = static_cast<uint32_t>(nbins);
  const int lane = tid & 63;

  for (int t = 0; t < kOoptTilesPerGroup; ++t) {
    const uint64_t tile0 = first + static_cast<uint64_t>(t) * kOoptTile;
    if (tile0 >= hi) break;  // uniform
    const uint64_t i0 = tile0 + static_cast<uint64_t>(tid) * kLane;
    const long long I0 = static_cast<long long>(i0);
    const bool any = i0 < hi && i0 + kLane > lo;
    const bool whole = i0 >= lo && i0 + kLane <= hi;  // hi <= n
    uint32_t acc = 0u;
    int cur = -1;
    if (any) {
      const uint64_t th0 = F + i0 * W;  // wrapping
      union {
        uint32_t w[4];
        uint8_t b[kLane];
      } v;
      bool have = false;
      if (in_aligned && whole) {
        const uint64_t th1 = th0 + static_cast<uint64_t>(kLane - 1) * W;
        const bool clear = (((th0 + (1ull << 62)) ^ (th1 + (1ull << 62))) >> 63) == 0;
        if (clear) {
          const long long s0 = shift_of(tbl, th0, aq, sf), s1 = shift_of(tbl, th1, aq, sf);
          if (s0 == s1 && I0 + s0 >= 0 && I0 + s0 + kLane <= N) {
            const uint64_t off = rbase + static_cast<uint64_t>(I0 + s0);
            const uint64_t a = off & ~3ull;
            const uint32_t sh = static_cast<uint32_t>(off & 3ull);
            if (a + (sh ? 20u : 16u) <= in_bytes) {
              const uint32_t* p = reinterpret_cast<const uint32_t*>(in + a);
              const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
              const uint32_t w4 = sh ? p[4] : 0u;
              v.w[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
              v.w[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
              v.w[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
              v.w[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
              have = true;
            }
          }
        }
      }
      uint64_t phi = i0 * G;  // wrapping
      if (have) {
#pragma unroll
        for (int s = 0; s < kLane; ++s, phi += G) {
          const int b = bin_of(phi, nb);
          if (b != cur) {
            if (cur >= 0) atomicAdd(&hist[cur], acc);
            cur = b;
            acc = 0u;
          }
          acc += v.b[s];
        }
      } else {
        uint64_t th = th0;
#pragma unroll
        for (int s = 0; s < kLane; ++s, th += W, phi += G) {
          const uint64_t i = i0 + static_cast<uint64_t>(s);
          if (i >= lo && i < hi) {
            const long long src = min(max(static_cast<long long>(i) + shift_of(tbl, th, aq, sf), 0ll), N - 1);
            const int b = bin_of(phi, nb);
            if (b != cur) {
              if (cur >= 0) atomicAdd(&hist[cur], acc);
              cur = b;
              acc = 0u;
            }
            acc += x[src];
          }
        }
      }
    }
    // what is left: one add for the wave when all its lanes sit in one bin
    const unsigned long long live = __ballot(cur >= 0);
    if (live != 0ull) {  // uniform
      const int firstl = __ffsll(static_cast<long long>(live)) - 1;
      const int b0 = __shfl(cur, firstl, 64);
      if (__ballot(cur >= 0 && cur != b0) == 0ull) {  // uniform
        uint32_t tot = cur >= 0 ? acc : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(tot, off, 64);
        if (lane == 0) atomicAdd(&hist[b0], tot);
      } else if (cur >= 0) {
        atomicAdd(&hist[cur], acc);
      }
    }
  }
  __syncthreads();
  uint32_t* out = fold + ((c * static_cast<uint64_t>(K) + static_cast<uint64_t>(k)) * static_cast<uint64_t>(nints) +
                          static_cast<uint64_t>(j)) * static_cast<uint64_t>(nbins);
  for (int e = tid; e < nbins; e += kOoptThreads) {
    const uint32_t h = hist[e];
    if (h) atomicAdd(out + e, h);
  }
}

// ------------------------------------------------------------- search ----
// The maximum over the wave, uniform (every lane must be active).
__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ unsigned long long pack_key(int32_t val, int32_t idx) {
  const uint32_t hi = static_cast<uint32_t>(val) ^ 0x80000000u;
  const uint32_t lo = ~static_cast<uint32_t>(idx);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// Orders this wave's LDS stores before its later LDS loads (and the reverse)
// for the compiler; the hardware runs one wave's LDS operations in order.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void oopt_init_kernel(unsigned long long* keys, size_t nkeys) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < nkeys) keys[i] = 0ull;
}

__global__ void oopt_decode_kernel(const unsigned long long* keys, size_t nkeys, int32_t* best_val, int32_t* best_idx) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nkeys) return;
  const unsigned long long k = keys[i];
  best_val[i] = static_cast<int32_t>(static_cast<uint32_t>(k >> 32) ^ 0x80000000u);
  best_idx[i] = static_cast<int32_t>(~static_cast<uint32_t>(k));
}

template <int NB>
__global__ __launch_bounds__(kOoptThreads) void orbopt_search_kernel(
    const int32_t* __restrict__ fold, const int32_t* __restrict__ hits, const int32_t* __restrict__ ms,
    const int32_t* __restrict__ st, int K, int nints, int nbins, int np, int nw, unsigned long long* keys,
    int32_t* tcurve, int32_t* centre, long long* msum) {
  extern __shared__ int32_t lds[];
  __shared__ int32_t wbest[kWaves][kOoptMaxWidths];
  __shared__ long long wsum[kWaves];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = static_cast<int>(blockIdx.x);
  const size_t cand = blockIdx.y;
  const int plane = nints * nbins;
  int32_t* A = lds;                           // [nints][nbins]
  int32_t* row = lds + plane + wave * nbins;  // this wave's box-sum row

  // ---- stage 1: d = fold - m hits (modulo 2^32: exact), and its sum
  {
    const int32_t* f = fold + (cand * static_cast<size_t>(K) + static_cast<size_t>(k)) * static_cast<size_t>(plane);
    const int32_t* h = hits + cand * static_cast<size_t>(plane);
    const uint32_t m = static_cast<uint32_t>(ms[cand]);
    long long sum = 0;
    for (int e = tid; e < plane; e += kOoptThreads) {
      const int32_t d = static_cast<int32_t>(static_cast<uint32_t>(f[e]) - m * static_cast<uint32_t>(h[e]));
      A[e] = d;
      sum += d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) wsum[wave] = sum;
  }
  __syncthreads();
  if (tid == 0) msum[cand * static_cast<size_t>(K) + static_cast<size_t>(k)] = wsum[0] + wsum[1] + wsum[2] + wsum[3];

  // ---- stage 2: the drift trials, one wave each in turn
  int bsafe[NB];
  bool act[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int b = lane + 64 * j;
    act[j] = b < nbins;
    bsafe[j] = act[j] ? b : 0;
  }
  int32_t bv[kOoptMaxWidths], bi[kOoptMaxWidths];
#pragma unroll
  for (int kk = 0; kk < kOoptMaxWidths; ++kk) {
    bv[kk] = kLowest;
    bi[kk] = INT32_MAX;
  }
  for (int l = wave; l < np; l += kWaves) {  // uniform per wave
    const int32_t* stl = st + static_cast<size_t>(l) * nints;
    int32_t S[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) S[j] = 0;
    for (int i = 0; i < nints; ++i) {
      const int sh = __builtin_amdgcn_readfirstlane(stl[i]);
      const int32_t* Ai = A + i * nbins;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        int x = bsafe[j] + sh;
        if (x >= nbins) x -= nbins;
        S[j] += Ai[x];
      }
    }
    const int32_t base = (k * np + l) * nbins;
    int32_t mine = kLowest;
#pragma unroll
    for (int kk = 0; kk < kOoptMaxWidths; ++kk) {
      if (kk < nw) {
        int32_t m = kLowest;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int32_t v = act[j] ? S[j] : kLowest;
          if (v > bv[kk]) {  // bins and trials come in ascending flat index: the first maximum stays
            bv[kk] = v;
            bi[kk] = base + lane + 64 * j;
          }
          m = max(m, v);
        }
        if (k == K / 2 && l == np / 2) {  // uniform
          m = wave_max(m);
          if (lane == kk) mine = m;
        }
        if (kk + 1 < nw) {
          const int w = 1 << kk;
          wave_lds_order();
#pragma unroll
          for (int j = 0; j < NB; ++j)
            if (act[j]) row[bsafe[j]] = S[j];
          wave_lds_order();
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            int x = bsafe[j] + w;
            if (x >= nbins) x -= nbins;
            S[j] += row[x];
          }
        }
      }
    }
    if (k == K / 2 && l == np / 2 && lane < nw) centre[cand * nw + lane] = mine;
  }

  // ---- the wave's bests: value and inverted index in one key
#pragma unroll
  for (int kk = 0; kk < kOoptMaxWidths; ++kk) {
    if (kk < nw) {
      unsigned long long key = pack_key(bv[kk], bi[kk]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
      }
      if (lane == 0) {
        wbest[wave][kk] = static_cast<int32_t>(static_cast<uint32_t>(key >> 32) ^ 0x80000000u);
        if (wave < np) atomicMax(keys + cand * nw + kk, key);
      }
    }
  }
  __syncthreads();
  if (tid < nw)
    tcurve[(cand * nw + tid) * static_cast<size_t>(K) + k] =
        max(max(wbest[0][tid], wbest[1][tid]), max(wbest[2][tid], wbest[3][tid]));
}

template <int NB>
void launch_search(const int32_t* fold, const int32_t* hits, const int32_t* m, const int32_t* st, int ncand, int K,
                   int nints, int nbins, int np, int nw, unsigned long long* keys, int32_t* tcurve, int32_t* centre,
                   int64_t* msum, hipStream_t s) {
  const size_t lds = static_cast<size_t>(nints * nbins + kWaves * nbins) * sizeof(int32_t);
  // above 64 KiB of dynamic LDS the limit has to be raised, once per instance and device
  if (lds > 65536 - 256) {
    static std::atomic<uint64_t> raised{0};
    int dev = 0;
    PSOUP_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = uint64_t(1) << (dev & 63);
    if (!(raised.load() & bit)) {
      PSOUP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&orbopt_search_kernel<NB>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (kOoptMaxPlane + kWaves * kOoptMaxBins) * static_cast<int>(sizeof(int32_t))));
      raised.fetch_or(bit);
    }
  }
  const dim3 grid(static_cast<unsigned>(K), static_cast<unsigned>(ncand));
  orbopt_search_kernel<NB><<<grid, kOoptThreads, lds, s>>>(fold, hits, m, st, K, nints, nbins, np, nw, keys, tcurve,
                                                           centre, reinterpret_cast<long long*>(msum));
  post_launch_check("orbopt_search_kernel", s);
}

}  // namespace

void orbopt_fold(const uint8_t* rows, uint64_t row_stride, uint64_t in_bytes, const int32_t* row_of, const uint64_t* G,
                 const OrbitQuant* q, int ncand, int K, uint64_t n, int nints, int nbins, const int32_t* table,
                 int32_t* fold, hipStream_t s) {
  PSOUP_CHECK(rows != nullptr && row_of != nullptr && G != nullptr && q != nullptr && table != nullptr &&
                  fold != nullptr,
              "orbopt_fold: missing buffer");
  PSOUP_CHECK(ncand >= 1 && ncand <= 65535, "orbopt_fold: 1..65535 candidates per launch");
  PSOUP_CHECK(K >= 1 && K <= kOoptMaxTemplates, "orbopt_fold: 1.." << kOoptMaxTemplates << " templates per launch");
  PSOUP_CHECK(n >= 1 && n <= kOrbitMaxSpan, "orbopt_fold: the span must be in 1..2^26");
  PSOUP_CHECK(row_stride >= n && in_bytes >= n, "orbopt_fold: a stride is shorter than the span");
  PSOUP_CHECK(nints >= 1 && nints <= kOoptMaxInts && nbins >= 2 && nbins <= kOoptMaxBins,
              "orbopt_fold: nints in 1.." << kOoptMaxInts << ", nbins in 2.." << kOoptMaxBins);
  const size_t cells = static_cast<size_t>(ncand) * K * nints * nbins;
  PSOUP_HIP_CHECK(hipMemsetAsync(fold, 0, cells * sizeof(int32_t), s));
  // a subint holds at most ceil(n / nints) samples, and its first lane span starts up to 15 samples early
  const uint64_t sub = (n + static_cast<uint64_t>(nints) - 1) / static_cast<uint64_t>(nints) + kLane;
  const uint64_t per = static_cast<uint64_t>(kOoptTile) * kOoptTilesPerGroup;
  const uint64_t slices = (sub + per - 1) / per;
  PSOUP_CHECK(slices * static_cast<uint64_t>(nints) < (1ull << 31), "orbopt_fold: row too long for one launch");
  const dim3 grid(static_cast<unsigned>(slices * static_cast<uint64_t>(nints)), static_cast<unsigned>(K),
                  static_cast<unsigned>(ncand));
  orbopt_fold_kernel<<<grid, kOoptThreads, 0, s>>>(rows, row_stride, in_bytes,
                                                   reinterpret_cast<uintptr_t>(rows) % 4 == 0 ? 1 : 0, row_of, G, q, K, n,
                                                   nints, nbins, static_cast<int>(slices), table,
                                                   reinterpret_cast<uint32_t*>(fold));
  post_launch_check("orbopt_fold_kernel", s);
}

void orbopt_search(const int32_t* fold, const int32_t* hits, const int32_t* m, const int32_t* st, int ncand, int K,
                   int nints, int nbins, int np, uint64_t* d_keys, int32_t* best_val, int32_t* best_idx, int32_t* tcurve,
                   int32_t* centre, int64_t* msum, hipStream_t s) {
  PSOUP_CHECK(nints >= 1 && nbins >= 2 && nbins <= kOoptMaxBins && nints * nbins <= kOoptMaxPlane,
              "orbopt_search: nbins must be in 2.." << kOoptMaxBins << " and nints * nbins at most " << kOoptMaxPlane);
  PSOUP_CHECK(K >= 1 && K <= kOoptMaxTemplates && np >= 1 && np <= 257, "orbopt_search: bad grid");
  PSOUP_CHECK(static_cast<uint64_t>(K) * np * nbins < (uint64_t(1) << 31),
              "orbopt_search: K np nbins >= 2^31: the trial bins do not fit 31 bits");
  PSOUP_CHECK(ncand >= 1 && ncand <= 65535, "orbopt_search: 1..65535 candidates per launch");
  const int nw = oopt_nwidths(nbins);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(d_keys);
  const size_t nkeys = static_cast<size_t>(ncand) * nw;
  oopt_init_kernel<<<static_cast<unsigned>((nkeys + 255) / 256), 256, 0, s>>>(keys, nkeys);
  post_launch_check("oopt_init_kernel", s);
  const int nb = (nbins + 63) / 64;
  if (nb == 1)
    launch_search<1>(fold, hits, m, st, ncand, K, nints, nbins, np, nw, keys, tcurve, centre, msum, s);
  else if (nb == 2)
    launch_search<2>(fold, hits, m, st, ncand, K, nints, nbins, np, nw, keys, tcurve, centre, msum, s);
  else if (nb == 3)
    launch_search<3>(fold, hits, m, st, ncand, K, nints, nbins, np, nw, keys, tcurve, centre, msum, s);
  else
    launch_search<4>(fold, hits, m, st, ncand, K, nints, nbins, np, nw, keys, tcurve, centre, msum, s);
  oopt_decode_kernel<<<static_cast<unsigned>((nkeys + 255) / 256), 256, 0, s>>>(keys, nkeys, best_val, best_idx);
  post_launch_check("oopt_decode_kernel", s);
}

}  // namespace kern
}  // namespace psoup
