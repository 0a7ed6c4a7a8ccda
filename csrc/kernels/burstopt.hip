// burstopt: the search of psoup/burstopt.hpp (step 3), all int32.
//
// One workgroup of four waves owns a candidate and up to eight profile rows of
// one plane.  A coarse row is a copy of a DM-time row: a wave reads it
// straight into registers.  The fine rows of a workgroup are built together:
// the waterfall is staged through LDS a few subbands at a time (two buffers;
// the next step's loads are issued before this step's sums and written after
// them, one barrier per step), a thread owns bin `tid` and every 256th after
// it, and every staged subband is read once per fine row at that row's shift
// (wave-uniform, from an SGPR: consecutive lanes read consecutive banks), with
// a bounds check in place of burstcube's window.  The finished rows go back to
// LDS and each wave takes rows in turn: a lane owns bin `lane` and every 64th
// after it, the box sums come from dyadic doubling S_2w[k] = S_w[k] + S_w[k +
// w] through the row in LDS, and value and smallest bin are reduced over the
// wave as one 64-bit key of biased value and inverted index.  A row has one
// owner, so curve / curve_bin are plain stores; a wave folds its bests into
// the plane's with one 64-bit atomic maximum per width, so every output is
// independent of the order of evaluation.  No floating point.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/burstopt.hpp"

namespace psoup {
namespace kern {

namespace {

static_assert(kBoptThreads == 256, "four waves per workgroup");
static_assert(kBoptRowsPerWg * kBoptMaxTime <= 2 * kBoptStage, "the finished rows reuse the staging buffers");
constexpr int kWaves = kBoptThreads / 64;
constexpr int kPrefetch = kBoptStage / kBoptThreads;

__device__ __forceinline__ unsigned long long pack_key(int32_t val, int32_t idx) {
  const uint32_t hi = static_cast<uint32_t>(val) ^ 0x80000000u;
  const uint32_t lo = ~static_cast<uint32_t>(idx);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}
__device__ __forceinline__ int32_t key_val(unsigned long long k) {
  return static_cast<int32_t>(static_cast<uint32_t>(k >> 32) ^ 0x80000000u);
}
__device__ __forceinline__ int32_t key_idx(unsigned long long k) { return static_cast<int32_t>(~static_cast<uint32_t>(k)); }

// The maximum over the wave, uniform.
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long key) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  return key;
}

// Orders this wave's LDS stores before its later LDS loads (and the reverse)
// for the compiler; the hardware runs one wave's LDS operations in order.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void bopt_decode_kernel(const unsigned long long* keys, size_t nkeys, int32_t* best_val, int32_t* best_idx) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nkeys) return;
  const unsigned long long k = keys[i];
  best_val[i] = key_val(k);
  best_idx[i] = key_idx(k);
}

// One profile row held as S[j] = P[lane + 64 j] (0 beyond ntime): every width's
// maximum and its smallest bin.  row: ntime dwords of LDS owned by this wave.
template <int NB>
__device__ __forceinline__ void scan_row(int32_t (&S)[NB], int32_t* row, int ntime, int nw, int lane, int r_local,
                                         int32_t* curve, int32_t* curve_bin, size_t out_stride,
                                         unsigned long long (&best)[kBoptMaxWidths]) {
#pragma unroll
  for (int kw = 0; kw < kBoptMaxWidths; ++kw) {
    if (kw < nw) {
      const int w = 1 << kw;
      const int last = ntime - w;  // S_w[k] exists for k <= last
      unsigned long long key = 0ull;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int k = lane + 64 * j;
        const unsigned long long c = pack_key(S[j], k);
        if (k <= last && c > key) key = c;
      }
      key = wave_max_key(key);
      const int32_t val = key_val(key), bin = key_idx(key);
      if (lane == 0) {
        curve[static_cast<size_t>(kw) * out_stride] = val;
        curve_bin[static_cast<size_t>(kw) * out_stride] = bin;
      }
      const unsigned long long flat = pack_key(val, r_local * ntime + bin);
      if (flat > best[kw]) best[kw] = flat;
      if (kw + 1 < nw) {
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int k = lane + 64 * j;
          if (k < ntime) row[k] = S[j];
        }
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int x = lane + 64 * j + w;
          S[j] += x < ntime ? row[x] : 0;
        }
      }
    }
  }
}

template <int NB>
__global__ __launch_bounds__(kBoptThreads) void burst_search_kernel(
    const int32_t* __restrict__ ds, const int32_t* __restrict__ dmt, const int32_t* __restrict__ sf, int ntime,
    int nsub, int ndm, int nfine, int nw, int coarse_groups, unsigned long long* keys, int32_t* curve,
    int32_t* curve_bin) {
  constexpr int NBT = NB >= 4 ? NB / 4 : 1;  // bins of a thread while the fine rows are built
  constexpr int KF = kBoptRowsPerWg;
  __shared__ int32_t lds[2 * kBoptStage];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t cand = blockIdx.y;
  const int nrows = ndm + nfine;
  const bool fine = static_cast<int>(blockIdx.x) >= coarse_groups;
  const int row0 = (fine ? static_cast<int>(blockIdx.x) - coarse_groups : static_cast<int>(blockIdx.x)) * KF;
  const int nr = min(KF, (fine ? nfine : ndm) - row0);
  int32_t* curve_c = curve + cand * static_cast<size_t>(nw) * nrows + (fine ? ndm : 0) + row0;
  int32_t* bin_c = curve_bin + cand * static_cast<size_t>(nw) * nrows + (fine ? ndm : 0) + row0;
  unsigned long long best[kBoptMaxWidths];
#pragma unroll
  for (int k = 0; k < kBoptMaxWidths; ++k) best[k] = 0ull;
  int32_t S[NB];

  if (!fine) {
    const int32_t* plane = dmt + (cand * ndm + row0) * static_cast<size_t>(ntime);
    for (int r = wave; r < nr; r += kWaves) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int k = lane + 64 * j;
        S[j] = k < ntime ? plane[static_cast<size_t>(r) * ntime + k] : 0;
      }
      scan_row<NB>(S, lds + wave * ntime, ntime, nw, lane, row0 + r, curve_c + r, bin_c + r,
                   static_cast<size_t>(nrows), best);
    }
  } else {
    // ---- the fine rows of this workgroup, all subbands
    const int32_t* dc = ds + cand * static_cast<size_t>(nsub) * ntime;
    const int32_t* sfc = sf + cand * static_cast<size_t>(nfine) * nsub;
    const int32_t* sfr[KF];
#pragma unroll
    for (int r = 0; r < KF; ++r) sfr[r] = sfc + static_cast<size_t>(min(row0 + r, nfine - 1)) * nsub;
    int32_t acc[KF][NBT];
#pragma unroll
    for (int r = 0; r < KF; ++r)
#pragma unroll
      for (int j = 0; j < NBT; ++j) acc[r][j] = 0;
    const int per = max(1, kBoptStage / ntime);  // subbands of a step
    const int nsteps = (nsub + per - 1) / per;
    int32_t pre[kPrefetch];
    {
      const int n0 = min(per, nsub) * ntime;
      for (int e = tid; e < n0; e += kBoptThreads) lds[e] = dc[e];
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
      const int s0 = st * per;
      const int cnt = min(per, nsub - s0);
      const int32_t* buf = lds + (st & 1) * kBoptStage;
      const bool more = st + 1 < nsteps;
      const int s1 = s0 + per;
      const int n1 = more ? min(per, nsub - s1) * ntime : 0;
      if (more) {
        const int32_t* src = dc + static_cast<size_t>(s1) * ntime;
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
          const int e = tid + i * kBoptThreads;
          pre[i] = e < n1 ? src[e] : 0;
        }
      }
      for (int sl = 0; sl < cnt; ++sl) {
        const int32_t* row = buf + sl * ntime;
#pragma unroll
        for (int r = 0; r < KF; ++r) {
          const int sh = sfr[r][s0 + sl];
#pragma unroll
          for (int j = 0; j < NBT; ++j) {
            const int x = tid + kBoptThreads * j + sh;
            acc[r][j] += static_cast<unsigned>(x) < static_cast<unsigned>(ntime) ? row[x] : 0;
          }
        }
      }
      if (more) {
        int32_t* dst = lds + ((st + 1) & 1) * kBoptStage;
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
          const int e = tid + i * kBoptThreads;
          if (e < n1) dst[e] = pre[i];
        }
      }
      __syncthreads();
    }
    // ---- the finished rows go to LDS (every thread is past its last staged read), then a wave per row
#pragma unroll
    for (int r = 0; r < KF; ++r)
#pragma unroll
      for (int j = 0; j < NBT; ++j) {
        const int k = tid + kBoptThreads * j;
        if (r < nr && k < ntime) lds[r * ntime + k] = acc[r][j];
      }
    __syncthreads();
    for (int r = wave; r < nr; r += kWaves) {
      int32_t* row = lds + r * ntime;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int k = lane + 64 * j;
        S[j] = k < ntime ? row[k] : 0;
      }
      scan_row<NB>(S, row, ntime, nw, lane, row0 + r, curve_c + r, bin_c + r, static_cast<size_t>(nrows), best);
    }
  }

  // ---- the wave's bests: value and inverted index in one key
  if (lane == 0) {
    unsigned long long* kc = keys + (cand * 2 + (fine ? 1 : 0)) * static_cast<size_t>(nw);
#pragma unroll
    for (int k = 0; k < kBoptMaxWidths; ++k)
      if (k < nw && best[k] != 0ull) atomicMax(kc + k, best[k]);
  }
}

template <int NB>
void launch_search(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* d_sf, const BoptDims& g, int ncand,
                   unsigned long long* keys, int32_t* d_curve, int32_t* d_curve_bin, hipStream_t s) {
  const int cg = (g.ndm + kBoptRowsPerWg - 1) / kBoptRowsPerWg;
  const int fg = (g.nfine + kBoptRowsPerWg - 1) / kBoptRowsPerWg;
  const dim3 grid(static_cast<unsigned>(cg + fg), static_cast<unsigned>(ncand));
  burst_search_kernel<NB><<<grid, kBoptThreads, 0, s>>>(d_ds, d_dmt, d_sf, g.ntime, g.nsub, g.ndm, g.nfine, g.nw, cg,
                                                        keys, d_curve, d_curve_bin);
  post_launch_check("burst_search_kernel", s);
}

}  // namespace

void burst_search(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* d_sf, const BoptDims& g, int ncand,
                  uint64_t* d_keys, int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_curve, int32_t* d_curve_bin,
                  hipStream_t s) {
  PSOUP_CHECK(g.ntime >= 2 && g.ntime <= kBoptMaxTime && g.nsub >= 1 && g.ndm >= 1 && g.ndm <= 65536 &&
                  g.nfine >= 1 && g.nfine <= kBoptMaxFine,
              "burst opt: ntime must be in 2.." << kBoptMaxTime << ", nsub and ndm at least 1, nfine in 1.."
                                                << kBoptMaxFine);
  PSOUP_CHECK(g.nw == bopt_nwidths(g.ntime) && g.nw <= kBoptMaxWidths, "burst opt: bad width count");
  PSOUP_CHECK(ncand >= 1 && ncand <= 65535, "burst opt: 1..65535 candidates per launch");
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(d_keys);
  const size_t nkeys = static_cast<size_t>(ncand) * 2 * g.nw;
  PSOUP_HIP_CHECK(hipMemsetAsync(keys, 0, nkeys * sizeof(unsigned long long), s));
  const int nb = (g.ntime + 63) / 64;
  if (nb <= 1)
    launch_search<1>(d_ds, d_dmt, d_sf, g, ncand, keys, d_curve, d_curve_bin, s);
  else if (nb <= 2)
    launch_search<2>(d_ds, d_dmt, d_sf, g, ncand, keys, d_curve, d_curve_bin, s);
  else if (nb <= 4)
    launch_search<4>(d_ds, d_dmt, d_sf, g, ncand, keys, d_curve, d_curve_bin, s);
  else if (nb <= 8)
    launch_search<8>(d_ds, d_dmt, d_sf, g, ncand, keys, d_curve, d_curve_bin, s);
  else
    launch_search<16>(d_ds, d_dmt, d_sf, g, ncand, keys, d_curve, d_curve_bin, s);
  bopt_decode_kernel<<<static_cast<unsigned>((nkeys + 255) / 256), 256, 0, s>>>(keys, nkeys, d_best_val, d_best_idx);
  post_launch_check("bopt_decode_kernel", s);
}

}  // namespace kern
}  // namespace psoup
