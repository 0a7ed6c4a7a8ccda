// cubeopt: the search of psoup/cubeopt.hpp (step 3), all int32.
//
// One workgroup of four waves handles (candidate, DM trial kd, a slice of the
// np x npd period / acceleration trials).  Stage 1 builds the plane A[i][b] =
// sum_s d[i][s][(b + sdm[kd][s]) % nbins] in LDS (at most 64 KiB; 69632 bytes
// with the four per-wave box-sum rows); d is read along b, one coalesced row
// segment per subband, and is shared through L2 by the ndm x slices workgroups
// of a candidate.  Each wave then takes trials in
// turn: a lane owns bin `lane` and every 64th bin after it (NB <= 4 of them),
// the loop over subints reads A at the rotated index (the shift is
// wave-uniform and sits in an SGPR, so consecutive lanes read consecutive
// banks), and the box sums come from dyadic doubling S_2w[b] = S_w[b] +
// S_w[(b + w) % nbins] through a per-wave LDS row.  Every lane keeps its own
// running best (value, smallest flat index) per width in registers; the
// per-trial maximum of a width, needed for the P-Pdot plane, is a DPP row
// reduction and four v_readlane.  A workgroup ends with integer atomic
// maxima: the global best packs the value and the inverted flat index into one
// 64-bit key, so every output is independent of the order of evaluation.
// No floating point.
#include <algorithm>
#include <atomic>

#include "device_common.hpp"
#include "psoup/cubeopt.hpp"

namespace psoup {
namespace kern {

namespace {

constexpr int32_t kLowest = INT32_MIN;
static_assert(kOptThreads == 256, "four waves per workgroup");
constexpr int kWaves = kOptThreads / 64;

__device__ __forceinline__ int32_t dpp_max(int32_t v, int32_t o) { return v > o ? v : o; }

// The maximum over the wave, uniform (every lane must be active).
__device__ __forceinline__ int32_t wave_max(int32_t v) {
  v = dpp_max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = dpp_max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = dpp_max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = dpp_max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, false));  // row_mirror
  const int32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const int32_t c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
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

__global__ void opt_init_kernel(unsigned long long* keys, size_t nkeys, int32_t* a, size_t na, int32_t* b, size_t nb,
                                int32_t* c, size_t nc) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < nkeys) keys[i] = 0ull;
  if (i < na) a[i] = kLowest;
  if (i < nb) b[i] = kLowest;
  if (i < nc) c[i] = kLowest;
}

__global__ void opt_decode_kernel(const unsigned long long* keys, size_t nkeys, int32_t* best_val, int32_t* best_idx) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nkeys) return;
  const unsigned long long k = keys[i];
  best_val[i] = static_cast<int32_t>(static_cast<uint32_t>(k >> 32) ^ 0x80000000u);
  best_idx[i] = static_cast<int32_t>(~static_cast<uint32_t>(k));
}

template <int NB>
__global__ __launch_bounds__(kOptThreads) void cube_search_kernel(
    const int32_t* __restrict__ d, const int32_t* __restrict__ sdm, const int32_t* __restrict__ st, int nints,
    int nsub, int nbins, int ndm, int np, int npd, int nw, int trials_per_wg, unsigned long long* keys,
    int32_t* dmcurve, int32_t* ppd, int32_t* centre) {
  extern __shared__ int32_t lds[];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kd = static_cast<int>(blockIdx.y);
  const size_t cand = blockIdx.z;
  const int ntr = np * npd;
  const int plane = nints * nbins;
  int32_t* A = lds;                           // [nints][nbins]
  int32_t* row = lds + plane + wave * nbins;  // this wave's box-sum row

  // ---- stage 1: the dedispersed plane of this DM trial
  {
    const int32_t* dc = d + cand * static_cast<size_t>(plane) * nsub;
    const int32_t* sd = sdm + (cand * ndm + kd) * static_cast<size_t>(nsub);
    for (int e = tid; e < plane; e += kOptThreads) {
      const int i = e / nbins;
      const int b = e - i * nbins;
      const int32_t* di = dc + static_cast<size_t>(i) * nsub * nbins;
      int32_t acc = 0;
      for (int s = 0; s < nsub; ++s) {
        int x = b + sd[s];
        if (x >= nbins) x -= nbins;
        acc += di[s * nbins + x];
      }
      A[e] = acc;
    }
  }
  __syncthreads();

  // ---- stage 2: the trials of this slice, one wave each in turn
  int bsafe[NB];
  bool act[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int b = lane + 64 * j;
    act[j] = b < nbins;
    bsafe[j] = act[j] ? b : 0;
  }
  int32_t bv[kOptMaxWidths], bi[kOptMaxWidths];
#pragma unroll
  for (int k = 0; k < kOptMaxWidths; ++k) {
    bv[k] = kLowest;
    bi[k] = INT32_MAX;
  }
  const int32_t* stc = st + cand * static_cast<size_t>(ntr) * nints;
  int32_t* ppdc = ppd + cand * static_cast<size_t>(nw) * ntr;
  const int t0 = static_cast<int>(blockIdx.x) * trials_per_wg;
  const int t1 = min(ntr, t0 + trials_per_wg);
  const int tcentre = (np / 2) * npd + npd / 2;
  for (int t = t0 + wave; t < t1; t += kWaves) {
    const int32_t* stt = stc + static_cast<size_t>(t) * nints;
    int32_t S[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) S[j] = 0;
    for (int i = 0; i < nints; ++i) {
      const int sh = __builtin_amdgcn_readfirstlane(stt[i]);
      const int32_t* Ai = A + i * nbins;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        int x = bsafe[j] + sh;
        if (x >= nbins) x -= nbins;
        S[j] += Ai[x];
      }
    }
    const int32_t base = (kd * ntr + t) * nbins;
    int32_t mine = kLowest;
#pragma unroll
    for (int k = 0; k < kOptMaxWidths; ++k) {
      if (k < nw) {
        int32_t m = kLowest;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int32_t v = act[j] ? S[j] : kLowest;
          if (v > bv[k]) {  // bins and trials come in ascending flat index: the first maximum stays
            bv[k] = v;
            bi[k] = base + lane + 64 * j;
          }
          m = max(m, v);
        }
        m = wave_max(m);
        if (lane == k) mine = m;
        if (k + 1 < nw) {
          const int w = 1 << k;
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
    if (lane < nw) {
      atomicMax(ppdc + static_cast<size_t>(lane) * ntr + t, mine);
      if (kd == ndm / 2 && t == tcentre) centre[cand * nw + lane] = mine;
    }
  }

  // ---- the wave's bests: value and inverted index in one key
#pragma unroll
  for (int k = 0; k < kOptMaxWidths; ++k) {
    if (k < nw) {
      unsigned long long key = pack_key(bv[k], bi[k]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
      }
      if (lane == 0) {
        atomicMax(keys + cand * nw + k, key);
        atomicMax(dmcurve + (cand * nw + k) * static_cast<size_t>(ndm) + kd,
                  static_cast<int32_t>(static_cast<uint32_t>(key >> 32) ^ 0x80000000u));
      }
    }
  }
}

template <int NB>
void launch_search(const int32_t* d_d, const int32_t* d_sdm, const int32_t* d_st, const OptDims& g, int ncand,
                   unsigned long long* keys, int32_t* d_dmcurve, int32_t* d_ppd, int32_t* d_centre, hipStream_t s) {
  const int ntr = g.np * g.npd;
  const int slices = (ntr + kOptTrialsPerWg - 1) / kOptTrialsPerWg;
  const int per = (ntr + slices - 1) / slices;
  const size_t lds = static_cast<size_t>(g.nints * g.nbins + kWaves * g.nbins) * sizeof(int32_t);
  // above 64 KiB of dynamic LDS the limit has to be raised, once per instance and device
  if (lds > 65536) {
    static std::atomic<uint64_t> raised{0};
    int dev = 0;
    PSOUP_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = uint64_t(1) << (dev & 63);
    if (!(raised.load() & bit)) {
      PSOUP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cube_search_kernel<NB>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (kOptMaxPlane + kWaves * kOptMaxBins) * static_cast<int>(sizeof(int32_t))));
      raised.fetch_or(bit);
    }
  }
  const dim3 grid(static_cast<unsigned>(slices), static_cast<unsigned>(g.ndm), static_cast<unsigned>(ncand));
  cube_search_kernel<NB><<<grid, kOptThreads, lds, s>>>(d_d, d_sdm, d_st, g.nints, g.nsub, g.nbins, g.ndm, g.np, g.npd,
                                                        g.nw, per, keys, d_dmcurve, d_ppd, d_centre);
  post_launch_check("cube_search_kernel", s);
}

}  // namespace

void cube_search(const int32_t* d_d, const int32_t* d_sdm, const int32_t* d_st, const OptDims& g, int ncand,
                 uint64_t* d_keys, int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_dmcurve, int32_t* d_ppd,
                 int32_t* d_centre, hipStream_t s) {
  PSOUP_CHECK(g.nints >= 1 && g.nsub >= 1 && g.nbins >= 2 && g.nbins <= kOptMaxBins &&
                  g.nints * g.nbins <= kOptMaxPlane,
              "cube opt: nbins must be in 2.." << kOptMaxBins << " and nints * nbins at most " << kOptMaxPlane);
  PSOUP_CHECK(g.ndm >= 1 && g.ndm <= 65535 && g.np >= 1 && g.npd >= 1 && g.nw == opt_nwidths(g.nbins) &&
                  g.nw <= kOptMaxWidths,
              "cube opt: bad grid");
  PSOUP_CHECK(static_cast<uint64_t>(g.ndm) * g.np * g.npd * g.nbins < (uint64_t(1) << 31),
              "cube opt: the trial bins do not fit 31 bits");
  PSOUP_CHECK(ncand >= 1 && ncand <= 65535, "cube opt: 1..65535 candidates per launch");
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(d_keys);
  const size_t nkeys = static_cast<size_t>(ncand) * g.nw;
  const size_t ndc = nkeys * g.ndm, npp = nkeys * g.np * g.npd;
  const size_t most = std::max(ndc, npp);
  opt_init_kernel<<<static_cast<unsigned>((most + 255) / 256), 256, 0, s>>>(keys, nkeys, d_dmcurve, ndc, d_ppd, npp,
                                                                            d_centre, nkeys);
  post_launch_check("opt_init_kernel", s);
  const int nb = (g.nbins + 63) / 64;
  if (nb == 1)
    launch_search<1>(d_d, d_sdm, d_st, g, ncand, keys, d_dmcurve, d_ppd, d_centre, s);
  else if (nb == 2)
    launch_search<2>(d_d, d_sdm, d_st, g, ncand, keys, d_dmcurve, d_ppd, d_centre, s);
  else if (nb == 3)
    launch_search<3>(d_d, d_sdm, d_st, g, ncand, keys, d_dmcurve, d_ppd, d_centre, s);
  else
    launch_search<4>(d_d, d_sdm, d_st, g, ncand, keys, d_dmcurve, d_ppd, d_centre, s);
  opt_decode_kernel<<<static_cast<unsigned>((nkeys + 255) / 256), 256, 0, s>>>(keys, nkeys, d_best_val, d_best_idx);
  post_launch_check("opt_decode_kernel", s);
}

}  // namespace kern
}  // namespace psoup
