// Filterbank fold into subint x subband x phase cubes (psoup/foldcube.hpp).
//
// Reference: src/kernels.cu fold_filterbank_kernel (K12), commented out there.
//
// One workgroup folds, for one candidate and one subint, a run of tiles of
// kCubeTile output samples into the subbands of one subband group.  The phase
// bin and the resampled source index depend only on the output sample, so each
// thread evaluates them once per tile (double precision, no FMA contraction)
// for its 8 samples (tid + 256 k: a wave reads consecutive LDS bytes) and
// keeps them in registers for every channel.  Within a tile the source index
// is monotone, so a channel's reads are one window of at most kCubeWindow
// bytes starting at src(first sample) + off[c]: it is staged in LDS with
// aligned 16-byte loads, the next channel's window in flight while the current
// one is summed.  The channels of a subband add per sample into int32
// registers; a finished subband goes into the LDS histogram [subband][bin]
// with integer LDS atomics (one per wave where the wave shares a bin), and the
// histogram leaves with 64-bit integer global atomics.  Integer sums: the
// result does not depend on any order.
#include <algorithm>
#include <cmath>

#include "device_common.hpp"
#include "psoup/foldcube.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kPer = kCubeTile / kThreads;  // samples per thread and tile
static_assert(kCubeWindow == 16 * kThreads, "every thread stages 16 bytes of the window");
static_assert((kCubeWindow & (kCubeWindow - 1)) == 0, "window indices are masked");

// fold_accumulate_kernel's expressions (fold.hip), unfused so that NumPy's
// separate multiplies and adds give the same bits.
__device__ __forceinline__ int64_t cube_src(double af, double h, double nm1, double d) {
#pragma clang fp contract(off)
  double r = rint(d + af * (((d - h) * (d - h)) - (h * h)));
  if (r < 0.0) r = 0.0;
  if (r > nm1) r = nm1;
  return static_cast<int64_t>(r);
}

__device__ __forceinline__ int cube_bin(double tsamp_by_period, int nbins, double d) {
#pragma clang fp contract(off)
  double ip;
  const double fp = modf(d * tsamp_by_period, &ip);
  int b = static_cast<int>(floor(fp * nbins));
  return b < 0 ? 0 : (b >= nbins ? nbins - 1 : b);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, dev::kWave);
  return v;
}

__global__ void __launch_bounds__(kThreads) fold_cube_kernel(
    const int8_t* __restrict__ x, uint64_t stride, int nchans, int bias, int nints, int nsub, int nbins, uint64_t n,
    const int32_t* __restrict__ active, const int32_t* __restrict__ sub_first, const int32_t* __restrict__ offsets,
    const CubeJob* __restrict__ jobs, int sub_per_group, int ngroups, int tiles_per_wg, int tiles_per_subint,
    unsigned long long* __restrict__ sums, int32_t* __restrict__ hits) {
  // hist: int32 [sub_per_group][nbins], then the hit counts [nbins].
  // 32-bit bound: one entry receives at most 255 (the largest raw sample) x
  // kCubeTile x tiles_per_wg samples x the channels of one subband; the
  // launcher checks that this stays below 2^31.
  extern __shared__ int32_t hist[];
  __shared__ __attribute__((aligned(16))) uint32_t win[2][kCubeWindow / 4];
  const int tid = threadIdx.x;
  const int lane = tid & (dev::kWave - 1);
  const int cand = blockIdx.z;
  const int subint = blockIdx.y / ngroups;
  const int group = blockIdx.y % ngroups;
  const int s0 = group * sub_per_group;
  const int s1 = min(nsub, s0 + sub_per_group);
  int32_t* hh = hist + sub_per_group * nbins;
  for (int e = tid; e < sub_per_group * nbins + nbins; e += kThreads) hist[e] = 0;
  const CubeJob J = jobs[cand];
  const int32_t* off = offsets + static_cast<uint64_t>(cand) * nchans;
  const int ia = dev::sload(sub_first, s0), ie = dev::sload(sub_first, s1);
  const uint64_t nps = n / static_cast<uint64_t>(nints);
  const double h = static_cast<double>(n) / 2.0;
  const double nm1 = static_cast<double>(n - 1);
  const bool do_hits = group == 0;
  __syncthreads();

  for (int tt = 0; tt < tiles_per_wg; ++tt) {
    const int tile = static_cast<int>(blockIdx.x) * tiles_per_wg + tt;
    if (tile >= tiles_per_subint) break;  // uniform
    const uint64_t jb = static_cast<uint64_t>(subint) * nps + static_cast<uint64_t>(tile) * kCubeTile;
    const uint64_t je = min(jb + static_cast<uint64_t>(kCubeTile), static_cast<uint64_t>(subint + 1) * nps);
    // monotone source index: the window is [src(jb), src(je - 1)]
    const int64_t src_min = cube_src(J.af, h, nm1, static_cast<double>(jb));
    const int64_t src_max = cube_src(J.af, h, nm1, static_cast<double>(je - 1));
    const int span = static_cast<int>(src_max - src_min) + 1;
    int bin[kPer], rel[kPer];
    unsigned valid = 0, uni = 0;  // bit k: sample k exists / its whole wave shares one bin
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint64_t j = jb + static_cast<uint64_t>(tid + kThreads * k);
      const bool ok = j < je;
      const double d = static_cast<double>(j);
      bin[k] = ok ? cube_bin(J.tsamp_by_period, nbins, d) : 0;
      rel[k] = ok ? static_cast<int>(cube_src(J.af, h, nm1, d) - src_min) : 0;
      valid |= (ok ? 1u : 0u) << k;
      const int b0 = __builtin_amdgcn_readfirstlane(bin[k]);
      if (__ballot(ok && bin[k] == b0) == ~0ull) uni |= 1u << k;
    }
    if (do_hits) {
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        if (uni >> k & 1) {
          if (lane == 0) atomicAdd(&hh[bin[k]], dev::kWave);
        } else if (valid >> k & 1) {
          atomicAdd(&hh[bin[k]], 1);
        }
      }
    }
    if (ia < ie) {
      // 16 bytes of channel active[ci]'s window per thread; nothing is read
      // past the window or past the row
      auto shift_of = [&](int ci) -> int {
        const int c = dev::sload(active, ci);
        return static_cast<int>((src_min + dev::sload(off, c)) & 15);
      };
      auto gload = [&](int ci) -> u32x4 {
        const int c = dev::sload(active, ci);
        const int64_t g0 = src_min + dev::sload(off, c);
        const int64_t pos = (g0 & ~static_cast<int64_t>(15)) + 16 * tid;
        const int need = span + static_cast<int>(g0 & 15);
        u32x4 v = {0u, 0u, 0u, 0u};
        if (16 * tid < need && pos + 16 <= static_cast<int64_t>(stride))
          v = *reinterpret_cast<const u32x4*>(x + static_cast<uint64_t>(c) * stride + pos);
        return v;
      };
      // int32 per-sample sums: at most 255 x the channels of a subband
      int acc[kPer];
#pragma unroll
      for (int k = 0; k < kPer; ++k) acc[k] = 0;
      int s = s0;
      while (dev::sload(sub_first, s + 1) <= ia) ++s;  // empty leading subbands (ia < ie: ends before s1)
      u32x4 r = gload(ia);
      int sh = shift_of(ia);
      for (int ci = ia; ci < ie; ++ci) {
        const int buf = (ci - ia) & 1;
        *reinterpret_cast<u32x4*>(&win[buf][4 * tid]) = r;
        const int shc = sh;
        if (ci + 1 < ie) {
          r = gload(ci + 1);
          sh = shift_of(ci + 1);
        }
        // one barrier per channel: the buffer written next was last read
        // before this barrier
        __syncthreads();
        const int8_t* wb = reinterpret_cast<const int8_t*>(win[buf]);
#pragma unroll
        for (int k = 0; k < kPer; ++k) acc[k] += wb[(rel[k] + shc) & (kCubeWindow - 1)];
        if (ci + 1 == dev::sload(sub_first, s + 1)) {  // uniform: subband s is complete
          const int add = bias * (ci + 1 - dev::sload(sub_first, s));
          int32_t* hrow = hist + (s - s0) * nbins;
#pragma unroll
          for (int k = 0; k < kPer; ++k) {
            if (uni >> k & 1) {
              const int v = wave_sum_i32(acc[k] + add);
              if (lane == 0) atomicAdd(&hrow[bin[k]], v);
            } else if (valid >> k & 1) {
              atomicAdd(&hrow[bin[k]], acc[k] + add);
            }
            acc[k] = 0;
          }
          ++s;
          while (s < s1 && dev::sload(sub_first, s + 1) <= ci + 1) ++s;  // empty subbands
        }
      }
    }
    __syncthreads();  // the next tile's first window reuses buffer 0
  }

  const uint64_t ci0 = static_cast<uint64_t>(cand) * nints + subint;
  const int nh = (s1 - s0) * nbins;
  unsigned long long* out = sums + (ci0 * nsub + s0) * static_cast<uint64_t>(nbins);
  for (int e = tid; e < nh; e += kThreads) {
    const int32_t v = hist[e];
    if (v) atomicAdd(&out[e], static_cast<unsigned long long>(v));
  }
  if (do_hits)
    for (int b = tid; b < nbins; b += kThreads)
      if (hh[b]) atomicAdd(&hits[ci0 * nbins + b], hh[b]);
}

}  // namespace

CubePlan cube_plan(const CubeGeom& g, int ncand, int max_sub_channels) {
  PSOUP_CHECK(g.nints >= 1 && g.nints <= 256, "fold cube: nints must be in 1..256");
  PSOUP_CHECK(g.nbins >= 2 && g.nbins <= 256, "fold cube: nbins must be in 2..256");
  PSOUP_CHECK(g.nsub >= 1 && g.nsub <= g.nchans, "fold cube: nsub must be in 1..nchans");
  PSOUP_CHECK(g.n >= static_cast<uint64_t>(g.nints) && g.n < (uint64_t(1) << 31),
              "fold cube: fold length must be in [nints, 2^31)");
  PSOUP_CHECK(ncand >= 1 && ncand <= 65535, "fold cube: 1..65535 candidates per launch");
  CubePlan p;
  const uint64_t nps = g.n / static_cast<uint64_t>(g.nints);
  const uint64_t tps = (nps + kCubeTile - 1) / kCubeTile;
  const int spg_max = std::max(1, kCubeHistMax / g.nbins);
  const int groups_min = (g.nsub + spg_max - 1) / spg_max;
  // enough workgroups to fill the device: split the subbands further when
  // candidates x subints x tiles are few (each group re-evaluates the bins)
  const uint64_t base = static_cast<uint64_t>(ncand) * g.nints * tps;
  const uint64_t want = (2048 + base - 1) / base;
  int groups = static_cast<int>(std::min<uint64_t>(std::max<uint64_t>(want, groups_min), g.nsub));
  p.sub_per_group = (g.nsub + groups - 1) / groups;
  p.ngroups = (g.nsub + p.sub_per_group - 1) / p.sub_per_group;
  // 32-bit LDS histogram: 255 x kCubeTile x tiles_per_wg x channels of a subband < 2^31
  const uint64_t per_tile = 255ull * kCubeTile * static_cast<uint64_t>(std::max(1, max_sub_channels));
  const uint64_t bound = ((uint64_t(1) << 31) - 1) / per_tile;
  PSOUP_CHECK(bound >= 1, "fold cube: " << max_sub_channels
                                        << " channels in one subband overflow the 32-bit partial sums; raise nsub");
  const uint64_t fill = base * p.ngroups / 8192;
  p.tiles_per_wg = static_cast<int>(std::max<uint64_t>(1, std::min({fill, bound, tps, uint64_t(64)})));
  PSOUP_CHECK(per_tile * static_cast<uint64_t>(p.tiles_per_wg) < (uint64_t(1) << 31),
              "fold cube: 32-bit partial sums would overflow");
  p.wgs_per_subint = static_cast<int>((tps + p.tiles_per_wg - 1) / p.tiles_per_wg);
  PSOUP_CHECK(static_cast<uint64_t>(g.nints) * p.ngroups <= 65535, "fold cube: too many subint x subband groups");
  return p;
}

void fold_cube(const int8_t* chan_major, const CubeGeom& g, const int32_t* d_active, const int32_t* d_sub_first,
               const int32_t* d_offsets, const CubeJob* d_jobs, int ncand, const CubePlan& plan, int64_t* d_sums,
               int32_t* d_hits, hipStream_t s) {
  PSOUP_CHECK((g.stride & 15) == 0 && (reinterpret_cast<uintptr_t>(chan_major) & 15) == 0,
              "fold cube: rows must be 16-byte aligned");
  PSOUP_CHECK(plan.sub_per_group >= 1 && plan.sub_per_group * g.nbins <= kCubeHistMax && plan.ngroups >= 1 &&
                  plan.tiles_per_wg >= 1 && plan.wgs_per_subint >= 1 &&
                  static_cast<uint64_t>(plan.sub_per_group) * plan.ngroups >= static_cast<uint64_t>(g.nsub),
              "fold cube: bad launch plan");
  const uint64_t nps = g.n / static_cast<uint64_t>(g.nints);
  const int tps = static_cast<int>((nps + kCubeTile - 1) / kCubeTile);
  const dim3 grid(static_cast<unsigned>(plan.wgs_per_subint), static_cast<unsigned>(g.nints * plan.ngroups),
                  static_cast<unsigned>(ncand));
  const size_t lds = static_cast<size_t>(plan.sub_per_group * g.nbins + g.nbins) * sizeof(int32_t);
  fold_cube_kernel<<<grid, kThreads, lds, s>>>(chan_major, g.stride, g.nchans, g.bias, g.nints, g.nsub, g.nbins, g.n,
                                               d_active, d_sub_first, d_offsets, d_jobs, plan.sub_per_group,
                                               plan.ngroups, plan.tiles_per_wg, tps,
                                               reinterpret_cast<unsigned long long*>(d_sums), d_hits);
  post_launch_check("fold_cube_kernel", s);
}

}  // namespace kern
}  // namespace psoup
