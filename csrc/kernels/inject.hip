// filinject kernel (psoup/inject.hpp): adds the expected value of dispersed
// pulsars and bursts to the channel-major byte rows in Q31 fixed point and
// rounds it into the samples with a counter-based dither.  Compiled without
// FMA contraction: the phase of a sample is the definition's chain of
// correctly rounded double operations.
//
// One workgroup per (channel, tile of 4096 samples); lanes run along time and
// a lane owns 16 adjacent samples: one aligned 16-byte load and at most one
// 16-byte store.  A channel's per-signal constants are workgroup-uniform and
// come through scalar loads (dev::sload).  Before any data load the workgroup
// decides which signals can touch its tile: a signal with A_q = 0 in this
// channel (a killed or dead channel has none other) never does, a burst only
// within its six-sigma window, widened by a sample against rounding.  A tile
// that no signal touches returns without a load or a store; the profile table
// is staged in LDS only by the tiles that go on.  A lane whose 16 samples all
// have E = 0 does not store.  Lanes past the end of the row and the lane that
// holds the row's tail (count % 16 != 0) take a bounds-checked path of byte
// loads and stores.  nclip and touched are summed in LDS and leave the
// workgroup as one vector atomic add each, when they are not zero.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/inject.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLane = kInjectLane;
constexpr double kReach = 6.0 * kInjectSteps + 0.5;  // u below this reaches T

union Bytes16 {
  u32x4 v;
  int8_t b[kLane];
};

// E of the n (FULL: 16) samples from absolute index tabs on, over the signals
// of `mask`; counts each signal's touched samples into s_touch when asked to.
template <bool FULL>
__device__ __forceinline__ void expected(uint64_t (&E)[kLane], int n, uint64_t tabs, uint64_t mask, int c, int nchans,
                                         const double* sigc, double tsamp, const double* delay, const double* inv_w,
                                         const uint32_t* A_q, const uint16_t* sT, unsigned int* s_touch, bool count) {
#pragma unroll
  for (int j = 0; j < kLane; ++j) E[j] = 0;
  while (mask) {
    const int s = __builtin_ctzll(mask);
    mask &= mask - 1;
    const uint64_t i = static_cast<uint64_t>(s) * static_cast<uint64_t>(nchans) + static_cast<uint64_t>(c);
    const uint32_t a = dev::sload(A_q, i);
    const double dl = dev::sload(delay, i);
    const double iw = dev::sload(inv_w, i);
    const double* k = sigc + static_cast<uint64_t>(s) * kInjectSigDoubles;
    const bool burst = dev::sload(k, 0) != 0.0;
    const double k1 = dev::sload(k, 1), k2 = dev::sload(k, 2), k3 = dev::sload(k, 3);
    unsigned int hit = 0;
#pragma unroll
    for (int j = 0; j < kLane; ++j) {
      if (FULL || j < n) {
        const double x = static_cast<double>(tabs + static_cast<uint64_t>(j)) - dl;
        double d;
        if (burst) {
          d = fabs(x - k1);
        } else {
          const double te = x * tsamp;
          double ph = (te - (k1 * te) * te) * k2 + k3;
          ph = ph - floor(ph);
          d = fmin(ph, 1.0 - ph);
        }
        const double u = d * iw;
        if (u < kReach) {
          const int kk = static_cast<int>(rint(u));
          E[j] += static_cast<uint64_t>(a) * static_cast<uint64_t>(sT[kk]);
          ++hit;
        }
      }
    }
    if (count && hit) atomicAdd(&s_touch[s], hit);
  }
}

// in + add for one sample, clipped; in is the raw value.
__device__ __forceinline__ int dithered(int in, uint64_t E, uint64_t seed_mul, uint64_t ckey, uint64_t t, int vmax,
                                        unsigned int& nclip) {
  if (E == 0) return in;
  const uint64_t z = inject_mix(seed_mul + (ckey | t));
  const uint64_t sum = static_cast<uint64_t>(in) + ((E + (z >> 33)) >> 31);
  if (sum > static_cast<uint64_t>(vmax)) {
    ++nclip;
    return vmax;
  }
  return static_cast<int>(sum);
}

__global__ __launch_bounds__(kInjectThreads) void inject_kernel(
    int8_t* __restrict__ rows, uint64_t stride, uint64_t count, int nchans, int vmax, int bias, uint64_t t0, int nsig,
    const double* __restrict__ sigc, double tsamp, const double* __restrict__ delay, const double* __restrict__ inv_w,
    const uint32_t* __restrict__ A_q, const uint16_t* __restrict__ T, uint64_t seed_mul,
    unsigned long long* __restrict__ nclip, unsigned long long* __restrict__ touched) {
  __shared__ uint16_t sT[kInjectTableLen + 1];
  __shared__ unsigned int s_touch[kInjectMaxSignals];
  __shared__ unsigned int s_clip;
  const int c = static_cast<int>(blockIdx.y);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kInjectTile;  // < count by the grid
  const uint64_t tile_n = min(static_cast<uint64_t>(kInjectTile), count - tile0);
  // which signals can touch this tile (uniform)
  const double ta = static_cast<double>(t0 + tile0), tb = static_cast<double>(t0 + tile0 + tile_n - 1);
  uint64_t mask = 0;
  for (int s = 0; s < nsig; ++s) {
    const uint64_t i = static_cast<uint64_t>(s) * static_cast<uint64_t>(nchans) + static_cast<uint64_t>(c);
    if (dev::sload(A_q, i) == 0u) continue;
    const double* k = sigc + static_cast<uint64_t>(s) * kInjectSigDoubles;
    if (dev::sload(k, 0) != 0.0) {
      const double centre = dev::sload(delay, i) + dev::sload(k, 1);
      const double half = kReach / dev::sload(inv_w, i) + 1.0;
      if (tb < centre - half || ta > centre + half) continue;
    }
    mask |= 1ull << s;
  }
  if (mask == 0) return;

  const int tid = static_cast<int>(threadIdx.x);
  for (int k = tid; k < kInjectTableLen; k += kInjectThreads) sT[k] = T[k];
  if (tid < kInjectMaxSignals) s_touch[tid] = 0;
  if (tid == 0) s_clip = 0;
  __syncthreads();

  const uint64_t i0 = tile0 + static_cast<uint64_t>(tid) * kLane;  // in the chunk
  int8_t* p = rows + static_cast<uint64_t>(c) * stride + i0;
  const uint64_t tabs = t0 + i0;
  const uint64_t ckey = static_cast<uint64_t>(c) << 40;
  const bool count_touch = touched != nullptr;
  unsigned int clipped = 0;
  uint64_t E[kLane];
  if (i0 + kLane <= count) {
    expected<true>(E, kLane, tabs, mask, c, nchans, sigc, tsamp, delay, inv_w, A_q, sT, s_touch, count_touch);
    uint64_t any = 0;
#pragma unroll
    for (int j = 0; j < kLane; ++j) any |= E[j];
    if (any) {
      Bytes16 x;
      x.v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
      for (int j = 0; j < kLane; ++j) {
        const int in = static_cast<int>(x.b[j]) + bias;
        x.b[j] = static_cast<int8_t>(dithered(in, E[j], seed_mul, ckey, tabs + j, vmax, clipped) - bias);
      }
      *reinterpret_cast<u32x4*>(p) = x.v;
    }
  } else if (i0 < count) {
    const int n = static_cast<int>(count - i0);  // 1..15: the row's tail
    expected<false>(E, n, tabs, mask, c, nchans, sigc, tsamp, delay, inv_w, A_q, sT, s_touch, count_touch);
#pragma unroll
    for (int j = 0; j < kLane; ++j) {
      if (j < n && E[j] != 0) {
        const int in = static_cast<int>(p[j]) + bias;
        p[j] = static_cast<int8_t>(dithered(in, E[j], seed_mul, ckey, tabs + j, vmax, clipped) - bias);
      }
    }
  }
  if (clipped) atomicAdd(&s_clip, clipped);
  __syncthreads();
  if (tid == 0 && s_clip) atomicAdd(nclip, static_cast<unsigned long long>(s_clip));
  if (count_touch && tid < nsig && s_touch[tid])
    atomicAdd(touched + tid, static_cast<unsigned long long>(s_touch[tid]));
}

}  // namespace

void inject(int8_t* rows, uint64_t stride, uint64_t count, int nchans, int nbits, int bias, uint64_t t0, int nsig,
            const double* sigc, double tsamp, const double* delay, const double* inv_w, const uint32_t* A_q,
            const uint16_t* T, uint64_t seed_mul, unsigned long long* nclip, unsigned long long* touched,
            hipStream_t s) {
  PSOUP_CHECK(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8, "inject: nbits must be 1/2/4/8");
  PSOUP_CHECK(nchans >= 1 && nchans <= 65535, "inject: 1..65535 channels");
  PSOUP_CHECK(nsig >= 1 && nsig <= kInjectMaxSignals, "inject: 1.." << kInjectMaxSignals << " signals");
  PSOUP_CHECK(bias >= 0 && bias <= 128, "inject: bias");
  PSOUP_CHECK(rows != nullptr && reinterpret_cast<uintptr_t>(rows) % 16 == 0 && stride % 16 == 0 && stride >= count,
              "inject: rows must be 16-byte aligned with a stride that is a multiple of 16 and >= count");
  PSOUP_CHECK(t0 < (1ull << 40) && count <= (1ull << 40) - t0, "inject: sample index beyond 2^40");
  PSOUP_CHECK(sigc && delay && inv_w && A_q && T && nclip, "inject: missing table");
  if (count == 0) return;
  const uint64_t tiles = (count + kInjectTile - 1) / kInjectTile;
  PSOUP_CHECK(tiles < (1ull << 31), "inject: too many samples in one launch");
  dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(nchans));
  inject_kernel<<<grid, kInjectThreads, 0, s>>>(rows, stride, count, nchans, (1 << nbits) - 1, bias, t0, nsig, sigc,
                                                tsamp, delay, inv_w, A_q, T, seed_mul, nclip, touched);
  post_launch_check("inject_kernel", s);
}

}  // namespace kern
}  // namespace psoup
