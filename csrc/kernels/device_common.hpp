// Shared device helpers for the gfx950 kernels (64-lane wavefronts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "psoup/common.hpp"
#include "psoup/kernels.hpp"

namespace psoup {
namespace kern {
namespace dev {

constexpr int kWave = 64;

// Workgroup-uniform read of read-only global memory through the constant
// address space: a scalar load into SGPRs (s_load, lgkmcnt) that no earlier
// store in the kernel can turn into a vector load and no vector-memory wait
// orders behind the streaming loads.  The memory must not be written while
// the kernel runs; idx must be uniform.
template <class T>
__device__ __forceinline__ T sload(const T* p, uint64_t idx) {
  static_assert(std::is_arithmetic<T>::value, "sload: scalar types (float2: sload2)");
#if __HIP_DEVICE_COMPILE__
  typedef const __attribute__((address_space(4))) T* cptr;
  return reinterpret_cast<cptr>(reinterpret_cast<uintptr_t>(p))[idx];
#else
  return p[idx];  // (the host pass of a device function: never run)
#endif
}
__device__ __forceinline__ float2 sload2(const float2* p, uint64_t idx) {
  const float* f = reinterpret_cast<const float*>(p);
  return make_float2(sload(f, 2 * idx), sload(f, 2 * idx + 1));
}

// Memory-bound launches: enough blocks to fill 256 CUs x 8, grid-stride the rest.
inline unsigned grid_for(uint64_t work_items, unsigned block, unsigned cap = 2048) {
  uint64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return static_cast<unsigned>(g);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// An 8-bit row's mean as the whitener pads with it, and the integer offset its centred sources take off every
// value before the transform (kernels.hpp f32_centre): one definition, so that every source and the kernel that
// adds n * offset back to X_0 agree bit for bit.
__device__ __forceinline__ float u8_mean(unsigned long long sum, uint64_t nvalid) {
  return nvalid ? static_cast<float>(static_cast<double>(sum) / static_cast<double>(nvalid)) : 0.f;
}
__device__ __forceinline__ float u8_centre(unsigned long long sum, uint64_t nvalid) {
  return rintf(u8_mean(sum, nvalid));
}

// Block-wide sum; `scratch` must hold blockDim.x/64 elements. Result valid
// in every thread.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int nw = (blockDim.x + kWave - 1) / kWave;
  v = wave_sum(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  T r = T(0);
  for (int i = 0; i < nw; ++i) r += scratch[i];
  __syncthreads();
  return r;
}

// Exact median of five (any correct network gives the identical value).
__device__ __forceinline__ float median5(float a, float b, float c, float d, float e) {
  float t;
#define PS_SORT2(x, y) \
  t = fminf(x, y);     \
  y = fmaxf(x, y);     \
  x = t;
  PS_SORT2(a, b);
  PS_SORT2(d, e);
  PS_SORT2(a, d);  // a = min of 4 (excluded)
  PS_SORT2(b, e);  // e = max of 4 (excluded)
  // median of {b, c, d}
  PS_SORT2(b, c);
  PS_SORT2(c, d);
  PS_SORT2(b, c);
#undef PS_SORT2
  return c;
}

__device__ __forceinline__ float median3(float a, float b, float c) {
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}

__device__ __forceinline__ float median4(float a, float b, float c, float d) {
  // mean of the two middle values
  float lo1 = fminf(a, b), hi1 = fmaxf(a, b);
  float lo2 = fminf(c, d), hi2 = fmaxf(c, d);
  float mid_lo = fmaxf(lo1, lo2);
  float mid_hi = fminf(hi1, hi2);
  return 0.5f * (mid_lo + mid_hi);
}

// cuCdivf as in CUDA's cuComplex.h (scaled division) for a real divisor,
// so dereddening reproduces the reference's rounding.
__device__ __forceinline__ float2 cdiv_real(float2 x, float f) {
  float s = fabsf(f);
  float oos = 1.0f / s;
  float ars = x.x * oos;
  float ais = x.y * oos;
  float brs = f * oos;
  float s2 = brs * brs;
  float oos2 = 1.0f / s2;
  return make_float2((ars * brs) * oos2, (ais * brs) * oos2);
}

// Amplitude |X| exactly as power_series_kernel (z * rsqrt(z)), 0 for z == 0.
__device__ __forceinline__ float amplitude(float2 x) {
  float z = x.x * x.x + x.y * x.y;
  return z > 0.f ? z * rsqrtf(z) : 0.f;
}

// Interbinned amplitude, bin_interbin_series_kernel semantics.
// The fused multiply-adds are explicit so every kernel that forms it (LDS or
// register neighbours) rounds identically whatever the compiler contracts.
__device__ __forceinline__ float interbin(float2 x, float2 xl) {
  float ampsq = __builtin_fmaf(x.x, x.x, x.y * x.y);
  float dre = x.x - xl.x, dim = x.y - xl.y;
  // 0.5 * (double) then rounding to float == the float product by 0.5f:
  // scaling by a power of two is exact (denormals are kept in both)
  float ampsq_diff = __builtin_fmaf(dre, dre, dim * dim) * 0.5f;
  return sqrtf(fmaxf(ampsq, ampsq_diff));
}

// a / b with IEEE round-to-nearest from rb = 1.0f / b (itself correctly
// rounded): the reciprocal product q = a rb is within an ulp, the residual
// a - q b is exact in an FMA, and one correction step q + r rb rounds to
// RN(a / b) (Markstein's theorem; checked on 8e8 random pairs, including
// all-ones divisor mantissas).  The spectrum normalisation thus equals the
// reference's division (src/kernels.cu:477-478) at the cost of two FMAs, not
// a full division, per bin.
__device__ __forceinline__ float div_rn(float a, float b, float rb) {
  const float q = a * rb;
  const float r = __builtin_fmaf(-q, b, a);
  return __builtin_fmaf(r, rb, q);
}

// resampleII read index (kernels.cu:338-379) in double precision, clamped
// to [0, nmax].  Shared by the resampler and the fused four-step FFT so both
// paths pick bit-identical samples.
__device__ __forceinline__ double accel_pos_ii(double af, double size, double d) { return d + d * af * (d - size); }

__device__ __forceinline__ uint64_t accel_index_ii(double af, double size, uint64_t id, uint64_t nmax) {
  const double r = accel_pos_ii(af, size, static_cast<double>(id));
  double rr = rint(r);
  if (rr < 0.0) rr = 0.0;
  const uint64_t j = static_cast<uint64_t>(rr);
  return j > nmax ? nmax : j;
}

// 32-bit form of accel_index_ii for series shorter than 2^31 samples (one
// conversion each way instead of the emulated 64-bit ones); same value.
__device__ __forceinline__ uint32_t accel_index_ii32(double af, double size, uint32_t id, uint32_t nmax) {
  const double r = accel_pos_ii(af, size, static_cast<double>(id));
  const double rr = fmin(fmax(rint(r), 0.0), static_cast<double>(nmax));
  return static_cast<uint32_t>(rr);
}

// Real-input FFT bin from the half-length complex FFT Z of the packed series:
//   X[k] = (Z[k] + conj Z[M-k])/2 - i/2 e^{-i pi k/M} (Z[k] - conj Z[M-k]),
// za = Z[k], zb = Z[M-k], (c, s) = (cos, sin) of -pi k / M; X[M-k] is
// r2c_combine(zb, za, -c, s).  Explicit FMAs: identical rounding in every
// kernel that forms it.
__device__ __forceinline__ float2 r2c_combine(float2 za, float2 zb, float c, float s) {
  const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
  const float dx = 0.5f * (za.x - zb.x), dy = 0.5f * (za.y + zb.y);
  const float ox = dy, oy = -dx;  // -i * d
  return make_float2(__builtin_fmaf(-s, oy, __builtin_fmaf(c, ox, ex)), __builtin_fmaf(s, ox, __builtin_fmaf(c, oy, ey)));
}

// e^{-i pi k / M} for 0 <= k <= M/2 from the two-level table of
// r2c_twiddle_table (harmsum.hip): rt[k & 2047] * rt[2048 + (k >> 11)], the
// product with explicit FMAs, so every kernel that forms a spectrum bin gets
// the same twiddle (the search's r2c and the screened harmonic sum's exact
// path recompute bins independently and must agree to the bit).
__device__ __forceinline__ float2 r2c_tw(const float2* __restrict__ rt, uint32_t k) {
  const float2 l = rt[k & 2047u], h = rt[2048u + (k >> 11)];
  return make_float2(__builtin_fmaf(h.x, l.x, -(h.y * l.y)), __builtin_fmaf(h.x, l.y, h.y * l.x));
}

// Screening byte of a normalised spectrum value for the harmonic sum's
// integer pre-screen (harmsum.hip): with v = rint(4 p) + 128, bytes 0..253
// hold v - 1 for v in [1, 254] (|p - (byte - 127) / 4| <= 1/8), 254 marks
// v >= 255 (or NaN) and 255 marks v <= 0.  The screen sends any bin whose
// terms include a byte >= 254 to the exact path, so every screened term is
// within 1/8 of its bin and below 32 in magnitude.
__device__ __forceinline__ uint8_t q8(float p) {
  const float v = rintf(p * 4.0f) + 128.0f;
  if (!(v < 255.0f)) return 254;  // also NaN
  return v <= 0.0f ? 255 : static_cast<uint8_t>(v - 1.0f);
}

}  // namespace dev

// Per-TU no-op kernel registered for psoup::warm_device (common.hpp): its
// launch makes HIP load this translation unit's code object.
namespace {
__global__ void tu_warm_kernel() {}
void tu_warm(hipStream_t s) { tu_warm_kernel<<<1, 1, 0, s>>>(); }
[[maybe_unused]] const bool tu_warm_registered = register_warmup(&tu_warm);
}  // namespace

}  // namespace kern
}  // namespace psoup
