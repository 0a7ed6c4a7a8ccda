// fildigi kernels (psoup/digi.hpp): the exact block statistics of a time-major
// filterbank of 8-bit, 16-bit or float samples, and its requantisation to 8
// bits.  Compiled without FMA contraction: the requantisation is two correctly
// rounded double operations and a round half to even, as the definition says.
//
// digi_block_sums: one workgroup per (tile of 64 adjacent channels, statistics
// block).  Lanes run along the channels, so a wave's load is contiguous in the
// file's order; a thread owns V adjacent channels (V = 16 / sizeof(sample)
// with 16-byte loads when the rows are 16-byte aligned, else V = 1) and the
// 256 threads walk the block's samples 256 V / 64 rows at a time.  Float input
// makes two sweeps: the first finds the per-channel maximum of the sign-cleared
// bit patterns of the finite samples and reduces it through LDS, the second
// re-reads the tile, scales by the exact power of two and forms N, S1, S2 in
// 64-bit lane partials.  The partials are added through LDS (integer addition:
// the order does not matter) and each cell gets one plain store.
//
// digi_quant: one thread per G adjacent output bytes of the time-major output
// (G = V with one 16-byte load when the rows allow it, else 4 bytes gathered
// with scalar loads); it reads {mean, gain} of the sample's interval from the
// table, reverses the channel order in registers when the band is flipped and
// stores whole dwords.  nclip takes one atomic add per workgroup.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/digi.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = kDigiThreads;
constexpr int L = kDigiStatBlock;

template <class T>
struct Vec16 {
  static constexpr int n = 16 / static_cast<int>(sizeof(T));
  union {
    u32x4 v;
    T e[n];
  };
};

// V adjacent samples at p (16-byte aligned when V > 1).
template <class T, int V>
__device__ __forceinline__ void load_group(const T* p, T (&out)[V]) {
  if constexpr (V == 1) {
    out[0] = *p;
  } else {
    static_assert(V == Vec16<T>::n, "a group is one 16-byte load");
    Vec16<T> u;
    u.v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < V; ++i) out[i] = u.e[i];
  }
}

__device__ __forceinline__ bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// double(x) without a floating-point instruction touching a subnormal float
// (whatever the kernel's denormal mode): a subnormal is mant x 2^-149.
__device__ __forceinline__ double exact_double(float x) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7f800000u) != 0u) return static_cast<double>(x);
  const double m = static_cast<double>(static_cast<int>(b & 0x007fffffu)) * 0x1p-149;
  return (b >> 31) ? -m : m;
}
template <class T>
__device__ __forceinline__ double sample_double(T v) {
  if constexpr (std::is_same<T, float>::value)
    return exact_double(v);
  else
    return static_cast<double>(v);
}

// E of the definition from the largest sign-cleared bit pattern (0: E = 0).
__device__ __forceinline__ int quantum_exp(uint32_t amax) {
  if (amax == 0u) return 0;
  const int e = static_cast<int>(amax >> 23);
  return (e < 1 ? 1 : e) - 127 - 22;
}

// 2^-E as a double, E in [-148, 105].
__device__ __forceinline__ double pow2_neg(int E) {
  return __longlong_as_double(static_cast<long long>(1023 - E) << 52);
}

template <class T, int V>
__global__ void __launch_bounds__(kThreads)
    digi_block_sums_kernel(const T* __restrict__ x, uint64_t count, int nchans, uint64_t b0, uint32_t* __restrict__ N,
                           int64_t* __restrict__ S1, uint64_t* __restrict__ S2, int32_t* __restrict__ E,
                           uint64_t nblk) {
  constexpr bool kFloat = std::is_same<T, float>::value;
  constexpr int kLanes = kDigiTile / V;     // threads along the channels
  constexpr int kRows = kThreads / kLanes;  // rows per step
  __shared__ unsigned long long red[kRows][kDigiTile];
  __shared__ uint32_t s_amax[kDigiTile];
  const int tid = threadIdx.x;
  const int cg = tid % kLanes;
  const int r = tid / kLanes;
  const int c0 = blockIdx.x * kDigiTile + cg * V;  // this thread's first channel
  const bool on = c0 < nchans;                     // V divides nchans: the group is whole
  const uint64_t ts = static_cast<uint64_t>(blockIdx.y) * L;
  const int len = static_cast<int>(min(static_cast<uint64_t>(L), count - ts));
  const T* base = x + ts * static_cast<uint64_t>(nchans) + (on ? c0 : 0);

  double scale[V];  // 2^-E per channel
#pragma unroll
  for (int i = 0; i < V; ++i) scale[i] = 1.0;
  if constexpr (kFloat) {
    uint32_t am[V];
#pragma unroll
    for (int i = 0; i < V; ++i) am[i] = 0u;
    if (on) {
#pragma unroll 4
      for (int t = r; t < len; t += kRows) {
        T g[V];
        load_group<T, V>(base + static_cast<uint64_t>(t) * nchans, g);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const uint32_t b = __float_as_uint(g[i]) & 0x7fffffffu;
          if (finite_bits(b)) am[i] = max(am[i], b);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) red[r][cg * V + i] = am[i];
    __syncthreads();
    if (tid < kDigiTile) {
      uint32_t m = 0u;
      for (int k = 0; k < kRows; ++k) m = max(m, static_cast<uint32_t>(red[k][tid]));
      s_amax[tid] = m;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) scale[i] = pow2_neg(quantum_exp(s_amax[cg * V + i]));
  }

  uint32_t n[V];
  long long s1[V];
  unsigned long long s2[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    n[i] = 0u;
    s1[i] = 0;
    s2[i] = 0ull;
  }
  if (on) {
#pragma unroll 4
    for (int t = r; t < len; t += kRows) {
      T g[V];
      load_group<T, V>(base + static_cast<uint64_t>(t) * nchans, g);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if constexpr (kFloat) {
          if (finite_bits(__float_as_uint(g[i]))) {
            const long long q = __double2int_rn(exact_double(g[i]) * scale[i]);  // exact product
            n[i] += 1u;
            s1[i] += q;
            s2[i] += static_cast<unsigned long long>(q * q);
          }
        } else {
          const long long q = static_cast<long long>(g[i]);
          n[i] += 1u;
          s1[i] += q;
          s2[i] += static_cast<unsigned long long>(q * q);
        }
      }
    }
  }

  // the rows' partials through LDS, one quantity at a time; thread c < 64
  // stores the cell of channel c of the tile
  const int c = blockIdx.x * kDigiTile + tid;
  const bool store = tid < kDigiTile && c < nchans;
  const uint64_t cell = static_cast<uint64_t>(store ? c : 0) * nblk + b0 + blockIdx.y;
  auto reduce = [&](auto&& get) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) red[r][cg * V + i] = get(i);
    __syncthreads();
    unsigned long long a = 0ull;
    if (tid < kDigiTile)
      for (int k = 0; k < kRows; ++k) a += red[k][tid];
    return a;
  };
  const unsigned long long tn = reduce([&](int i) { return static_cast<unsigned long long>(n[i]); });
  const unsigned long long t1 = reduce([&](int i) { return static_cast<unsigned long long>(s1[i]); });  // mod 2^64
  const unsigned long long t2 = reduce([&](int i) { return s2[i]; });
  if (store) {
    N[cell] = static_cast<uint32_t>(tn);
    S1[cell] = static_cast<int64_t>(t1);
    S2[cell] = t2;
    int e = 0;
    if constexpr (kFloat) e = quantum_exp(s_amax[tid]);
    E[cell] = e;
  }
}

// ----------------------------------------------------------------- quant ----
// VEC: V = 16 / sizeof(T) divides nchans and the rows are 16-byte aligned: a
// group is V adjacent channels of one sample.  Otherwise a group is 4 adjacent
// bytes of the flat output, which may cross a sample's end.
template <class T, bool VEC>
__global__ void __launch_bounds__(kThreads)
    digi_quant_kernel(const T* __restrict__ x, uint64_t total, int nchans, uint64_t t0, int J,
                      const double2* __restrict__ tab, int flip, uint8_t* __restrict__ y, uint64_t ngroups,
                      unsigned long long* __restrict__ nclip) {
  constexpr bool kFloat = std::is_same<T, float>::value;
  constexpr int G = VEC ? Vec16<T>::n : 4;
  __shared__ unsigned long long red[kThreads / dev::kWave];
  unsigned long long clipped = 0ull;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < ngroups; g += stride) {
    const uint64_t i0 = g * G;  // first output byte of the group
    uint64_t t = i0 / static_cast<uint64_t>(nchans);
    int co = static_cast<int>(i0 - t * static_cast<uint64_t>(nchans));  // output channel
    T v[G];
    if constexpr (VEC) {
      // the V input channels of the group, ascending: [ci, ci + G)
      const int ci = flip ? nchans - G - co : co;
      T in[G];
      load_group<T, G>(x + t * static_cast<uint64_t>(nchans) + ci, in);
#pragma unroll
      for (int k = 0; k < G; ++k) v[k] = flip ? in[G - 1 - k] : in[k];
    }
    uint32_t w[G / 4];
#pragma unroll
    for (int k = 0; k < G / 4; ++k) w[k] = 0u;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      int yq = 0;  // the padding past the last sample
      if (VEC || i0 + k < total) {
        const int ci = flip ? nchans - 1 - co : co;
        if constexpr (!VEC) v[k] = x[t * static_cast<uint64_t>(nchans) + ci];
        const uint64_t blk = (t0 + t) / L;
        const uint64_t j = J > 0 ? blk / static_cast<uint64_t>(J) : 0;
        const double2 mg = tab[j * static_cast<uint64_t>(nchans) + ci];
        bool good = mg.y != 0.0;
        if constexpr (kFloat) good = good && finite_bits(__float_as_uint(v[k]));
        yq = 128;
        if (good) {
          const double d = sample_double(v[k]) - mg.x;
          const double p = d * mg.y;
          const double q = rint(p) + 128.0;
          if (q < 0.0) {
            yq = 0;
            ++clipped;
          } else if (q > 255.0) {
            yq = 255;
            ++clipped;
          } else {
            yq = static_cast<int>(q);
          }
        }
        if (++co == nchans) {
          co = 0;
          ++t;
        }
      }
      w[k >> 2] |= static_cast<uint32_t>(yq) << (8 * (k & 3));
    }
    if constexpr (G == 16) {
      *reinterpret_cast<u32x4*>(y + i0) = u32x4{w[0], w[1], w[2], w[3]};
    } else if constexpr (G == 8) {
      *reinterpret_cast<uint2*>(y + i0) = make_uint2(w[0], w[1]);
    } else {
      *reinterpret_cast<uint32_t*>(y + i0) = w[0];
    }
  }
  clipped = dev::block_sum(clipped, red);
  if (threadIdx.x == 0 && clipped != 0ull) atomicAdd(nclip, clipped);
}

template <class T>
void launch_sums(const void* x, uint64_t count, int nchans, uint64_t b0, uint32_t* N, int64_t* S1, uint64_t* S2,
                 int32_t* E, uint64_t nblk, hipStream_t s) {
  constexpr int V = Vec16<T>::n;
  const uint64_t nb = (count + L - 1) / L;
  const dim3 grid(static_cast<unsigned>((nchans + kDigiTile - 1) / kDigiTile), static_cast<unsigned>(nb));
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && nchans % V == 0;
  const T* p = static_cast<const T*>(x);
  if (vec)
    digi_block_sums_kernel<T, V><<<grid, kThreads, 0, s>>>(p, count, nchans, b0, N, S1, S2, E, nblk);
  else
    digi_block_sums_kernel<T, 1><<<grid, kThreads, 0, s>>>(p, count, nchans, b0, N, S1, S2, E, nblk);
  post_launch_check("digi_block_sums_kernel", s);
}

template <class T>
void launch_quant(const void* x, uint64_t count, int nchans, uint64_t t0, int J, const double2* tab, bool flip,
                  uint8_t* y, unsigned long long* nclip, hipStream_t s) {
  constexpr int V = Vec16<T>::n;
  const uint64_t total = count * static_cast<uint64_t>(nchans);
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && nchans % V == 0;
  const T* p = static_cast<const T*>(x);
  if (vec) {
    const uint64_t ng = total / V;
    digi_quant_kernel<T, true><<<dev::grid_for(ng, kThreads, 8192), kThreads, 0, s>>>(p, total, nchans, t0, J, tab,
                                                                                     flip ? 1 : 0, y, ng, nclip);
  } else {
    const uint64_t ng = (total + 3) / 4;
    digi_quant_kernel<T, false><<<dev::grid_for(ng, kThreads, 8192), kThreads, 0, s>>>(p, total, nchans, t0, J, tab,
                                                                                      flip ? 1 : 0, y, ng, nclip);
  }
  post_launch_check("digi_quant_kernel", s);
}

}  // namespace

void digi_block_sums(const void* x, DigiType type, uint64_t count, int nchans, uint64_t t0, uint32_t* N, int64_t* S1,
                     uint64_t* S2, int32_t* E, uint64_t nblk, hipStream_t s) {
  PSOUP_CHECK(x != nullptr && count >= 1 && nchans >= 1, "digi_block_sums: empty input");
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(x) & static_cast<uintptr_t>(digi_type_bytes(type) - 1)) == 0,
              "digi_block_sums: x must be aligned to its sample type");
  PSOUP_CHECK(t0 % L == 0 && (t0 + count + L - 1) / L <= nblk, "digi_block_sums: blocks past the table");
  PSOUP_CHECK((count + L - 1) / L <= 65535, "digi_block_sums: at most 65535 blocks per launch");
  const uint64_t b0 = t0 / L;
  switch (type) {
    case DigiType::U8: launch_sums<uint8_t>(x, count, nchans, b0, N, S1, S2, E, nblk, s); break;
    case DigiType::I8: launch_sums<int8_t>(x, count, nchans, b0, N, S1, S2, E, nblk, s); break;
    case DigiType::U16: launch_sums<uint16_t>(x, count, nchans, b0, N, S1, S2, E, nblk, s); break;
    case DigiType::F32: launch_sums<float>(x, count, nchans, b0, N, S1, S2, E, nblk, s); break;
    default: PSOUP_THROW("digi_block_sums: bad sample type");
  }
}

void digi_quant(const void* x, DigiType type, uint64_t count, int nchans, uint64_t t0, int J, int nint,
                const double2* tab, bool flip, uint8_t* y, unsigned long long* nclip, hipStream_t s) {
  PSOUP_CHECK(x != nullptr && count >= 1 && nchans >= 1, "digi_quant: empty input");
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(x) & static_cast<uintptr_t>(digi_type_bytes(type) - 1)) == 0,
              "digi_quant: x must be aligned to its sample type");
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(y) & 15) == 0, "digi_quant: y must be 16-byte aligned");
  PSOUP_CHECK(J >= 0 && nint >= 1, "digi_quant: bad interval plan");
  const uint64_t last_blk = (t0 + count - 1) / L;
  PSOUP_CHECK((J > 0 ? last_blk / static_cast<uint64_t>(J) : 0) < static_cast<uint64_t>(nint),
              "digi_quant: samples past the last interval of the table");
  switch (type) {
    case DigiType::U8: launch_quant<uint8_t>(x, count, nchans, t0, J, tab, flip, y, nclip, s); break;
    case DigiType::I8: launch_quant<int8_t>(x, count, nchans, t0, J, tab, flip, y, nclip, s); break;
    case DigiType::U16: launch_quant<uint16_t>(x, count, nchans, t0, J, tab, flip, y, nclip, s); break;
    case DigiType::F32: launch_quant<float>(x, count, nchans, t0, J, tab, flip, y, nclip, s); break;
    default: PSOUP_THROW("digi_quant: bad sample type");
  }
}

}  // namespace kern
}  // namespace psoup
