// sbsearch kernels (psoup/sideband.hpp): sb_power, the band-normalised powers
// of the whitened spectra, and sb_search, the short FFTs of those powers with
// the per-segment maximum and the event records.
//
// sb_search: one workgroup of 512 threads per (row, window of 8192 bins, hop
// 4096).  The window is staged in LDS once (clipped, less 1, zero past the
// band) and serves the M = 8192 segment that is the window and, for every
// smaller M, the segments that start in its first half; all of them end inside
// it.  Two real segments ride one complex transform.  The transforms run in
// place in LDS as decimation-in-frequency passes of radix 8 (one leading radix
// 2 or 4), a butterfly reading and writing only its own points, so one barrier
// per pass; the result stays digit-reversed and is read through
// sbk::position.  The work buffer of the M = 8192 transform (64 KiB) overlays
// the staged window, which is why that size runs last and why the input is
// held in registers across a barrier before it is written.
#include <hip/hip_runtime.h>

#include "psoup/sideband.hpp"

namespace psoup {
namespace kern {

namespace {

// ------------------------------------------------------------ sb_power ----
__device__ __forceinline__ bool zapped(const uint32_t* mask, int64_t k) {
  return mask != nullptr && ((mask[k >> 5] >> (k & 31)) & 1u) != 0;
}

__device__ __forceinline__ double power_of(float2 v) {
  return static_cast<double>(v.x) * static_cast<double>(v.x) + static_cast<double>(v.y) * static_cast<double>(v.y);
}

__global__ __launch_bounds__(kSbRangeLanes) void sb_power_partial_kernel(const float2* __restrict__ spec,
                                                                         uint64_t spec_stride,
                                                                         const uint32_t* __restrict__ mask, int64_t k_lo,
                                                                         int64_t k_hi, double* __restrict__ partials,
                                                                         int nranges) {
  __shared__ double a[kSbRangeLanes];
  const int t = threadIdx.x;
  const int64_t base = k_lo + static_cast<int64_t>(blockIdx.x) * kSbRange;
  const float2* row = spec + static_cast<uint64_t>(blockIdx.y) * spec_stride;
  double acc = 0.0;
  for (int u = 0; u < kSbRange / kSbRangeLanes; ++u) {
    const int64_t k = base + t + kSbRangeLanes * u;
    if (k < k_hi && !zapped(mask, k)) acc += power_of(row[k]);
  }
  a[t] = acc;
  __syncthreads();
  for (int s = kSbRangeLanes / 2; s >= 1; s >>= 1) {
    if (t < s) a[t] += a[t + s];
    __syncthreads();
  }
  if (t == 0) partials[static_cast<uint64_t>(blockIdx.y) * nranges + blockIdx.x] = a[0];
}

__global__ void sb_power_finish_kernel(const double* __restrict__ partials, int nranges, int nrows, uint64_t count,
                                       double* __restrict__ mu) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  double sum = 0.0;
  for (int i = 0; i < nranges; ++i) sum += partials[static_cast<uint64_t>(r) * nranges + i];
  mu[r] = sum / static_cast<double>(count);
}

__global__ __launch_bounds__(256) void sb_power_norm_kernel(const float2* __restrict__ spec, uint64_t spec_stride,
                                                            const uint32_t* __restrict__ mask, int64_t k_lo,
                                                            int64_t k_hi, const double* __restrict__ mu,
                                                            float* __restrict__ P, uint64_t stride) {
  const int64_t k = k_lo + static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (k >= k_hi) return;
  const uint64_t r = blockIdx.y;
  float v = 1.0f;
  if (!zapped(mask, k)) v = static_cast<float>(power_of(spec[r * spec_stride + k]) / mu[r]);
  P[r * stride + k] = v;
}

// ----------------------------------------------------------- sb_search ----
struct SbArgs {
  const float* P;
  uint64_t stride;
  int64_t k_lo, k_hi;
  int m_lo, m_hi, j_min, dm0;
  float clip, min_power;
  int64_t nseg[kSbMaxM - kSbMinM + 1];  // by m - m_lo
  int64_t seg_stride;
  const float2* tw;
  float* best_S;
  int32_t* best_j;
  SbEvent* events;
  uint32_t capacity;
  uint32_t* count;
};

template <int R>
__device__ __forceinline__ void pass(float2* buf, const float2* tw, int m, int L, int npoints) {
  for (int b = threadIdx.x; b < npoints / R; b += kSbThreads) sbk::butterfly<R>(buf, tw, m, L, b);
}

__global__ __launch_bounds__(kSbThreads) void sb_search_kernel(const SbArgs a) {
  // 8192 complex points; the staged window is its upper half
  __shared__ __attribute__((aligned(16))) float2 buf[kSbWindow];
  __shared__ unsigned long long segkey[kSbWindow >> kSbMinM];
  float* const win = reinterpret_cast<float*>(buf) + kSbWindow;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = blockIdx.x;
  const int row = blockIdx.y;
  const int64_t g0 = a.k_lo + static_cast<int64_t>(w) * kSbHop;  // first bin of the window
  const int64_t gend = (g0 + kSbWindow < a.k_hi) ? g0 + kSbWindow : a.k_hi;
  const float* prow = a.P + static_cast<uint64_t>(row) * a.stride;

  bool hot = false;
  // stage: groups of 4 bins at 16-byte aligned addresses; a group that is
  // wholly inside [g0, gend) is one wide load, the head and the tail go bin by bin
  {
    const int64_t a0 = g0 & ~static_cast<int64_t>(3);
    const int head = static_cast<int>(g0 - a0);
    for (int q = tid; q < kSbWindow / 4 + 1; q += kSbThreads) {
      const int64_t ga = a0 + 4 * static_cast<int64_t>(q);
      const int i0 = 4 * q - head;
      float v[4] = {1.f, 1.f, 1.f, 1.f};  // x = 0 past the band
      if (ga >= g0 && ga + 4 <= gend) {
        const float4 f = *reinterpret_cast<const float4*>(prow + ga);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ga + e >= g0 && ga + e < gend) v[e] = prow[ga + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e;
        if (i >= 0 && i < kSbWindow) {
          const float x = fminf(v[e], a.clip) - 1.0f;
          hot = hot || x > kSbPairLimit;
          win[i] = x;
        }
      }
    }
  }
  const bool hotw = __syncthreads_or(hot ? 1 : 0) != 0;  // (also the barrier behind the staging)

  for (int m = a.m_lo; m <= a.m_hi; ++m) {
    const int nsl = sbk::owned(m);
    const int64_t nseg = a.nseg[m - a.m_lo];
    const int64_t s0 = static_cast<int64_t>(w) * nsl;  // the window's first segment of this size
    if (s0 >= nseg) continue;                          // (uniform)
    int r[5];
    const int nst = sbk::radices(m, r);
    const int npoints = sbk::points(m);
    const int per = npoints / kSbThreads;  // 8 or 16

    if (tid < nsl) segkey[tid] = 0ull;  // (ordered before the atomics by the barriers below)
    for (int ps = 0; ps < sbk::passes(m, hotw); ++ps) {
    const int sel = sbk::pass_sel(m, hotw, ps);
    // input -> registers -> (barrier: the m = 13 buffer overlays the window; a second pass: the read-out of the
    // first is over) -> buffer
    float2 x[kSbWindow / kSbThreads];
#pragma unroll
    for (int k = 0; k < kSbWindow / kSbThreads; ++k)
      if (k < per) x[k] = sbk::load_elem(win, m, tid + k * kSbThreads, sel);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSbWindow / kSbThreads; ++k)
      if (k < per) buf[tid + k * kSbThreads] = x[k];
    __syncthreads();

    int L = 1 << m;
    for (int s = 0; s < nst; ++s) {
      if (r[s] == 8) pass<8>(buf, a.tw, m, L, npoints);
      else if (r[s] == 4) pass<4>(buf, a.tw, m, L, npoints);
      else pass<2>(buf, a.tw, m, L, npoints);
      L /= r[s];
      __syncthreads();
    }

    // read-out: consecutive lanes take consecutive j of one transform; the key
    // (S, lowest j) is reduced over the lanes that share a transform, then one
    // LDS atomic per group and segment
    const int half = 1 << (m - 1);
    const int nitems = (m == kSbMaxM) ? half : npoints / 2;
    const int G = half < 64 ? half : 64;
    for (int it = tid; it < nitems; it += kSbThreads) {  // (nitems is a multiple of 512)
      int c, j;
      float sa, sb;
      sbk::item(buf, m, r, nst, it, &c, &j, &sa, &sb);
      unsigned long long ka = 0ull, kb = 0ull;
      if (j >= a.j_min) {
        ka = sbk::key_of(sa, j);
        kb = sbk::key_of(sb, j);
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const unsigned long long oa = __shfl_xor(ka, off, 64), ob = __shfl_xor(kb, off, 64);
        ka = oa > ka ? oa : ka;
        kb = ob > kb ? ob : kb;
      }
      if ((lane & (G - 1)) == 0) {
        if (m == kSbMaxM) {
          atomicMax(&segkey[0], ka);
        } else if (sel == 0) {
          atomicMax(&segkey[2 * c], ka);
          atomicMax(&segkey[2 * c + 1], kb);
        } else {
          atomicMax(&segkey[2 * c + sel - 1], ka);
        }
      }
    }
    __syncthreads();
    }  // passes

    // one record per segment the band holds; one counter atomic per wave
    {
      bool has = false;
      float S = 0.f;
      int j = 0;
      const int64_t seg = s0 + tid;
      if (tid < nsl && seg < nseg) {
        sbk::key_split(segkey[tid], &S, &j);
        if (a.best_S != nullptr) {
          const uint64_t o =
              (static_cast<uint64_t>(row) * (a.m_hi - a.m_lo + 1) + (m - a.m_lo)) * a.seg_stride + seg;
          a.best_S[o] = S;
          a.best_j[o] = j;
        }
        has = S >= a.min_power;
      }
      const unsigned long long mask = __ballot(has);
      if (mask != 0ull) {  // (wave-uniform)
        const int leader = __ffsll(static_cast<long long>(mask)) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.count, static_cast<uint32_t>(__popcll(mask)));
        base = __shfl(base, leader, 64);
        if (has) {
          const uint32_t idx = base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
          if (idx < a.capacity) {
            SbEvent e;
            e.dm_idx = a.dm0 + row;
            e.m = m;
            e.seg = static_cast<int32_t>(seg);
            e.j = j;
            e.S = S;
            a.events[idx] = e;
          }
        }
      }
    }
    // (the next size resets segkey[t] from thread t, which has read it above,
    // and rewrites buf only after its first barrier)
  }
}

}  // namespace

void sb_power(const float2* spec, uint64_t spec_stride, int nrows, const uint32_t* zapmask, int64_t k_lo, int64_t k_hi,
              uint64_t count, double* partials, double* mu, float* P, uint64_t stride, hipStream_t s) {
  PSOUP_CHECK(nrows >= 1 && nrows <= 65535, "sb_power: 1..65535 rows per launch");
  PSOUP_CHECK(k_lo >= 0 && k_lo < k_hi, "sb_power: an empty band");
  PSOUP_CHECK(static_cast<uint64_t>(k_hi) <= spec_stride && static_cast<uint64_t>(k_hi) <= stride,
              "sb_power: the band passes a row");
  PSOUP_CHECK(count >= 1 && count <= static_cast<uint64_t>(k_hi - k_lo), "sb_power: the count of unzapped bins");
  const int64_t band = k_hi - k_lo;
  const int nranges = static_cast<int>((band + kSbRange - 1) / kSbRange);
  sb_power_partial_kernel<<<dim3(static_cast<unsigned>(nranges), static_cast<unsigned>(nrows)), kSbRangeLanes, 0, s>>>(
      spec, spec_stride, zapmask, k_lo, k_hi, partials, nranges);
  sb_power_finish_kernel<<<(nrows + 63) / 64, 64, 0, s>>>(partials, nranges, nrows, count, mu);
  sb_power_norm_kernel<<<dim3(static_cast<unsigned>((band + 255) / 256), static_cast<unsigned>(nrows)), 256, 0, s>>>(
      spec, spec_stride, zapmask, k_lo, k_hi, mu, P, stride);
  PSOUP_HIP_CHECK(hipGetLastError());
}

void sb_search(const float* P, uint64_t stride, int nrows, const SbGeometry& g, const SbParams& p, int dm0,
               const float2* tw, float* best_S, int32_t* best_j, SbEvent* events, uint32_t capacity, uint32_t* count,
               hipStream_t s) {
  PSOUP_CHECK(nrows >= 1 && nrows <= 65535, "sb_search: 1..65535 rows per launch");
  PSOUP_CHECK(p.m_lo >= kSbMinM && p.m_hi <= kSbMaxM && p.m_lo <= p.m_hi && g.m_lo == p.m_lo && g.m_hi == p.m_hi &&
                  g.nseg.size() == static_cast<size_t>(p.m_hi - p.m_lo + 1),
              "sb_search: the sizes are outside 5..13 or not the geometry's");
  PSOUP_CHECK(p.j_min >= 1 && p.j_min < (1 << p.m_lo) / 2, "sb_search: j_min outside [1, 2^m_lo / 2)");
  PSOUP_CHECK(p.clip > 1.0f, "sb_search: clip must be above 1");
  PSOUP_CHECK(g.k_lo >= 0 && g.k_lo <= g.k_hi && static_cast<uint64_t>(g.k_hi) <= stride,
              "sb_search: the band passes a row");
  PSOUP_CHECK(stride % 4 == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0,
              "sb_search: P must be 16-byte aligned with a stride that is a multiple of 4");
  PSOUP_CHECK((best_S == nullptr) == (best_j == nullptr), "sb_search: best_S and best_j come together");
  PSOUP_CHECK(events != nullptr || capacity == 0, "sb_search: a capacity without a buffer");
  PSOUP_CHECK(count != nullptr && tw != nullptr, "sb_search: the counter and the twiddles are required");
  if (g.nwin <= 0) return;  // no segment of any size
  SbArgs a;
  a.P = P;
  a.stride = stride;
  a.k_lo = g.k_lo;
  a.k_hi = g.k_hi;
  a.m_lo = p.m_lo;
  a.m_hi = p.m_hi;
  a.j_min = p.j_min;
  a.dm0 = dm0;
  a.clip = p.clip;
  a.min_power = p.min_power;
  for (int i = 0; i <= kSbMaxM - kSbMinM; ++i) a.nseg[i] = i < static_cast<int>(g.nseg.size()) ? g.nseg[i] : 0;
  // the windows must own every segment and hold it whole
  for (int m = p.m_lo; m <= p.m_hi; ++m) {
    const int64_t n = g.nsegs_of(m);
    PSOUP_CHECK(n == sb_nseg(g.k_hi - g.k_lo, m) && n <= g.seg_stride, "sb_search: segment counts that are not the band's");
    PSOUP_CHECK(n == 0 || (n - 1) / sbk::owned(m) < g.nwin, "sb_search: a segment outside the windows");
  }
  a.seg_stride = g.seg_stride;
  a.tw = tw;
  a.best_S = best_S;
  a.best_j = best_j;
  a.events = events;
  a.capacity = capacity;
  a.count = count;
  sb_search_kernel<<<dim3(static_cast<unsigned>(g.nwin), static_cast<unsigned>(nrows)), kSbThreads, 0, s>>>(a);
  PSOUP_HIP_CHECK(hipGetLastError());
}

}  // namespace kern
}  // namespace psoup
