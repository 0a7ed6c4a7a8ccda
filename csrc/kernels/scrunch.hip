// filscrunch kernels (psoup/scrunch.hpp): subbanded, time-scrunched exact sums
// of the channel-major int8 rows with their block statistics, and the
// requantisation to 8 bits.
//
// scrunch_sums: one workgroup per (subband, tile of output samples); a tile
// lies in one statistics block.  Per unkilled channel of the subband the source
// window [f u0 + rel[c], + f T) is staged in LDS with aligned 16-byte loads,
// the next channel's window in flight while the current one is summed.  Each
// channel's window is staged on its own, so the spread of rel inside a subband
// costs no LDS: no rel is too large (a high DM moves the window, it does not
// widen it).  An output belongs to 2^lanes_log2 adjacent lanes (1 for f < 16,
// 32 for f = 256); they walk the output's dwords of the window, clear the bytes
// outside the bin and add the four bytes by the packed integer dot product
// (f = 1 reads its byte directly); the lanes' int32 partials are added by
// shuffles after the last channel and the bias is added arithmetically,
// bias f nactive.  A is written once by plain stores; the tile's sum A and
// sum A^2 go to the block's cell by one 64-bit atomic add each per workgroup:
// integer addition, so the result does not depend on the order.
//
// The pass reads nchans x nsamps bytes once and writes 4 nsub nout bytes; the
// LDS holds 2 x 12 KiB per workgroup (six workgroups per CU).
#include <algorithm>

#include "device_common.hpp"
#include "psoup/scrunch.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = kScrunchThreads;
constexpr int kLoads = kScrunchWindow / (16 * kThreads);  // 16-byte loads per thread and window
constexpr int L = kScrunchStatBlock;
static_assert(kLoads * 16 * kThreads == kScrunchWindow, "the threads' loads tile the window");

template <bool F1>
__global__ void __launch_bounds__(kThreads)
    scrunch_sums_kernel(const int8_t* __restrict__ x, uint64_t stride, int bias, int f, int T, int tpb, int lg,
                        const int32_t* __restrict__ active, const int32_t* __restrict__ sub_first,
                        const int32_t* __restrict__ rel, uint64_t u0, uint64_t count, int32_t* __restrict__ A,
                        uint64_t a_stride, unsigned long long* __restrict__ S1, unsigned long long* __restrict__ S2,
                        uint64_t nblk) {
  __shared__ __attribute__((aligned(16))) uint32_t win[2][kScrunchWindow / 4];
  __shared__ unsigned long long red[kThreads / dev::kWave];
  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const uint32_t bl = blockIdx.x / static_cast<uint32_t>(tpb);
  const uint32_t j = blockIdx.x - bl * static_cast<uint32_t>(tpb);
  const uint64_t ub = u0 + static_cast<uint64_t>(bl) * L;  // the block's first output
  const uint64_t us = ub + static_cast<uint64_t>(j) * T;
  const uint64_t ue = min(min(ub + L, us + T), u0 + count);
  if (us >= ue) return;  // uniform: the block's last tile may be empty
  const int nb = static_cast<int>(ue - us);
  const int ia = dev::sload(sub_first, static_cast<uint64_t>(s));
  const int nch = dev::sload(sub_first, static_cast<uint64_t>(s) + 1) - ia;
  const int G = 1 << lg;
  const int g = tid & (G - 1);
  const int grp = tid >> lg;
  const int ngroups = kThreads >> lg;
  const int span = nb * f;  // bytes of the tile's bins, <= kScrunchWindow - 16
  const int64_t base = static_cast<int64_t>(us) * f;

  int acc[kScrunchMaxOut];
#pragma unroll
  for (int n = 0; n < kScrunchMaxOut; ++n) acc[n] = 0;

  // channel q of the subband: this thread's part of its window.  A load holds
  // at least one byte of the window, and the window ends before nsamps <=
  // stride (a multiple of 16), so every load stays inside its row.
  auto fetch = [&](int q, u32x4 (&r)[kLoads], int& shift) {
    const int c = dev::sload(active, static_cast<uint64_t>(ia + q));
    const int64_t g0 = base + dev::sload(rel, static_cast<uint64_t>(c));
    shift = static_cast<int>(g0 & 15);
    const int64_t g0a = g0 - shift;
    const int need = span + shift;
    const int8_t* row = x + static_cast<uint64_t>(c) * stride;
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      const int p = 16 * (tid + kThreads * l);
      const int64_t pos = g0a + p;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (p < need && pos + 16 <= static_cast<int64_t>(stride)) v = *reinterpret_cast<const u32x4*>(row + pos);
      r[l] = v;
    }
  };

  if (nch > 0) {
    u32x4 r[kLoads];
    int shift_next;
    fetch(0, r, shift_next);
    for (int q = 0; q < nch; ++q) {
      const int buf = q & 1;
      const int shift = shift_next;
      const int need = span + shift;
#pragma unroll
      for (int l = 0; l < kLoads; ++l)
        if (16 * (tid + kThreads * l) < need) *reinterpret_cast<u32x4*>(&win[buf][4 * (tid + kThreads * l)]) = r[l];
      if (q + 1 < nch) fetch(q + 1, r, shift_next);
      // one barrier per channel: the buffer written next was last read
      // before this barrier
      __syncthreads();
      const uint32_t* wb = win[buf];
#pragma unroll
      for (int n = 0; n < kScrunchMaxOut; ++n) {
        const int o = n * ngroups + grp;
        if (o < nb) {
          if (F1) {
            acc[n] += reinterpret_cast<const int8_t*>(wb)[o + shift];
          } else {
            const int a = o * f + shift, b = a + f;
            int sum = acc[n];
            for (int k = (a >> 2) + g; 4 * k < b; k += G) {
              const int first = max(a - 4 * k, 0), last = min(b - 4 * k, 4);  // bytes [first, last) of the dword
              uint32_t m = last >= 4 ? 0xffffffffu : ((1u << (8 * last)) - 1u);
              m &= 0xffffffffu << (8 * first);
              sum = __builtin_amdgcn_sdot4(static_cast<int>(wb[k] & m), 0x01010101, sum, false);
            }
            acc[n] = sum;
          }
        }
      }
    }
  }

  // the group's partials, the stores, the tile's statistics
  unsigned long long t1 = 0, t2 = 0;
  const int add = bias * f * nch;
  int32_t* out = A + static_cast<uint64_t>(s) * a_stride + (us - u0);
#pragma unroll
  for (int n = 0; n < kScrunchMaxOut; ++n) {
    int v = acc[n];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
      if (o < G) v += __shfl_xor(v, o, dev::kWave);  // uniform
    const int o = n * ngroups + grp;
    if (g == 0 && o < nb) {
      v += add;  // the raw sum, >= 0 and < 2^26
      out[o] = v;
      t1 += static_cast<unsigned long long>(v);
      t2 += static_cast<unsigned long long>(v) * static_cast<unsigned long long>(v);
    }
  }
  t1 = dev::block_sum(t1, red);
  t2 = dev::block_sum(t2, red);
  if (tid == 0) {
    const uint64_t cell = static_cast<uint64_t>(s) * nblk + us / L;
    atomicAdd(&S1[cell], t1);
    atomicAdd(&S2[cell], t2);
  }
}

// ----------------------------------------------------------------- quant ----
// One thread per 16 outputs of a subband: four 16-byte loads of A, one 16-byte
// store of y - 128.
__global__ void __launch_bounds__(256)
    scrunch_quant_kernel(const int32_t* __restrict__ A, uint64_t a_stride, uint64_t count,
                         const int32_t* __restrict__ M, const uint8_t* __restrict__ live, int32_t mul,
                         int8_t* __restrict__ y, uint64_t y_stride) {
  const int s = blockIdx.y;
  const uint64_t u = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) * 16;
  if (u >= count) return;
  const int32_t* a = A + static_cast<uint64_t>(s) * a_stride + u;
  const int m = M[s];
  const bool on = live[s] != 0;
  int v[16];
  if (u + 16 <= count) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 t = reinterpret_cast<const int4*>(a)[q];
      v[4 * q] = t.x;
      v[4 * q + 1] = t.y;
      v[4 * q + 2] = t.z;
      v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (u + q < count) ? a[q] : m;
  }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t d = ((static_cast<int64_t>(v[q]) - m) * mul + 32768) >> 16;  // arithmetic: floors
    int yq = static_cast<int>(min(max(d + 128, static_cast<int64_t>(0)), static_cast<int64_t>(255)));
    if (!on) yq = 128;
    if (u + q >= count) yq = 128;  // the row's padding up to 16 bytes
    w[q >> 2] |= static_cast<uint32_t>((yq - 128) & 0xff) << (8 * (q & 3));
  }
  *reinterpret_cast<u32x4*>(y + static_cast<uint64_t>(s) * y_stride + u) = u32x4{w[0], w[1], w[2], w[3]};
}

}  // namespace

void scrunch_sums(const int8_t* rows, uint64_t stride, uint64_t nsamps, int bias, int f, const int32_t* d_active,
                  const int32_t* d_sub_first, const int32_t* d_rel, int nsub, uint64_t u0, uint64_t count, int32_t* A,
                  uint64_t a_stride, uint64_t* S1, uint64_t* S2, uint64_t nblk, hipStream_t s) {
  PSOUP_CHECK((stride & 15) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0 && stride >= nsamps &&
                  stride < (uint64_t(1) << 62),
              "scrunch_sums: rows must be 16-byte aligned with a stride that is a multiple of 16 and >= nsamps");
  PSOUP_CHECK(f >= 1 && f <= kScrunchMaxF, "scrunch_sums: tscrunch must be in 1.." << kScrunchMaxF);
  PSOUP_CHECK(nsub >= 1 && nsub <= 65535, "scrunch_sums: 1..65535 subbands");
  PSOUP_CHECK(bias >= 0 && bias <= 128, "scrunch_sums: bias");
  PSOUP_CHECK(count >= 1 && u0 % L == 0 && a_stride >= count, "scrunch_sums: bad chunk");
  PSOUP_CHECK((u0 + count) <= nsamps / static_cast<uint64_t>(f) && (u0 + count + L - 1) / L <= nblk,
              "scrunch_sums: outputs past the rows or the block table");
  const int T = scrunch_tile(f);
  const int lg = scrunch_lanes_log2(f);
  const int tpb = (L + T - 1) / T;
  PSOUP_CHECK(T >= 1 && T * f + 16 <= kScrunchWindow && (T + (kThreads >> lg) - 1) / (kThreads >> lg) <= kScrunchMaxOut,
              "scrunch_sums: bad tile plan");
  const uint64_t tiles = (count + L - 1) / L * static_cast<uint64_t>(tpb);
  PSOUP_CHECK(tiles < (1ull << 31), "scrunch_sums: too many tiles in one chunk");
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(nsub));
  auto* s1 = reinterpret_cast<unsigned long long*>(S1);
  auto* s2 = reinterpret_cast<unsigned long long*>(S2);
  if (f == 1)
    scrunch_sums_kernel<true><<<grid, kThreads, 0, s>>>(rows, stride, bias, f, T, tpb, lg, d_active, d_sub_first,
                                                        d_rel, u0, count, A, a_stride, s1, s2, nblk);
  else
    scrunch_sums_kernel<false><<<grid, kThreads, 0, s>>>(rows, stride, bias, f, T, tpb, lg, d_active, d_sub_first,
                                                         d_rel, u0, count, A, a_stride, s1, s2, nblk);
  post_launch_check("scrunch_sums_kernel", s);
}

void scrunch_quant(const int32_t* A, uint64_t a_stride, int nsub, uint64_t count, const int32_t* d_M,
                   const uint8_t* d_live, int32_t mul, int8_t* y, uint64_t y_stride, hipStream_t s) {
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(A) & 15) == 0 && a_stride % 4 == 0 && a_stride >= count,
              "scrunch_quant: A must be 16-byte aligned with a stride that is a multiple of 4 and >= count");
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(y) & 15) == 0 && y_stride % 16 == 0 && y_stride >= count,
              "scrunch_quant: y must be 16-byte aligned with a stride that is a multiple of 16 and >= count");
  PSOUP_CHECK(nsub >= 1 && nsub <= 65535 && count >= 1 && mul >= 1, "scrunch_quant: bad shape or mul");
  const uint64_t gx = (count + 4095) / 4096;
  PSOUP_CHECK(gx < (1ull << 31), "scrunch_quant: too many samples");
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(nsub));
  scrunch_quant_kernel<<<grid, 256, 0, s>>>(A, a_stride, count, d_M, d_live, mul, y, y_stride);
  post_launch_check("scrunch_quant_kernel", s);
}

}  // namespace kern
}  // namespace psoup
