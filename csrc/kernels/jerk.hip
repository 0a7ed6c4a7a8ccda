// jerksearch kernel (psoup/jerk.hpp): re-indexes dedispersed byte rows by the
// definition's cubic shift, K jerk factors per row in one launch.  Compiled
// without FMA contraction: g(i) is the definition's chain of three correctly
// rounded double multiplications.
//
// Grid (time tiles, jerk factors, rows); lanes run along time and a lane owns
// 16 adjacent outputs: one aligned 16-byte store.  Fast path: when the lane's
// span holds neither stationary point of the cubic (the host passes both as
// sample indices; a margin of a sample covers their rounding) and the shifts at
// its two ends agree, the shift is one value throughout (jerk.hpp), so the 16
// source bytes are contiguous: five aligned dword loads and a byte alignment
// (v_alignbyte_b32) assemble them.  The copy region n <= i < nrow takes the
// same path with a shift of 0.  The fast path needs the whole source span
// inside [0, n) (no clamp) and its aligned window inside the input bytes.
// Every other lane -- a stationary point, a changing shift, a clamp, the row's
// tail -- computes g per sample in double and loads bytes.  Rows of `out` that
// are not 16-byte aligned are stored by bytes.  No atomics, no LDS.
#include <algorithm>
#include <cmath>

#include "device_common.hpp"
#include "psoup/jerk.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLane = kJerkLane;

union Bytes16 {
  u32x4 v;
  uint32_t w[4];
  uint8_t b[kLane];
};

// the definition's s(i)
__device__ __forceinline__ long long shift_of(long long i, long long h, long long n, double jf) {
  const double g = ((static_cast<double>(i) * static_cast<double>(i - h)) * static_cast<double>(i - n)) * jf;
  return static_cast<long long>(rint(g));
}

__global__ __launch_bounds__(kJerkThreads) void jerk_resample_kernel(
    const uint8_t* __restrict__ in, uint64_t row_stride, uint64_t nrow, uint64_t n, const double* __restrict__ jf,
    int K, uint8_t* __restrict__ out, uint64_t out_stride, long long sp0, long long sp1, uint64_t in_bytes,
    int in_aligned) {
  const int k = static_cast<int>(blockIdx.y);
  const uint64_t r = blockIdx.z;
  const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kJerkTile + static_cast<uint64_t>(threadIdx.x) * kLane;
  if (i0 >= nrow) return;
  const double f = jf[k];
  const uint8_t* x = in + r * row_stride;
  uint8_t* y = out + (r * static_cast<uint64_t>(K) + static_cast<uint64_t>(k)) * out_stride + i0;
  const long long N = static_cast<long long>(n), H = N / 2, I0 = static_cast<long long>(i0);
  const bool full = i0 + kLane <= nrow;
  Bytes16 v;
  v.v = u32x4{0u, 0u, 0u, 0u};
  bool have = false;
  if (in_aligned && full) {
    long long src = -1;  // first source sample of a contiguous span, if there is one
    if (I0 >= N) {
      src = I0;
    } else if (I0 + kLane <= N) {
      const bool clear = (sp0 < I0 - 1 || sp0 > I0 + kLane) && (sp1 < I0 - 1 || sp1 > I0 + kLane);
      if (clear) {
        const long long s0 = shift_of(I0, H, N, f), s1 = shift_of(I0 + kLane - 1, H, N, f);
        if (s0 == s1 && I0 + s0 >= 0 && I0 + s0 + kLane <= N) src = I0 + s0;
      }
    }
    if (src >= 0) {
      const uint64_t off = r * row_stride + static_cast<uint64_t>(src);  // byte offset in `in`
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
  if (!have) {
#pragma unroll
    for (int j = 0; j < kLane; ++j) {
      const long long i = I0 + j;
      if (i < static_cast<long long>(nrow)) {
        long long src = i;
        if (i < N) src = min(max(i + shift_of(i, H, N, f), 0ll), N - 1);
        v.b[j] = x[src];
      }
    }
  }
  if (full && (reinterpret_cast<uintptr_t>(y) & 15u) == 0) {
    *reinterpret_cast<u32x4*>(y) = v.v;
  } else {
#pragma unroll
    for (int j = 0; j < kLane; ++j)
      if (i0 + static_cast<uint64_t>(j) < nrow) y[j] = v.b[j];
  }
}

}  // namespace

void jerk_resample(const uint8_t* in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, const double* jf,
                   int K, uint8_t* out, uint64_t out_stride, int64_t sp0, int64_t sp1, hipStream_t s) {
  PSOUP_CHECK(in != nullptr && out != nullptr && jf != nullptr, "jerk_resample: missing buffer");
  PSOUP_CHECK(nrows >= 1 && nrows <= 65535, "jerk_resample: 1..65535 rows");
  PSOUP_CHECK(K >= 1 && K <= kJerkMaxTrials, "jerk_resample: 1.." << kJerkMaxTrials << " jerk factors");
  PSOUP_CHECK(n >= 1 && n <= nrow, "jerk_resample: the span must be in 1..nrow");
  PSOUP_CHECK(n <= kJerkMaxSpan, "jerk: series longer than 2^26 samples");
  PSOUP_CHECK(row_stride >= nrow && out_stride >= nrow, "jerk_resample: a stride is shorter than the row");
  PSOUP_CHECK(sp0 <= sp1, "jerk_resample: stationary points out of order");
  const uint64_t tiles = (nrow + kJerkTile - 1) / kJerkTile;
  PSOUP_CHECK(tiles < (1ull << 31), "jerk_resample: row too long for one launch");
  const uint64_t in_bytes = static_cast<uint64_t>(nrows - 1) * row_stride + nrow;
  const uint64_t out_bytes = (static_cast<uint64_t>(nrows) * static_cast<uint64_t>(K) - 1) * out_stride + nrow;
  const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
  PSOUP_CHECK(ia + in_bytes <= oa || oa + out_bytes <= ia, "jerk_resample: in and out overlap");
  dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(K), static_cast<unsigned>(nrows));
  jerk_resample_kernel<<<grid, kJerkThreads, 0, s>>>(in, row_stride, nrow, n, jf, K, out, out_stride,
                                                     static_cast<long long>(sp0), static_cast<long long>(sp1),
                                                     in_bytes, ia % 4 == 0 ? 1 : 0);
  post_launch_check("jerk_resample_kernel", s);
}

}  // namespace kern
}  // namespace psoup
