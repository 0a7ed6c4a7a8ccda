// orbsearch kernel (psoup/orbit.hpp): re-indexes dedispersed byte rows by the
// definition's circular-orbit shift, K quantised templates per row in one
// launch.  The shift is integer arithmetic throughout: a wrapping 64-bit phase,
// a Q30 sine table with integer linear interpolation, one multiply and an
// arithmetic shift.
//
// Grid (groups of time tiles, templates, rows); lanes run along time and a lane
// owns 16 adjacent outputs: one aligned 16-byte store.  A workgroup copies the
// 16 KiB sine table into LDS once and then walks kOrbitTilesPerGroup tiles, so
// the table costs at most half the bytes a full group writes.  Neighbouring
// lanes are 16 samples apart, 65536 / pb table entries with pb in samples: for
// any orbit longer than 65536 samples they read the same or the next entry,
// which is a broadcast or a distinct bank of the 32 a dword read has, so a
// group of 32 lanes is conflict-free.  Only orbits of a few thousand samples
// spread a group over more than 32 entries and conflict.  The template {W, F,
// Aq} is the same for the whole workgroup and comes through scalar loads.
//
// Fast path: when the lane's span holds no turning point of the sine (the top
// bit of th + 2^62 agrees at its two ends) and the shifts at its two ends
// agree, the shift is one value throughout (orbit.hpp), so the 16 source bytes
// are contiguous: five aligned dword loads and a byte alignment
// (v_alignbyte_b32) assemble them.  The copy region n <= i < nrow takes the
// same path with a shift of 0.  The fast path needs the whole source span
// inside [0, n) (no clamp) and its aligned window inside the input bytes.
// Every other lane -- a turning point, a changing shift, a clamp, the row's
// tail -- computes s per sample and loads bytes.  Rows of `out` that are not
// 16-byte aligned are stored by bytes.  No atomics.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/orbit.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLane = kOrbitLane;

union Bytes16 {
  u32x4 v;
  uint32_t w[4];
  uint8_t b[kLane];
};

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

__global__ __launch_bounds__(kOrbitThreads) void orbit_resample_kernel(
    const uint8_t* __restrict__ in, uint64_t row_stride, uint64_t nrow, uint64_t n, const OrbitQuant* __restrict__ q,
    int K, const int32_t* __restrict__ table, uint8_t* __restrict__ out, uint64_t out_stride, uint64_t in_bytes,
    int in_aligned) {
  __shared__ int32_t tbl[kOrbitTable];
  for (int e = static_cast<int>(threadIdx.x); e < kOrbitTable; e += kOrbitThreads) tbl[e] = table[e];
  __syncthreads();
  const int k = static_cast<int>(blockIdx.y);
  const uint64_t r = blockIdx.z;
  const uint64_t W = q[k].W, F = q[k].F;
  const long long aq = q[k].Aq;
  const long long sf = sine_of(tbl, F);
  const uint8_t* x = in + r * row_stride;
  uint8_t* yrow = out + (r * static_cast<uint64_t>(K) + static_cast<uint64_t>(k)) * out_stride;
  const long long N = static_cast<long long>(n);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kOrbitTilesPerGroup;
  for (int t = 0; t < kOrbitTilesPerGroup; ++t) {
    const uint64_t i0 = (tile0 + static_cast<uint64_t>(t)) * kOrbitTile + static_cast<uint64_t>(threadIdx.x) * kLane;
    if (i0 >= nrow) break;
    uint8_t* y = yrow + i0;
    const long long I0 = static_cast<long long>(i0);
    const bool full = i0 + kLane <= nrow;
    const uint64_t th0 = F + i0 * W;  // wrapping
    Bytes16 v;
    v.v = u32x4{0u, 0u, 0u, 0u};
    bool have = false;
    if (in_aligned && full) {
      long long src = -1;  // first source sample of a contiguous span, if there is one
      if (I0 >= N) {
        src = I0;
      } else if (I0 + kLane <= N) {
        const uint64_t th1 = th0 + static_cast<uint64_t>(kLane - 1) * W;
        const bool clear = (((th0 + (1ull << 62)) ^ (th1 + (1ull << 62))) >> 63) == 0;
        if (clear) {
          const long long s0 = shift_of(tbl, th0, aq, sf), s1 = shift_of(tbl, th1, aq, sf);
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
      uint64_t th = th0;
#pragma unroll
      for (int j = 0; j < kLane; ++j, th += W) {
        const long long i = I0 + j;
        if (i < static_cast<long long>(nrow)) {
          long long src = i;
          if (i < N) src = min(max(i + shift_of(tbl, th, aq, sf), 0ll), N - 1);
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
}

}  // namespace

void orbit_resample(const uint8_t* in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, const OrbitQuant* q,
                    int K, const int32_t* table, uint8_t* out, uint64_t out_stride, hipStream_t s) {
  PSOUP_CHECK(in != nullptr && out != nullptr && q != nullptr && table != nullptr, "orbit_resample: missing buffer");
  PSOUP_CHECK(nrows >= 1 && nrows <= 65535, "orbit_resample: 1..65535 rows");
  PSOUP_CHECK(K >= 1 && K <= kOrbitMaxPerLaunch, "orbit_resample: 1.." << kOrbitMaxPerLaunch << " templates per launch");
  PSOUP_CHECK(n >= 1 && n <= nrow, "orbit_resample: the span must be in 1..nrow");
  PSOUP_CHECK(n <= kOrbitMaxSpan, "orbit: series longer than 2^26 samples");
  PSOUP_CHECK(row_stride >= nrow && out_stride >= nrow, "orbit_resample: a stride is shorter than the row");
  const uint64_t tiles = (nrow + kOrbitTile - 1) / kOrbitTile;
  const uint64_t groups = (tiles + kOrbitTilesPerGroup - 1) / kOrbitTilesPerGroup;
  PSOUP_CHECK(groups < (1ull << 31), "orbit_resample: row too long for one launch");
  const uint64_t in_bytes = static_cast<uint64_t>(nrows - 1) * row_stride + nrow;
  const uint64_t out_bytes = (static_cast<uint64_t>(nrows) * static_cast<uint64_t>(K) - 1) * out_stride + nrow;
  const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
  PSOUP_CHECK(ia + in_bytes <= oa || oa + out_bytes <= ia, "orbit_resample: in and out overlap");
  dim3 grid(static_cast<unsigned>(groups), static_cast<unsigned>(K), static_cast<unsigned>(nrows));
  orbit_resample_kernel<<<grid, kOrbitThreads, 0, s>>>(in, row_stride, nrow, n, q, K, table, out, out_stride, in_bytes,
                                                       ia % 4 == 0 ? 1 : 0);
  post_launch_check("orbit_resample_kernel", s);
}

}  // namespace kern
}  // namespace psoup
