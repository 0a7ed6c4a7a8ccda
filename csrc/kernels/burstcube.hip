// Burst cutouts: time-scrunched, dedispersed sums of the channel-major int8
// rows around a single-pulse candidate (psoup/burstcube.hpp).
//
// Subbands and DM trials are the same thing here: an output row with a run of
// channels and one sample offset per channel.  One workgroup forms, for one
// tile of rows (BurstTile) and one tile of time bins, every (row, bin) sum of
// f consecutive samples.  Per channel the union of the rows' source windows
// (the bins' samples plus the spread of the rows' offsets, at most
// kBurstWindow bytes: the host plan sizes the tiles so) is staged once in LDS
// with aligned 16-byte loads, the next channel's window in flight while the
// current one is summed; adjacent DM rows read windows that differ by a few
// samples, so a tile of them shares most of its bytes.  A tile degrades to one
// row where the spread is too large (a high-DM candidate's low channels).
//
// A (row, bin) output belongs to 2^lanes_log2 adjacent lanes: 1 for f < 16,
// up to a whole wave for f >= 512.  They walk the output's dwords of the
// window, clear the bytes outside [first, last) sample of the bin and outside
// [0, N) of the row, and add the four bytes by the packed integer dot
// product; the lanes' int32 partials are added by shuffles after the last
// channel.  hits is the clipped interval length per channel, summed, and the
// bias is added per counted sample.  A workgroup owns its outputs: plain
// stores, no atomics, nothing to zero.  Integer sums: the result does not
// depend on any order.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/burstcube.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = kBurstThreads;
constexpr int kLoads = kBurstWindow / (16 * kThreads);  // 16-byte loads per thread and window
static_assert(kLoads * 16 * kThreads == kBurstWindow, "the threads' loads tile the window");
static_assert(kBurstMaxRows <= kThreads, "one thread stages one row's offset");
static_assert(kBurstWindow < 65536 && kBurstMaxRows <= 32768, "a lane's output packs (row << 16) | byte position");

// uniform per (tile, channel): where the staged window lies in its row
struct Win {
  int shift;   // bytes of the first 16 staged that precede the window
  int need;    // bytes staged
  int lo, hi;  // staged bytes [lo, hi) are samples [0, N) of the row
};

__global__ void __launch_bounds__(kThreads)
    burst_cube_kernel(const int8_t* __restrict__ x, uint64_t stride, int64_t nsamps, int bias, int ntime, int nrows_out,
                      const int32_t* __restrict__ active, const BurstTile* __restrict__ tiles,
                      const BurstJob* __restrict__ jobs, const int32_t* __restrict__ rel,
                      const int32_t* __restrict__ win_tab, int32_t* __restrict__ sums, int32_t* __restrict__ hits) {
  __shared__ __attribute__((aligned(16))) uint32_t win[2][kBurstWindow / 4];
  __shared__ int32_t rowrel[2][kBurstMaxRows];
  const int tid = threadIdx.x;
  const BurstTile T = tiles[blockIdx.x];
  const BurstJob J = jobs[T.cand];
  const int f = J.f;
  const int kb = static_cast<int>(blockIdx.y) * J.bins_per_tile;
  if (kb >= ntime) return;  // uniform: this job has fewer time tiles than the grid
  const int nb = min(ntime, kb + J.bins_per_tile) - kb;
  const int lg = J.lanes_log2;
  const int G = 1 << lg;
  const int g = tid & (G - 1);
  const int grp = tid >> lg;
  const int ngroups = kThreads >> lg;
  const int nout = T.nrows * nb;
  const int nper = (nout + ngroups - 1) / ngroups;  // <= kBurstMaxOut (host plan)
  const int span = nb * f;                          // bytes of one row's bins
  const int64_t base = J.t0 + static_cast<int64_t>(kb) * f;
  const int nch = T.ie - T.ia;

  // this lane group's outputs: (row << 16) | first byte of the bin within the row's span
  int desc[kBurstMaxOut], acc[kBurstMaxOut], cnt[kBurstMaxOut];
#pragma unroll
  for (int n = 0; n < kBurstMaxOut; ++n) {
    const int o = n * ngroups + grp;
    const int row = o / nb;
    desc[n] = (n < nper && o < nout) ? ((row << 16) | ((o - row * nb) * f)) : -1;
    acc[n] = 0;
    cnt[n] = 0;
  }

  // channel q of the tile: the window's uniform values and this thread's part
  // of it; nothing is read before the row, past the window or past the row
  auto fetch = [&](int q, u32x4 (&r)[kLoads], int& rr, Win& w) {
    const int c = dev::sload(active, static_cast<uint64_t>(T.ia + q));
    const int mn = dev::sload(win_tab, 2 * (static_cast<uint64_t>(T.win0) + q));
    const int spread = dev::sload(win_tab, 2 * (static_cast<uint64_t>(T.win0) + q) + 1);
    const int64_t g0 = base + mn;
    w.shift = static_cast<int>(g0 & 15);
    const int64_t g0a = g0 - w.shift;
    const int need = span + spread + w.shift;  // <= kBurstWindow (host plan)
    w.need = need;
    w.lo = static_cast<int>(min(max(-g0a, static_cast<int64_t>(0)), static_cast<int64_t>(kBurstWindow)));
    w.hi = static_cast<int>(min(max(nsamps - g0a, static_cast<int64_t>(0)), static_cast<int64_t>(kBurstWindow)));
    const int8_t* row = x + static_cast<uint64_t>(c) * stride;
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      const int p = 16 * (tid + kThreads * l);
      const int64_t pos = g0a + p;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (p < need && p < w.hi && p + 16 > w.lo && pos >= 0 && pos + 16 <= static_cast<int64_t>(stride))
        v = *reinterpret_cast<const u32x4*>(row + pos);
      r[l] = v;
    }
    rr = 0;
    if (tid < T.nrows) rr = rel[static_cast<uint64_t>(T.rel0) + static_cast<uint64_t>(q) * T.nrows + tid];
  };

  if (nch > 0) {
    u32x4 r[kLoads];
    int rr;
    Win wn;
    fetch(0, r, rr, wn);
    for (int q = 0; q < nch; ++q) {
      const int buf = q & 1;
#pragma unroll
      for (int l = 0; l < kLoads; ++l)
        if (16 * (tid + kThreads * l) < wn.need) *reinterpret_cast<u32x4*>(&win[buf][4 * (tid + kThreads * l)]) = r[l];
      if (tid < T.nrows) rowrel[buf][tid] = rr;
      const Win w = wn;
      if (q + 1 < nch) fetch(q + 1, r, rr, wn);
      // one barrier per channel: the buffer written next was last read
      // before this barrier
      __syncthreads();
      const uint32_t* wb = win[buf];
#pragma unroll
      for (int n = 0; n < kBurstMaxOut; ++n) {
        const int d = desc[n];  // -1 from n = nper on
        if (d >= 0) {
          int a = (d & 0xffff) + rowrel[buf][d >> 16] + w.shift;
          int b = a + f;
          a = max(a, w.lo);
          b = min(b, w.hi);
          if (b > a) {
            cnt[n] += b - a;
            int s = acc[n];
            for (int k = (a >> 2) + g; 4 * k < b; k += G) {
              const int first = max(a - 4 * k, 0), last = min(b - 4 * k, 4);  // bytes [first, last) of the dword
              uint32_t m = last >= 4 ? 0xffffffffu : ((1u << (8 * last)) - 1u);
              m &= 0xffffffffu << (8 * first);
              s = __builtin_amdgcn_sdot4(static_cast<int>(wb[k] & m), 0x01010101, s, false);
            }
            acc[n] = s;
          }
        }
      }
    }
  }

  // the group's partials; every lane of it holds the same count
#pragma unroll
  for (int n = 0; n < kBurstMaxOut; ++n) {
    int s = acc[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      if (o < G) s += __shfl_xor(s, o, dev::kWave);  // uniform
    if (g == 0 && desc[n] >= 0) {
      const int o = n * ngroups + grp;
      const int row = o / nb;
      const uint64_t at =
          (static_cast<uint64_t>(T.cand) * nrows_out + T.row0 + row) * static_cast<uint64_t>(ntime) + kb + (o - row * nb);
      sums[at] = s + bias * cnt[n];
      hits[at] = cnt[n];
    }
  }
}

}  // namespace

void burst_cube(const int8_t* chan_major, const BurstGeom& g, const int32_t* d_active, const BurstTile* d_tiles,
                uint32_t ntiles, const BurstJob* d_jobs, const int32_t* d_rel, const int32_t* d_win, int bin_tiles,
                int32_t* d_sums, int32_t* d_hits, hipStream_t s) {
  PSOUP_CHECK((g.stride & 15) == 0 && (reinterpret_cast<uintptr_t>(chan_major) & 15) == 0,
              "burst cube: rows must be 16-byte aligned");
  PSOUP_CHECK(g.nsamps <= g.stride && g.stride < (uint64_t(1) << 62), "burst cube: rows shorter than their valid length");
  PSOUP_CHECK(g.ntime >= 1 && g.nrows >= 1 && g.nchans >= 1, "burst cube: empty geometry");
  PSOUP_CHECK(ntiles >= 1 && bin_tiles >= 1 && bin_tiles <= 65535, "burst cube: bad launch plan");
  const dim3 grid(ntiles, static_cast<unsigned>(bin_tiles));
  burst_cube_kernel<<<grid, kThreads, 0, s>>>(chan_major, g.stride, static_cast<int64_t>(g.nsamps), g.bias, g.ntime,
                                              g.nrows, d_active, d_tiles, d_jobs, d_rel, d_win, d_sums, d_hits);
  post_launch_check("burst_cube_kernel", s);
}

}  // namespace kern
}  // namespace psoup
