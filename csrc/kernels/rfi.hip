// RFI excision kernels (psoup/rfi.hpp): exact block sums of the channel-major
// int8 rows, the mask / zero-DM apply pass, and the corner turn back to packed
// SIGPROC bytes.  All stores are ordinary vector stores; no atomics.
#include "device_common.hpp"
#include "psoup/rfi.hpp"

namespace psoup {
namespace kern {

namespace {

// ------------------------------------------------------------ block sums ----
// One workgroup per channel and run of blocks; each wave sums one block at a
// time: 16-byte loads (64 lanes x 16 B = 1024 samples per step), sum x' and
// sum x'^2 of the stored int8 values x' = x - bias by the 4-way int8 dot
// product into int32 partials per lane.  Bounds per lane and block, at the
// longest block L = 65536 (64 steps): |sum x'| <= 64 * 16 * 128 = 2^17 and
// sum x'^2 <= 64 * 16 * 128^2 = 2^24; over the whole block |sum x'| <= 2^23
// and sum x'^2 <= 2^30, so the cross-lane reduction stays in int32 too.  The
// bias correction to raw sums is exact in 64 bits:
//   S1 = S1' + bias len,  S2 = S2' + 2 bias S1' + bias^2 len.
constexpr int kSumsWaves = 4;

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, dev::kWave);
  return v;
}

// keeps the low `valid` (0..4) bytes of a word
__device__ __forceinline__ int keep_bytes(int w, int valid) {
  if (valid >= 4) return w;
  if (valid <= 0) return 0;
  return w & ((1 << (8 * valid)) - 1);
}

__global__ void __launch_bounds__(kSumsWaves* dev::kWave)
    rfi_block_sums_kernel(const int8_t* __restrict__ rows, uint64_t stride, uint64_t nsamps, uint32_t L, uint32_t nblk,
                          uint32_t run, int bias, uint64_t* __restrict__ S1, uint64_t* __restrict__ S2) {
  const int lane = threadIdx.x & (dev::kWave - 1);
  const uint32_t wave = threadIdx.x / dev::kWave;
  const uint32_t c = blockIdx.y;
  const int8_t* row = rows + static_cast<uint64_t>(c) * stride;
  const uint32_t b_end = min(nblk, (blockIdx.x + 1) * run);
  for (uint32_t b = blockIdx.x * run + wave; b < b_end; b += kSumsWaves) {
    const uint64_t t0 = static_cast<uint64_t>(b) * L;
    const uint32_t len = static_cast<uint32_t>(min<uint64_t>(L, nsamps - t0));
    const int4* src = reinterpret_cast<const int4*>(row + t0);  // 16-byte aligned: stride and L are multiples of 16
    int a1 = 0, a2 = 0;
#pragma unroll 4
    for (uint32_t i = static_cast<uint32_t>(lane) * 16; i < len; i += dev::kWave * 16) {
      // the row's stride covers the 16 bytes around a short tail; mask them
      int4 v = src[i >> 4];
      const int rem = static_cast<int>(len - i);
      if (rem < 16) {
        v.x = keep_bytes(v.x, rem);
        v.y = keep_bytes(v.y, rem - 4);
        v.z = keep_bytes(v.z, rem - 8);
        v.w = keep_bytes(v.w, rem - 12);
      }
      a1 = __builtin_amdgcn_sdot4(v.x, 0x01010101, a1, false);
      a1 = __builtin_amdgcn_sdot4(v.y, 0x01010101, a1, false);
      a1 = __builtin_amdgcn_sdot4(v.z, 0x01010101, a1, false);
      a1 = __builtin_amdgcn_sdot4(v.w, 0x01010101, a1, false);
      a2 = __builtin_amdgcn_sdot4(v.x, v.x, a2, false);
      a2 = __builtin_amdgcn_sdot4(v.y, v.y, a2, false);
      a2 = __builtin_amdgcn_sdot4(v.z, v.z, a2, false);
      a2 = __builtin_amdgcn_sdot4(v.w, v.w, a2, false);
    }
    a1 = wave_sum_i32(a1);
    a2 = wave_sum_i32(a2);
    if (lane == 0) {
      const int64_t s1 = a1, s2 = a2, bl = static_cast<int64_t>(bias), n = len;
      const uint64_t o = static_cast<uint64_t>(c) * nblk + b;
      S1[o] = static_cast<uint64_t>(s1 + bl * n);
      S2[o] = static_cast<uint64_t>(s2 + 2 * bl * s1 + bl * bl * n);
    }
  }
}

// ----------------------------------------------------------------- apply ----
// One workgroup (16 waves) per tile of kRfiTile = 256 samples, which lies in
// one block b.  A wave covers 4 rows x 256 B per load: lane = (r, j), row r of
// the group, samples [16 j, 16 j + 16) of the tile.  Sweep 1 sums the
// unflagged rows' samples into 16 int32 registers per lane (|Z'| <= 32768 *
// 128 = 2^22), reduces them over the 4 row lanes by shuffles and over the 16
// waves through LDS, and forms delta_t = G_b - zbar_t.  Sweep 2 re-reads the
// rows and stores y.  Without zero-DM sweep 1 is skipped and only flagged
// cells are written (out of place: the rest is copied).
constexpr int kApplyWaves = 16;
constexpr int kApplyThreads = kApplyWaves * dev::kWave;
constexpr int kRowsPerStep = kApplyWaves * 4;  // 64
constexpr int kUnroll = 4;

__device__ __forceinline__ void add_bytes(int (&z)[16], const int4& v) {
  const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    z[4 * k + 0] += static_cast<int8_t>(w[k]);
    z[4 * k + 1] += static_cast<int8_t>(w[k] >> 8);
    z[4 * k + 2] += static_cast<int8_t>(w[k] >> 16);
    z[4 * k + 3] += w[k] >> 24;
  }
}

__device__ __forceinline__ int4 shift_clamp(const int4& v, const int (&delta)[16], int bias, int vmax) {
  const int w[4] = {v.x, v.y, v.z, v.w};
  int o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = static_cast<int8_t>(w[k] >> (8 * q)) + bias;  // raw
      const int y = min(max(x + delta[4 * k + q], 0), vmax) - bias;
      acc |= (y & 0xff) << (8 * q);
    }
    o[k] = acc;
  }
  return make_int4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ void store16(int8_t* dst, const int4& v, uint64_t t, uint64_t nsamps) {
  if (t + 16 <= nsamps) {
    *reinterpret_cast<int4*>(dst) = v;
  } else {  // the row's tail: bytes past nsamps stay as they are
    const int w[4] = {v.x, v.y, v.z, v.w};
    for (int q = 0; q < 16; ++q)
      if (t + q < nsamps) dst[q] = static_cast<int8_t>(w[q >> 2] >> (8 * (q & 3)));
  }
}

template <bool ZeroDm>
__global__ void __launch_bounds__(kApplyThreads)
    rfi_apply_kernel(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans, uint64_t nsamps,
                     uint32_t L, int bias, int vmax, const uint8_t* __restrict__ cell_t,
                     const int32_t* __restrict__ fill, const int32_t* __restrict__ G, const int32_t* __restrict__ nb,
                     const int32_t* __restrict__ nflag) {
  extern __shared__ uint8_t flg[];  // nchans flag bytes of block b
  __shared__ int zpart[ZeroDm ? kApplyWaves : 1][kRfiTile];
  __shared__ int delta_s[kRfiTile];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kRfiTile;
  const uint32_t b = static_cast<uint32_t>(t0 / L);
  const bool in_place = (rows == dst);
  if (!ZeroDm && in_place && nflag[b] == 0) return;  // uniform: nothing to write in this tile
  for (int i = threadIdx.x; i < nchans; i += kApplyThreads) flg[i] = cell_t[static_cast<uint64_t>(b) * nchans + i];
  __syncthreads();
  const int lane = threadIdx.x & (dev::kWave - 1);
  const int wave = threadIdx.x / dev::kWave;
  const int r = lane >> 4, j = lane & 15;
  const uint64_t t = t0 + static_cast<uint64_t>(j) * 16;
  const bool in = t < nsamps;  // the 16-byte group holds a sample (its load stays inside the stride)
  const int cfirst = wave * 4 + r;
  int delta[16];
  if (ZeroDm) {
    int z[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) z[q] = 0;
    for (int c0 = cfirst; c0 < nchans; c0 += kRowsPerStep * kUnroll) {
      int4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * kRowsPerStep;
        const bool on = in && c < nchans && flg[min(c, nchans - 1)] == 0;
        v[u] = on ? *reinterpret_cast<const int4*>(rows + static_cast<uint64_t>(c) * stride + t) : make_int4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) add_bytes(z, v[u]);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      z[q] += __shfl_xor(z[q], 16, dev::kWave);
      z[q] += __shfl_xor(z[q], 32, dev::kWave);
    }
    if (r == 0) {
#pragma unroll
      for (int q = 0; q < 16; ++q) zpart[wave][j * 16 + q] = z[q];
    }
    __syncthreads();
    if (threadIdx.x < kRfiTile) {
      int zs = 0;
#pragma unroll
      for (int w = 0; w < kApplyWaves; ++w) zs += zpart[w][threadIdx.x];
      const int n = nb[b];
      const int Z = zs + n * bias;  // raw band sum, >= 0
      const int zbar = n > 0 ? (2 * Z + n) / (2 * n) : 0;
      delta_s[threadIdx.x] = G[b] - zbar;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) delta[q] = delta_s[j * 16 + q];
  }
  if (!in) return;
  for (int c = cfirst; c < nchans; c += kRowsPerStep) {
    int8_t* out = dst + static_cast<uint64_t>(c) * dst_stride + t;
    if (flg[c]) {
      const int f = (fill[c] - bias) & 0xff;
      const int w = f * 0x01010101;
      store16(out, make_int4(w, w, w, w), t, nsamps);
    } else if (ZeroDm) {
      const int4 v = *reinterpret_cast<const int4*>(rows + static_cast<uint64_t>(c) * stride + t);
      store16(out, shift_clamp(v, delta, bias, vmax), t, nsamps);
    } else if (!in_place) {
      store16(out, *reinterpret_cast<const int4*>(rows + static_cast<uint64_t>(c) * stride + t), t, nsamps);
    }
  }
}

// -------------------------------------------------------- pack transpose ----
// Tile: 64 channels x 256 samples through LDS (the unpack's corner turn run
// backwards): 64-byte row segments in, one sample's packed bytes out per
// thread.
constexpr int TS = 256;
constexpr int TC = 64;
constexpr int LDS_ROW = TS + 16;

__global__ void __launch_bounds__(256)
    pack_transpose_kernel(const int8_t* __restrict__ rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits,
                          int bias, uint8_t* __restrict__ packed) {
  __shared__ __attribute__((aligned(16))) int8_t tile[TC * LDS_ROW];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * TS;
  const int c0 = blockIdx.y * TC;
  {
    const int row = threadIdx.x >> 2;
    const int seg = threadIdx.x & 3;
    const int c = c0 + row;
    const uint64_t tbeg = t0 + seg * 64;
    if (c < nchans && tbeg < nsamps) {
      const int8_t* src = rows + static_cast<uint64_t>(c) * stride + tbeg;
      int8_t* dstl = tile + row * LDS_ROW + seg * 64;
      if (tbeg + 64 <= nsamps && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<int4*>(dstl)[q] = reinterpret_cast<const int4*>(src)[q];
      } else {
        for (int q = 0; q < 64; ++q)
          if (tbeg + q < nsamps) dstl[q] = src[q];
      }
    }
  }
  __syncthreads();
  const uint64_t t = t0 + threadIdx.x;
  if (t >= nsamps) return;
  const uint64_t bps = static_cast<uint64_t>(nchans) * nbits / 8;
  const int mask = (1 << nbits) - 1;
  const int per_byte = 8 / nbits;
  const int nc = min(TC, nchans - c0);
  const int nbytes = nc * nbits / 8;  // whole bytes: c0 and nchans * nbits are multiples of 8 bits
  uint8_t* dst = packed + t * bps + (static_cast<uint64_t>(c0) * nbits) / 8;
  auto byte_at = [&](int bidx) -> uint32_t {
    uint32_t v = 0;
    for (int q = 0; q < per_byte; ++q) {
      const int c = bidx * per_byte + q;
      v |= static_cast<uint32_t>((tile[c * LDS_ROW + threadIdx.x] + bias) & mask) << (q * nbits);
    }
    return v;
  };
  int bdone = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    for (; bdone + 4 <= nbytes; bdone += 4) {
      const uint32_t w =
          byte_at(bdone) | (byte_at(bdone + 1) << 8) | (byte_at(bdone + 2) << 16) | (byte_at(bdone + 3) << 24);
      *reinterpret_cast<uint32_t*>(dst + bdone) = w;
    }
  }
  for (; bdone < nbytes; ++bdone) dst[bdone] = static_cast<uint8_t>(byte_at(bdone));
}

void check_rows(const void* p, uint64_t stride, uint64_t nsamps, const char* what) {
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride % 16 == 0 && stride >= nsamps,
              what << ": rows must be 16-byte aligned with a stride that is a multiple of 16 and >= nsamps");
}

}  // namespace

void rfi_block_sums(const int8_t* rows, uint64_t stride, int nchans, uint64_t nsamps, uint64_t block, int bias,
                    uint64_t* S1, uint64_t* S2, hipStream_t s) {
  PSOUP_CHECK(block >= 256 && block <= 65536 && block % 256 == 0, "rfi block must be a multiple of 256 in [256, 65536]");
  PSOUP_CHECK(nchans > 0 && nchans <= 65535 && nsamps > 0, "rfi_block_sums: empty input or too many channels");
  PSOUP_CHECK(bias >= 0 && bias <= 128, "rfi_block_sums: bias");
  check_rows(rows, stride, nsamps, "rfi_block_sums");
  const uint64_t nblk = (nsamps + block - 1) / block;
  PSOUP_CHECK(nblk < (1ull << 31), "rfi_block_sums: too many blocks");
  // at least 64 KiB of a row per workgroup
  const uint32_t run = kSumsWaves * static_cast<uint32_t>(std::max<uint64_t>(1, 16384 / block));
  dim3 grid(static_cast<unsigned>((nblk + run - 1) / run), static_cast<unsigned>(nchans));
  rfi_block_sums_kernel<<<grid, kSumsWaves * dev::kWave, 0, s>>>(rows, stride, nsamps, static_cast<uint32_t>(block),
                                                                 static_cast<uint32_t>(nblk), run, bias, S1, S2);
  post_launch_check("rfi_block_sums_kernel", s);
}

void rfi_apply(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans, uint64_t nsamps,
               uint64_t block, int nbits, int bias, bool zero_dm, const uint8_t* cell_t, const int32_t* fill,
               const int32_t* G, const int32_t* nb, const int32_t* nflag, hipStream_t s) {
  PSOUP_CHECK(block >= 256 && block <= 65536 && block % kRfiTile == 0, "rfi block must be a multiple of 256 in [256, 65536]");
  PSOUP_CHECK(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8, "nbits must be 1/2/4/8");
  PSOUP_CHECK(nchans > 0 && nchans <= kRfiMaxChans && nsamps > 0, "rfi_apply: 1.." << kRfiMaxChans << " channels");
  PSOUP_CHECK(bias >= 0 && bias <= 128, "rfi_apply: bias");
  check_rows(rows, stride, nsamps, "rfi_apply");
  check_rows(dst, dst_stride, nsamps, "rfi_apply (dst)");
  const uint64_t tiles = (nsamps + kRfiTile - 1) / kRfiTile;
  PSOUP_CHECK(tiles < (1ull << 31), "rfi_apply: too many samples");
  const int vmax = (1 << nbits) - 1;
  const unsigned grid = static_cast<unsigned>(tiles);
  const size_t lds = (static_cast<size_t>(nchans) + 15) / 16 * 16;
  if (zero_dm)
    rfi_apply_kernel<true><<<grid, kApplyThreads, lds, s>>>(rows, stride, dst, dst_stride, nchans, nsamps,
                                                          static_cast<uint32_t>(block), bias, vmax, cell_t, fill, G, nb,
                                                          nflag);
  else
    rfi_apply_kernel<false><<<grid, kApplyThreads, lds, s>>>(rows, stride, dst, dst_stride, nchans, nsamps,
                                                           static_cast<uint32_t>(block), bias, vmax, cell_t, fill, G, nb,
                                                           nflag);
  post_launch_check("rfi_apply_kernel", s);
}

void pack_transpose(const int8_t* rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias,
                    uint8_t* packed, hipStream_t s) {
  PSOUP_CHECK(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8, "nbits must be 1/2/4/8");
  PSOUP_CHECK((static_cast<uint64_t>(nchans) * nbits) % 8 == 0, "nchans*nbits must be a multiple of 8");
  PSOUP_CHECK(stride >= nsamps, "stride too small");
  if (nsamps == 0) return;
  const uint64_t gx = (nsamps + TS - 1) / TS;
  PSOUP_CHECK(gx < (1ull << 31), "too many samples");
  dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>((nchans + TC - 1) / TC));
  pack_transpose_kernel<<<grid, 256, 0, s>>>(rows, stride, nsamps, nchans, nbits, bias, packed);
  post_launch_check("pack_transpose_kernel", s);
}

}  // namespace kern
}  // namespace psoup
