// fits2fil kernel (psoup/psrfits.hpp): the packed DATA bytes of PSRFITS rows,
// with their per-row scale, offset and weight tables, to float32 samples
// [count][nchan] time-major.  Compiled without FMA contraction: a sample is
// the definition's four (six with two polarisations) correctly rounded double
// operations and one rounding to float.
//
// fits_decode: lanes run along the channels.  A thread owns a group of 8
// adjacent channels, which is NBITS bytes per polarisation in one load (16-byte
// loads at 16 bits, down to one byte at 1 bit) and 32 bytes per sample in two
// 16-byte stores; a wave covers 512 adjacent channels.  A workgroup of four
// waves takes 64 groups x 128 samples of one row slot: each wave walks every
// fourth sample, so a thread converts its group's scale, offset and weight to
// double once and keeps them in registers for 32 samples.  grid = (groups / 64,
// slots, NSBLK / 128).  A dropped slot is filled with NaN without a load.  The
// last group of a row may hold fewer than 8 channels (NCHAN not a multiple of
// 8): it, and every group when the rows are not aligned for the wide accesses,
// goes through byte loads and scalar stores.
#include <algorithm>

#include "device_common.hpp"
#include "psoup/psrfits.hpp"

namespace psoup {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kQuietNaN = 0x7fc00000u;
constexpr int G = kFitsGroup;
constexpr int kLanes = 64;                       // groups along the channels per workgroup
constexpr int kRows = kFitsThreads / kLanes;     // samples in flight per workgroup

// double(x) without a floating-point instruction touching a subnormal float
// (whatever the kernel's denormal mode): a subnormal is mant x 2^-149.
__device__ __forceinline__ double exact_double(float x) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7f800000u) != 0u) return static_cast<double>(x);
  const double m = static_cast<double>(static_cast<int>(b & 0x007fffffu)) * 0x1p-149;
  return (b >> 31) ? -m : m;
}

// The bits of float32(v), round to nearest even, without a floating-point
// instruction producing a subnormal float: below 2^-126 the mantissa is
// rint(|v| 2^149), an exact scaling and one rounding (2^23 is the smallest
// normal's encoding).  A NaN gives the quiet NaN of the definition.
__device__ __forceinline__ uint32_t exact_float_bits(double v) {
  if (v != v) return kQuietNaN;
  const double a = fabs(v);
  if (a < 0x1p-126) {
    const uint32_t sign = static_cast<uint32_t>(__double2hiint(v)) & 0x80000000u;
    return sign | static_cast<uint32_t>(rint(a * 0x1p149));
  }
  return __float_as_uint(static_cast<float>(v));
}

// The NB bytes of a group at p: one load when `wide`, else nb <= NB byte loads.
template <int NB>
__device__ __forceinline__ void load_bytes(const uint8_t* p, bool wide, int nb, uint8_t (&b)[NB]) {
  if (wide) {
    if constexpr (NB == 16) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p);
      __builtin_memcpy(b, &v, 16);
    } else if constexpr (NB == 8) {
      const u32x2 v = *reinterpret_cast<const u32x2*>(p);
      __builtin_memcpy(b, &v, 8);
    } else if constexpr (NB == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
      __builtin_memcpy(b, &v, 4);
    } else if constexpr (NB == 2) {
      const uint16_t v = *reinterpret_cast<const uint16_t*>(p);
      __builtin_memcpy(b, &v, 2);
    } else {
      b[0] = p[0];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NB; ++i) b[i] = i < nb ? p[i] : static_cast<uint8_t>(0);
  }
}

// Channel i of a group from its NBITS bytes: most-significant bits first below
// 8 bits, big-endian at 16.
template <int NBITS>
__device__ __forceinline__ int raw_value(const uint8_t (&b)[NBITS], int i, bool is_signed) {
  if constexpr (NBITS == 1) {
    return (b[0] >> (7 - i)) & 1;
  } else if constexpr (NBITS == 2) {
    return (b[i >> 2] >> (6 - 2 * (i & 3))) & 3;
  } else if constexpr (NBITS == 4) {
    return (b[i >> 1] >> ((i & 1) ? 0 : 4)) & 15;
  } else if constexpr (NBITS == 8) {
    return is_signed ? static_cast<int>(static_cast<int8_t>(b[i])) : static_cast<int>(b[i]);
  } else {
    const uint32_t v = (static_cast<uint32_t>(b[2 * i]) << 8) | static_cast<uint32_t>(b[2 * i + 1]);
    return is_signed ? static_cast<int>(static_cast<int16_t>(v)) : static_cast<int>(v);
  }
}

template <int NBITS, bool TWO>
__global__ void __launch_bounds__(kFitsThreads)
    fits_decode_kernel(FitsDecodeArgs a, uint64_t k0, uint64_t t0, uint64_t count, float* __restrict__ out, int wide_in,
                       int wide_out) {
  const int lane = threadIdx.x % kLanes;
  const int ty = threadIdx.x / kLanes;
  const int c0 = (static_cast<int>(blockIdx.x) * kLanes + lane) * G;  // this thread's first channel
  if (c0 >= a.nchan) return;
  const int nv = min(G, a.nchan - c0);  // channels of the group (a tail group is short)
  const uint64_t k = k0 + blockIdx.y;   // the row slot
  const int row = a.slot_row[blockIdx.y];
  const int s_begin = static_cast<int>(blockIdx.z) * kFitsBlockSamples;
  const int s_end = min(a.nsblk, s_begin + kFitsBlockSamples);
  const uint64_t nchan = static_cast<uint64_t>(a.nchan);

  double sa[G], oa[G], sb[G], ob[G], w[G];
  uint32_t dead = 0u;  // bit i: WTS == 0
#pragma unroll
  for (int i = 0; i < G; ++i) {
    sa[i] = oa[i] = sb[i] = ob[i] = w[i] = 0.0;
    if (row >= 0 && i < nv) {
      const uint64_t r = static_cast<uint64_t>(row);
      const uint64_t ia = (r * static_cast<uint64_t>(a.npol) + static_cast<uint64_t>(a.pol_a)) * nchan + c0 + i;
      sa[i] = exact_double(a.scl[ia]);
      oa[i] = exact_double(a.offs[ia]);
      if constexpr (TWO) {
        const uint64_t ib = (r * static_cast<uint64_t>(a.npol) + static_cast<uint64_t>(a.pol_b)) * nchan + c0 + i;
        sb[i] = exact_double(a.scl[ib]);
        ob[i] = exact_double(a.offs[ib]);
      }
      const float wt = a.wts[r * nchan + c0 + i];
      if (wt == 0.0f) dead |= 1u << i;
      w[i] = exact_double(wt);
    }
  }

  const uint64_t sbytes = nchan * static_cast<uint64_t>(NBITS) / 8;  // one polarisation of one sample
  const int nb = nv * NBITS / 8;                                     // bytes of this group
  const bool wide_load = wide_in != 0 && nv == G;
  const bool wide_store = wide_out != 0 && nv == G;
  const bool is_signed = a.is_signed != 0;
  const uint8_t* base = nullptr;
  if (row >= 0)
    base = a.data + static_cast<uint64_t>(row) * (static_cast<uint64_t>(a.nsblk) * static_cast<uint64_t>(a.npol) * sbytes) +
           static_cast<uint64_t>(c0) * NBITS / 8;

  for (int s = s_begin + ty; s < s_end; s += kRows) {
    const uint64_t t = k * static_cast<uint64_t>(a.nsblk) + static_cast<uint64_t>(s);
    if (t < t0 || t >= t0 + count) continue;
    uint32_t o[G];
    if (row < 0) {
#pragma unroll
      for (int i = 0; i < G; ++i) o[i] = kQuietNaN;
    } else {
      const uint64_t sp = static_cast<uint64_t>(s) * static_cast<uint64_t>(a.npol);
      uint8_t ba[NBITS], bb[NBITS];
      load_bytes<NBITS>(base + (sp + static_cast<uint64_t>(a.pol_a)) * sbytes, wide_load, nb, ba);
      if constexpr (TWO) load_bytes<NBITS>(base + (sp + static_cast<uint64_t>(a.pol_b)) * sbytes, wide_load, nb, bb);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const double da = static_cast<double>(raw_value<NBITS>(ba, i, is_signed)) - a.z;
        const double pa = da * sa[i];
        double u = pa + oa[i];
        if constexpr (TWO) {
          const double db = static_cast<double>(raw_value<NBITS>(bb, i, is_signed)) - a.z;
          const double pb = db * sb[i];
          const double ub = pb + ob[i];
          u = u + ub;
        }
        const double v = u * w[i];
        o[i] = ((dead >> i) & 1u) ? kQuietNaN : exact_float_bits(v);
      }
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (t - t0) * nchan + static_cast<uint64_t>(c0);
    if (wide_store) {
      *reinterpret_cast<u32x4*>(dst) = u32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<u32x4*>(dst + 4) = u32x4{o[4], o[5], o[6], o[7]};
    } else {
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (i < nv) dst[i] = o[i];
    }
  }
}

template <int NBITS>
void launch(const FitsDecodeArgs& a, uint64_t k0, uint64_t t0, uint64_t count, float* out, const dim3& grid,
            int wide_in, int wide_out, hipStream_t s) {
  if (a.pol_b >= 0)
    fits_decode_kernel<NBITS, true><<<grid, kFitsThreads, 0, s>>>(a, k0, t0, count, out, wide_in, wide_out);
  else
    fits_decode_kernel<NBITS, false><<<grid, kFitsThreads, 0, s>>>(a, k0, t0, count, out, wide_in, wide_out);
  post_launch_check("fits_decode_kernel", s);
}

}  // namespace

int fits_decode(const FitsDecodeArgs& args, uint64_t t0, uint64_t count, float* out, hipStream_t s) {
  PSOUP_CHECK(out != nullptr && count >= 1, "fits_decode: empty output");
  PSOUP_CHECK(args.slot_row != nullptr, "fits_decode: no slot table");
  PSOUP_CHECK(args.nsblk >= 1 && args.npol >= 1 && args.nchan >= 1 && args.nrows >= 0, "fits_decode: bad shape");
  PSOUP_CHECK(args.nbits == 1 || args.nbits == 2 || args.nbits == 4 || args.nbits == 8 || args.nbits == 16,
              "fits_decode: NBITS must be 1, 2, 4, 8 or 16, got " << args.nbits);
  PSOUP_CHECK((static_cast<uint64_t>(args.nchan) * static_cast<uint64_t>(args.nbits)) % 8 == 0,
              "fits_decode: NCHAN x NBITS must be a multiple of 8");
  PSOUP_CHECK(args.pol_a >= 0 && args.pol_a < args.npol && args.pol_b < args.npol,
              "fits_decode: polarisation out of range");
  PSOUP_CHECK(args.nrows == 0 || (args.data != nullptr && args.scl != nullptr && args.offs != nullptr && args.wts != nullptr),
              "fits_decode: rows without their data or tables");
  PSOUP_CHECK((reinterpret_cast<uintptr_t>(out) & 3) == 0, "fits_decode: out must be aligned to float");
  const uint64_t nsblk = static_cast<uint64_t>(args.nsblk);
  const uint64_t k_first = t0 / nsblk, k_last = (t0 + count - 1) / nsblk;
  const int wide_in = (reinterpret_cast<uintptr_t>(args.data) & 15) == 0 && args.nchan % G == 0;
  const int wide_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && args.nchan % G == 0;
  const unsigned gx = static_cast<unsigned>((args.nchan + G * kLanes - 1) / (G * kLanes));
  const unsigned gz = static_cast<unsigned>((args.nsblk + kFitsBlockSamples - 1) / kFitsBlockSamples);
  PSOUP_CHECK(gz <= 65535, "fits_decode: NSBLK too large");
  int launches = 0;
  for (uint64_t k0 = k_first; k0 <= k_last; k0 += kFitsMaxSlots) {
    const uint64_t k1 = std::min<uint64_t>(k_last, k0 + kFitsMaxSlots - 1);
    // the samples of [t0, t0 + count) in slots k0 .. k1
    const uint64_t ta = std::max(t0, k0 * nsblk), tb = std::min(t0 + count, (k1 + 1) * nsblk);
    FitsDecodeArgs a = args;
    a.slot_row = args.slot_row + (k0 - k_first);
    const dim3 grid(gx, static_cast<unsigned>(k1 - k0 + 1), gz);
    float* o = out + (ta - t0) * static_cast<uint64_t>(args.nchan);
    switch (args.nbits) {
      case 1: launch<1>(a, k0, ta, tb - ta, o, grid, wide_in, wide_out, s); break;
      case 2: launch<2>(a, k0, ta, tb - ta, o, grid, wide_in, wide_out, s); break;
      case 4: launch<4>(a, k0, ta, tb - ta, o, grid, wide_in, wide_out, s); break;
      case 8: launch<8>(a, k0, ta, tb - ta, o, grid, wide_in, wide_out, s); break;
      default: launch<16>(a, k0, ta, tb - ta, o, grid, wide_in, wide_out, s); break;
    }
    ++launches;
  }
  return launches;
}

}  // namespace kern
}  // namespace psoup
