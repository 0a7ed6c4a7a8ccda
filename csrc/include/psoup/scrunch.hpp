// filscrunch: subband and time-scrunch a filterbank on the device into an
// ordinary 8-bit SIGPROC file, an extension beyond the reference.  Kernels in
// csrc/kernels/scrunch.hip, the host steps (offsets, scale, plan) in
// csrc/src/scrunch_host.cpp, Scruncher and the file pipeline in
// csrc/src/scrunch.cpp, CLI bin/filscrunch (csrc/apps/scrunch_main.cpp).
//
// Definition.  Raw samples x[c][t] in 0..V, V = 2^nbits - 1, c < nchans,
// t < nsamps; the device rows hold x - bias.  Input killmask k[c] (0 = killed).
// foff must be negative (the delay table is only meaningful for that channel
// order).  Parameters: dm (float, >= 0), nsub in 1..nchans dividing nchans
// (w = nchans / nsub), f = tscrunch in 1..256, sigma_out > 0 (default 16).
//
// 1. Offsets: off[c] = dm_delay_samples(dm, delays[c]) with the delay table of
//    DedispGeometry::make; c_s = s w is the first (highest-frequency) channel
//    of subband s; rel[c] = off[c] - off[c_s] >= 0 for c in subband s;
//    R = max rel[c]; nout = floor((nsamps - R) / f), refused if nout < 1.
// 2. Sums (device), u < nout:
//      A[s][u] = sum over unkilled c in subband s, i in [0, f) of x[c][f u + i + rel[c]]   (int32)
//    nactive[s] = unkilled channels of s.  Bound, checked before any launch:
//    V f max_s nactive[s] < 2^26.  Every read is inside [0, nsamps).
// 3. Block sums (device): L = 4096 output samples per block, nblk =
//    ceil(nout / L), the last block may be short; S1[s][b] = sum A,
//    S2[s][b] = sum A^2, exact, as uint64 (A^2 L < 2^64).
// 4. Scale (host, double, only correctly rounded operations on exact integers,
//    no FMA contraction): m = S1 / len_b; v = (len_b S2 - S1^2) / len_b^2 with
//    the numerator formed exactly in 128-bit integers and converted to double
//    once.  Per subband med_m, med_v = medians over its blocks (an even count
//    takes the mean of the two middle values, as numpy.median).
//    M[s] = floor(med_m + 0.5).  A subband is live if nactive[s] > 0 and
//    med_v > 0.  sigma_ref = median over live s of sqrt(med_v); no live
//    subband is refused.
//      mul = clamp(floor(sigma_out / sigma_ref * 65536 + 0.5), 1, 2^31 - 1)
//    One scale for the file, one offset per subband: the band sum of the
//    output keeps the channel weights of a plain dedispersion at dm.
// 5. Requantise (device, int64):
//      y[s][u] = clamp(((int64(A[s][u] - M[s]) * mul + 32768) >> 16) + 128, 0, 255)
//    (arithmetic shift: it floors).  A subband that is not live gives 128
//    everywhere and is 0 in the output killmask.
// 6. Output: a SIGPROC .fil with nbits = 8, samples y[s][u] time-major
//    (pack_transpose).  Every header key of the input is written again with
//    nchans = nsub, foff = w foff, tsamp = f tsamp, nbits = 8, nsamples = nout
//    (where the key was present) and refdm = dm; fch1 is unchanged: channel s
//    of the output sits at the frequency of c_s, the channel its subband was
//    aligned to, so a downstream tool's own delay table is the right one.
//    Written to a temporary file and renamed.
// 7. Plan (host only): nu = centre of the lowest channel in GHz,
//      unit = tsamp * (nu * nu * nu) / (8.3e-6 * |foff_MHz|)     (the DM at which t_ch = tsamp)
//    t_ch(d) = d tsamp / unit; the factor at DM d is the largest power of two
//    <= max(1, d / unit), capped at 64.  Tier 2^k covers [dm_lo, dm_hi) with
//    dm_lo = 2^k unit (0 for k = 0) and dm_hi the next tier's dm_lo; the tiers
//    over [0, D] end at D.
//
// The sums are recomputed rather than kept: Scruncher::run makes one pass for
// S1 / S2, the host step, and a second pass of sums + requantise per time
// chunk, so the int32 A of one chunk is all that is held (4 nsub bytes per
// output sample would otherwise be up to four times the input).  When the
// whole file is one chunk, A is kept from the first pass and not recomputed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/common.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kScrunchStatBlock = 4096;  // L: output samples per statistics block
constexpr int kScrunchTile = 2048;       // most output samples per workgroup
constexpr int kScrunchWindow = 12288;    // bytes of a channel staged in LDS per tile (x 2 buffers)
constexpr int kScrunchMaxF = 256;
constexpr int kScrunchThreads = 256;
constexpr int kScrunchMaxOut = 8;        // outputs per lane group
static_assert(kScrunchStatBlock % kScrunchTile == 0, "whole tiles per statistics block");

// lanes that share one output: a power of two in 1..32
inline int scrunch_lanes_log2(int f) {
  int lg = 0;
  while (lg < 5 && (16 << lg) <= f) ++lg;
  return lg;
}
// output samples per workgroup at scrunch factor f: the window holds them with
// up to 15 bytes of alignment in front
inline int scrunch_tile(int f) {
  const int fit = (kScrunchWindow - 16) / f;
  return fit < kScrunchTile ? fit : kScrunchTile;
}

// rows: int8 [nchans][stride] (x - bias), 16-byte aligned, stride a multiple
// of 16 and >= nsamps.  active: the unkilled channels in ascending order,
// sub_first [nsub + 1]: subband s owns active[sub_first[s] .. sub_first[s+1]).
// rel: int32 [nchans].  Output samples [u0, u0 + count) with u0 a multiple of
// L: A[s][u - u0] (int32 [nsub][a_stride]) by plain stores, and S1 / S2
// (uint64 [nsub][nblk], block index u / L) by 64-bit atomic adds: their cells
// must be zero before the launch.  Every source sample f u + i + rel[c] must
// lie inside [0, nsamps) (the caller's choice of nout).
void scrunch_sums(const int8_t* rows, uint64_t stride, uint64_t nsamps, int bias, int f, const int32_t* d_active,
                  const int32_t* d_sub_first, const int32_t* d_rel, int nsub, uint64_t u0, uint64_t count, int32_t* A,
                  uint64_t a_stride, uint64_t* S1, uint64_t* S2, uint64_t nblk, hipStream_t s);
// A: int32 [nsub][a_stride] (16-byte aligned, a_stride a multiple of 4), M
// int32 [nsub], live uint8 [nsub] -> y: int8 [nsub][y_stride] holding y - 128,
// 16-byte aligned with a stride that is a multiple of 16 (pack_transpose's
// layout); bytes [count, roundup16(count)) of a row are written as 0.
void scrunch_quant(const int32_t* A, uint64_t a_stride, int nsub, uint64_t count, const int32_t* d_M,
                   const uint8_t* d_live, int32_t mul, int8_t* y, uint64_t y_stride, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
struct ScrunchParams {
  float dm = 0.f;
  int nsub = 0;  // 0 = nchans
  int tscrunch = 1;
  double sigma_out = 16.0;
};
// Throws by name unless dm >= 0, nsub divides nchans (0 = nchans), tscrunch is
// in 1..256 and sigma_out > 0; returns the parameters with nsub filled in.
ScrunchParams scrunch_check_params(const ScrunchParams& p, int nchans);

// filscrunch options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct ScrunchCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string killfilename;
  std::string killoutfilename;  // --kill_out
  float dm = 0.f;
  int nsub = 0;  // 0 = nchans
  int tscrunch = 1;
  double sigma_out = 16.0;
  bool plan = false;
  double dm_end = -1.0;  // --plan only
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_filscrunch.fil" in UTC.
std::string default_scrunch_output_filename();
bool parse_scrunch_cmdline(ScrunchCmdLineOptions& args, const std::vector<std::string>& argv,
                           bool* exit_now = nullptr);
ScrunchParams scrunch_params_from(const ScrunchCmdLineOptions& args);

// ----------------------------------------------------------- host steps ----
struct ScrunchOffsets {
  std::vector<int32_t> rel;  // [nchans]
  int32_t R = 0;
};
// Step 1.  delays: float [nchans], non-decreasing within a subband (foff < 0).
ScrunchOffsets scrunch_offsets(float dm, const std::vector<float>& delays, int nsub);

struct ScrunchScale {
  std::vector<int32_t> M;     // [nsub]
  std::vector<uint8_t> live;  // [nsub]
  int32_t mul = 1;
  double sigma_ref = 0;
  int nlive = 0;
};
// Step 4 on the table of block sums S1, S2 [nsub][nblk], nblk = ceil(nout / L).
ScrunchScale scrunch_scale(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nsub, uint64_t nout,
                           const std::vector<int32_t>& nactive, double sigma_out);

struct ScrunchTier {
  double dm_lo = 0, dm_hi = 0;
  int tscrunch = 1;
};
// Step 7: the tiers over [0, dm_end].
std::vector<ScrunchTier> scrunch_plan(double tsamp, double fch1, double foff, int nchans, double dm_end);

// ------------------------------------------------------------ scruncher ----
struct ScrunchResult {
  uint64_t nout = 0, nblk = 0;
  int32_t R = 0;
  int nsub = 0, chunks = 0;
  std::vector<int32_t> rel, nactive;
  std::vector<uint64_t> S1, S2;  // [nsub][nblk], first pass
  ScrunchScale scale;
  std::vector<int> killmask;  // [nsub] output killmask (0 = not live)
};

class Scruncher {
 public:
  static constexpr size_t kDefaultBudgetBytes = size_t(1) << 30;
  // Raw rows: int8 [nchans][stride] at d_rows (x - bias), nsamps valid samples
  // per row, with explicit delays (float [nchans]) and killmask (int [nchans],
  // empty = none killed).  budget_bytes: device bytes the int32 sums of one
  // time chunk may hold (a chunk is at least L outputs).  Validates everything
  // (parameters, foff < 0, nout >= 1, the 2^26 bound, an unkilled channel) and
  // throws by name; launches and uploads nothing.
  Scruncher(const int8_t* d_rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias, double foff,
            const std::vector<float>& delays, const std::vector<int>& killmask, const ScrunchParams& p,
            hipStream_t stream, size_t budget_bytes = kDefaultBudgetBytes);
  // Steps 2 to 5 into d_y: int8 [nsub][y_stride] (y - 128), 16-byte aligned,
  // y_stride a multiple of 16 and >= nout.  Synchronises the stream.
  ScrunchResult run(int8_t* d_y, uint64_t y_stride);
  uint64_t nout() const { return nout_; }
  int nsub() const { return p_.nsub; }
  uint64_t chunk_outputs() const { return chunk_; }
  uint64_t launches() const { return nlaunch_; }  // kernel launches so far
  const std::vector<int32_t>& nactive() const { return nactive_; }

  // The two kernels alone with explicit host tables (the torch ops' path);
  // both synchronise the stream.  sums: every output of [0, nout) into d_A
  // (int32 [nsub][a_stride]) and d_S1 / d_S2 (uint64 [nsub][ceil(nout / L)]),
  // which it zeroes first; checks that every read stays inside the rows.
  static void sums(const int8_t* d_rows, uint64_t stride, uint64_t nsamps, int nchans, int bias, int f, int nsub,
                   const std::vector<int32_t>& rel, const std::vector<int>& killmask, uint64_t nout, int32_t* d_A,
                   uint64_t a_stride, uint64_t* d_S1, uint64_t* d_S2, hipStream_t stream);
  static void quant(const int32_t* d_A, uint64_t a_stride, int nsub, uint64_t nout, const std::vector<int32_t>& M,
                    const std::vector<uint8_t>& live, int32_t mul, int8_t* d_y, uint64_t y_stride, hipStream_t stream);

 private:
  const int8_t* x_;
  uint64_t stride_, nsamps_;
  int nchans_, nbits_, bias_;
  ScrunchParams p_;
  hipStream_t stream_;
  ScrunchOffsets off_;
  uint64_t nout_ = 0, chunk_ = 0;
  std::vector<int32_t> nactive_, active_, sub_first_;
  uint64_t nlaunch_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct ScrunchRun {
  ScrunchResult result;
  std::map<std::string, double> timers;  // reading, scrunching, writing, total (s)
};
// Reads the filterbank, applies the killfile, scrunches on the current device
// and writes the .fil (temporary file + rename) and, with --kill_out, the
// subband killfile in the -k format.
ScrunchRun run_scrunch_pipeline(const ScrunchCmdLineOptions& args);

}  // namespace psoup
