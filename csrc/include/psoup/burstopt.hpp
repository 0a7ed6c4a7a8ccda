// burstopt: a search over DM rows, boxcar widths and start bins on the burst
// cutouts of burstcube (what cubeopt is to foldcube), an extension beyond the
// reference.  Kernel in csrc/kernels/burstopt.hip, the host steps in
// csrc/src/burstopt_host.cpp (no device code), BurstOptimiser / reader /
// pipeline / file writer in csrc/src/burstopt.cpp, CLI bin/burstopt
// (csrc/apps/burstopt_main.cpp).
//
// Definition.  Input is one candidate of a PSBRST01 file (burstcube.hpp):
// ds_sums, ds_hits int32 [nsub][ntime], dmt_sums, dmt_hits int32 [ndm][ntime],
// nactive[nsub], dms[ndm]; sample, width, tscrunch (f), t0, dm, snr; the
// header's tsamp fch1 foff nchans.  No filterbank is read.  Parameters: nfine
// (odd, 1..257) fine DM rows and fine_half_range (a DM, >= 0; 0 = the spacing
// of two coarse rows, double(dms[ndm / 2]) - double(dms[ndm / 2 - 1]), and 0
// when ndm == 1).
//
// 1. Prepare (host; integers, and double arithmetic on exact integers, left to
//    right, no FMA contraction).  A "row" r is a waterfall subband or a DM row;
//    a bin has samples where hits > 0.
//      O          = {k : k < ntime / 4 or k >= ntime - ntime / 4}      (the off-pulse bins; integer divisions)
//      Href[r]    = max_k hits[r][k]
//      q[r][k]    = (2 sums Href[r] + hits) // (2 hits)                 (int64, floor) where hits > 0
//      cnt[r]     = number of k in O with hits > 0
//      B[r]       = (sum of q over those k) // cnt[r]                   (floor)
//      a row with Href <= 0 or cnt == 0 is dead: d = 0 throughout (a killed subband has no hits and is dead)
//      d[r][k]    = q - B[r] where hits > 0, 0 elsewhere
//      Moff[r]    = sum of d, V2[r] = sum of d^2 over the same off-pulse bins (exact integers; 0 for a dead row)
//      V          = sum over live waterfall rows s, ascending, of double(V2[s]) / double(cnt[s])
//      Mbar_ds    = sum over live waterfall rows s, ascending, of double(Moff[s]) / double(cnt[s])
//      Mbar_j     = double(Moff[j]) / double(cnt[j]) for DM row j (0 for a dead row)
//    V is the off-pulse variance of one bin of the band-summed profile: unlike
//    cubeopt's it does not hold the pulse's own power, because burstcube
//    centres the pulse in the window.  A candidate is refused by name
//    ("candidate K ...") before anything is launched, in this order: when
//    ntime < 8; when no waterfall row is live; when a d does not fit int32;
//    when max|d_ds| x (live subbands) x (ntime / 2) >= 2^31; when max|d_dmt| x
//    (ntime / 2) >= 2^31.  With these bounds every box sum fits int32 and
//    every V2 fits int64.  A candidate whose dm is negative or not finite, or
//    whose tscrunch is 0, is refused likewise.
//
// 2. Fine DM rows and shifts (host, double, left to right, no FMA contraction).
//      fine_half  = fine_half_range if > 0, else the default above
//      step       = fine_half / (nfine / 2), 0 when nfine == 1
//      dmf[kf]    = float32(max(0, double(float(dm)) + (kf - nfine / 2) * step))   (row nfine / 2 is exactly dm)
//      delays     = the float32 delay table of the header (generate_delay_table)
//      subband s owns the channels c0..c1 with floor(c nsub / nchans) == s (killed ones included)
//      dsub[s]    = 0.5 * (double(delays[c0]) + double(delays[c1]))
//      sf[kf][s]  = rint((double(dmf[kf]) - double(float(dm))) * dsub[s] / f), clamped to [-ntime, ntime], int32
//
// 3. Search (device, int32).  There are ndm + nfine profile rows:
//      P[j][k]        = d_dmt[j][k]                              for j < ndm          (the coarse plane)
//      P[ndm + kf][k] = sum over s of d_ds[s][k + sf[kf][s]]     (the fine plane; a term whose index falls outside
//                                                                 [0, ntime) is 0)
//    Widths w = 1, 2, 4, ... while w <= ntime / 2 (nw of them, at most 10).
//    S_w[r][k] = P[r][k] + ... + P[r][k + w - 1] for 0 <= k <= ntime - w: the
//    box is not circular.  For each of the two planes (rows r_local of its
//    own, from 0) and each width:
//      best_val[plane][w] = max over the plane's rows and k
//      best_idx[plane][w] = the smallest flat index r_local ntime + k attaining it
//      curve[w][r]        = max over k                           (r over all ndm + nfine rows)
//      curve_bin[w][r]    = the smallest k attaining it
//    Every output is an integer maximum with the smallest index on a tie, so
//    it does not depend on the order of evaluation: two runs, and the kernel
//    and the NumPy oracle, agree exactly.  Values may all be negative.
//
// 4. Finish (host, double, left to right).
//      snr(S, w, Mbar) = (S - w * Mbar) / sqrt(V * w), 0 when V == 0
//    Coarse plane: a width's S/N is snr(best_val[0][w], w, Mbar_j) with j =
//    best_idx[0][w] / ntime; the optimum width maximises it, ties go to the
//    smallest w.  Reported: snr_coarse with coarse_row (j), coarse_dm
//    (dms[j]), coarse_width (w f, samples) and coarse_bin; snr_in, the maximum
//    over widths of snr(curve[w][ndm / 2], w, Mbar_{ndm / 2}); snr_dm0, the
//    same over curve[.][0] with Mbar_0 when dms[0] == 0, else 0 with flag bit 0
//    set.  Fine plane, with Mbar_ds throughout: snr, opt_kf and opt_bin from
//    best_idx[1], opt_dm = dmf[opt_kf], opt_width = w f (samples), opt_sample
//    = t0 + opt_bin f (int64).
//      profile[ntime] = the fine optimum's P row
//      band[s]        = the box sum of d_ds[s] at the optimum's shift, bin and width (int32 [nsub]; terms outside the
//                       window are 0; 0 for dead rows)
//      frac_pos       = the share of live subbands with double(band[s]) - w * (double(Moff[s]) / double(cnt[s])) > 0
//    profile and band are recomputed on the host from d.
//
// Caveats.  The resolution is f samples: fine DM shifts are whole bins, so
// they cannot resolve below the smearing of one bin per subband.  Edge bins
// with few hits are noisier than V says.  A DM row far from the candidate's DM
// smears the pulse into its own off-pulse bins.
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

constexpr int kBoptMaxTime = 1024;   // bins of a row (burstcube's --ntime limit)
constexpr int kBoptMaxWidths = 10;   // 1 .. 512
constexpr int kBoptThreads = 256;
constexpr int kBoptRowsPerWg = 8;    // profile rows of one workgroup
constexpr int kBoptStage = 4096;     // dwords of waterfall staged per step (x 2 buffers)
constexpr int kBoptMaxFine = 257;

struct BoptDims {
  int ntime = 0, nsub = 0, ndm = 0, nfine = 0;
  int nw = 0;
};

inline int bopt_nwidths(int ntime) {
  int nw = 1;
  for (int w = 2; w <= ntime / 2; w *= 2) ++nw;
  return nw;
}

// d_ds int32 [ncand][nsub][ntime], d_dmt int32 [ncand][ndm][ntime], sf int32
// [ncand][nfine][nsub] (any value: reads outside a row give 0).  Outputs, all
// written here: best_val, best_idx int32 [ncand][2][nw] (the coarse plane
// first); curve, curve_bin int32 [ncand][nw][ndm + nfine].  keys: scratch,
// uint64 [ncand][2][nw].
void burst_search(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* d_sf, const BoptDims& g, int ncand,
                  uint64_t* d_keys, int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_curve, int32_t* d_curve_bin,
                  hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// burstopt options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct BurstOptCmdLineOptions {
  std::string infilename;   // a PSBRST01 file
  std::string outfilename;
  int nfine = 65;
  double fine_half_range = 0;  // 0 = the spacing of two coarse DM rows
  int limit = 1000;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_burstopt.bopt" in UTC.
std::string default_bopt_output_filename();
bool parse_bopt_cmdline(BurstOptCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// ---------------------------------------------------------- definitions ----
struct BurstOptGrid {
  int nfine = 65;
  double fine_half_range = 0;
};

// What the search needs of a PSBRST01 header.
struct BurstOptGeom {
  int ntime = 0, nsub = 0, ndm = 0, nchans = 0;
  double tsamp = 0, fch1 = 0, foff = 0;
};

struct BurstOptInput {
  uint64_t sample = 0;
  uint32_t width = 1;
  uint32_t tscrunch = 1;  // f
  int64_t t0 = 0;
  float dm = 0;
  float snr = 0;
  std::vector<float> dms;                   // [ndm]
  std::vector<int32_t> nactive;             // [nsub]
  std::vector<int32_t> ds_sums, ds_hits;    // [nsub][ntime]
  std::vector<int32_t> dmt_sums, dmt_hits;  // [ndm][ntime]
};

struct BurstOptPrepared {
  std::vector<int32_t> d_ds;                   // [nsub][ntime]
  std::vector<int32_t> d_dmt;                  // [ndm][ntime]
  std::vector<int32_t> cnt_ds, cnt_dmt;        // [nsub], [ndm]; 0 for a dead row
  std::vector<int64_t> moff_ds, moff_dmt;      // [nsub], [ndm]
  std::vector<int64_t> v2_ds, v2_dmt;          // [nsub], [ndm]
  double v = 0, mbar_ds = 0;
  std::vector<double> mbar_dmt;                // [ndm]
};

struct BurstOptShifts {
  std::vector<float> dmf;   // [nfine]
  std::vector<int32_t> sf;  // [nfine][nsub]
};

struct BurstOptSearch {
  std::vector<int32_t> best_val, best_idx;  // [2][nw], the coarse plane first
  std::vector<int32_t> curve, curve_bin;    // [nw][ndm + nfine]
};

struct BurstOptResult {
  double snr = 0, snr_coarse = 0, snr_in = 0, snr_dm0 = 0, frac_pos = 0;
  double v = 0, mbar_ds = 0;
  int64_t opt_sample = 0;
  float opt_dm = 0, coarse_dm = 0;
  uint32_t opt_width = 1, opt_kf = 0, opt_bin = 0;           // opt_width in samples
  uint32_t coarse_row = 0, coarse_width = 1, coarse_bin = 0;  // coarse_width in samples
  uint32_t flags = 0;  // bit 0: dms[0] != 0, snr_dm0 not available
  std::vector<float> dms;        // [ndm], the input's
  std::vector<float> dmf;        // [nfine]
  std::vector<double> mbar_dmt;  // [ndm]
  BurstOptSearch search;
  std::vector<int32_t> band;     // [nsub]
  std::vector<int32_t> profile;  // [ntime]
};

// Steps 1, 2 and 4 of the definition (burstopt_host.cpp).  k: the candidate's
// index, for the error text.
void burst_opt_check_grid(const BurstOptGrid& grid);
BurstOptPrepared burst_opt_prepare(size_t k, const BurstOptGeom& g, const BurstOptInput& in);
BurstOptShifts burst_opt_shifts(const BurstOptGeom& g, const BurstOptGrid& grid, float dm, uint32_t f,
                                const std::vector<float>& dms, const std::vector<float>& delays);
BurstOptResult burst_opt_finish(const BurstOptGeom& g, const BurstOptGrid& grid, const BurstOptInput& in,
                                const BurstOptPrepared& prep, const BurstOptShifts& sh, const BurstOptSearch& found);
double burst_opt_snr(double s, int w, double mbar, double v);
// Step 3 on the host, from the definition (unit tests and the tiniest inputs only).
BurstOptSearch burst_opt_search_host(const BurstOptGeom& g, int nfine, const std::vector<int32_t>& d_ds,
                                     const std::vector<int32_t>& d_dmt, const std::vector<int32_t>& sf);

// ------------------------------------------------------------ optimiser ----
class BurstOptimiser {
 public:
  static constexpr size_t kDefaultBatchBytes = size_t(1) << 30;
  BurstOptimiser(const BurstOptGeom& g, const BurstOptGrid& grid, hipStream_t stream,
                 size_t batch_bytes = kDefaultBatchBytes);
  ~BurstOptimiser();
  // Validates every candidate first (nothing is launched on an error), then
  // searches in batches; results in input order.  delays: float [nchans].
  std::vector<BurstOptResult> optimise(const std::vector<BurstOptInput>& cands, const std::vector<float>& delays);
  // Step 3 alone with explicit tables: d_ds [ncand][nsub][ntime], d_dmt
  // [ncand][ndm][ntime], sf [ncand][nfine][nsub]; shifts outside [-ntime,
  // ntime] are refused by candidate.
  std::vector<BurstOptSearch> search(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* sf, size_t ncand);
  // As search() with the tables and the results on the device: outputs int32
  // best_val, best_idx [ncand][2][nw], curve, curve_bin [ncand][nw][ndm +
  // nfine].  Nothing crosses to the host and nothing is awaited: the torch
  // op's path.
  void search_device(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* d_sf, size_t ncand,
                     int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_curve, int32_t* d_curve_bin);
  size_t bytes_per_candidate() const;
  int batch_size() const;
  uint64_t batches() const { return nbatches_; }  // launches so far
  const BurstOptGeom& geom() const { return g_; }
  const BurstOptGrid& grid() const { return grid_; }
  int nwidths() const { return dims_.nw; }

 private:
  BurstOptGeom g_;
  BurstOptGrid grid_;
  kern::BoptDims dims_;
  hipStream_t stream_;
  size_t batch_bytes_;
  uint64_t nbatches_ = 0;
  DeviceBuffer<uint64_t> d_keys_;  // search_device's scratch
};

// ------------------------------------------------------------ pipeline ----
struct BurstFile {
  BurstOptGeom geom;
  uint32_t nbits = 0;
  uint64_t nsamps = 0;
  std::vector<BurstOptInput> candidates;
};
// Reads a PSBRST01 file (burstcube.hpp), at most `limit` candidates from the
// top (limit < 0: all); a wrong magic or a truncated file is an error.
BurstFile read_burst_file(const std::string& path, int limit = -1);

struct BoptFileHeader {
  uint32_t ncand = 0, ntime = 0, nsub = 0, ndm = 0, nchans = 0, nbits = 0, nfine = 0, nw = 0;
  uint64_t nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0, fine_half_range = 0;
};

struct BurstOptRun {
  BoptFileHeader header;
  std::vector<BurstOptInput> candidates;  // the scalars only (the planes are dropped)
  std::vector<BurstOptResult> results;
  std::map<std::string, double> timers;  // reading, searching, total (s)
};
// Reads args.infilename, searches on device 0 and writes args.outfilename.
BurstOptRun run_bopt_pipeline(const BurstOptCmdLineOptions& args);
// Little-endian: "PSBOPT01", uint32 ncand ntime nsub ndm nchans nbits nfine nw
// (40 bytes so far), uint64 nsamps, double tsamp fch1 foff fine_half_range (80
// bytes); per candidate uint64 sample, uint32 width, uint32 tscrunch, int64
// t0, float dm, float snr of the input (32 bytes), double snr snr_coarse snr_in
// snr_dm0 frac_pos v mbar_ds, int64 opt_sample, float opt_dm coarse_dm, uint32
// opt_width opt_kf opt_bin coarse_row coarse_width coarse_bin flags and a zero
// (136 bytes), then float dms[ndm], float dmf[nfine], double mbar_dmt[ndm],
// int32 best_val[2][nw], best_idx[2][nw], curve[nw][ndm + nfine],
// curve_bin[nw][ndm + nfine], band[nsub], profile[ntime].  Written to a
// temporary file, then renamed.
void write_bopt_file(const std::string& path, const BoptFileHeader& h, const std::vector<BurstOptInput>& cands,
                     const std::vector<BurstOptResult>& results);

}  // namespace psoup
