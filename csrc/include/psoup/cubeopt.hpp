// cubeopt: a brute-force search over DM, period-drift and acceleration-drift
// trials on the fold cubes of foldcube (the prepfold / pdmp step), an extension
// beyond the reference.  Kernel in csrc/kernels/cubeopt.hip, the host steps in
// csrc/src/cubeopt_host.cpp (no device code), CubeOptimiser / readers /
// pipeline / file writer in csrc/src/cubeopt.cpp, CLI bin/cubeopt
// (csrc/apps/cubeopt_main.cpp).
//
// Definition.  Input is one candidate of a PSCUBE01 file: sums int64
// [nints][nsub][nbins], hits int32 [nints][nbins], nactive[nsub]; period, dm,
// acc; the header's tsamp fch1 foff nchans fold_nsamps.  No filterbank is read.
// The grid is ndm DM rows, np period-drift trials of p_step bins and npd
// acceleration-drift trials of pd_step bins (np, npd odd).
//
// 1. Prepare (host; integers, and double arithmetic on exact integers).  A
//    candidate is refused by name ("candidate K ...") before anything is
//    launched when a hits[i][b] is 0, when nints * nbins > 16384, when the
//    trial count ndm * np * npd * nbins >= 2^31, when its period is not
//    positive and finite or its dm / acc not finite, or when a bound below
//    fails.
//      Href[i]    = max_b hits[i][b]
//      q[i][s][b] = (2 sums Href[i] + hits[i][b]) // (2 hits[i][b])   (int64, floor;
//                   |2 sums Href| < 2^63 must hold)
//      B[i][s]    = (sum_b q) // nbins                                (floor)
//      d          = q - B where nactive[s] > 0, d = 0 where nactive[s] == 0
//      d must fit int32, and max|d| * nints * (subbands with nactive > 0) *
//      (nbins / 2) < 2^31 must hold (every box sum then fits int32)
//      Mtot = sum d, V2 = sum d^2 (exact integers), V = double(V2) / nbins
//
// 2. Shift tables (host, double, evaluated left to right, no FMA
//    contraction).  All shifts are rounded half to even (rint), then reduced
//    into [0, nbins).
//      dms[kd]     = burst_dms(dm, ndm, dm_half_range)  (burstcube.hpp: row ndm / 2 is exactly dm;
//                    row 0 is DM 0 when dm_half_range is 0 and ndm is even)
//      delays      = the float32 delay table of the header (generate_delay_table)
//      subband s owns the channels c0..c1 with floor(c nsub / nchans) == s (killed ones included)
//      dsub[s]     = 0.5 * (double(delays[c0]) + double(delays[c1]))
//      tbp         = double(float(tsamp)) / period
//      sdm[kd][s]  = rint((double(dms[kd]) - double(float(dm))) * dsub[s] * tbp * nbins)
//      u_i         = (i + 0.5) / nints
//      L           = (kp - np / 2) * p_step,  Q = (kpd - npd / 2) * pd_step   (integer divisions)
//      st[kp][kpd][i] = rint(L * (u_i - 0.5) + Q * (4.0 * u_i * (1.0 - u_i)))
//
// 3. Search (device, int32).  For every (kd, kp, kpd):
//      A[i][b] = sum_s d[i][s][(b + sdm[kd][s]) % nbins]
//      prof[b] = sum_i A[i][(b + st[kp][kpd][i]) % nbins]
//    Widths w = 1, 2, 4, ... while w <= nbins / 2 (nw of them; nbins >= 2).
//    S_w[b] = prof[b] + ... + prof[(b + w - 1) % nbins].  Per width:
//      best_val[w]           = max over all trials and bins
//      best_idx[w]           = the smallest flat index ((kd np + kp) npd + kpd) nbins + b attaining it
//      dmcurve[w][kd]        = max over kp, kpd, b
//      ppd[w][kp][kpd]       = max over kd, b
//      centre[w]             = max over b at the unshifted trial (ndm / 2, np / 2, npd / 2)
//    Every output is an integer maximum, so it does not depend on the order of
//    evaluation: two runs, and the kernel and the NumPy oracle, agree exactly.
//
// 4. Finish (host, double, left to right).
//      snr(S, w) = (S - w * double(Mtot) / nbins) / sqrt(V * w * (1.0 - double(w) / nbins)),
//                  0 when V == 0
//      The optimum width maximises snr(best_val[w], w); ties go to the smallest w.
//      snr      = that maximum; snr_in the same maximum taken over centre;
//      snr_dm0  the same taken over dmcurve[.][0] when dms[0] == 0, else 0 with flag bit 0 set
//      opt_dm   = dms[kd]; opt_width, opt_bin, opt_kd, opt_kp, opt_kpd from best_idx
//      T = fold_nsamps * double(float(tsamp));  ts = double(float(tsamp))
//      opt_period = 1 / (1 / period - L / (nbins * T))
//      opt_acc    = double(acc) - (8 c Q period) / (nbins ts ts fold_nsamps fold_nsamps)
//      profile    = prof of the optimum trial, int32 [nbins], recomputed on the host from d
//    (A pulse that arrives L bins later at the end of the fold than at its
//    start has a period longer than the folding period; a pulse that arrives Q
//    bins later in the middle than at the ends was folded with too large an
//    acceleration.)  V includes the pulse's own power, so the S/N of a very
//    bright pulsar is understated.
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

// nints * nbins: the A plane in LDS, at most 64 KiB; with the four waves' box-sum
// rows of nbins dwords a workgroup holds at most 65536 + 4096 = 69632 bytes
constexpr int kOptMaxPlane = 16384;
constexpr int kOptMaxBins = 256;
constexpr int kOptMaxWidths = 8;     // 1 .. 128
constexpr int kOptThreads = 256;
constexpr int kOptTrialsPerWg = 256;  // (kp, kpd) trials of one workgroup, about

struct OptDims {
  int nints = 0, nsub = 0, nbins = 0;
  int ndm = 0, np = 0, npd = 0;
  int nw = 0;
};

inline int opt_nwidths(int nbins) {
  int nw = 1;
  for (int w = 2; w <= nbins / 2; w *= 2) ++nw;
  return nw;
}

// d int32 [ncand][nints][nsub][nbins], sdm int32 [ncand][ndm][nsub], st int32
// [ncand][np][npd][nints], every shift in [0, nbins) (checked by the caller:
// the kernel indexes with them).  Outputs, all written here: best_val,
// best_idx, centre int32 [ncand][nw]; dmcurve int32 [ncand][nw][ndm]; ppd
// int32 [ncand][nw][np][npd].  keys: scratch, uint64 [ncand][nw].
void cube_search(const int32_t* d_d, const int32_t* d_sdm, const int32_t* d_st, const OptDims& g, int ncand,
                 uint64_t* d_keys, int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_dmcurve, int32_t* d_ppd,
                 int32_t* d_centre, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// cubeopt options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct CubeOptCmdLineOptions {
  std::string infilename;   // a PSCUBE01 file
  std::string outfilename;
  int ndm = 64;
  float dm_half_range = 0;  // 0 = the candidate's DM: rows span 0..2 DM
  int np = 65;
  double p_step = 1.0;      // bins of drift across the fold
  int npd = 33;
  double pd_step = 1.0;     // bins of curvature at the middle of the fold
  int limit = 1000;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_cubeopt.opt" in UTC.
std::string default_opt_output_filename();
bool parse_opt_cmdline(CubeOptCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// ---------------------------------------------------------- definitions ----
struct CubeOptGrid {
  int ndm = 64;
  float dm_half_range = 0;
  int np = 65;
  double p_step = 1.0;
  int npd = 33;
  double pd_step = 1.0;
};

// What the search needs of a PSCUBE01 header.
struct CubeOptGeom {
  int nints = 0, nsub = 0, nbins = 0, nchans = 0;
  uint64_t fold_nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0;
};

struct CubeOptInput {
  double period = 0;
  float dm = 0;
  float acc = 0;
  std::vector<int32_t> nactive;  // [nsub]
  std::vector<int32_t> hits;     // [nints][nbins]
  std::vector<int64_t> sums;     // [nints][nsub][nbins]
};

struct CubeOptPrepared {
  std::vector<int32_t> d;  // [nints][nsub][nbins]
  int64_t mtot = 0;
  int64_t v2 = 0;
  double v = 0;
};

struct CubeOptShifts {
  std::vector<float> dms;    // [ndm]
  std::vector<int32_t> sdm;  // [ndm][nsub]
  std::vector<int32_t> st;   // [np][npd][nints]
};

struct CubeOptSearch {
  std::vector<int32_t> best_val, best_idx, centre;  // [nw]
  std::vector<int32_t> dmcurve;                     // [nw][ndm]
  std::vector<int32_t> ppd;                         // [nw][np][npd]
};

struct CubeOptResult {
  double snr = 0, snr_in = 0, snr_dm0 = 0;
  double opt_period = 0, opt_acc = 0;
  float opt_dm = 0;
  uint32_t opt_width = 1, opt_bin = 0, opt_kd = 0, opt_kp = 0, opt_kpd = 0;
  uint32_t flags = 0;  // bit 0: dms[0] != 0, snr_dm0 not available
  int64_t mtot = 0;
  double v = 0;
  std::vector<float> dms;
  CubeOptSearch search;
  std::vector<int32_t> profile;  // [nbins]
};

// Steps 1, 2 and 4 of the definition (cubeopt_host.cpp).  k: the candidate's
// index, for the error text.
void cube_opt_check_grid(const CubeOptGrid& grid);
CubeOptPrepared cube_opt_prepare(size_t k, const CubeOptGeom& g, const CubeOptGrid& grid, const CubeOptInput& in);
CubeOptShifts cube_opt_shifts(const CubeOptGeom& g, const CubeOptGrid& grid, double period, float dm,
                              const std::vector<float>& delays);
CubeOptResult cube_opt_finish(const CubeOptGeom& g, const CubeOptGrid& grid, double period, float acc,
                              const CubeOptPrepared& prep, const CubeOptShifts& sh, const CubeOptSearch& found);
double cube_opt_snr(double s, int w, int64_t mtot, double v, int nbins);
// Step 3 on the host, from the definition (unit tests and the tiniest inputs only).
CubeOptSearch cube_opt_search_host(const CubeOptGeom& g, const CubeOptGrid& grid, const std::vector<int32_t>& d,
                                   const CubeOptShifts& sh);

// ------------------------------------------------------------ optimiser ----
class CubeOptimiser {
 public:
  static constexpr size_t kDefaultBatchBytes = size_t(1) << 30;
  CubeOptimiser(const CubeOptGeom& g, const CubeOptGrid& grid, hipStream_t stream,
                size_t batch_bytes = kDefaultBatchBytes);
  ~CubeOptimiser();
  // Validates every candidate first (nothing is launched on an error), then
  // searches in batches; results in input order.  delays: float [nchans].
  std::vector<CubeOptResult> optimise(const std::vector<CubeOptInput>& cands, const std::vector<float>& delays);
  // Step 3 alone with explicit tables: d [ncand][nints][nsub][nbins], sdm
  // [ncand][ndm][nsub], st [ncand][np][npd][nints]; shifts outside [0, nbins)
  // are refused by candidate.
  std::vector<CubeOptSearch> search(const int32_t* d, const int32_t* sdm, const int32_t* st, size_t ncand);
  // As search() with the tables and the results on the device: d_d, d_sdm,
  // d_st as above, outputs int32 best_val, best_idx, centre [ncand][nw],
  // dmcurve [ncand][nw][ndm], ppd [ncand][nw][np][npd].  The kernel indexes
  // with the shifts: the caller has checked that every one lies in [0, nbins).
  // Nothing crosses to the host and nothing is awaited: the torch op's path.
  void search_device(const int32_t* d_d, const int32_t* d_sdm, const int32_t* d_st, size_t ncand, int32_t* d_best_val,
                     int32_t* d_best_idx, int32_t* d_dmcurve, int32_t* d_ppd, int32_t* d_centre);
  size_t bytes_per_candidate() const;
  int batch_size() const;
  uint64_t batches() const { return nbatches_; }  // launches so far
  const CubeOptGeom& geom() const { return g_; }
  const CubeOptGrid& grid() const { return grid_; }
  int nwidths() const { return dims_.nw; }

 private:
  CubeOptGeom g_;
  CubeOptGrid grid_;
  kern::OptDims dims_;
  hipStream_t stream_;
  size_t batch_bytes_;
  uint64_t nbatches_ = 0;
  DeviceBuffer<uint64_t> d_keys_;  // search_device's scratch
};

// ------------------------------------------------------------ pipeline ----
struct CubeFile {
  CubeOptGeom geom;
  uint32_t nbits = 0;
  std::vector<CubeOptInput> candidates;
};
// Reads a PSCUBE01 file (foldcube.hpp), at most `limit` candidates from the
// top (limit < 0: all); a wrong magic or a truncated file is an error.
CubeFile read_cube_file(const std::string& path, int limit = -1);

struct OptFileHeader {
  uint32_t ncand = 0, nints = 0, nsub = 0, nbins = 0, nchans = 0, ndm = 0, np = 0, npd = 0, nw = 0;
  uint64_t fold_nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0, p_step = 0, pd_step = 0, dm_half_range = 0;
};

struct CubeOptRun {
  OptFileHeader header;
  std::vector<CubeOptInput> candidates;  // period, dm, acc only (the cubes are dropped)
  std::vector<CubeOptResult> results;
  std::map<std::string, double> timers;  // reading, searching, total (s)
};
// Reads args.infilename, searches on device 0 and writes args.outfilename.
CubeOptRun run_opt_pipeline(const CubeOptCmdLineOptions& args);
// Little-endian: "PSOPT001", uint32 ncand nints nsub nbins nchans ndm np npd
// nw and a zero (48 bytes so far), uint64 fold_nsamps, double tsamp fch1 foff
// p_step pd_step dm_half_range (104 bytes); per candidate double period, float
// dm, float acc, double snr snr_in snr_dm0 opt_period opt_acc, float opt_dm,
// uint32 opt_width opt_bin opt_kd opt_kp opt_kpd flags and a zero, int64 mtot,
// double v (104 bytes), then float dms[ndm], int32 best_val[nw], best_idx[nw],
// centre[nw], dmcurve[nw][ndm], ppd[nw][np][npd], profile[nbins].  Written to
// a temporary file, then renamed.
void write_opt_file(const std::string& path, const OptFileHeader& h, const std::vector<CubeOptInput>& cands,
                    const std::vector<CubeOptResult>& results);

}  // namespace psoup
