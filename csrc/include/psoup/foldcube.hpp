// Folding the filterbank into subint x subband x phase cubes per periodicity
// candidate (the reference's commented-out fold_filterbank_kernel, K12), an
// extension beyond the reference.  Kernel in csrc/kernels/foldcube.hip,
// CubeFolder / pipeline / file writer in csrc/src/foldcube.cpp, CLI
// bin/foldcube (csrc/apps/foldcube_main.cpp).
//
// Definition.  The raw sample is x[c][t] = stored int8 + bias (>= 0).  For a
// candidate (period, dm, acc) and a fold length n:
//   off[c] = int32(float(dm) * delays[c] + 0.5f)           (max(off) + n <= nsamps)
//   af     = (double(float(acc)) * float(tsamp)) / (2 c)
//   h = n / 2.0, nps = n / nints; for j in [0, nints * nps), d = double(j):
//     subint = j / nps
//     bin    = clamp(floor(frac(d * (tsamp / period)) * nbins), 0, nbins - 1)
//     src    = clamp(rint(d + af * ((d - h) * (d - h) - h * h)), 0, n - 1)
//   (fold_accumulate_kernel's expressions, evaluated without FMA contraction)
//   hits[subint][bin] += 1
//   sums[subint][s][bin] += x[c][src + off[c]] for every unkilled channel c,
//     s = floor(c * nsub / nchans)
//   nactive[s] = unkilled channels of subband s
// Every output is an integer, so the result is independent of the summation
// order: two runs, and the kernel and the NumPy oracle, agree to the byte.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/common.hpp"
#include "psoup/engine.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kCubeTile = 2048;     // output samples per workgroup step (256 threads x 8)
constexpr int kCubeWindow = 4096;   // bytes of a channel staged in LDS per tile
constexpr int kCubeHistMax = 8192;  // LDS histogram entries (subbands of a group x bins)
// The resampled index advances by 1 + 2 af (j - h) per output sample.  Slopes
// within [1 - kCubeMaxSlope, 1 + kCubeMaxSlope] keep a tile's source window
// (<= 1.9 * 2047 + 2 samples + 15 bytes of alignment) inside kCubeWindow.
constexpr double kCubeMaxSlope = 0.9;

struct CubeJob {
  double tsamp_by_period;
  double af;
};

struct CubeGeom {
  int nchans = 0;       // rows of the filterbank
  uint64_t stride = 0;  // bytes per row (a multiple of 16); reads stay inside a row
  int bias = 0;
  int nints = 0, nsub = 0, nbins = 0;
  uint64_t n = 0;       // fold length
};

// Launch plan (host): how the subbands and tiles are shared among workgroups.
struct CubePlan {
  int sub_per_group = 0;  // subbands per workgroup (the LDS histogram's rows)
  int ngroups = 0;
  int tiles_per_wg = 0;   // consecutive tiles of one subint per workgroup
  int wgs_per_subint = 0;
};
// max_sub_channels: the most unkilled channels in one subband.
CubePlan cube_plan(const CubeGeom& g, int ncand, int max_sub_channels);

// chan_major: int8 [nchans][stride], 16-byte aligned.  active: the unkilled
// channels in ascending order; sub_first: int32 [nsub + 1], subband s owns
// active[sub_first[s] .. sub_first[s + 1]).  offsets: int32 [ncand][nchans].
// sums (int64 [ncand][nints][nsub][nbins]) and hits (int32
// [ncand][nints][nbins]) are added to: zero them first.
void fold_cube(const int8_t* chan_major, const CubeGeom& g, const int32_t* d_active, const int32_t* d_sub_first,
               const int32_t* d_offsets, const CubeJob* d_jobs, int ncand, const CubePlan& plan, int64_t* d_sums,
               int32_t* d_hits, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// foldcube options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct FoldCubeCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string candfilename;
  std::string overviewfilename;  // read by the Python driver only (python -m peasoup_amd cube)
  std::string killfilename;
  int nints = 16;
  int nsub = 32;  // capped at nchans
  int nbins = 64;
  uint64_t fold_nsamps = 0;  // 0 = default_fold_nsamps
  int limit = 1000;
  int top = 16;              // --overview: candidates taken
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_foldcube.cubes" in UTC.
std::string default_cube_output_filename();
bool parse_cube_cmdline(FoldCubeCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// --------------------------------------------------------------- folder ----
struct CubeParams {
  int nints = 16;
  int nsub = 32;
  int nbins = 64;
  uint64_t fold_nsamps = 0;
};

struct CubeCandidate {
  double period = 0;  // s
  float dm = 0;
  float acc = 0;      // m/s^2
};

struct CubeResult {
  std::vector<int32_t> nactive;  // [nsub]
  std::vector<int32_t> hits;     // [nints][nbins]
  std::vector<int64_t> sums;     // [nints][nsub][nbins]
};

// Candidate file: '#' lines skipped, else "period_s dm acc" (extra columns
// ignored); a malformed line is an error naming its line number.  At most
// `limit` candidates from the top (limit < 0: all).
std::vector<CubeCandidate> read_cube_candfile(const std::string& path, int limit = -1);

// The length run_pipeline folds: prev_power_of_two(nsamps - max offset) for a
// geometry whose DM list holds the largest-DM candidate.
uint64_t default_fold_nsamps(const DedispGeometry& g);

class CubeFolder {
 public:
  static constexpr size_t kDefaultBatchBytes = size_t(1) << 30;
  // The filterbank (and its geometry's delays, killmask, bias) must outlive
  // the folder.  batch_bytes: device bytes a batch of candidates may hold.
  CubeFolder(const DeviceFilterbank& fb, const CubeParams& p, hipStream_t stream,
             size_t batch_bytes = kDefaultBatchBytes);
  // Raw rows: int8 [nchans][stride] at d_chan_major with explicit delays
  // (float [nchans]) and killmask (int [nchans], empty = none killed);
  // row_valid = samples of a row that may be folded.
  CubeFolder(const int8_t* d_chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias, double tsamp,
             const std::vector<float>& delays, const std::vector<int>& killmask, const CubeParams& p,
             hipStream_t stream, size_t batch_bytes = kDefaultBatchBytes);
  ~CubeFolder();
  // Validates every candidate first (nothing is launched on an error), then
  // folds in batches; results in input order.
  std::vector<CubeResult> fold(const std::vector<CubeCandidate>& cands);
  // As fold() with explicit offsets [ncand][nchans] and the results left on
  // the device (d_sums int64 [ncand][nints][nsub][nbins], d_hits int32
  // [ncand][nints][nbins], both zeroed here): the torch op's path.
  void fold_offsets(const int32_t* h_offsets, const std::vector<double>& periods, const std::vector<float>& accs,
                    int64_t* d_sums, int32_t* d_hits);
  const CubeParams& params() const { return p_; }
  const std::vector<int32_t>& nactive() const { return nactive_; }
  int batch_size() const;            // candidates per launch
  uint64_t batches() const { return nbatches_; }  // launches so far

 private:
  void init(const std::vector<int>& killmask);
  void check_candidate(size_t i, const CubeCandidate& c, const int32_t* off) const;
  kern::CubeJob job_of(double period, float acc) const;
  void launch(const int32_t* h_off, const kern::CubeJob* h_jobs, int ncand, int64_t* d_sums, int32_t* d_hits);
  const int8_t* x_;
  uint64_t stride_, row_valid_;
  int nchans_, bias_;
  float tsamp_;
  std::vector<float> delays_;
  CubeParams p_;
  hipStream_t stream_;
  size_t batch_bytes_;
  int max_sub_channels_ = 0;
  std::vector<int32_t> nactive_;
  DeviceBuffer<int32_t> d_active_, d_sub_first_, d_off_, d_hits_;
  DeviceBuffer<kern::CubeJob> d_jobs_;
  DeviceBuffer<int64_t> d_sums_;
  uint64_t nbatches_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct CubeFileHeader {
  uint32_t ncand = 0, nints = 0, nsub = 0, nbins = 0, nchans = 0, nbits = 0;
  uint64_t fold_nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0;
};

struct CubeRun {
  CubeFileHeader header;
  std::vector<CubeCandidate> candidates;
  std::vector<CubeResult> cubes;
  std::map<std::string, double> timers;  // reading, folding, total (s)
};
// Reads the filterbank and the candidate file, applies the killfile, folds on
// device 0 and writes args.outfilename.
CubeRun run_cube_pipeline(const FoldCubeCmdLineOptions& args);
// As run_cube_pipeline with the candidates given (the --overview path).
CubeRun run_cube_pipeline(const FoldCubeCmdLineOptions& args, const std::vector<CubeCandidate>& cands);
// Little-endian: "PSCUBE01", uint32 ncand nints nsub nbins nchans nbits,
// uint64 fold_nsamps, double tsamp fch1 foff; per candidate double period,
// float dm, float acc, int32 nactive[nsub], int32 hits[nints][nbins], int64
// sums[nints][nsub][nbins].  Written to a temporary file, then renamed.
void write_cube_file(const std::string& path, const CubeFileHeader& h, const std::vector<CubeCandidate>& cands,
                     const std::vector<CubeResult>& cubes);

}  // namespace psoup
