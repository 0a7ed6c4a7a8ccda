// Single-pulse (transient) search on the dedispersed trials: a boxcar matched
// filter over power-of-two widths on every DM trial, an extension beyond the
// reference (which searches periodicities only).  Kernels in
// csrc/kernels/singlepulse.hip, engine / clustering / pipeline in
// csrc/src/singlepulse.cpp, CLI bin/spsearch (csrc/apps/sp_main.cpp).
//
// For one trial u[0..n) (uint8):
//   trend : ffa_detrend's block-mean trend (exact integer block sums over
//           `baseline` samples, linear between block centres, flat outside)
//   x[i]  = u[i] - trend(i);  sigma = sqrt(mean(x^2)) (double, fixed order)
//   w_k   = 2^k, k = 0..K, 2^K the largest power of two <= min(wmax, n / 2)
//   snr_k[i] = (x[i] + ... + x[i + w_k - 1]) / (sigma sqrt(w_k)), 0 <= i <= n - w_k
//   event : per width and aligned block of 64 start samples the maximum of
//           snr_k (lowest index on a tie), recorded when >= thresh.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/cli.hpp"
#include "psoup/common.hpp"
#include "psoup/rfi.hpp"

namespace psoup {

// One above-threshold block maximum (the device record).
struct SpEvent {
  uint32_t sample;     // first sample of the boxcar
  int32_t width_log2;  // k: width 2^k samples
  float snr;
  int32_t dm_idx;
};
static_assert(sizeof(SpEvent) == 16, "SpEvent layout");

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kSpTile = 8192;       // start samples per workgroup of the search kernel
constexpr int kSpBlock = 64;        // start samples per block maximum
constexpr int kSpMaxLog2 = 12;      // widest boxcar 2^12 (the halo held in LDS)
constexpr int kSpSigmaParts = 64;   // partial sums of x^2 per DM

// Rows: [ndm][row_stride] uint8 (row_stride a multiple of 4, >= n), n samples
// used of each.  means: float [ndm][nblk], nblk = ceil(n / baseline).
void sp_block_means(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, float* means,
                    hipStream_t s);
// partials: double [ndm][kSpSigmaParts], sums of x^2 over fixed sample ranges.
void sp_sigma(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, const float* means,
              double* partials, hipStream_t s);
// The fused search: block maxima of every width 2^k, k <= kmax, of every DM;
// maxima >= thresh are appended to events (*count may exceed capacity; no
// record is written at or past capacity).  best_snr / best_arg (optional,
// tests): [ndm][kmax + 1][ceil(n / 64)] maximum and its sample of every
// block; blocks without a valid start hold 0 and 0xffffffff.
void sp_search(const uint8_t* rows, uint64_t row_stride, int ndm, uint64_t n, uint64_t baseline, const float* means,
               const double* partials, int kmax, float thresh, int dm_idx0, SpEvent* events, uint32_t* count,
               uint32_t capacity, float* best_snr, uint32_t* best_arg, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// spsearch options: the FFA pipeline's I/O and DM flags with its defaults,
// plus the search's own.  Declared here and not in cli.hpp, which is part of
// the checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct SpCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string killfilename;
  int max_num_threads = 14;
  float dm_start = 0.0f;
  float dm_end = 100.0f;
  float dm_tol = 1.10f;
  float dm_pulse_width = 64.0f;
  bool verbose = false;
  bool progress_bar = false;
  float min_snr = 6.5f;
  int boxcar_max = 4096;   // samples
  double baseline = 2.0;   // s
  int limit = 1000;
  std::string dedisp_kernel = "auto";
  // RFI excision before the search (psoup/rfi.hpp); off by default
  bool rfi = false;
  bool zero_dm = false;  // implies rfi
  int rfi_block = 4096;
  double rfi_thresh = 5.0;
  double rfi_chan_frac = 0.3;
  double rfi_block_frac = 0.3;
  std::string rfi_maskfilename;  // --rfi_mask_out
};
RfiParams sp_rfi_params(const SpCmdLineOptions& args);
// "%Y-%m-%d-%H:%M_spsearch.output" in UTC.
std::string default_sp_output_filename();
bool parse_sp_cmdline(SpCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// --------------------------------------------------------------- engine ----
struct SpParams {
  double tsamp = 64e-6;
  float min_snr = 6.5f;
  int boxcar_max = 4096;         // widest boxcar (samples); at most 2^kSpMaxLog2
  double baseline_s = 2.0;       // trend block length (s)
  uint64_t baseline_samples = 0;  // trend block length in samples; 0 = from baseline_s
  uint32_t capacity = 1u << 16;  // initial record buffer (grown on overflow)
};

struct SpCandidate {
  uint64_t sample = 0;  // first sample of the strongest event's boxcar
  double time_s = 0;    // centre of that boxcar (s)
  int width = 0;        // samples
  float snr = 0;
  float dm = 0;
  int dm_idx = 0;
  int members = 1;      // events absorbed, the strongest included
  uint64_t first_sample = 0, last_sample = 0;  // extent of the members' boxcars (inclusive)
  int dm_idx_lo = 0, dm_idx_hi = 0;
};
using SpCandidateList = std::vector<SpCandidate>;

// Widths 2^k, k = 0..K (empty when n < 2 or wmax < 1).
std::vector<int> sp_widths(uint64_t n, int wmax);
// Trend block length in samples for a series of n samples.
uint64_t sp_baseline_samples(const SpParams& p, uint64_t n);

// Greedy clustering (host only, deterministic).  Events are taken in
// descending S/N (ties: dm_idx, width_log2, sample); with t = sample + w / 2,
// an event is absorbed by the first accepted candidate (t0, w0, dm0) with
//   |t - t0| <= (w + w0) / 2 + |dm - dm0| * band_delay_per_dm / tsamp,
// band_delay_per_dm the dispersion delay across the band per unit DM in
// seconds (generate_delay_table's last entry, which is in samples, times
// tsamp): a burst seen at a wrong DM is displaced by at most that much.
// Returns the candidates in descending S/N.
SpCandidateList sp_cluster(const std::vector<SpEvent>& events, const std::vector<float>& dm_list,
                           double band_delay_per_dm, double tsamp);

class SinglePulseEngine {
 public:
  SinglePulseEngine(const SpParams& p, uint64_t nsamps, hipStream_t stream);
  ~SinglePulseEngine();
  // d_rows: device [ndm][row_stride] uint8 trials (Dedisperser::run's
  // layout); row i is DM index dm_idx0 + i.  Returns the events sorted by
  // (dm_idx, width_log2, sample).  d_best_snr / d_best_arg: optional dense
  // outputs of kern::sp_search.
  std::vector<SpEvent> search_block(const uint8_t* d_rows, uint64_t row_stride, int ndm, int dm_idx0,
                                    float* d_best_snr = nullptr, uint32_t* d_best_arg = nullptr);
  uint64_t nsamps() const { return n_; }
  uint64_t baseline() const { return baseline_; }
  int kmax() const { return kmax_; }
  const std::vector<int>& widths() const { return widths_; }
  // Counters
  uint64_t events() const { return nevents_; }
  uint64_t reruns() const { return nreruns_; }

 private:
  SpParams p_;
  uint64_t n_, baseline_, nblk_;
  hipStream_t stream_;
  std::vector<int> widths_;
  int kmax_ = 0;
  uint32_t cap_;
  DeviceBuffer<float> means_;
  DeviceBuffer<double> partials_;
  DeviceBuffer<SpEvent> d_events_;
  DeviceBuffer<uint32_t> d_count_;
  uint64_t nevents_ = 0, nreruns_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct SpResult {
  SpCandidateList candidates;  // clustered over all DMs, S/N descending, limited
  std::vector<float> dm_list;
  std::vector<int> devices;
  std::map<std::string, double> timers;  // reading, dedispersion, searching, total (s)
  uint64_t nsamps = 0;                   // dedispersed series length searched
  double tsamp = 0;
  std::vector<int> widths;
  uint64_t baseline = 0;
  uint64_t events = 0, reruns = 0;
  std::string rfi_comment;  // "# rfi: ..." header lines; empty without --rfi
};
SpParams sp_params_from(const SpCmdLineOptions& args, double tsamp);
// Reads the filterbank, dedisperses on min(-t, devices) GPUs (one thread per
// GPU pulling DM chunks, the next chunk's dedispersion on a side stream
// beside the current chunk's search), clusters the events of all DMs.
SpResult run_sp_pipeline(const SpCmdLineOptions& args);
// Text output (one candidate per line after a commented header).
void write_sp_output(const std::string& path, const SpCmdLineOptions& args, const SpResult& res);

}  // namespace psoup
