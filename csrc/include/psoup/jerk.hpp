// jerksearch: jerk trials as an outer loop over the acceleration search.  A
// jerk trial is a dedispersed uint8 row re-indexed by a pure cubic that is zero
// at both ends and at the middle of the searched span; the unchanged
// SearchEngine then searches the re-indexed row over its acceleration list.
// The kernel in csrc/kernels/jerk.hip, the host steps (plan, factor, checks,
// distillation, frequency correction, a host transcription of the gather) in
// csrc/src/jerk_host.cpp, JerkSearcher and the file pipeline in
// csrc/src/jerk.cpp, CLI bin/jerksearch (csrc/apps/jerk_main.cpp).
//
// Definition.  Every double operation below is one correctly rounded IEEE
// operation, in the order written (no FMA contraction).
//
// Row and span.  x[0..nrow) is a dedispersed row and fft_size the search
// length.  The resampled span is n = min(nrow, fft_size); h = n / 2 (integer
// division).
//
// Jerk factor.  For a jerk trial `jerk` (m/s^3, float32) and the float32 tsamp
// the engine uses,
//     jf = (((double)jerk * (double)tsamp) * (double)tsamp) / 1798754748.0
// (the divisor is 6 c, c = 299792458 m/s).
//
// Shift and gather.
//     g(i) = ((double(i) * double(i - h)) * double(i - n)) * jf
//     s(i) = (int64) rint(g(i))                      (half to even)
//     y[i] = x[clamp(i + s(i), 0, n - 1)]            for i < n
//     y[i] = x[i]                                    for n <= i < nrow
// g alone is rounded, not i + g.  For n <= 2^26 the first product is an exact
// integer and every later step is one monotone rounding, so s is monotone
// wherever p(i) = i (i - h)(i - n) is: on a span of consecutive samples that
// holds neither stationary point of p, equal shifts at the two ends mean one
// shift throughout.  The kernel uses that for its wide-load path; the host
// passes the two stationary points as sample indices,
//     sp = floor(((h + n) -/+ sqrt((h + n)^2 - 3 h n)) / 3)
// (n/2 -/+ n/(2 sqrt 3) for even n), and the kernel treats a lane span
// [i0, i0 + 15] as clear of one when sp < i0 - 1 or sp > i0 + 16.
//
// Convention.  A pulsar's phase is (te - accel te^2/(2c) - jerk te^3/(6c)) / P
// (utils/synthetic.py), te the emission-frame time.  After the resample at the
// true jerk the residual phase is
//     t (1 + jerk T^2/(12c)) - (accel + jerk T/2) t^2/(2c),     T = n tsamp,
// so the matching acceleration trial is the acceleration at mid-span, and the
// apparent frequency is the true one times 1 + jerk T^2/(12c).  The `acc` of a
// jerk candidate is that mid-span acceleration.  Reported frequencies and
// periods are corrected back: freq / (1 + jerk T^2/(12c)), period times it
// (jerk_freq_factor).  The engine's own candidates (Candidate::freq) stay
// apparent.
//
// Plan (JerkPlan, per DM).  w is the effective width AccelPlan::step takes at
// that DM, sqrt(t_dm^2 + pulse_width^2 + tsamp^2) in float32 microseconds,
// times 1e-6.  The step is
//     ((2 w) sqrt(tol^2 - 1)) (72 sqrt(3) c) / T^3,
// the jerk offset whose residual cubic peaks at w sqrt(tol^2 - 1) at half a
// step; --jerk_step > 0 replaces it.  Trials are (float)(k step) for every
// integer k with jerk_start <= k step <= jerk_end, which includes 0 when the
// range brackets it; when jerk_start == jerk_end the only trial is that value.
//
// Refused by name before any launch: n > 2^26; a trial with |jf| n^2 / 2 > 0.9
// (more than 0.9 samples per sample at the ends, foldcube's rule); more than
// 4096 jerk trials per DM; jerk_start > jerk_end; a non-finite value; a range
// that holds no trial.
//
// Jerk distillation (host, per DM, after each trial's acceleration
// distillation).  Candidates are taken in descending S/N (a stable sort).  One
// absorbs a weaker one when AccelerationDistiller's relation holds with the
// frequency tolerance f0 tol widened by f0 |jerk0 - jerk| T^2/(12c); as there,
// absorbed candidates are still tested and appended.  With one jerk trial
// nothing changes.  The scan is the plain one, unique candidates times all
// candidates of the DM (no frequency index as the other distillers have above
// a few thousand candidates): fine for tens of jerk trials, a host cost to
// watch at hundreds.  The survivors of all DMs then go through the existing DM
// and harmonic distillers and the scorer unchanged; a candidate's jerk rides
// along in the wrapper record JerkCandidate.
//
// Caveats.  The jerk resample runs on the dedispersed bytes, before whitening.
// Two nearest-neighbour resamplings compose (jerk, then the engine's
// acceleration).  On a padded series (nrow < fft_size) the acceleration's zero
// points are those of fft_size while the jerk's are those of n.  The cost is
// linear in the number of jerk trials.  One device only: -t N, multi-rank runs
// and checkpoints are not supported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "psoup/candidates.hpp"
#include "psoup/cli.hpp"
#include "psoup/common.hpp"
#include "psoup/engine.hpp"
#include "psoup/pipeline.hpp"
#include "psoup/plan.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kJerkThreads = 256;
constexpr int kJerkLane = 16;                            // outputs per lane: one 16-byte store
constexpr int kJerkTile = kJerkThreads * kJerkLane;      // outputs per workgroup

// in: uint8 [nrows][row_stride], each row holding nrow samples; jf: K jerk
// factors on the device; out[(r K + k) out_stride + i] = the definition's y of
// row r at factor k, i < nrow.  n <= nrow is the resampled span.  sp0 <= sp1
// are the stationary points (jerk_stationary).  Any alignment and stride is
// accepted: rows that are not 16-byte aligned in `out` are stored by bytes, and
// an `in` that is not 4-byte aligned is read by bytes.  in and out must not
// overlap.  K <= 4096, nrows <= 65535, n <= 2^26.
void jerk_resample(const uint8_t* in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, const double* jf,
                   int K, uint8_t* out, uint64_t out_stride, int64_t sp0, int64_t sp1, hipStream_t s);

}  // namespace kern

// ---------------------------------------------------------- host steps ----
constexpr uint64_t kJerkMaxSpan = 1ull << 26;
constexpr int kJerkMaxTrials = 4096;
constexpr double kJerkSixC = 6.0 * 299792458.0;

// The definition's jf.
double jerk_factor(float jerk, float tsamp);
// The definition's s(i) for a span n.
int64_t jerk_shift(uint64_t i, uint64_t n, double jf);
// The two stationary points as sample indices, lo <= hi.
void jerk_stationary(uint64_t n, int64_t* lo, int64_t* hi);
// 1 + jerk T^2/(12c), T = n tsamp: apparent frequency over true frequency.
double jerk_freq_factor(float jerk, uint64_t n, float tsamp);
// Throws by name: n > 2^26, a non-finite factor, |jf| n^2 / 2 > 0.9.
void jerk_check(uint64_t n, const std::vector<double>& jf);
// Host transcription of the kernel: x [nrows][row_stride] -> y [nrows K][out_stride].
void jerk_resample_host(const uint8_t* x, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n,
                        const std::vector<double>& jf, uint8_t* y, uint64_t out_stride);

class JerkPlan {
 public:
  JerkPlan() = default;
  // pulse_width [us], tsamp, cfreq and bw as AccelPlan takes them; n is the
  // resampled span; step > 0 replaces the plan's.  Throws by name on a
  // non-finite value and on jerk_start > jerk_end.
  JerkPlan(float jerk_start, float jerk_end, float tol, float step, float pulse_width, uint64_t n, float tsamp,
           float cfreq, float bw, AccelConvention conv = AccelConvention::Legacy);
  double width(float dm) const;  // w, seconds
  double step(float dm) const;
  // Throws by name above 4096 trials and when the range holds none.
  std::vector<float> generate(float dm) const;
  uint64_t span() const { return n_; }

 private:
  float lo_ = 0.f, hi_ = 0.f, tol_ = 1.1f, step_ = 0.f, pulse_width_ = 64.f, tsamp_ = 0.f, cfreq_ = 0.f, bw_ = 0.f;
  uint64_t n_ = 0;
};

// A candidate of the jerk search: the engine's candidate (apparent frequency)
// and the jerk trial it was found at.
struct JerkCandidate {
  Candidate cand;
  float jerk = 0.f;
};
using JerkCandidateList = std::vector<JerkCandidate>;

// The definition's jerk distillation of one DM's candidates.  tobs is the
// acceleration distiller's (fft_size x tsamp, float), span_s = T.
JerkCandidateList jerk_distill(JerkCandidateList cands, float tobs, double span_s, float tol, bool keep_related = true);

// ------------------------------------------------------------- options ----
struct JerkCmdLineOptions {
  CmdLineOptions search;    // peasoup's options of the same names and defaults
  std::string outfilename;  // -o
  float jerk_start = 0.f;
  float jerk_end = 0.f;
  float jerk_tol = 1.10f;
  float jerk_step = 0.f;    // 0 = from the plan
};
// "%Y-%m-%d-%H:%M_jerksearch.output" in UTC.
std::string default_jerk_output_filename();
bool parse_jerk_cmdline(JerkCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// --------------------------------------------------------------- setup ----
struct JerkSetup {
  SearchSetup search;   // the plain search's setup for the same options
  uint64_t nrow = 0;    // samples of a dedispersed row
  uint64_t span = 0;    // n
  JerkPlan plan;
  std::vector<std::vector<float>> jerks;  // per DM
  size_t total_trials = 0;                 // jerk trials over all DMs
};
// Everything that follows from the options and the header; every refusal of
// the definition is raised here, before any device work.
JerkSetup make_jerk_setup(const JerkCmdLineOptions& args, const SigprocHeader& hdr);

// ------------------------------------------------------------ searcher ----
// One device.  Works per DM chunk: dedisperse the chunk, then per group of
// jerk trials resample the chunk's rows into a second buffer, whiten them as
// one batch (SearchEngine::prepare) and search them (search_prepared_many);
// the lists are tagged with their jerk and jerk-distilled per DM.
class JerkSearcher {
 public:
  JerkSearcher(const JerkSetup& setup, const DeviceFilterbank& fb, hipStream_t stream);
  // The per-DM jerk-distilled candidates of DMs [d0, d1) (d1 < 0: all), by DM index.
  JerkCandidateList search(int d0 = 0, int d1 = -1);
  // Folds the first npdmp candidates (1 ms < P < 10 s) on their DM-jerk rows,
  // re-made here, and sorts by max(snr, folded_snr) as the plain search does.
  void fold(JerkCandidateList& cands, int npdmp);
  uint64_t accel_trials() const { return accel_trials_; }
  uint64_t jerk_trials() const { return jerk_trials_; }

 private:
  void resample(const uint8_t* rows, int nrows, const std::vector<float>& jerks, size_t k0, int kc, uint8_t* out);
  const JerkSetup& setup_;
  const DeviceFilterbank& fb_;
  hipStream_t stream_;
  std::unique_ptr<Dedisperser> dd_;
  std::unique_ptr<SearchEngine> engine_;
  uint64_t rstride_ = 0;
  int64_t sp0_ = 0, sp1_ = 0;
  DeviceBuffer<uint8_t> rows_, resampled_;
  DeviceBuffer<double> d_jf_;
  uint64_t accel_trials_ = 0, jerk_trials_ = 0;
};

// DM and harmonic distillation and scoring of the jerk-distilled candidates of
// all DMs (global_distill_and_score on the wrapped candidates).
JerkCandidateList jerk_global_distill(JerkCandidateList cands, const JerkCmdLineOptions& args, const JerkSetup& setup);

// ------------------------------------------------------------ pipeline ----
struct JerkRun {
  JerkCandidateList candidates;  // final, sorted, limited
  JerkSetup setup;
  std::map<std::string, double> timers;  // reading/searching/folding/total (s)
  uint64_t accel_trials = 0, jerk_trials = 0;
};
JerkRun run_jerk_pipeline(const JerkCmdLineOptions& args);
// The text of the output file: the commented header, then one line per
// candidate `period_s dm acc jerk freq nh snr folded_snr dm_idx`.
std::string jerk_output_text(const JerkCmdLineOptions& args, const JerkSetup& setup, const JerkCandidateList& cands);
// Writes it to a temporary file and renames it to args.outfilename.
void write_jerk_output(const JerkCmdLineOptions& args, const JerkSetup& setup, const JerkCandidateList& cands);

}  // namespace psoup
