// orbsearch: circular-orbit templates as an outer loop over the acceleration
// search.  A template (pb, a1, ph) re-indexes a dedispersed uint8 row by the
// Roemer delay of a circular orbit, which makes the row uniform in the orbit
// frame; the unchanged SearchEngine then searches the re-indexed row over its
// acceleration list.  The kernel in csrc/kernels/orbit.hip, the host steps
// (sine table, quantisation, shift, checks, bank parser, grid, distillation, a
// host transcription of the gather, the output text) in
// csrc/src/orbit_host.cpp, OrbitSearcher and the file pipeline in
// csrc/src/orbit.cpp, CLI bin/orbsearch (csrc/apps/orbit_main.cpp).
//
// Definition.  Every double operation below is one correctly rounded IEEE
// operation, in the order written (no FMA contraction).
//
// Signal model.  A pulse emitted at orbit-frame time tau arrives at
//     t = tau + D(tau),   D(tau) = a1 [sin 2 pi (tau / pb + ph) - sin 2 pi ph],
// a1 = a sin i / c in light-seconds, pb in seconds, ph in turns.
//
// Row and span.  x[0..nrow) is a dedispersed row and fft_size the search
// length.  The resampled span is n = min(nrow, fft_size), n <= 2^26 as in
// jerk.hpp.
//
// Quantisation (host).  tsamp is the float32 value the engine uses.
//     W  = (uint64) rint(ldexp((double)tsamp / pb, 64))      pb >= 64 tsamp, so W <= 2^58
//     r  = ph - floor(ph), set to 0 when r >= 1;  F = (uint64) ldexp(r, 64)
//     Aq = (int64) rint(((double)a1 / (double)tsamp) * 256.0)      0 <= Aq < 2^30
//
// Sine table.  int32 T[0..4096], a turn in 4096 steps, Q30.  For j <= 1024
//     T[j] = (int32) rint(ldexp(sin((double)j * (M_PI / 2048)), 30)),
// T[2048 - j] = T[j], and T[2048 + j] = -T[j] for j <= 2048.  So T[1024] = 2^30
// and T[0] = T[2048] = T[4096] = 0.  Built once on the host and passed to the
// kernel, as inject's profile table is.
//
// Sine.  For a uint64 phase th (2^64 = one turn):
//     j = th >> 52,   f = (th >> 32) & 0xFFFFF,
//     S(th) = T[j] + (((int64)(T[j + 1] - T[j]) * f + 2^19) >> 20)
// (an arithmetic shift).
//
// Shift and gather.
//     th_i = F + (uint64)i * W                       (wrapping)
//     s(i) = (Aq * (S(th_i) - S(F)) + 2^37) >> 38    (arithmetic; |Aq (S - S(F))| < 2^61)
//     y[i] = x[clamp(i + s(i), 0, n - 1)]            for i < n
//     y[i] = x[i]                                    for n <= i < nrow
// A template with a1 = 0 is the identity.
//
// Monotonicity.  S is monotone on each half turn between the turning points
// th = 2^62 and 3 2^62: the table is the rounding of a monotone function there
// and the interpolation never leaves [T[j], T[j + 1]].  16 consecutive samples
// cover less than a quarter turn (15 W < 2^62).  So on a lane span with no
// turning point inside, equal shifts at the two ends mean one shift throughout;
// and a span holds a turning point only if the top bit of th + 2^62 differs
// between its ends.  The kernel uses that for its wide-load path.
//
// Convention.  After the resample at the true template the series is uniform
// in tau: the reported frequency is the intrinsic one and needs no correction
// factor, and a residual `acc` is what the template left over.
//
// Refused by name before any launch: n > 2^26; a non-finite value; pb < 64
// tsamp; a1 < 0; Aq >= 2^30; 2 pi a1 / pb > 0.9 (more than 0.9 samples per
// sample, foldcube's rule); an empty bank; more than 2^20 templates; -t other
// than 1.
//
// Templates.  Exactly one source: --bankfile FILE with lines `pb_s a1_ls phase`
// (`#` starts a comment, further columns are ignored, a malformed line is
// refused by its line number), or a regular grid from --pb_start --pb_end --npb
// (geometric: pb_start (pb_end / pb_start)^(k / (npb - 1)), the last one pb_end
// itself), --a1_start --a1_end --na1 (linear: a1_start + (a1_end - a1_start)
// (k / (na1 - 1)), the last one a1_end itself) and --nphase (k / nphase),
// enumerated with pb slowest and phase fastest.  The same bank is used at
// every DM.
//
// Orbit distillation (host, per DM, after each template's acceleration
// distillation; only when the bank has more than one template).  Candidates
// are taken in descending S/N (a stable sort).  A surviving candidate (f0, its
// template's beta0) absorbs a weaker candidate (f, beta) of another template
// when |f / f0 - 1| <= freq_tol + beta0 + beta, beta = ((2 pi) a1) / pb the
// template's largest v/c; as in the other distillers an absorbed candidate is
// still tested against later survivors and appended as an associate.  The
// candidates are looked up through a frequency-sorted index, so the scan is not
// quadratic.  The survivors of all DMs then go through the existing DM and
// harmonic distillers and the scorer unchanged; a candidate's template rides
// along in the wrapper record OrbitCandidate.
//
// Caveats.  The resample runs on the dedispersed bytes, before whitening, so
// the cost is one whitening plus the acceleration list per template and DM.
// Re-indexing is nearest-neighbour.  Clamped ends repeat up to 2 A edge
// samples (A = a1 / tsamp).  One device only: -t N, multi-rank runs and
// checkpoints are not supported.
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

// A quantised template: what the kernel takes.
struct OrbitQuant {
  uint64_t W = 0;   // phase step per sample, 2^64 = one turn
  uint64_t F = 0;   // phase of sample 0
  int64_t Aq = 0;   // amplitude in samples, Q8
};

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kOrbitThreads = 256;
constexpr int kOrbitLane = 16;                               // outputs per lane: one 16-byte store
constexpr int kOrbitTile = kOrbitThreads * kOrbitLane;       // outputs per pass of a workgroup
constexpr int kOrbitTilesPerGroup = 8;                       // passes per workgroup: one table load serves them all
constexpr int kOrbitTable = 4097;                            // entries of the sine table

// in: uint8 [nrows][row_stride], each row holding nrow samples; q: K quantised
// templates on the device; table: the 4097-entry sine table on the device;
// out[(r K + k) out_stride + i] = the definition's y of row r at template k,
// i < nrow.  n <= nrow is the resampled span.  Any alignment and stride is
// accepted: rows that are not 16-byte aligned in `out` are stored by bytes, and
// an `in` that is not 4-byte aligned is read by bytes.  in and out must not
// overlap.  K <= 4096, nrows <= 65535, n <= 2^26.  The templates' ranges (W <=
// 2^58, 0 <= Aq < 2^30) are the caller's to check (orbit_check_quant).
void orbit_resample(const uint8_t* in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, const OrbitQuant* q,
                    int K, const int32_t* table, uint8_t* out, uint64_t out_stride, hipStream_t s);

}  // namespace kern

// ---------------------------------------------------------- host steps ----
constexpr uint64_t kOrbitMaxSpan = 1ull << 26;
constexpr int kOrbitMaxPerLaunch = 4096;
constexpr size_t kOrbitMaxTemplates = 1u << 20;

struct OrbitTemplate {
  double pb = 0.0;  // s
  double a1 = 0.0;  // light-seconds
  double ph = 0.0;  // turns
  bool operator==(const OrbitTemplate& o) const { return pb == o.pb && a1 == o.a1 && ph == o.ph; }
};

// The definition's T[0..4096].
std::vector<int32_t> orbit_sine_table();
// The definition's S(th) on a table of 4097 entries.
int64_t orbit_sine(const int32_t* table, uint64_t th);
// The definition's W, F, Aq.  Throws by name: a non-finite value, pb < 64
// tsamp, a1 < 0, Aq >= 2^30.
OrbitQuant orbit_quantise(double pb, double a1, double ph, float tsamp);
// Throws when a quantised template is outside W <= 2^58, 0 <= Aq < 2^30.
void orbit_check_quant(const OrbitQuant& q);
// The definition's s(i).
int64_t orbit_shift(const int32_t* table, const OrbitQuant& q, uint64_t i);
// ((2 pi) a1) / pb.
double orbit_beta(const OrbitTemplate& t);
// Throws by name: n > 2^26, an empty bank, more than 2^20 templates, and per
// template what orbit_quantise refuses and 2 pi a1 / pb > 0.9.
void orbit_check(uint64_t n, const std::vector<OrbitTemplate>& bank, float tsamp);
// The templates of a bank file's text; a malformed line is refused by its number.
std::vector<OrbitTemplate> orbit_parse_bank(const std::string& text);
// The regular grid, pb slowest and phase fastest.  Throws on a count below 1
// and above 2^20 templates.
std::vector<OrbitTemplate> orbit_grid(double pb_start, double pb_end, int npb, double a1_start, double a1_end, int na1,
                                      int nphase);
// Host transcription of the kernel: x [nrows][row_stride] -> y [nrows K][out_stride].
void orbit_resample_host(const uint8_t* x, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n,
                         const std::vector<OrbitQuant>& q, uint8_t* y, uint64_t out_stride);

// A candidate of the orbit search: the engine's candidate and the index of the
// template it was found at.
struct OrbitCandidate {
  Candidate cand;
  uint32_t tmpl = 0;
};
using OrbitCandidateList = std::vector<OrbitCandidate>;

// The definition's orbit distillation of one DM's candidates; beta[t] is
// orbit_beta of template t.
OrbitCandidateList orbit_distill(OrbitCandidateList cands, const std::vector<double>& beta, float tol,
                                 bool keep_related = true);

// ------------------------------------------------------------- options ----
struct OrbitCmdLineOptions {
  CmdLineOptions search;    // peasoup's options of the same names and defaults
  std::string outfilename;  // -o
  std::string bankfile;     // --bankfile
  double pb_start = 0.0, pb_end = 0.0;
  double a1_start = 0.0, a1_end = 0.0;
  int npb = 0, na1 = 0, nphase = 0;  // 0 0 0: no grid
};
// "%Y-%m-%d-%H:%M_orbsearch.output" in UTC.
std::string default_orbit_output_filename();
bool parse_orbit_cmdline(OrbitCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// --------------------------------------------------------------- setup ----
struct OrbitSetup {
  SearchSetup search;   // the plain search's setup for the same options
  uint64_t nrow = 0;    // samples of a dedispersed row
  uint64_t span = 0;    // n
  std::vector<OrbitTemplate> bank;
  std::vector<OrbitQuant> quant;  // per template
  std::vector<double> beta;       // per template
};
// The bank the options name (file or grid; throws unless exactly one is given).
std::vector<OrbitTemplate> orbit_bank_of(const OrbitCmdLineOptions& args);
// Everything that follows from the options and the header; every refusal of
// the definition is raised here, before any device work.
OrbitSetup make_orbit_setup(const OrbitCmdLineOptions& args, const SigprocHeader& hdr);

// ------------------------------------------------------------ searcher ----
// One device.  Works per DM chunk: dedisperse the chunk, then per group of
// templates resample the chunk's rows into a second buffer, whiten them as one
// batch (SearchEngine::prepare) and search them (search_prepared_many); the
// lists are tagged with their template and orbit-distilled per DM.
class OrbitSearcher {
 public:
  OrbitSearcher(const OrbitSetup& setup, const DeviceFilterbank& fb, hipStream_t stream);
  // The per-DM orbit-distilled candidates of DMs [d0, d1) (d1 < 0: all), by DM index.
  OrbitCandidateList search(int d0 = 0, int d1 = -1);
  // Folds the first npdmp candidates (1 ms < P < 10 s) on their DM-template
  // rows, re-made here, and sorts by max(snr, folded_snr) as the plain search does.
  void fold(OrbitCandidateList& cands, int npdmp);
  uint64_t accel_trials() const { return accel_trials_; }
  uint64_t template_trials() const { return template_trials_; }

 private:
  void resample(const uint8_t* rows, int nrows, size_t k0, int kc, uint8_t* out);
  const OrbitSetup& setup_;
  const DeviceFilterbank& fb_;
  hipStream_t stream_;
  std::unique_ptr<Dedisperser> dd_;
  std::unique_ptr<SearchEngine> engine_;
  uint64_t rstride_ = 0;
  DeviceBuffer<uint8_t> rows_, resampled_;
  DeviceBuffer<OrbitQuant> d_q_;
  DeviceBuffer<int32_t> d_table_;
  uint64_t accel_trials_ = 0, template_trials_ = 0;
};

// DM and harmonic distillation and scoring of the orbit-distilled candidates
// of all DMs (global_distill_and_score on the wrapped candidates).
OrbitCandidateList orbit_global_distill(OrbitCandidateList cands, const OrbitCmdLineOptions& args,
                                        const OrbitSetup& setup);

// ------------------------------------------------------------ pipeline ----
struct OrbitRun {
  OrbitCandidateList candidates;  // final, sorted, limited
  OrbitSetup setup;
  std::map<std::string, double> timers;  // reading/searching/folding/total (s)
  uint64_t accel_trials = 0, template_trials = 0;
};
OrbitRun run_orbit_pipeline(const OrbitCmdLineOptions& args);
// The text of the output file: the commented header, then one line per
// candidate `period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx`.
std::string orbit_output_text(const OrbitCmdLineOptions& args, const OrbitSetup& setup,
                              const OrbitCandidateList& cands);
// Writes it to a temporary file and renames it to args.outfilename.
void write_orbit_output(const OrbitCmdLineOptions& args, const OrbitSetup& setup, const OrbitCandidateList& cands);

}  // namespace psoup
