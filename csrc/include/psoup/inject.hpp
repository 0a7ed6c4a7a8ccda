// filinject: add dispersed pulsars and single bursts to a SIGPROC filterbank of
// 1, 2, 4 or 8 bits, in fixed point with a seeded, counter-based dither, and
// write a file of the same width.  The kernel in csrc/kernels/inject.hip, the
// host steps (tables, sigma, the injection file, the truth numbers, every
// refusal) in csrc/src/inject_host.cpp, the Injector and the file pipeline in
// csrc/src/inject.cpp, CLI bin/filinject (csrc/apps/inject_main.cpp).
//
// Definition.  c is the channel in file order, t the absolute sample index in
// the file, L = 2^nbits - 1.  f_c = fch1 + c foff (MHz), f_mid = fch1 +
// foff (nchans - 1) / 2.  Every double operation below is one correctly
// rounded IEEE operation, in the order written (no FMA contraction).
//
// Injection file: '#' starts a comment; blank lines are skipped; columns are
// positional and separated by blanks:
//     pulsar  period_s  dm  amp  [duty=0.05]  [acc=0]  [phase=0]  [alpha=0]
//     burst   time_s    dm  amp  [width_s=0.005]  [alpha=0]
// as utils/synthetic.py's PulsarSpec / BurstSpec: amp is the peak in units of
// the channel's noise sigma (--units sigma) or in raw levels (--units level);
// duty (turns) and width_s are FWHM; times refer to arrival in channel 0; a
// positive acc (m/s^2) lowers the apparent spin frequency; alpha is a spectral
// index about f_mid.  1 to 64 signals.  Refused by name: an unknown kind, a
// missing or unreadable column, too many columns, a non-finite value, amp < 0,
// period <= 0, duty <= 0, duty > 1, width <= 0, dm < 0, more than 64 signals,
// none at all.
//
// Tables (host, double):
//   D[c]        plan.hpp's generate_delay_table(nchans, tsamp, fch1, foff)[c],
//               the float the dedisperser multiplies the DM with, widened.
//   delay[s][c] = dm_s * D[c]                               (samples, unrounded)
//   sigma[c]    from the exact integer block sums S1, S2 of rfi_block_sums over
//               blocks of 4096 samples: with v_b = (n S2 - S1^2) / (n n) (the
//               numerator an exact integer, n the block's length), sigma[c] =
//               sqrt(median of v_b over the full blocks), the median of an even
//               count being the mean of the two middle values; a file shorter
//               than one block uses its one short block.  A channel of zero
//               variance has sigma 0.  unit[c] = sigma[c] (--units sigma) or 1
//               (--units level), and 0 for a channel the killfile names: such
//               a channel and a dead one are left untouched.
//   widths      w0 = FWHM / 2.3548 (samples for a burst: width_s / tsamp /
//               2.3548; turns for a pulsar: duty / 2.3548).  With smearing
//               sm[c] = 8.3e-6 * dm * |foff| / (f_c / 1000)^3 seconds, taken as
//               sm / tsamp samples for a burst and sm * f0 turns for a pulsar,
//               w[s][c] = sqrt(w0 w0 + sm sm); without, w = w0.
//   inv_w[s][c] = 256 / w[s][c]              (profile-table steps per unit of d)
//   A_q[s][c]   = rint(65536 * (((amp * unit[c]) * pow(f_c / f_mid, alpha)) *
//               (w0 / w[s][c]))), uint32 in Q16 levels; the factor pow(..) is
//               left out when alpha == 0.  Refused by name: any A_q >= 2^24.
//   T[k]        = rint(32768 * exp(-(k k) / (2 * 256 * 256))), k = 0 .. 1536
//               (six sigma in steps of sigma / 256); beyond it a signal adds 0.
//   af = acc / (2 * 299792458), f0 = 1 / period, t_burst = time_s / tsamp.
//
// Per sample (the kernel and utils/reference.py's inject_apply):
//   x = (double)t - delay[s][c]
//   pulsar: te = x * tsamp;  ph = (te - (af * te) * te) * f0 + phase;
//           ph = ph - floor(ph);  d = min(ph, 1 - ph)
//   burst:  d = |x - t_burst|
//   u = d * inv_w[s][c];  if u < 1536.5: k = (int)rint(u)  (ties to even)
//       E += (uint64)A_q[s][c] * T[k]            (Q31 levels over s, < 2^45)
//   z = (seed + 1) * 0x9E3779B97F4A7C15 + (((uint64)c << 40) | t)  (mod 2^64)
//   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB
//   z = z ^ z >> 31
//   add = (E + (z >> 33)) >> 31
//   out = min(in + add, L);  nclip += (in + add > L)
// One draw per sample however many signals overlap, a function of the absolute
// (c, t) alone: chunking, tiling and the launch shape cannot change a byte.
// E = 0 gives add = 0.  touched[s] counts the samples (c, t) with A_q[s][c] > 0
// and u < 1536.5.  t < 2^40 and nchans <= 65535.
//
// Truth numbers, per signal: npulses, the pulses whose peak reaches channel 0
// inside the file (a burst: 1 if 0 <= t_burst < nsamps; a pulsar: with
// ph(te) as above, max(0, floor(ph((nsamps - 1) tsamp)) - ceil(phase) + 1));
// peak, the mean of A_q / 65536 over the channels with unit > 0; snr =
// sqrt(sum_c (A_c / sigma_c)^2 * npulses * ws_c * sqrt(pi)) over those
// channels, A_c = A_q / 65536 and ws_c the width in samples (w for a burst,
// w * period / tsamp for a pulsar): the matched-filter S/N of the expected
// signal in Gaussian noise.  It ignores quantisation, clipping, the dither's
// variance and pulses cut by the file's ends, and is 0 with --units level,
// where no sigma is measured.
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

constexpr int kInjectStatBlock = 4096;  // samples per statistics block
constexpr int kInjectThreads = 256;
constexpr int kInjectLane = 16;                              // samples per lane: one 16-byte load
constexpr int kInjectTile = kInjectThreads * kInjectLane;    // samples per workgroup
constexpr int kInjectMaxSignals = 64;
constexpr int kInjectSteps = 256;                            // profile-table steps per sigma
constexpr int kInjectTableLen = 6 * kInjectSteps + 1;        // T[0 .. 1536]
constexpr int kInjectSigDoubles = 4;                         // per signal: kind, then three constants

// rows: int8 [nchans][stride] (x - bias), 16-byte aligned, stride a multiple of
// 16 and >= count, holding samples [t0, t0 + count) of the file; changed in
// place.  sigc: double [nsig][4] = {0, af, f0, phase} (pulsar) or {1, t_burst,
// 0, 0} (burst); delay, inv_w: double [nsig][nchans]; A_q: uint32
// [nsig][nchans]; T: uint16 [kInjectTableLen].  seed_mul = (seed + 1) *
// 0x9E3779B97F4A7C15.  nclip (one uint64) takes one atomic add per workgroup
// that clipped; touched (uint64 [nsig], may be null) one per signal and
// workgroup.  Both are zeroed by the caller.  No table may be written while
// the kernel runs.
void inject(int8_t* rows, uint64_t stride, uint64_t count, int nchans, int nbits, int bias, uint64_t t0, int nsig,
            const double* sigc, double tsamp, const double* delay, const double* inv_w, const uint32_t* A_q,
            const uint16_t* T, uint64_t seed_mul, unsigned long long* nclip, unsigned long long* touched,
            hipStream_t s);

}  // namespace kern

// The dither's 64-bit draw for sample (c, t): the definition's z.
constexpr uint64_t kInjectGolden = 0x9E3779B97F4A7C15ull;
inline uint64_t inject_seed_mul(uint64_t seed) { return (seed + 1ull) * kInjectGolden; }
__host__ __device__ inline uint64_t inject_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t inject_hash(uint64_t seed, uint64_t c, uint64_t t) {
  return inject_mix(inject_seed_mul(seed) + ((c << 40) | t));
}

// -------------------------------------------------------------- signals ----
enum class InjectKind : int { Pulsar = 0, Burst = 1 };

struct InjectSignal {
  InjectKind kind = InjectKind::Pulsar;
  double t = 0.25;      // period (pulsar) or arrival time in channel 0 (burst), seconds
  double dm = 0;        // pc cm^-3
  double amp = 0;       // peak, in sigma or levels
  double width = 0.05;  // FWHM: duty in turns (pulsar), seconds (burst)
  double acc = 0;       // m/s^2 (pulsar)
  double phase = 0;     // turns (pulsar)
  double alpha = 0;     // spectral index about the band centre
};
// Throws by name (see the definition) unless every signal can be injected.
void inject_check_signals(const std::vector<InjectSignal>& signals);
// The injection file's text / the file itself; checked.
std::vector<InjectSignal> inject_parse(const std::string& text);
std::vector<InjectSignal> inject_read_file(const std::string& path);

struct InjectGeometry {
  int nchans = 0, nbits = 8;
  uint64_t nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0;
};
// Throws by name unless nbits is 1/2/4/8, 1 <= nchans <= 65535 with nchans *
// nbits a multiple of 8, 1 <= nsamps < 2^40, tsamp > 0, foff != 0 and every
// channel's frequency is positive.
void inject_check_geometry(const InjectGeometry& g);

// ---------------------------------------------------------- host tables ----
struct InjectTables {
  int nsig = 0, nchans = 0;
  double tsamp = 0;
  std::vector<double> sigc;    // [nsig][4]
  std::vector<double> delay;   // [nsig][nchans]
  std::vector<double> inv_w;   // [nsig][nchans]
  std::vector<double> w;       // [nsig][nchans] the width (samples or turns)
  std::vector<uint32_t> A_q;   // [nsig][nchans]
  std::vector<uint16_t> T;     // [kInjectTableLen]
  int nlive = 0;               // channels with unit > 0
};
std::vector<uint16_t> inject_profile_table();
// sigma[c] from the block sums S1, S2 [nchans][nblk] of blocks of 4096 samples.
std::vector<double> inject_sigma(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nchans,
                                 uint64_t nsamps);
// unit[c]: sigma[c] (or 1 when sigma is empty: --units level), 0 where killed.
std::vector<double> inject_unit(const std::vector<double>& sigma, const std::vector<int>& killmask, int nchans);
// Checks the signals and the geometry and builds the tables; throws by name
// when an A_q reaches 2^24.
InjectTables inject_tables(const std::vector<InjectSignal>& signals, const InjectGeometry& g,
                           const std::vector<double>& unit, bool smear);

struct InjectTruth {
  uint64_t npulses = 0;
  double peak = 0, snr = 0;
};
// sigma empty (--units level): snr = 0.
std::vector<InjectTruth> inject_truth(const std::vector<InjectSignal>& signals, const InjectTables& tab,
                                      const InjectGeometry& g, const std::vector<double>& unit,
                                      const std::vector<double>& sigma);
// One line per signal: the kind, its parameters as parsed (%.17g), then
// npulses, peak and snr; '#' header lines in front.
std::string inject_truth_text(const std::vector<InjectSignal>& signals, const std::vector<InjectTruth>& truth,
                              const std::string& units, uint64_t seed);

// -------------------------------------------------------------- options ----
// filinject options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct InjectCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string injfilename;    // --injfile
  std::string killfilename;   // -k
  std::string truthfilename;  // --truth_out
  uint64_t seed = 0;
  std::string units = "sigma";  // sigma | level
  bool no_smear = false;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_filinject.fil" in UTC.
std::string default_inject_output_filename();
bool parse_inject_cmdline(InjectCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// ------------------------------------------------------------- injector ----
struct InjectResult {
  uint64_t nsamps = 0, nclip = 0;
  int nchans = 0, chunks = 0, nlive = 0;
  std::vector<double> sigma;      // [nchans]; empty with level units
  std::vector<uint64_t> touched;  // [nsig]
  std::vector<InjectTruth> truth; // [nsig]
  InjectTables tables;
};

class Injector {
 public:
  static constexpr size_t kDefaultBudgetBytes = size_t(2) << 30;
  // h_packed: the file's data block in host memory, nsamps * nchans * nbits / 8
  // bytes.  budget_bytes: device bytes the packed bytes and the unpacked rows
  // of one time chunk may hold (a chunk is a whole number of 4096-blocks, at
  // least one).  Validates everything (signals, geometry, the killmask's size,
  // the units) and throws by name; launches and uploads nothing.
  Injector(const uint8_t* h_packed, const InjectGeometry& g, const std::vector<InjectSignal>& signals,
           const std::vector<int>& killmask, bool sigma_units, bool smear, uint64_t seed, hipStream_t stream,
           size_t budget_bytes = kDefaultBudgetBytes);
  // The whole chain into h_out (as many bytes as the input): the statistics
  // pass (sigma units only), the tables, the injection pass.  Synchronises.
  InjectResult run(uint8_t* h_out);
  uint64_t chunk_samples() const { return chunk_; }

  // The kernel alone on device rows with explicit host tables (the torch op's
  // path); uploads the tables, synchronises the stream, returns nclip.
  static uint64_t apply(int8_t* d_rows, uint64_t stride, uint64_t count, int nbits, int bias, uint64_t t0,
                        const InjectTables& tab, uint64_t seed, std::vector<uint64_t>* touched, hipStream_t stream);

 private:
  const uint8_t* x_;
  InjectGeometry g_;
  std::vector<InjectSignal> signals_;
  std::vector<int> kill_;
  bool sigma_units_, smear_;
  uint64_t seed_;
  hipStream_t stream_;
  uint64_t chunk_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct InjectRun {
  InjectResult result;
  std::vector<InjectSignal> signals;
  std::map<std::string, double> timers;  // reading, injecting, writing, total (s)
};
// Reads the filterbank, the injection file and the killfile, injects on the
// current device and writes the .fil (the header bytes verbatim; temporary
// file + rename) and, with --truth_out, the truth file.
InjectRun run_inject_pipeline(const InjectCmdLineOptions& args);

}  // namespace psoup
