// orbopt: refines an orbsearch candidate (period, dm, pb, a1, phase) by folding
// its dedispersed row on a dense local grid of circular-orbit templates and
// searching every fold plane over period drift and boxcar width; orbopt is to
// orbsearch what cubeopt is to foldcube.  Kernels in csrc/kernels/orbopt.hip,
// the host steps (grid, steps, sign fold, G, hits, moments, drift table, finish,
// host transcriptions of both kernels, the candidate parser, the file's bytes)
// in csrc/src/orbopt_host.cpp (no device code), OrbitOptimiser / pipeline in
// csrc/src/orbopt.cpp, CLI bin/orbopt (csrc/apps/orbopt_main.cpp).
//
// Definition.  Every double operation below is one correctly rounded IEEE
// operation, evaluated left to right (no FMA contraction); the device part is
// integer throughout.  Two runs agree exactly, and so do the kernels, their
// host transcriptions and the NumPy oracle.
//
// Input.  A candidate is `period_s dm acc pb_s a1_ls phase`, the first six
// columns of an orbsearch output line (`#` starts a comment, further columns
// are ignored, a malformed line is refused by its number).  dm and acc are
// taken as float32.  x[0..nrow) is the dedispersed uint8 row of the filterbank
// at float(dm): DedispGeometry::make on the sorted unique DMs of the accepted
// candidates, then Dedisperser::run_list.  n = min(nrow, fft_size), fft_size as
// in orbsearch (the power of two below the file's samples unless --fft_size):
// the span and the phase origin are the ones the candidate was found with.
// acc is read and written back but NOT used by the fold.
//
// 1. Grid (host).  P = period, ts = double(float(tsamp)), T = n ts, the centre
//    (pb0, a10, ph0).  A step is the user's --pb_step / --a1_step /
//    --phase_step when positive, else
//      da1 = P / (2 nbins)
//      dph = min(1 / 16, P / ((4 pi) a10 nbins))
//      dpb = min(pb0 / 16, (pb0 pb0 P) / ((4 pi) a10 T nbins))
//    (with |a10| for a negative a10, whose centre template is sign-folded as
//    below), and with a10 == 0 a default dph or dpb is 0 and its count becomes 1 (each
//    default is the offset that moves a pulse by about half a phase bin at the
//    worst point of the span).  With odd counts npb, na1, nphase
//      pb = pb0 + (kb - npb / 2) dpb,  a1 = a10 + (ka - na1 / 2) da1,
//      ph = ph0 + (kp - nphase / 2) dph             (integer divisions)
//    enumerated with pb slowest and phase fastest (as orbit_grid); K = npb na1
//    nphase, template K / 2 is the candidate's own.  A negative a1 becomes |a1|
//    at ph + 0.5 (the same delay).  Every template goes through orbit_quantise
//    and orbit_check's rule 2 pi a1 / pb <= 0.9 unchanged.
//
// 2. Fold (device).  G = (uint64) rint(ldexp(ts / P, 64)).  For i < n
//      phi_i = (uint64) i * G (wrapping),  b(i) = ((phi_i >> 32) * nbins) >> 32,
//      j(i) = (i * nints) / n.
//    With s_k(i) = orbit_shift of template k,
//      fold[k][j][b] = sum over i with j(i) = j, b(i) = b of x[clamp(i + s_k(i), 0, n - 1)]
//    kept modulo 2^32 in an int32, and hits[j][b] the number of such i (the same
//    for every template).
//
// 3. Row moments (exact integers).  m = (sum_{i<n} x[i] + n / 2) / n (integer
//    division), V1 = sum_{i<n} (x[i] - m)^2, d[k][j][b] = fold[k][j][b] - m
//    hits[j][b] (modulo 2^32, which is exact: d is a sum of x - m over distinct
//    samples).  A candidate with max(m, 255 - m) * n >= 2^31 is refused: below
//    it every d and every box sum fits an int32.
//
// 4. Search (device, int32): cubeopt's step 3 with the template in place of
//    the DM row.
//      u_j = (j + 0.5) / nints,  L = (l - np / 2) p_step,
//      st[l][j] = rint(L (u_j - 0.5)) reduced into [0, nbins)
//      prof[b] = sum_j d[k][j][(b + st[l][j]) % nbins]
//    Widths w = 1, 2, 4, ... while w <= nbins / 2 (nw of them), S_w[b] the
//    cyclic box sum prof[b] + ... + prof[(b + w - 1) % nbins].  Per width:
//      best_val[w]  = max over all (k, l, b)
//      best_idx[w]  = the smallest flat index (k np + l) nbins + b attaining it
//      tcurve[w][k] = max over l, b
//      centre[w]    = max over b at (K / 2, np / 2)
//    and msum[k] = sum_{j,b} d[k][j][b] as int64.
//
// 5. Finish (host, double).
//      V = double(V1) / nbins
//      snr(S, w, k) = (S - w double(msum[k]) / nbins) / sqrt(V w (1.0 - double(w) / nbins)), 0 when V == 0
//    The optimum width maximises snr(best_val[w], w, k(best_idx[w])); ties go to
//    the smallest w.  snr = that maximum, snr_in the same maximum taken over
//    centre (k = K / 2).  opt_pb, opt_a1, opt_phase are the optimum template
//    after the sign fold; opt_period = 1 / (1 / P - L / (nbins T)); opt_width,
//    opt_bin, opt_k, opt_l from best_idx.  The optimum template's fold plane is
//    copied back from the device and its prof recomputed from it on the host.
//    Flags: bit 0, the optimum lies on a face of the template grid (in a
//    dimension with more than one value) or on the first or last of several
//    drift trials: widen the grid; bit 1, ((|acc| T T) / ((2 c) P)) nbins > 1:
//    the acceleration alone moves a pulse by more than a phase bin over T.
//    V contains the pulse's own power (cubeopt's caveat too).
//
// Ranges: nbins 2..256, nints 1..64, nints * nbins <= 16384, the counts odd,
// K <= 4096, np odd in 1..257.  Refused by name before any launch, as
// "candidate K ..." where it concerns a candidate: everything orbit_quantise or
// orbit_check refuses for any grid template; a period that is not finite or
// below 2 tsamp; a non-finite or negative DM; n > 2^26; the int32 bound of step
// 3; K np nbins >= 2^31; an even count; an empty candidate file; -t other than 1.
//
// Result file, little-endian: "PSOOPT01", uint32 ncand nints nbins npb na1
// nphase np nw (40 bytes so far), uint64 n, double tsamp p_step (64 bytes);
// per candidate double period, float dm, float acc, double pb a1 phase, double
// dpb da1 dph, double snr snr_in opt_period opt_pb opt_a1 opt_phase, uint32
// opt_width opt_bin opt_k opt_l flags, uint32 npb na1 nphase (the counts used:
// K = their product), int64 m V1 (160 bytes), then int32 best_val[nw],
// best_idx[nw], centre[nw], tcurve[nw][K], int64 msum[K], int32
// hits[nints][nbins], fold[nints][nbins], profile[nbins].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "psoup/common.hpp"
#include "psoup/engine.hpp"
#include "psoup/orbit.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kOoptThreads = 256;
constexpr int kOoptLane = 16;                            // samples per lane and pass: one 16-byte window
constexpr int kOoptTile = kOoptThreads * kOoptLane;      // samples per pass of a workgroup
constexpr int kOoptTilesPerGroup = 8;                    // passes per workgroup: one table load serves them all
constexpr int kOoptMaxBins = 256;
constexpr int kOoptMaxInts = 64;
constexpr int kOoptMaxPlane = 16384;                     // nints * nbins: the search keeps the plane in LDS
constexpr int kOoptMaxWidths = 8;
constexpr int kOoptMaxTemplates = 4096;

inline int oopt_nwidths(int nbins) {
  int nw = 1;
  for (int w = 2; w <= nbins / 2; w *= 2) ++nw;
  return nw;
}

// rows: uint8 [..][row_stride] on the device, in_bytes the bytes readable from
// `rows`; candidate c folds row row_of[c] (device int32 [ncand]) with G[c]
// (device uint64 [ncand]) at the templates q[c K .. c K + K) (device), table
// the 4097-entry sine table on the device.  fold: int32 [ncand][K][nints][nbins],
// zeroed and written here.  Any alignment and stride of rows is accepted.  The
// ranges of q (orbit_check_quant), row_of[c] (its row inside in_bytes) and n <=
// 2^26 are the caller's to check.
void orbopt_fold(const uint8_t* rows, uint64_t row_stride, uint64_t in_bytes, const int32_t* row_of, const uint64_t* G,
                 const OrbitQuant* q, int ncand, int K, uint64_t n, int nints, int nbins, const int32_t* table,
                 int32_t* fold, hipStream_t s);

// fold int32 [ncand][K][nints][nbins], hits int32 [ncand][nints][nbins], m
// int32 [ncand], st int32 [np][nints] with every shift in [0, nbins) (checked
// by the caller: the kernel indexes with them).  Outputs, all written here:
// best_val, best_idx, centre int32 [ncand][nw]; tcurve int32 [ncand][nw][K];
// msum int64 [ncand][K].  keys: scratch, uint64 [ncand][nw].
void orbopt_search(const int32_t* fold, const int32_t* hits, const int32_t* m, const int32_t* st, int ncand, int K,
                   int nints, int nbins, int np, uint64_t* keys, int32_t* best_val, int32_t* best_idx, int32_t* tcurve,
                   int32_t* centre, int64_t* msum, hipStream_t s);

}  // namespace kern

// ------------------------------------------------------------- options ----
// orbopt options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct OrbOptCmdLineOptions {
  std::string infilename;    // -i: the filterbank
  std::string candfilename;  // -c: candidate lines (an orbsearch output)
  std::string outfilename;   // -o
  std::string killfilename;  // -k
  unsigned size = 0;         // --fft_size, as orbsearch
  int max_num_threads = 1;   // -t: only 1
  int nbins = 64, nints = 16;
  int npb = 9, na1 = 9, nphase = 9;
  double pb_step = 0.0, a1_step = 0.0, phase_step = 0.0;  // 0: the definition's default
  int np = 33;
  double p_step = 1.0;
  int limit = 100;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_orbopt.oopt" in UTC.
std::string default_oopt_output_filename();
bool parse_oopt_cmdline(OrbOptCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// ---------------------------------------------------------- definitions ----
struct OrbOptParams {
  int nbins = 64, nints = 16;
  int npb = 9, na1 = 9, nphase = 9;
  double pb_step = 0.0, a1_step = 0.0, phase_step = 0.0;
  int np = 33;
  double p_step = 1.0;
};
OrbOptParams oopt_params_of(const OrbOptCmdLineOptions& args);

struct OrbOptCandidate {
  double period = 0;
  float dm = 0, acc = 0;
  double pb = 0, a1 = 0, ph = 0;
};

struct OrbOptGrid {
  int npb = 1, na1 = 1, nphase = 1;  // the counts used
  double dpb = 0, da1 = 0, dph = 0;  // the steps used
  std::vector<OrbitTemplate> tmpl;   // [K], after the sign fold
  std::vector<OrbitQuant> quant;     // [K]
  uint64_t G = 0;
};

struct OrbOptMoments {
  int64_t m = 0, v1 = 0;
};

struct OrbOptSearch {
  std::vector<int32_t> best_val, best_idx, centre;  // [nw]
  std::vector<int32_t> tcurve;                      // [nw][K]
  std::vector<int64_t> msum;                        // [K]
};

struct OrbOptResult {
  OrbOptCandidate cand;
  int npb = 1, na1 = 1, nphase = 1;
  double dpb = 0, da1 = 0, dph = 0;
  double snr = 0, snr_in = 0, opt_period = 0, opt_pb = 0, opt_a1 = 0, opt_phase = 0;
  uint32_t opt_width = 1, opt_bin = 0, opt_k = 0, opt_l = 0, flags = 0;
  int64_t m = 0, v1 = 0;
  OrbOptSearch search;
  std::vector<int32_t> hits, fold;  // [nints][nbins]
  std::vector<int32_t> profile;     // [nbins]
};

// The ranges of the parameters (an even count and the rest), by name.
void oopt_check_params(const OrbOptParams& p);
// Step 1 and G with every refusal that concerns candidate k (its index, for the text).
OrbOptGrid oopt_grid(size_t k, const OrbOptParams& p, const OrbOptCandidate& c, uint64_t n, float tsamp);
// hits int32 [nints][nbins] of step 2.
std::vector<int32_t> oopt_hits(uint64_t G, uint64_t n, int nints, int nbins);
// Step 3 on a row's first n samples; refuses candidate k at the int32 bound.
OrbOptMoments oopt_moments(size_t k, const uint8_t* x, uint64_t n);
// st int32 [np][nints] of step 4.
std::vector<int32_t> oopt_drift_table(const OrbOptParams& p);
// Host transcription of orbopt_fold for one row: int32 [K][nints][nbins].
std::vector<int32_t> orbopt_fold_host(const uint8_t* x, uint64_t n, uint64_t G, const std::vector<OrbitQuant>& q,
                                      int nints, int nbins);
// Host transcription of orbopt_search for one candidate.
OrbOptSearch orbopt_search_host(const int32_t* fold, const int32_t* hits, int32_t m, const int32_t* st, int K, int nints,
                                int nbins, int np);
double oopt_snr(double s, int w, int64_t msum, double v, int nbins);
// Step 5's optimum: the width index, template, drift trial and bin, snr and snr_in.
struct OrbOptOptimum {
  int kw = 0;
  uint32_t k = 0, l = 0, b = 0;
  double snr = 0, snr_in = 0;
};
OrbOptOptimum oopt_optimum(const OrbOptParams& p, const OrbOptGrid& g, const OrbOptMoments& mom,
                           const OrbOptSearch& found);
// Step 5.  fold_opt: the fold plane [nints][nbins] of the optimum's template.
OrbOptResult oopt_finish(const OrbOptParams& p, const OrbOptCandidate& c, const OrbOptGrid& g, uint64_t n, float tsamp,
                         const OrbOptMoments& mom, const std::vector<int32_t>& hits, const std::vector<int32_t>& st,
                         const OrbOptSearch& found, const int32_t* fold_opt);
// The candidates of a file's text; a malformed line is refused by its number.
std::vector<OrbOptCandidate> oopt_parse_candidates(const std::string& text);
// The sorted unique float DMs of the candidates (refuses a non-finite or negative DM by candidate).
std::vector<float> oopt_dm_list(const std::vector<OrbOptCandidate>& cands);

struct OrbOptFileHeader {
  uint32_t ncand = 0, nints = 0, nbins = 0, npb = 0, na1 = 0, nphase = 0, np = 0, nw = 0;
  uint64_t n = 0;
  double tsamp = 0, p_step = 0;
};
// The bytes of the result file (the layout above).
std::vector<char> oopt_file_bytes(const OrbOptFileHeader& h, const std::vector<OrbOptResult>& results);
// Writes them to a temporary file and renames it.
void write_orbopt_file(const std::string& path, const OrbOptFileHeader& h, const std::vector<OrbOptResult>& results);

// ------------------------------------------------------------ optimiser ----
// One device.  fb's geometry holds the DM list oopt_dm_list made of the
// candidates (a candidate's DM must be in it).
class OrbitOptimiser {
 public:
  static constexpr size_t kDefaultBatchBytes = size_t(1) << 30;
  OrbitOptimiser(const OrbOptParams& p, const DeviceFilterbank& fb, uint64_t fft_size, hipStream_t stream,
                 size_t batch_bytes = kDefaultBatchBytes);
  ~OrbitOptimiser();
  // Validates every candidate first (nothing is launched on an error), then
  // works in batches sized to the HBM budget; results in input order.
  std::vector<OrbOptResult> optimise(const std::vector<OrbOptCandidate>& cands);
  // The dedispersed row of DM index d, nrow bytes, on the host.
  std::vector<uint8_t> row(int d);
  uint64_t span() const { return n_; }
  uint64_t nrow() const { return nrow_; }
  float tsamp() const { return tsamp_; }
  uint64_t batches() const { return nbatches_; }
  const OrbOptParams& params() const { return p_; }
  int nwidths() const { return kern::oopt_nwidths(p_.nbins); }

 private:
  OrbOptParams p_;
  const DeviceFilterbank& fb_;
  hipStream_t stream_;
  size_t batch_bytes_;
  uint64_t nrow_ = 0, n_ = 0, rstride_ = 0;
  float tsamp_ = 0;
  uint64_t nbatches_ = 0;
  std::unique_ptr<Dedisperser> dd_;
  DeviceBuffer<int32_t> d_table_;
};

// ------------------------------------------------------------ pipeline ----
struct OrbOptRun {
  OrbOptFileHeader header;
  std::vector<OrbOptResult> results;
  std::map<std::string, double> timers;  // reading, searching, total (s)
};
// Reads args.infilename and args.candfilename, optimises on device 0 and writes args.outfilename.
OrbOptRun run_orbopt_pipeline(const OrbOptCmdLineOptions& args);
// One line of -v.
std::string oopt_verbose_line(const OrbOptResult& r);

}  // namespace psoup
