// jerksearch, host side (no device code): the jerk factor, the shift, the
// checks, JerkPlan, the jerk distillation, the frequency correction, a host
// transcription of the gather and the text of the output file.  See
// psoup/jerk.hpp.  Compiled without FMA contraction.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <sstream>

#include "psoup/jerk.hpp"

namespace psoup {

namespace {
constexpr double kC = 299792458.0;
}

double jerk_factor(float jerk, float tsamp) {
  return ((static_cast<double>(jerk) * static_cast<double>(tsamp)) * static_cast<double>(tsamp)) / kJerkSixC;
}

int64_t jerk_shift(uint64_t i, uint64_t n, double jf) {
  const int64_t I = static_cast<int64_t>(i), N = static_cast<int64_t>(n), H = N / 2;
  const double g = ((static_cast<double>(I) * static_cast<double>(I - H)) * static_cast<double>(I - N)) * jf;
  return static_cast<int64_t>(std::rint(g));
}

void jerk_stationary(uint64_t n, int64_t* lo, int64_t* hi) {
  const double h = static_cast<double>(n / 2), N = static_cast<double>(n);
  const double b = h + N;
  const double d = std::sqrt(std::max(0.0, b * b - 3.0 * h * N));
  *lo = static_cast<int64_t>(std::floor((b - d) / 3.0));
  *hi = static_cast<int64_t>(std::floor((b + d) / 3.0));
}

double jerk_freq_factor(float jerk, uint64_t n, float tsamp) {
  const double T = static_cast<double>(n) * static_cast<double>(tsamp);
  return 1.0 + ((static_cast<double>(jerk) * T) * T) / (12.0 * kC);
}

void jerk_check(uint64_t n, const std::vector<double>& jf) {
  PSOUP_CHECK(n >= 1, "jerk: empty series");
  PSOUP_CHECK(n <= kJerkMaxSpan, "jerk: series longer than 2^26 samples (n = " << n << ")");
  const double N = static_cast<double>(n);
  for (double f : jf) {
    PSOUP_CHECK(std::isfinite(f), "jerk: a non-finite value (jerk factor)");
    PSOUP_CHECK(!((std::fabs(f) * N) * N / 2.0 > 0.9),
                "jerk: a trial moves more than 0.9 samples per sample at the ends (|jf| n^2 / 2 = "
                    << (std::fabs(f) * N) * N / 2.0 << ")");
  }
}

void jerk_resample_host(const uint8_t* x, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n,
                        const std::vector<double>& jf, uint8_t* y, uint64_t out_stride) {
  PSOUP_CHECK(x != nullptr && y != nullptr, "jerk_resample: missing buffer");
  PSOUP_CHECK(nrows >= 1 && !jf.empty(), "jerk_resample: no rows or no jerk factors");
  PSOUP_CHECK(n >= 1 && n <= nrow, "jerk_resample: the span must be in 1..nrow");
  PSOUP_CHECK(n <= kJerkMaxSpan, "jerk: series longer than 2^26 samples");
  PSOUP_CHECK(row_stride >= nrow && out_stride >= nrow, "jerk_resample: a stride is shorter than the row");
  const size_t K = jf.size();
  const int64_t N = static_cast<int64_t>(n);
  for (int r = 0; r < nrows; ++r)
    for (size_t k = 0; k < K; ++k) {
      const uint8_t* xr = x + static_cast<uint64_t>(r) * row_stride;
      uint8_t* yr = y + (static_cast<uint64_t>(r) * K + k) * out_stride;
      for (uint64_t i = 0; i < n; ++i) {
        const int64_t j = static_cast<int64_t>(i) + jerk_shift(i, n, jf[k]);
        yr[i] = xr[std::min(std::max<int64_t>(j, 0), N - 1)];
      }
      for (uint64_t i = n; i < nrow; ++i) yr[i] = xr[i];
    }
}

// ----------------------------------------------------------------- plan ----
JerkPlan::JerkPlan(float jerk_start, float jerk_end, float tol, float step, float pulse_width, uint64_t n, float tsamp,
                   float cfreq, float bw, AccelConvention conv)
    : lo_(jerk_start), hi_(jerk_end), tol_(tol), step_(step), pulse_width_(pulse_width), tsamp_(tsamp), cfreq_(cfreq),
      bw_(std::fabs(bw)), n_(n) {
  PSOUP_CHECK(std::isfinite(jerk_start) && std::isfinite(jerk_end) && std::isfinite(tol) && std::isfinite(step) &&
                  std::isfinite(pulse_width) && std::isfinite(tsamp) && std::isfinite(cfreq) && std::isfinite(bw),
              "jerk: a non-finite value (plan)");
  PSOUP_CHECK(!(jerk_start > jerk_end), "jerk: jerk_start > jerk_end (" << jerk_start << " > " << jerk_end << ")");
  PSOUP_CHECK(step >= 0.f, "jerk: jerk_step must not be negative");
  PSOUP_CHECK(n >= 1 && tsamp > 0.f, "jerk: empty series or non-positive tsamp");
  if (conv == AccelConvention::Reference) pulse_width_ = static_cast<float>(pulse_width_ / 1.0e3);
}

double JerkPlan::width(float dm) const {
  // AccelPlan::step's effective width (float32 microseconds)
  float tdm = static_cast<float>(std::pow(8.3 * bw_ / std::pow(static_cast<double>(cfreq_), 3.0) * dm, 2.0));
  float tpulse = pulse_width_ * pulse_width_;
  float ttsamp = tsamp_ * tsamp_;
  float w_us = std::sqrt(tdm + tpulse + ttsamp);
  return static_cast<double>(w_us) * 1.0e-6;
}

double JerkPlan::step(float dm) const {
  if (step_ > 0.f) return static_cast<double>(step_);
  const double T = static_cast<double>(n_) * static_cast<double>(tsamp_);
  const double tol = static_cast<double>(tol_);
  return ((2.0 * width(dm)) * std::sqrt(tol * tol - 1.0)) * ((72.0 * std::sqrt(3.0)) * kC) / ((T * T) * T);
}

std::vector<float> JerkPlan::generate(float dm) const {
  std::vector<float> list;
  if (lo_ == hi_) {
    list.push_back(lo_);
    return list;
  }
  const double st = step(dm), lo = lo_, hi = hi_;
  PSOUP_CHECK(std::isfinite(st) && st > 0.0, "jerk: a non-finite value (the jerk step is " << st << ")");
  const double ka = std::ceil(lo / st), kb = std::floor(hi / st);
  PSOUP_CHECK(kb - ka + 1.0 <= 2.0 * kJerkMaxTrials,
              "jerk: more than " << kJerkMaxTrials << " jerk trials per DM (step " << st << " over [" << lo << ", "
                                 << hi << "])");
  int64_t k0 = static_cast<int64_t>(ka), k1 = static_cast<int64_t>(kb);
  // the divisions round: settle the ends on the products themselves
  while (static_cast<double>(k0) * st < lo) ++k0;
  while (static_cast<double>(k0 - 1) * st >= lo) --k0;
  while (static_cast<double>(k1) * st > hi) --k1;
  while (static_cast<double>(k1 + 1) * st <= hi) ++k1;
  PSOUP_CHECK(k1 - k0 + 1 <= kJerkMaxTrials,
              "jerk: more than " << kJerkMaxTrials << " jerk trials per DM (step " << st << " over [" << lo << ", "
                                 << hi << "])");
  PSOUP_CHECK(k1 >= k0, "jerk: no trial k * step in [" << lo << ", " << hi << "] (step " << st << ")");
  for (int64_t k = k0; k <= k1; ++k) list.push_back(static_cast<float>(static_cast<double>(k) * st));
  return list;
}

// --------------------------------------------------------- distillation ----
JerkCandidateList jerk_distill(JerkCandidateList cands, float tobs, double span_s, float tol, bool keep_related) {
  std::stable_sort(cands.begin(), cands.end(),
                   [](const JerkCandidate& a, const JerkCandidate& b) { return a.cand.snr > b.cand.snr; });
  const size_t size = cands.size();
  const double toc = tobs / kC;  // as AccelerationDistiller: float tobs over c
  const double jw = (span_s * span_s) / (12.0 * kC);
  std::vector<char> unique(size, 1);
  for (size_t idx = 0; idx < size; ++idx) {
    if (!unique[idx]) continue;
    const double f0 = cands[idx].cand.freq, a0 = cands[idx].cand.acc, j0 = cands[idx].jerk;
    for (size_t ii = idx + 1; ii < size; ++ii) {
      const double edge = f0 * tol + (f0 * std::fabs(j0 - static_cast<double>(cands[ii].jerk))) * jw;
      const double acc_freq = static_cast<float>(f0 + (a0 - cands[ii].cand.acc) * f0 * toc);
      const double f = cands[ii].cand.freq;
      const bool rel = acc_freq > f0 ? (f > f0 - edge && f < acc_freq + edge) : (f < f0 + edge && f > acc_freq - edge);
      if (rel) {
        if (keep_related) cands[idx].cand.append(cands[ii].cand);
        unique[ii] = 0;
      }
    }
  }
  JerkCandidateList out;
  for (size_t i = 0; i < size; ++i)
    if (unique[i]) out.push_back(std::move(cands[i]));
  return out;
}

// --------------------------------------------------------------- output ----
std::string jerk_output_text(const JerkCmdLineOptions& args, const JerkSetup& setup, const JerkCandidateList& cands) {
  const CmdLineOptions& a = args.search;
  const float tsamp = setup.search.search.tsamp;
  std::ostringstream os;
  char b[512];
  os << "# jerksearch: jerk trials as an outer loop over the acceleration search\n";
  os << "# input " << a.infilename << "\n";
  std::snprintf(b, sizeof b, "# dm_start %g dm_end %g dm_tol %g dm_pulse_width %g\n", a.dm_start, a.dm_end, a.dm_tol,
                a.dm_pulse_width);
  os << b;
  std::snprintf(b, sizeof b, "# acc_start %g acc_end %g acc_tol %g acc_pulse_width %g accel_convention %s\n",
                a.acc_start, a.acc_end, a.acc_tol, a.acc_pulse_width, a.accel_convention.c_str());
  os << b;
  std::snprintf(b, sizeof b, "# jerk_start %g jerk_end %g jerk_tol %g jerk_step %g\n", args.jerk_start, args.jerk_end,
                args.jerk_tol, args.jerk_step);
  os << b;
  std::snprintf(b, sizeof b, "# nharmonics %d min_snr %g min_freq %g max_freq %g npdmp %d limit %d dedisp_kernel %s\n",
                a.nharmonics, a.min_snr, a.min_freq, a.max_freq, a.npdmp, a.limit, a.dedisp_kernel.c_str());
  os << b;
  std::snprintf(b, sizeof b, "# fft_size %llu row_samples %llu span %llu tsamp %.9g\n",
                static_cast<unsigned long long>(setup.search.fft_size), static_cast<unsigned long long>(setup.nrow),
                static_cast<unsigned long long>(setup.span), static_cast<double>(tsamp));
  os << b;
  os << "# killfile " << (a.killfilename.empty() ? "-" : a.killfilename) << " zapfile "
     << (a.zapfilename.empty() ? "-" : a.zapfilename) << "\n";
  os << "# jerk trials per DM (dm: trials, first, last):\n";
  for (size_t d = 0; d < setup.jerks.size(); ++d) {
    const std::vector<float>& j = setup.jerks[d];
    std::snprintf(b, sizeof b, "#   %.9g: %zu %.9g %.9g\n", static_cast<double>(setup.search.dm_list[d]), j.size(),
                  static_cast<double>(j.front()), static_cast<double>(j.back()));
    os << b;
  }
  os << "# acc is the acceleration at mid-span (accel + jerk T / 2, T = span x tsamp).\n";
  os << "# period_s and freq are corrected for the jerk resample: freq = apparent / (1 + jerk T^2 / (12 c)).\n";
  os << "# period_s dm acc jerk freq nh snr folded_snr dm_idx\n";
  for (const JerkCandidate& c : cands) {
    const double k = jerk_freq_factor(c.jerk, setup.span, tsamp);
    const double freq = static_cast<double>(c.cand.freq) / k;
    std::snprintf(b, sizeof b, "%.12g %.9g %.9g %.9g %.12g %d %.9g %.9g %d\n", 1.0 / freq,
                  static_cast<double>(c.cand.dm), static_cast<double>(c.cand.acc), static_cast<double>(c.jerk), freq,
                  c.cand.nh, static_cast<double>(c.cand.snr), static_cast<double>(c.cand.folded_snr), c.cand.dm_idx);
    os << b;
  }
  return os.str();
}

}  // namespace psoup
