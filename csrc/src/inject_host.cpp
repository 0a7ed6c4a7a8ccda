// filinject, host steps: the signal checks, the injection file's parser, the
// geometry checks, sigma from the block sums, the per-channel tables, the
// profile table and the truth numbers of psoup/inject.hpp.  No device code
// here (the native unit tests link this file with plan.cpp and common.cpp
// alone) and no FMA contraction: the double arithmetic is the definition's,
// operation by operation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "psoup/inject.hpp"
#include "psoup/plan.hpp"

namespace psoup {

namespace {

constexpr double kFwhm = 2.3548;
constexpr double kLight = 299792458.0;

// numpy.median: the mean of the two middle values for an even count
double median_of(std::vector<double> v) {
  const size_t n = v.size();
  std::sort(v.begin(), v.end());
  return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

bool parse_double(const std::string& s, double& out) {
  if (s.empty()) return false;
  char* end = nullptr;
  out = std::strtod(s.c_str(), &end);
  return end == s.c_str() + s.size();
}

const char* kind_name(InjectKind k) { return k == InjectKind::Burst ? "burst" : "pulsar"; }

double pulsar_phase(double te, double af, double f0, double phase) { return (te - (af * te) * te) * f0 + phase; }

}  // namespace

void inject_check_signals(const std::vector<InjectSignal>& signals) {
  PSOUP_CHECK(!signals.empty(), "inject: no signal to inject");
  PSOUP_CHECK(signals.size() <= static_cast<size_t>(kern::kInjectMaxSignals),
              "inject: more than 64 signals (" << signals.size() << ")");
  for (size_t i = 0; i < signals.size(); ++i) {
    const InjectSignal& s = signals[i];
    const bool burst = s.kind == InjectKind::Burst;
    PSOUP_CHECK(s.kind == InjectKind::Pulsar || burst, "inject: signal " << i << ": unknown kind");
    PSOUP_CHECK(std::isfinite(s.t) && std::isfinite(s.dm) && std::isfinite(s.amp) && std::isfinite(s.width) &&
                    std::isfinite(s.acc) && std::isfinite(s.phase) && std::isfinite(s.alpha),
                "inject: signal " << i << ": a value is not finite");
    PSOUP_CHECK(s.amp >= 0, "inject: signal " << i << ": amp must not be negative, got " << s.amp);
    PSOUP_CHECK(s.dm >= 0, "inject: signal " << i << ": dm must not be negative, got " << s.dm);
    if (burst) {
      PSOUP_CHECK(s.width > 0, "inject: signal " << i << ": width must be positive, got " << s.width);
    } else {
      PSOUP_CHECK(s.t > 0, "inject: signal " << i << ": period must be positive, got " << s.t);
      PSOUP_CHECK(s.width > 0, "inject: signal " << i << ": duty must be positive, got " << s.width);
      PSOUP_CHECK(s.width <= 1, "inject: signal " << i << ": duty must not exceed 1, got " << s.width);
    }
  }
}

std::vector<InjectSignal> inject_parse(const std::string& text) {
  std::vector<InjectSignal> out;
  std::istringstream in(text);
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    std::istringstream ls(line);
    std::vector<std::string> tok;
    for (std::string w; ls >> w;) tok.push_back(w);
    if (tok.empty()) continue;
    InjectSignal s;
    size_t maxcol;
    if (tok[0] == "pulsar") {
      s.kind = InjectKind::Pulsar;
      s.width = 0.05;
      maxcol = 8;
    } else if (tok[0] == "burst") {
      s.kind = InjectKind::Burst;
      s.width = 0.005;
      maxcol = 6;
    } else {
      PSOUP_THROW("inject: line " << lineno << ": unknown kind '" << tok[0] << "' (pulsar or burst)");
    }
    PSOUP_CHECK(tok.size() >= 4, "inject: line " << lineno << ": " << tok[0] << " needs at least "
                                                 << (s.kind == InjectKind::Burst ? "time_s" : "period_s")
                                                 << ", dm and amp");
    PSOUP_CHECK(tok.size() <= maxcol, "inject: line " << lineno << ": too many columns for a " << tok[0]);
    double* pulsar_cols[] = {&s.t, &s.dm, &s.amp, &s.width, &s.acc, &s.phase, &s.alpha};
    double* burst_cols[] = {&s.t, &s.dm, &s.amp, &s.width, &s.alpha};
    double** cols = s.kind == InjectKind::Burst ? burst_cols : pulsar_cols;
    for (size_t i = 1; i < tok.size(); ++i)
      PSOUP_CHECK(parse_double(tok[i], *cols[i - 1]),
                  "inject: line " << lineno << ": cannot read column " << i << " '" << tok[i] << "'");
    out.push_back(s);
    PSOUP_CHECK(out.size() <= static_cast<size_t>(kern::kInjectMaxSignals), "inject: more than 64 signals");
  }
  inject_check_signals(out);
  return out;
}

std::vector<InjectSignal> inject_read_file(const std::string& path) {
  std::ifstream in(path);
  PSOUP_CHECK(static_cast<bool>(in), "inject: cannot open the injection file " << path);
  std::ostringstream ss;
  ss << in.rdbuf();
  return inject_parse(ss.str());
}

void inject_check_geometry(const InjectGeometry& g) {
  PSOUP_CHECK(g.nbits == 1 || g.nbits == 2 || g.nbits == 4 || g.nbits == 8,
              "inject: nbits must be 1, 2, 4 or 8, got " << g.nbits);
  PSOUP_CHECK(g.nchans >= 1 && g.nchans <= 65535, "inject: nchans must be in 1..65535, got " << g.nchans);
  PSOUP_CHECK((static_cast<uint64_t>(g.nchans) * static_cast<uint64_t>(g.nbits)) % 8 == 0,
              "inject: nchans * nbits must be a multiple of 8");
  PSOUP_CHECK(g.nsamps >= 1, "inject: the input is shorter than one sample");
  PSOUP_CHECK(g.nsamps < (1ull << 40), "inject: too many samples");
  PSOUP_CHECK(std::isfinite(g.tsamp) && g.tsamp > 0, "inject: tsamp must be positive");
  PSOUP_CHECK(std::isfinite(g.foff) && g.foff != 0, "inject: foff must not be zero");
  const double f_last = g.fch1 + static_cast<double>(g.nchans - 1) * g.foff;
  PSOUP_CHECK(std::isfinite(g.fch1) && g.fch1 > 0 && f_last > 0, "inject: every channel's frequency must be positive");
}

std::vector<uint16_t> inject_profile_table() {
  std::vector<uint16_t> T(static_cast<size_t>(kern::kInjectTableLen));
  const double two_s2 = 2.0 * kern::kInjectSteps * kern::kInjectSteps;
  for (int k = 0; k < kern::kInjectTableLen; ++k) {
    const double kk = static_cast<double>(k) * static_cast<double>(k);
    T[static_cast<size_t>(k)] = static_cast<uint16_t>(std::rint(32768.0 * std::exp(-kk / two_s2)));
  }
  return T;
}

std::vector<double> inject_sigma(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nchans,
                                 uint64_t nsamps) {
  constexpr uint64_t kL = kern::kInjectStatBlock;
  PSOUP_CHECK(nchans >= 1 && nsamps >= 1, "inject_sigma: empty table");
  const size_t nc = static_cast<size_t>(nchans);
  const size_t nblk = static_cast<size_t>((nsamps + kL - 1) / kL);
  PSOUP_CHECK(S1.size() == nc * nblk && S2.size() == nc * nblk, "inject_sigma: S1 and S2 must be [nchans][nblk]");
  const size_t nfull = static_cast<size_t>(nsamps / kL);
  std::vector<double> sigma(nc, 0.0), v;
  for (size_t c = 0; c < nc; ++c) {
    v.clear();
    const size_t nuse = nfull ? nfull : 1;
    for (size_t b = 0; b < nuse; ++b) {
      const uint64_t n = nfull ? kL : nsamps;
      const size_t i = c * nblk + b;
      const unsigned __int128 lhs = static_cast<unsigned __int128>(n) * S2[i];
      const unsigned __int128 rhs = static_cast<unsigned __int128>(S1[i]) * S1[i];
      PSOUP_CHECK(lhs >= rhs, "inject_sigma: channel " << c << " block " << b << ": S1^2 exceeds n S2");
      const double dn = static_cast<double>(n);
      v.push_back(static_cast<double>(static_cast<uint64_t>(lhs - rhs)) / (dn * dn));
    }
    sigma[c] = std::sqrt(median_of(v));
  }
  return sigma;
}

std::vector<double> inject_unit(const std::vector<double>& sigma, const std::vector<int>& killmask, int nchans) {
  const size_t nc = static_cast<size_t>(nchans);
  PSOUP_CHECK(sigma.empty() || sigma.size() == nc, "inject: sigma size != nchans");
  PSOUP_CHECK(killmask.empty() || killmask.size() == nc, "inject: killmask size != nchans");
  std::vector<double> unit(nc, 1.0);
  for (size_t c = 0; c < nc; ++c) {
    if (!sigma.empty()) unit[c] = sigma[c];
    if (!killmask.empty() && killmask[c] == 0) unit[c] = 0.0;
  }
  return unit;
}

InjectTables inject_tables(const std::vector<InjectSignal>& signals, const InjectGeometry& g,
                           const std::vector<double>& unit, bool smear) {
  inject_check_signals(signals);
  inject_check_geometry(g);
  const size_t nc = static_cast<size_t>(g.nchans), ns = signals.size();
  PSOUP_CHECK(unit.size() == nc, "inject: unit size != nchans");
  for (double u : unit) PSOUP_CHECK(std::isfinite(u) && u >= 0, "inject: a channel's unit is negative or not finite");
  InjectTables t;
  t.nsig = static_cast<int>(ns);
  t.nchans = g.nchans;
  t.tsamp = g.tsamp;
  t.sigc.assign(ns * kern::kInjectSigDoubles, 0.0);
  t.delay.resize(ns * nc);
  t.inv_w.resize(ns * nc);
  t.w.resize(ns * nc);
  t.A_q.resize(ns * nc);
  t.T = inject_profile_table();
  for (double u : unit) t.nlive += u > 0;
  const std::vector<float> D = generate_delay_table(g.nchans, g.tsamp, g.fch1, g.foff);
  const double f_mid = g.fch1 + g.foff * static_cast<double>(g.nchans - 1) / 2.0;
  for (size_t s = 0; s < ns; ++s) {
    const InjectSignal& sg = signals[s];
    const bool burst = sg.kind == InjectKind::Burst;
    double* k = &t.sigc[s * kern::kInjectSigDoubles];
    const double f0 = burst ? 0.0 : 1.0 / sg.t;
    if (burst) {
      k[0] = 1.0;
      k[1] = sg.t / g.tsamp;
    } else {
      k[0] = 0.0;
      k[1] = sg.acc / (2.0 * kLight);
      k[2] = f0;
      k[3] = sg.phase;
    }
    const double w0 = burst ? sg.width / g.tsamp / kFwhm : sg.width / kFwhm;
    for (size_t c = 0; c < nc; ++c) {
      const size_t i = s * nc + c;
      const double f_c = g.fch1 + static_cast<double>(c) * g.foff;
      t.delay[i] = sg.dm * static_cast<double>(D[c]);
      double w = w0;
      if (smear) {
        const double fg = f_c / 1000.0;
        const double sm_s = 8.3e-6 * sg.dm * std::fabs(g.foff) / (fg * fg * fg);
        const double sm = burst ? sm_s / g.tsamp : sm_s * f0;
        w = std::sqrt(w0 * w0 + sm * sm);
      }
      t.w[i] = w;
      t.inv_w[i] = static_cast<double>(kern::kInjectSteps) / w;
      double a = sg.amp * unit[c];
      if (sg.alpha != 0) a = a * std::pow(f_c / f_mid, sg.alpha);
      a = a * (w0 / w);
      const double q = std::rint(65536.0 * a);
      PSOUP_CHECK(q < 16777216.0, "inject: signal " << s << " (" << kind_name(sg.kind) << ") channel " << c
                                                    << ": the amplitude reaches 256 levels (A_q >= 2^24)");
      t.A_q[i] = static_cast<uint32_t>(q);
    }
  }
  return t;
}

std::vector<InjectTruth> inject_truth(const std::vector<InjectSignal>& signals, const InjectTables& tab,
                                      const InjectGeometry& g, const std::vector<double>& unit,
                                      const std::vector<double>& sigma) {
  const size_t nc = static_cast<size_t>(g.nchans), ns = signals.size();
  PSOUP_CHECK(tab.nsig == static_cast<int>(ns) && tab.nchans == g.nchans && unit.size() == nc &&
                  (sigma.empty() || sigma.size() == nc),
              "inject_truth: the tables do not fit the signals");
  std::vector<InjectTruth> out(ns);
  const double root_pi = std::sqrt(3.14159265358979323846);
  for (size_t s = 0; s < ns; ++s) {
    const InjectSignal& sg = signals[s];
    const bool burst = sg.kind == InjectKind::Burst;
    const double* k = &tab.sigc[s * kern::kInjectSigDoubles];
    InjectTruth& tr = out[s];
    if (burst) {
      tr.npulses = (k[1] >= 0 && k[1] < static_cast<double>(g.nsamps)) ? 1 : 0;
    } else {
      const double te = static_cast<double>(g.nsamps - 1) * g.tsamp;
      const double n = std::floor(pulsar_phase(te, k[1], k[2], k[3])) - std::ceil(k[3]) + 1.0;
      tr.npulses = n > 0 ? static_cast<uint64_t>(n) : 0;
    }
    double sum_a = 0, sum_q = 0;
    size_t live = 0;
    for (size_t c = 0; c < nc; ++c) {
      if (!(unit[c] > 0)) continue;
      const size_t i = s * nc + c;
      const double a = static_cast<double>(tab.A_q[i]) / 65536.0;
      ++live;
      sum_a += a;
      if (!sigma.empty() && sigma[c] > 0) {
        const double ws = burst ? tab.w[i] : tab.w[i] * sg.t / g.tsamp;
        const double r = a / sigma[c];
        sum_q += ((r * r) * static_cast<double>(tr.npulses)) * (ws * root_pi);
      }
    }
    tr.peak = live ? sum_a / static_cast<double>(live) : 0.0;
    tr.snr = std::sqrt(sum_q);
  }
  return out;
}

std::string inject_truth_text(const std::vector<InjectSignal>& signals, const std::vector<InjectTruth>& truth,
                              const std::string& units, uint64_t seed) {
  PSOUP_CHECK(signals.size() == truth.size(), "inject_truth_text: sizes differ");
  std::ostringstream os;
  os << "# filinject truth: units " << units << " seed " << seed << "\n";
  os << "# pulsar period_s dm amp duty acc phase alpha npulses peak_levels snr\n";
  os << "# burst time_s dm amp width_s alpha npulses peak_levels snr\n";
  char buf[512];
  for (size_t i = 0; i < signals.size(); ++i) {
    const InjectSignal& s = signals[i];
    const InjectTruth& t = truth[i];
    if (s.kind == InjectKind::Burst)
      std::snprintf(buf, sizeof(buf), "burst %.17g %.17g %.17g %.17g %.17g %llu %.17g %.17g\n", s.t, s.dm, s.amp,
                    s.width, s.alpha, static_cast<unsigned long long>(t.npulses), t.peak, t.snr);
    else
      std::snprintf(buf, sizeof(buf), "pulsar %.17g %.17g %.17g %.17g %.17g %.17g %.17g %llu %.17g %.17g\n", s.t, s.dm,
                    s.amp, s.width, s.acc, s.phase, s.alpha, static_cast<unsigned long long>(t.npulses), t.peak,
                    t.snr);
    os << buf;
  }
  return os.str();
}

}  // namespace psoup
