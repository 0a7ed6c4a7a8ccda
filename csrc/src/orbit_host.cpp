// orbsearch, host side (no device code): the sine table, the quantisation, the
// shift, the checks, the bank parser, the grid, the orbit distillation, a host
// transcription of the gather and the text of the output file.  See
// psoup/orbit.hpp.  Compiled without FMA contraction.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "psoup/orbit.hpp"

namespace psoup {

// ---------------------------------------------------------------- sine ----
std::vector<int32_t> orbit_sine_table() {
  std::vector<int32_t> t(4097, 0);
  for (int j = 0; j <= 1024; ++j)
    t[static_cast<size_t>(j)] =
        static_cast<int32_t>(std::rint(std::ldexp(std::sin(static_cast<double>(j) * (M_PI / 2048)), 30)));
  for (int j = 0; j <= 1024; ++j) t[static_cast<size_t>(2048 - j)] = t[static_cast<size_t>(j)];
  for (int j = 0; j <= 2048; ++j) t[static_cast<size_t>(2048 + j)] = -t[static_cast<size_t>(j)];
  return t;
}

int64_t orbit_sine(const int32_t* table, uint64_t th) {
  const uint64_t j = th >> 52;
  const int64_t f = static_cast<int64_t>((th >> 32) & 0xFFFFFull);
  const int64_t t0 = table[j], t1 = table[j + 1];
  const int64_t v = (t1 - t0) * f + (int64_t{1} << 19);
  // an arithmetic shift, written so that it is one for a negative v in every C++ dialect
  return t0 + (v >= 0 ? v >> 20 : -((-v + ((int64_t{1} << 20) - 1)) >> 20));
}

// -------------------------------------------------------- quantisation ----
OrbitQuant orbit_quantise(double pb, double a1, double ph, float tsamp) {
  PSOUP_CHECK(std::isfinite(pb) && std::isfinite(a1) && std::isfinite(ph) && std::isfinite(tsamp),
              "orbit: a non-finite value (pb " << pb << " a1 " << a1 << " phase " << ph << ")");
  const double ts = static_cast<double>(tsamp);
  PSOUP_CHECK(ts > 0.0, "orbit: non-positive tsamp");
  PSOUP_CHECK(!(pb < 64.0 * ts), "orbit: pb < 64 tsamp (pb = " << pb << " s)");
  PSOUP_CHECK(!(a1 < 0.0), "orbit: a1 < 0 (a1 = " << a1 << ")");
  OrbitQuant q;
  q.W = static_cast<uint64_t>(std::rint(std::ldexp(ts / pb, 64)));
  double r = ph - std::floor(ph);
  if (r >= 1.0) r = 0.0;
  q.F = static_cast<uint64_t>(std::ldexp(r, 64));
  const double aq = std::rint((a1 / ts) * 256.0);
  PSOUP_CHECK(aq < 1073741824.0, "orbit: Aq >= 2^30 (a1 / tsamp = " << a1 / ts << " samples)");
  q.Aq = static_cast<int64_t>(aq);
  return q;
}

void orbit_check_quant(const OrbitQuant& q) {
  PSOUP_CHECK(q.W <= (1ull << 58), "orbit: pb < 64 tsamp (W > 2^58)");
  PSOUP_CHECK(q.Aq >= 0, "orbit: a1 < 0 (Aq < 0)");
  PSOUP_CHECK(q.Aq < (int64_t{1} << 30), "orbit: Aq >= 2^30");
}

int64_t orbit_shift(const int32_t* table, const OrbitQuant& q, uint64_t i) {
  const uint64_t th = q.F + i * q.W;  // wrapping
  const int64_t v = q.Aq * (orbit_sine(table, th) - orbit_sine(table, q.F)) + (int64_t{1} << 37);
  return v >= 0 ? v >> 38 : -((-v + ((int64_t{1} << 38) - 1)) >> 38);
}

double orbit_beta(const OrbitTemplate& t) { return ((2.0 * M_PI) * t.a1) / t.pb; }

void orbit_check(uint64_t n, const std::vector<OrbitTemplate>& bank, float tsamp) {
  PSOUP_CHECK(n >= 1, "orbit: empty series");
  PSOUP_CHECK(n <= kOrbitMaxSpan, "orbit: series longer than 2^26 samples (n = " << n << ")");
  PSOUP_CHECK(!bank.empty(), "orbit: an empty bank");
  PSOUP_CHECK(bank.size() <= kOrbitMaxTemplates, "orbit: more than 2^20 templates (" << bank.size() << ")");
  for (size_t k = 0; k < bank.size(); ++k) {
    orbit_quantise(bank[k].pb, bank[k].a1, bank[k].ph, tsamp);
    const double b = orbit_beta(bank[k]);
    PSOUP_CHECK(!(b > 0.9), "orbit: template " << k << " moves more than 0.9 samples per sample (2 pi a1 / pb = " << b
                                               << ")");
  }
}

// ---------------------------------------------------------------- bank ----
std::vector<OrbitTemplate> orbit_parse_bank(const std::string& text) {
  std::vector<OrbitTemplate> bank;
  std::istringstream is(text);
  std::string line;
  size_t ln = 0;
  while (std::getline(is, line)) {
    ++ln;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ls(line);
    std::string tok;
    double v[3];
    int got = 0;
    while (got < 3 && ls >> tok) {
      char* end = nullptr;
      v[got] = std::strtod(tok.c_str(), &end);
      PSOUP_CHECK(end != tok.c_str() && *end == '\0', "orbit: bank line " << ln << " is malformed");
      ++got;
    }
    if (got == 0) continue;  // blank or comment
    PSOUP_CHECK(got == 3, "orbit: bank line " << ln << " is malformed");
    PSOUP_CHECK(bank.size() < kOrbitMaxTemplates, "orbit: more than 2^20 templates");
    bank.push_back(OrbitTemplate{v[0], v[1], v[2]});
  }
  return bank;
}

std::vector<OrbitTemplate> orbit_grid(double pb_start, double pb_end, int npb, double a1_start, double a1_end, int na1,
                                      int nphase) {
  PSOUP_CHECK(npb >= 1 && na1 >= 1 && nphase >= 1, "orbit: --npb, --na1 and --nphase must be at least 1");
  const double total = static_cast<double>(npb) * static_cast<double>(na1) * static_cast<double>(nphase);
  PSOUP_CHECK(total <= static_cast<double>(kOrbitMaxTemplates), "orbit: more than 2^20 templates (" << total << ")");
  std::vector<OrbitTemplate> bank;
  bank.reserve(static_cast<size_t>(total));
  for (int p = 0; p < npb; ++p) {
    double pb = pb_start;
    if (p > 0)
      pb = p == npb - 1 ? pb_end
                        : pb_start * std::pow(pb_end / pb_start, static_cast<double>(p) / static_cast<double>(npb - 1));
    for (int a = 0; a < na1; ++a) {
      double a1 = a1_start;
      if (a > 0)
        a1 = a == na1 - 1 ? a1_end
                          : a1_start + (a1_end - a1_start) * (static_cast<double>(a) / static_cast<double>(na1 - 1));
      for (int f = 0; f < nphase; ++f)
        bank.push_back(OrbitTemplate{pb, a1, static_cast<double>(f) / static_cast<double>(nphase)});
    }
  }
  return bank;
}

std::vector<OrbitTemplate> orbit_bank_of(const OrbitCmdLineOptions& args) {
  const bool grid = args.npb != 0 || args.na1 != 0 || args.nphase != 0;
  PSOUP_CHECK(grid != !args.bankfile.empty(),
              "orbit: give exactly one source of templates (--bankfile, or the grid --pb_start --pb_end --npb "
              "--a1_start --a1_end --na1 --nphase)");
  if (grid) return orbit_grid(args.pb_start, args.pb_end, args.npb, args.a1_start, args.a1_end, args.na1, args.nphase);
  std::ifstream in(args.bankfile);
  PSOUP_CHECK(static_cast<bool>(in), "orbit: cannot open the bank file " << args.bankfile);
  std::ostringstream os;
  os << in.rdbuf();
  return orbit_parse_bank(os.str());
}

// -------------------------------------------------------------- gather ----
void orbit_resample_host(const uint8_t* x, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n,
                         const std::vector<OrbitQuant>& q, uint8_t* y, uint64_t out_stride) {
  PSOUP_CHECK(x != nullptr && y != nullptr, "orbit_resample: missing buffer");
  PSOUP_CHECK(nrows >= 1 && !q.empty(), "orbit_resample: no rows or no templates");
  PSOUP_CHECK(n >= 1 && n <= nrow, "orbit_resample: the span must be in 1..nrow");
  PSOUP_CHECK(n <= kOrbitMaxSpan, "orbit: series longer than 2^26 samples");
  PSOUP_CHECK(row_stride >= nrow && out_stride >= nrow, "orbit_resample: a stride is shorter than the row");
  for (const OrbitQuant& t : q) orbit_check_quant(t);
  const std::vector<int32_t> table = orbit_sine_table();
  const size_t K = q.size();
  const int64_t N = static_cast<int64_t>(n);
  for (int r = 0; r < nrows; ++r)
    for (size_t k = 0; k < K; ++k) {
      const uint8_t* xr = x + static_cast<uint64_t>(r) * row_stride;
      uint8_t* yr = y + (static_cast<uint64_t>(r) * K + k) * out_stride;
      for (uint64_t i = 0; i < n; ++i) {
        const int64_t j = static_cast<int64_t>(i) + orbit_shift(table.data(), q[k], i);
        yr[i] = xr[std::min(std::max<int64_t>(j, 0), N - 1)];
      }
      for (uint64_t i = n; i < nrow; ++i) yr[i] = xr[i];
    }
}

// --------------------------------------------------------- distillation ----
OrbitCandidateList orbit_distill(OrbitCandidateList cands, const std::vector<double>& beta, float tol,
                                 bool keep_related) {
  std::stable_sort(cands.begin(), cands.end(),
                   [](const OrbitCandidate& a, const OrbitCandidate& b) { return a.cand.snr > b.cand.snr; });
  const size_t size = cands.size();
  double bmax = 0.0;
  for (const OrbitCandidate& c : cands) {
    PSOUP_CHECK(c.tmpl < beta.size(), "orbit: a candidate names a template outside the bank");
    bmax = std::max(bmax, beta[c.tmpl]);
  }
  // the candidates by frequency: a survivor looks only at the stretch its widest tolerance reaches
  std::vector<size_t> byf(size);
  for (size_t i = 0; i < size; ++i) byf[i] = i;
  std::sort(byf.begin(), byf.end(), [&](size_t a, size_t b) {
    return cands[a].cand.freq != cands[b].cand.freq ? cands[a].cand.freq < cands[b].cand.freq : a < b;
  });
  std::vector<double> fs(size);
  for (size_t p = 0; p < size; ++p) fs[p] = cands[byf[p]].cand.freq;
  const double t0 = static_cast<double>(tol);
  std::vector<char> unique(size, 1);
  std::vector<size_t> hit;
  for (size_t idx = 0; idx < size; ++idx) {
    if (!unique[idx]) continue;
    const double f0 = cands[idx].cand.freq, b0 = beta[cands[idx].tmpl];
    const double reach = std::fabs(f0) * ((t0 + b0) + bmax), slack = std::fabs(f0) * 1.0e-9;
    const size_t p0 = static_cast<size_t>(std::lower_bound(fs.begin(), fs.end(), f0 - reach - slack) - fs.begin());
    const size_t p1 = static_cast<size_t>(std::upper_bound(fs.begin(), fs.end(), f0 + reach + slack) - fs.begin());
    hit.clear();
    for (size_t p = p0; p < p1; ++p) {
      const size_t ii = byf[p];
      if (ii <= idx || cands[ii].tmpl == cands[idx].tmpl) continue;
      const double f = cands[ii].cand.freq;
      if (std::fabs(f / f0 - 1.0) <= (t0 + b0) + beta[cands[ii].tmpl]) hit.push_back(ii);
    }
    std::sort(hit.begin(), hit.end());
    for (size_t ii : hit) {
      if (keep_related) cands[idx].cand.append(cands[ii].cand);
      unique[ii] = 0;
    }
  }
  OrbitCandidateList out;
  for (size_t i = 0; i < size; ++i)
    if (unique[i]) out.push_back(std::move(cands[i]));
  return out;
}

// --------------------------------------------------------------- output ----
std::string orbit_output_text(const OrbitCmdLineOptions& args, const OrbitSetup& setup,
                              const OrbitCandidateList& cands) {
  const CmdLineOptions& a = args.search;
  const float tsamp = setup.search.search.tsamp;
  std::ostringstream os;
  char b[512];
  os << "# orbsearch: circular-orbit templates as an outer loop over the acceleration search\n";
  os << "# input " << a.infilename << "\n";
  std::snprintf(b, sizeof b, "# dm_start %g dm_end %g dm_tol %g dm_pulse_width %g\n", a.dm_start, a.dm_end, a.dm_tol,
                a.dm_pulse_width);
  os << b;
  std::snprintf(b, sizeof b, "# acc_start %g acc_end %g acc_tol %g acc_pulse_width %g accel_convention %s\n",
                a.acc_start, a.acc_end, a.acc_tol, a.acc_pulse_width, a.accel_convention.c_str());
  os << b;
  os << "# bankfile " << (args.bankfile.empty() ? "-" : args.bankfile) << "\n";
  std::snprintf(b, sizeof b, "# pb_start %.17g pb_end %.17g npb %d a1_start %.17g a1_end %.17g na1 %d nphase %d\n",
                args.pb_start, args.pb_end, args.npb, args.a1_start, args.a1_end, args.na1, args.nphase);
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
  os << "# templates " << setup.bank.size() << " (the same bank at each of " << setup.search.dm_list.size()
     << " DMs)\n";
  os << "# A row is re-indexed by the Roemer delay a1_ls [sin 2 pi (t / pb_s + phase) - sin 2 pi phase] of its "
        "template.\n";
  os << "# period_s and freq are intrinsic (orbit frame), no correction factor; acc is what the template left over.\n";
  os << "# period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx\n";
  for (const OrbitCandidate& c : cands) {
    PSOUP_CHECK(c.tmpl < setup.bank.size(), "orbit: a candidate names a template outside the bank");
    const OrbitTemplate& t = setup.bank[c.tmpl];
    const double freq = static_cast<double>(c.cand.freq);
    std::snprintf(b, sizeof b, "%.12g %.9g %.9g %.17g %.17g %.17g %.12g %d %.9g %.9g %d\n", 1.0 / freq,
                  static_cast<double>(c.cand.dm), static_cast<double>(c.cand.acc), t.pb, t.a1, t.ph, freq, c.cand.nh,
                  static_cast<double>(c.cand.snr), static_cast<double>(c.cand.folded_snr), c.cand.dm_idx);
    os << b;
  }
  return os.str();
}

}  // namespace psoup
