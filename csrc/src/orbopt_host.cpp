// orbopt, host side (no device code): the grid with its steps and sign fold,
// G, hits, the row moments, the drift table, host transcriptions of both
// kernels, the finish, the candidate parser and the bytes of the result file.
// See psoup/orbopt.hpp.  Compiled without FMA contraction.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <sstream>

#include "psoup/orbopt.hpp"

namespace psoup {

namespace {

constexpr double kC = 299792458.0;

std::string who(size_t k, const OrbOptCandidate& c) {
  std::ostringstream s;
  s << "orbopt: candidate " << k << " (period " << c.period << " s, dm " << c.dm << ", pb " << c.pb << " s, a1 " << c.a1
    << " ls, phase " << c.ph << ")";
  return s.str();
}

// rint(x) reduced into [0, n); x finite.
int32_t reduced_shift(double x, int n) {
  double r = std::fmod(std::rint(x), static_cast<double>(n));  // exact
  if (r < 0) r += n;
  return static_cast<int32_t>(r);
}

template <class T>
void put(std::vector<char>& b, const T& v) {
  static_assert(std::is_trivially_copyable<T>::value, "put: plain values");
  const char* p = reinterpret_cast<const char*>(&v);  // gfx950 hosts are little-endian
  b.insert(b.end(), p, p + sizeof(T));
}

template <class T>
void put_all(std::vector<char>& b, const std::vector<T>& v) {
  const char* p = reinterpret_cast<const char*>(v.data());
  b.insert(b.end(), p, p + v.size() * sizeof(T));
}

// prof[b] = sum_j d[j][(b + st[j]) % nbins], d = fold - m hits modulo 2^32
std::vector<int32_t> profile_of(const int32_t* fold, const int32_t* hits, int32_t m, const int32_t* st, int nints,
                                int nbins) {
  std::vector<int32_t> prof(static_cast<size_t>(nbins), 0);
  for (int j = 0; j < nints; ++j)
    for (int b = 0; b < nbins; ++b) {
      const size_t e = static_cast<size_t>(j) * nbins + static_cast<size_t>((b + st[j]) % nbins);
      const uint32_t d = static_cast<uint32_t>(fold[e]) - static_cast<uint32_t>(m) * static_cast<uint32_t>(hits[e]);
      prof[static_cast<size_t>(b)] = static_cast<int32_t>(static_cast<uint32_t>(prof[static_cast<size_t>(b)]) + d);
    }
  return prof;
}

}  // namespace

OrbOptParams oopt_params_of(const OrbOptCmdLineOptions& a) {
  OrbOptParams p;
  p.nbins = a.nbins;
  p.nints = a.nints;
  p.npb = a.npb;
  p.na1 = a.na1;
  p.nphase = a.nphase;
  p.pb_step = a.pb_step;
  p.a1_step = a.a1_step;
  p.phase_step = a.phase_step;
  p.np = a.np;
  p.p_step = a.p_step;
  return p;
}

void oopt_check_params(const OrbOptParams& p) {
  PSOUP_CHECK(p.nbins >= 2 && p.nbins <= kern::kOoptMaxBins, "orbopt: nbins must be in 2.." << kern::kOoptMaxBins);
  PSOUP_CHECK(p.nints >= 1 && p.nints <= kern::kOoptMaxInts, "orbopt: nints must be in 1.." << kern::kOoptMaxInts);
  PSOUP_CHECK(p.nints * p.nbins <= kern::kOoptMaxPlane,
              "orbopt: nints * nbins = " << p.nints * p.nbins << " exceeds " << kern::kOoptMaxPlane);
  PSOUP_CHECK(p.npb >= 1 && p.na1 >= 1 && p.nphase >= 1 && p.npb % 2 == 1 && p.na1 % 2 == 1 && p.nphase % 2 == 1,
              "orbopt: an even count (--npb, --na1 and --nphase must be odd and at least 1)");
  PSOUP_CHECK(p.np >= 1 && p.np <= 257 && p.np % 2 == 1, "orbopt: an even count (--np must be odd and in 1..257)");
  const uint64_t K = static_cast<uint64_t>(p.npb) * static_cast<uint64_t>(p.na1) * static_cast<uint64_t>(p.nphase);
  PSOUP_CHECK(K <= static_cast<uint64_t>(kern::kOoptMaxTemplates),
              "orbopt: more than " << kern::kOoptMaxTemplates << " templates per candidate (" << K << ")");
  PSOUP_CHECK(K * static_cast<uint64_t>(p.np) * static_cast<uint64_t>(p.nbins) < (uint64_t(1) << 31),
              "orbopt: K np nbins >= 2^31: the trial bins do not fit 31 bits");
  PSOUP_CHECK(std::isfinite(p.p_step) && p.p_step >= 0 && std::isfinite(p.pb_step) && p.pb_step >= 0 &&
                  std::isfinite(p.a1_step) && p.a1_step >= 0 && std::isfinite(p.phase_step) && p.phase_step >= 0,
              "orbopt: the steps must be finite and non-negative");
}

// ---------------------------------------------------------------- grid ----
OrbOptGrid oopt_grid(size_t k, const OrbOptParams& p, const OrbOptCandidate& c, uint64_t n, float tsamp) {
  oopt_check_params(p);
  const std::string w = who(k, c);
  const double ts = static_cast<double>(tsamp);
  PSOUP_CHECK(std::isfinite(ts) && ts > 0.0, "orbopt: non-positive tsamp");
  PSOUP_CHECK(n >= 1, "orbopt: the dedispersed series is empty");
  PSOUP_CHECK(n <= kOrbitMaxSpan, "orbopt: series longer than 2^26 samples (n = " << n << ")");
  const double P = c.period;
  PSOUP_CHECK(std::isfinite(P) && !(P < 2.0 * ts), w << ": the period is not finite or below 2 tsamp");
  PSOUP_CHECK(std::isfinite(c.dm) && !(c.dm < 0.f), w << ": a non-finite or negative DM");
  PSOUP_CHECK(std::isfinite(c.acc), w << ": a non-finite acceleration");
  PSOUP_CHECK(std::isfinite(c.pb) && std::isfinite(c.a1) && std::isfinite(c.ph),
              w << ": orbit: a non-finite value (pb " << c.pb << " a1 " << c.a1 << " phase " << c.ph << ")");
  const double pb0 = c.pb, a10 = c.a1, ph0 = c.ph;
  const double T = static_cast<double>(n) * ts;
  const double nb = static_cast<double>(p.nbins);
  OrbOptGrid g;
  g.npb = p.npb;
  g.na1 = p.na1;
  g.nphase = p.nphase;
  g.da1 = p.a1_step > 0 ? p.a1_step : P / (2.0 * nb);
  if (p.phase_step > 0) {
    g.dph = p.phase_step;
  } else if (a10 == 0.0) {
    g.dph = 0.0;
    g.nphase = 1;
  } else {
    g.dph = std::min(1.0 / 16.0, P / ((4.0 * M_PI) * std::fabs(a10) * nb));
  }
  if (p.pb_step > 0) {
    g.dpb = p.pb_step;
  } else if (a10 == 0.0) {
    g.dpb = 0.0;
    g.npb = 1;
  } else {
    g.dpb = std::min(pb0 / 16.0, (pb0 * pb0 * P) / ((4.0 * M_PI) * std::fabs(a10) * T * nb));
  }
  g.G = static_cast<uint64_t>(std::rint(std::ldexp(ts / P, 64)));
  for (int kb = 0; kb < g.npb; ++kb)
    for (int ka = 0; ka < g.na1; ++ka)
      for (int kp = 0; kp < g.nphase; ++kp) {
        OrbitTemplate t;
        t.pb = pb0 + static_cast<double>(kb - g.npb / 2) * g.dpb;
        t.a1 = a10 + static_cast<double>(ka - g.na1 / 2) * g.da1;
        t.ph = ph0 + static_cast<double>(kp - g.nphase / 2) * g.dph;
        if (t.a1 < 0.0) {
          t.a1 = -t.a1;
          t.ph = t.ph + 0.5;
        }
        try {
          g.quant.push_back(orbit_quantise(t.pb, t.a1, t.ph, tsamp));
          const double beta = orbit_beta(t);
          PSOUP_CHECK(!(beta > 0.9),
                      "orbit: a template moves more than 0.9 samples per sample (2 pi a1 / pb = " << beta << ")");
        } catch (const std::exception& e) {
          PSOUP_THROW(w << ": grid template " << g.tmpl.size() << " (pb " << t.pb << " a1 " << t.a1 << " phase " << t.ph
                        << "): " << e.what());
        }
        g.tmpl.push_back(t);
      }
  return g;
}

// ---------------------------------------------------------------- hits ----
std::vector<int32_t> oopt_hits(uint64_t G, uint64_t n, int nints, int nbins) {
  std::vector<int32_t> hits(static_cast<size_t>(nints) * nbins, 0);
  uint64_t phi = 0;
  for (uint64_t i = 0; i < n; ++i, phi += G) {
    const uint64_t b = ((phi >> 32) * static_cast<uint64_t>(nbins)) >> 32;
    const uint64_t j = (i * static_cast<uint64_t>(nints)) / n;
    ++hits[j * nbins + b];
  }
  return hits;
}

OrbOptMoments oopt_moments(size_t k, const uint8_t* x, uint64_t n) {
  PSOUP_CHECK(x != nullptr && n >= 1, "orbopt: an empty row");
  uint64_t s1 = 0, s2 = 0;
  for (uint64_t i = 0; i < n; ++i) {
    s1 += x[i];
    s2 += static_cast<uint64_t>(x[i]) * x[i];
  }
  OrbOptMoments mom;
  mom.m = static_cast<int64_t>((s1 + n / 2) / n);
  // sum (x - m)^2 = s2 - 2 m s1 + n m^2
  mom.v1 = static_cast<int64_t>(s2) - 2 * mom.m * static_cast<int64_t>(s1) + static_cast<int64_t>(n) * mom.m * mom.m;
  const int64_t big = std::max<int64_t>(mom.m, 255 - mom.m);
  PSOUP_CHECK(big * static_cast<int64_t>(n) < (int64_t{1} << 31),
              "orbopt: candidate " << k << ": max(m, 255 - m) * n >= 2^31 (m = " << mom.m << ", n = " << n
                                   << "): the fold does not fit int32");
  return mom;
}

std::vector<int32_t> oopt_drift_table(const OrbOptParams& p) {
  oopt_check_params(p);
  std::vector<int32_t> st(static_cast<size_t>(p.np) * p.nints);
  for (int l = 0; l < p.np; ++l) {
    const double L = (l - p.np / 2) * p.p_step;
    for (int j = 0; j < p.nints; ++j) {
      const double u = (j + 0.5) / p.nints;
      st[static_cast<size_t>(l) * p.nints + j] = reduced_shift(L * (u - 0.5), p.nbins);
    }
  }
  return st;
}

// -------------------------------------------------- host transcriptions ----
std::vector<int32_t> orbopt_fold_host(const uint8_t* x, uint64_t n, uint64_t G, const std::vector<OrbitQuant>& q,
                                      int nints, int nbins) {
  PSOUP_CHECK(x != nullptr && n >= 1 && n <= kOrbitMaxSpan, "orbopt_fold: the span must be in 1..2^26");
  PSOUP_CHECK(nints >= 1 && nints <= kern::kOoptMaxInts && nbins >= 2 && nbins <= kern::kOoptMaxBins,
              "orbopt_fold: nints in 1.." << kern::kOoptMaxInts << ", nbins in 2.." << kern::kOoptMaxBins);
  PSOUP_CHECK(!q.empty() && q.size() <= static_cast<size_t>(kern::kOoptMaxTemplates),
              "orbopt_fold: 1.." << kern::kOoptMaxTemplates << " templates per launch");
  for (const OrbitQuant& t : q) orbit_check_quant(t);
  const std::vector<int32_t> table = orbit_sine_table();
  const size_t plane = static_cast<size_t>(nints) * nbins;
  std::vector<uint32_t> acc(q.size() * plane, 0u);
  const int64_t N = static_cast<int64_t>(n);
  for (size_t k = 0; k < q.size(); ++k) {
    uint64_t phi = 0;
    for (uint64_t i = 0; i < n; ++i, phi += G) {
      const uint64_t b = ((phi >> 32) * static_cast<uint64_t>(nbins)) >> 32;
      const uint64_t j = (i * static_cast<uint64_t>(nints)) / n;
      const int64_t src = static_cast<int64_t>(i) + orbit_shift(table.data(), q[k], i);
      acc[k * plane + j * nbins + b] += x[std::min(std::max<int64_t>(src, 0), N - 1)];
    }
  }
  std::vector<int32_t> out(acc.size());
  std::memcpy(out.data(), acc.data(), acc.size() * sizeof(int32_t));
  return out;
}

OrbOptSearch orbopt_search_host(const int32_t* fold, const int32_t* hits, int32_t m, const int32_t* st, int K, int nints,
                                int nbins, int np) {
  const int nw = kern::oopt_nwidths(nbins);
  const size_t plane = static_cast<size_t>(nints) * nbins;
  const int32_t lo = std::numeric_limits<int32_t>::min();
  OrbOptSearch out;
  out.best_val.assign(static_cast<size_t>(nw), lo);
  out.best_idx.assign(static_cast<size_t>(nw), 0);
  out.centre.assign(static_cast<size_t>(nw), lo);
  out.tcurve.assign(static_cast<size_t>(nw) * K, lo);
  out.msum.assign(static_cast<size_t>(K), 0);
  for (size_t e = 0; e < static_cast<size_t>(np) * nints; ++e)
    PSOUP_CHECK(st[e] >= 0 && st[e] < nbins, "orbopt_search: a drift shift outside [0, nbins)");
  std::vector<int32_t> box, next(static_cast<size_t>(nbins));
  for (int k = 0; k < K; ++k) {
    const int32_t* f = fold + static_cast<size_t>(k) * plane;
    int64_t ms = 0;
    for (size_t e = 0; e < plane; ++e)
      ms += static_cast<int32_t>(static_cast<uint32_t>(f[e]) - static_cast<uint32_t>(m) * static_cast<uint32_t>(hits[e]));
    out.msum[static_cast<size_t>(k)] = ms;
    for (int l = 0; l < np; ++l) {
      box = profile_of(f, hits, m, st + static_cast<size_t>(l) * nints, nints, nbins);
      for (int kw = 0, w = 1; kw < nw; ++kw, w *= 2) {
        for (int b = 0; b < nbins; ++b) {
          const int32_t v = box[static_cast<size_t>(b)];
          if (v > out.best_val[static_cast<size_t>(kw)]) {
            out.best_val[static_cast<size_t>(kw)] = v;
            out.best_idx[static_cast<size_t>(kw)] = (k * np + l) * nbins + b;
          }
          int32_t& tc = out.tcurve[static_cast<size_t>(kw) * K + k];
          tc = std::max(tc, v);
          if (k == K / 2 && l == np / 2)
            out.centre[static_cast<size_t>(kw)] = std::max(out.centre[static_cast<size_t>(kw)], v);
        }
        for (int b = 0; b < nbins; ++b)
          next[static_cast<size_t>(b)] = static_cast<int32_t>(static_cast<uint32_t>(box[static_cast<size_t>(b)]) +
                                                              static_cast<uint32_t>(box[static_cast<size_t>((b + w) % nbins)]));
        box.swap(next);
        next.resize(static_cast<size_t>(nbins));
      }
    }
  }
  return out;
}

// -------------------------------------------------------------- finish ----
double oopt_snr(double s, int w, int64_t msum, double v, int nbins) {
  if (!(v > 0)) return 0.0;
  return (s - w * static_cast<double>(msum) / nbins) / std::sqrt(v * w * (1.0 - static_cast<double>(w) / nbins));
}

OrbOptOptimum oopt_optimum(const OrbOptParams& p, const OrbOptGrid& g, const OrbOptMoments& mom,
                           const OrbOptSearch& found) {
  const int nb = p.nbins, nw = kern::oopt_nwidths(nb);
  const int K = static_cast<int>(g.tmpl.size());
  PSOUP_CHECK(K >= 1 && K == g.npb * g.na1 * g.nphase, "orbopt: the grid has the wrong size");
  PSOUP_CHECK(found.best_val.size() == static_cast<size_t>(nw) && found.best_idx.size() == static_cast<size_t>(nw) &&
                  found.centre.size() == static_cast<size_t>(nw) &&
                  found.tcurve.size() == static_cast<size_t>(nw) * K && found.msum.size() == static_cast<size_t>(K),
              "orbopt: search outputs have the wrong shape");
  const double v = static_cast<double>(mom.v1) / static_cast<double>(nb);
  OrbOptOptimum o;
  double best_in = 0;
  for (int kw = 0, w = 1; kw < nw; ++kw, w *= 2) {
    const int64_t idx = found.best_idx[static_cast<size_t>(kw)];
    PSOUP_CHECK(idx >= 0 && idx < static_cast<int64_t>(K) * p.np * nb, "orbopt: a best index is out of range");
    const size_t k = static_cast<size_t>(idx / nb / p.np);
    const double s = oopt_snr(static_cast<double>(found.best_val[static_cast<size_t>(kw)]), w, found.msum[k], v, nb);
    if (kw == 0 || s > o.snr) {
      o.snr = s;
      o.kw = kw;
    }
    const double si = oopt_snr(static_cast<double>(found.centre[static_cast<size_t>(kw)]), w,
                               found.msum[static_cast<size_t>(K / 2)], v, nb);
    if (kw == 0 || si > best_in) best_in = si;
  }
  o.snr_in = best_in;
  const int64_t idx = found.best_idx[static_cast<size_t>(o.kw)];
  o.b = static_cast<uint32_t>(idx % nb);
  o.l = static_cast<uint32_t>((idx / nb) % p.np);
  o.k = static_cast<uint32_t>(idx / nb / p.np);
  return o;
}

OrbOptResult oopt_finish(const OrbOptParams& p, const OrbOptCandidate& c, const OrbOptGrid& g, uint64_t n, float tsamp,
                         const OrbOptMoments& mom, const std::vector<int32_t>& hits, const std::vector<int32_t>& st,
                         const OrbOptSearch& found, const int32_t* fold_opt) {
  const int nb = p.nbins;
  const size_t plane = static_cast<size_t>(p.nints) * nb;
  PSOUP_CHECK(hits.size() == plane && st.size() == static_cast<size_t>(p.np) * p.nints && fold_opt != nullptr,
              "orbopt: finish inputs have the wrong shape");
  const OrbOptOptimum o = oopt_optimum(p, g, mom, found);
  OrbOptResult r;
  r.cand = c;
  r.npb = g.npb;
  r.na1 = g.na1;
  r.nphase = g.nphase;
  r.dpb = g.dpb;
  r.da1 = g.da1;
  r.dph = g.dph;
  r.snr = o.snr;
  r.snr_in = o.snr_in;
  r.opt_width = 1u << o.kw;
  r.opt_bin = o.b;
  r.opt_k = o.k;
  r.opt_l = o.l;
  const OrbitTemplate& t = g.tmpl[o.k];
  r.opt_pb = t.pb;
  r.opt_a1 = t.a1;
  r.opt_phase = t.ph;
  const double ts = static_cast<double>(tsamp);
  const double T = static_cast<double>(n) * ts;
  const double L = (static_cast<int>(o.l) - p.np / 2) * p.p_step;
  r.opt_period = 1.0 / (1.0 / c.period - L / (nb * T));
  const int kp = static_cast<int>(o.k) % g.nphase, ka = (static_cast<int>(o.k) / g.nphase) % g.na1,
            kb = static_cast<int>(o.k) / g.nphase / g.na1;
  auto face = [](int i, int cnt) { return cnt > 1 && (i == 0 || i == cnt - 1); };
  if (face(kp, g.nphase) || face(ka, g.na1) || face(kb, g.npb) || face(static_cast<int>(o.l), p.np)) r.flags |= 1u;
  if (((std::fabs(static_cast<double>(c.acc)) * T * T) / ((2.0 * kC) * c.period)) * nb > 1.0) r.flags |= 2u;
  r.m = mom.m;
  r.v1 = mom.v1;
  r.search = found;
  r.hits = hits;
  r.fold.assign(fold_opt, fold_opt + plane);
  r.profile = profile_of(fold_opt, hits.data(), static_cast<int32_t>(mom.m), st.data() + static_cast<size_t>(o.l) * p.nints,
                         p.nints, nb);
  return r;
}

// -------------------------------------------------------------- parser ----
std::vector<OrbOptCandidate> oopt_parse_candidates(const std::string& text) {
  std::vector<OrbOptCandidate> out;
  std::istringstream is(text);
  std::string line;
  size_t ln = 0;
  while (std::getline(is, line)) {
    ++ln;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ls(line);
    std::string tok;
    double v[6];
    int got = 0;
    while (got < 6 && ls >> tok) {
      char* end = nullptr;
      v[got] = std::strtod(tok.c_str(), &end);
      PSOUP_CHECK(end != tok.c_str() && *end == '\0', "orbopt: candidate line " << ln << " is malformed");
      ++got;
    }
    if (got == 0) continue;  // blank or comment
    PSOUP_CHECK(got == 6, "orbopt: candidate line " << ln << " is malformed");
    OrbOptCandidate c;
    c.period = v[0];
    c.dm = static_cast<float>(v[1]);
    c.acc = static_cast<float>(v[2]);
    c.pb = v[3];
    c.a1 = v[4];
    c.ph = v[5];
    out.push_back(c);
  }
  return out;
}

std::vector<float> oopt_dm_list(const std::vector<OrbOptCandidate>& cands) {
  std::vector<float> dms;
  for (size_t k = 0; k < cands.size(); ++k) {
    PSOUP_CHECK(std::isfinite(cands[k].dm) && !(cands[k].dm < 0.f),
                who(k, cands[k]) << ": a non-finite or negative DM");
    dms.push_back(cands[k].dm);
  }
  std::sort(dms.begin(), dms.end());
  dms.erase(std::unique(dms.begin(), dms.end()), dms.end());
  return dms;
}

// ---------------------------------------------------------------- file ----
std::vector<char> oopt_file_bytes(const OrbOptFileHeader& h, const std::vector<OrbOptResult>& results) {
  PSOUP_CHECK(results.size() == h.ncand, "orbopt file: candidate count mismatch");
  const size_t nw = h.nw, plane = static_cast<size_t>(h.nints) * h.nbins;
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'O', 'O', 'P', 'T', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  for (uint32_t v : {h.ncand, h.nints, h.nbins, h.npb, h.na1, h.nphase, h.np, h.nw}) put(b, v);
  put(b, h.n);
  put(b, h.tsamp);
  put(b, h.p_step);
  for (size_t i = 0; i < results.size(); ++i) {
    const OrbOptResult& r = results[i];
    const size_t K = static_cast<size_t>(r.npb) * r.na1 * r.nphase;
    PSOUP_CHECK(r.search.best_val.size() == nw && r.search.best_idx.size() == nw && r.search.centre.size() == nw &&
                    r.search.tcurve.size() == nw * K && r.search.msum.size() == K && r.hits.size() == plane &&
                    r.fold.size() == plane && r.profile.size() == h.nbins,
                "orbopt file: candidate " << i << " has the wrong shape");
    put(b, r.cand.period);
    put(b, r.cand.dm);
    put(b, r.cand.acc);
    for (double v : {r.cand.pb, r.cand.a1, r.cand.ph, r.dpb, r.da1, r.dph, r.snr, r.snr_in, r.opt_period, r.opt_pb,
                     r.opt_a1, r.opt_phase})
      put(b, v);
    for (uint32_t v : {r.opt_width, r.opt_bin, r.opt_k, r.opt_l, r.flags, static_cast<uint32_t>(r.npb),
                       static_cast<uint32_t>(r.na1), static_cast<uint32_t>(r.nphase)})
      put(b, v);
    put(b, r.m);
    put(b, r.v1);
    put_all(b, r.search.best_val);
    put_all(b, r.search.best_idx);
    put_all(b, r.search.centre);
    put_all(b, r.search.tcurve);
    put_all(b, r.search.msum);
    put_all(b, r.hits);
    put_all(b, r.fold);
    put_all(b, r.profile);
  }
  return b;
}

void write_orbopt_file(const std::string& path, const OrbOptFileHeader& h, const std::vector<OrbOptResult>& results) {
  const std::vector<char> b = oopt_file_bytes(h, results);
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open orbopt output " << tmp);
  bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  ok = (std::fclose(fo) == 0) && ok;
  if (!ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write orbopt output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

std::string oopt_verbose_line(const OrbOptResult& r) {
  char b[512];
  std::snprintf(b, sizeof b, "%.12g %.12g %.6g %.6g %.9g %.9g %.9g %.9g %.9g %.9g %u %.3f %.3f %u", r.cand.period,
                r.opt_period, static_cast<double>(r.cand.dm), static_cast<double>(r.cand.acc), r.cand.pb, r.opt_pb,
                r.cand.a1, r.opt_a1, r.cand.ph, r.opt_phase, r.opt_width, r.snr, r.snr_in, r.flags);
  return b;
}

}  // namespace psoup
