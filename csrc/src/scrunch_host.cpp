// filscrunch, host steps: parameters, offsets (step 1), scale (step 4) and the
// plan (step 7) of psoup/scrunch.hpp.  No device code here (the native unit
// tests link this file alone) and no FMA contraction: the double arithmetic is
// the definition's, operation by operation.
#include <algorithm>
#include <cmath>

#include "psoup/plan.hpp"
#include "psoup/scrunch.hpp"

namespace psoup {

ScrunchParams scrunch_check_params(const ScrunchParams& p, int nchans) {
  PSOUP_CHECK(nchans >= 1, "scrunch: no channels");
  ScrunchParams q = p;
  if (q.nsub == 0) q.nsub = nchans;
  PSOUP_CHECK(std::isfinite(q.dm) && q.dm >= 0, "scrunch: dm must be finite and non-negative, got " << q.dm);
  PSOUP_CHECK(q.nsub >= 1 && q.nsub <= nchans && nchans % q.nsub == 0,
              "scrunch: nsub must divide nchans (" << nchans << "), got " << q.nsub);
  PSOUP_CHECK(q.tscrunch >= 1 && q.tscrunch <= kern::kScrunchMaxF,
              "scrunch: tscrunch must be in 1.." << kern::kScrunchMaxF << ", got " << q.tscrunch);
  PSOUP_CHECK(std::isfinite(q.sigma_out) && q.sigma_out > 0, "scrunch: sigma_out must be positive");
  return q;
}

ScrunchParams scrunch_params_from(const ScrunchCmdLineOptions& a) {
  ScrunchParams p;
  p.dm = a.dm;
  p.nsub = a.nsub;
  p.tscrunch = a.tscrunch;
  p.sigma_out = a.sigma_out;
  return p;
}

ScrunchOffsets scrunch_offsets(float dm, const std::vector<float>& delays, int nsub) {
  const int nchans = static_cast<int>(delays.size());
  PSOUP_CHECK(nsub >= 1 && nchans >= 1 && nchans % nsub == 0, "scrunch_offsets: nsub must divide nchans");
  const int w = nchans / nsub;
  ScrunchOffsets o;
  o.rel.resize(static_cast<size_t>(nchans));
  for (int c = 0; c < nchans; ++c) {
    const int rel = dm_delay_samples(dm, delays[static_cast<size_t>(c)]) -
                    dm_delay_samples(dm, delays[static_cast<size_t>(c / w * w)]);
    PSOUP_CHECK(rel >= 0, "scrunch_offsets: channel " << c << " leads its subband's first channel (foff must be < 0)");
    o.rel[static_cast<size_t>(c)] = rel;
    o.R = std::max(o.R, rel);
  }
  return o;
}

namespace {

// numpy.median: the mean of the two middle values for an even count
double median_of(std::vector<double> v) {
  const size_t n = v.size();
  std::sort(v.begin(), v.end());
  return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

}  // namespace

ScrunchScale scrunch_scale(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nsub, uint64_t nout,
                           const std::vector<int32_t>& nactive, double sigma_out) {
  PSOUP_CHECK(nsub >= 1 && nout >= 1, "scrunch_scale: empty table");
  PSOUP_CHECK(std::isfinite(sigma_out) && sigma_out > 0, "scrunch: sigma_out must be positive");
  const uint64_t L = kern::kScrunchStatBlock;
  const size_t nblk = static_cast<size_t>((nout + L - 1) / L);
  const size_t ns = static_cast<size_t>(nsub);
  PSOUP_CHECK(S1.size() == ns * nblk && S2.size() == ns * nblk, "scrunch_scale: S1 / S2 must be [nsub][nblk]");
  PSOUP_CHECK(nactive.size() == ns, "scrunch_scale: nactive must be [nsub]");
  ScrunchScale sc;
  sc.M.assign(ns, 0);
  sc.live.assign(ns, 0);
  std::vector<double> mean(nblk), var(nblk), sig;
  for (size_t s = 0; s < ns; ++s) {
    for (size_t b = 0; b < nblk; ++b) {
      const uint64_t len = (b + 1 < nblk) ? L : nout - (nblk - 1) * L;
      const uint64_t s1 = S1[s * nblk + b], s2 = S2[s * nblk + b];
      const unsigned __int128 lhs = static_cast<unsigned __int128>(len) * s2;
      const unsigned __int128 rhs = static_cast<unsigned __int128>(s1) * s1;
      PSOUP_CHECK(lhs >= rhs, "scrunch_scale: subband " << s << " block " << b << ": S1^2 exceeds len S2");
      mean[b] = static_cast<double>(s1) / static_cast<double>(len);
      var[b] = static_cast<double>(lhs - rhs) / static_cast<double>(len * len);
    }
    const double med_m = median_of(mean), med_v = median_of(var);
    PSOUP_CHECK(med_m < 2147483647.0, "scrunch_scale: subband " << s << ": mean out of range");
    sc.M[s] = static_cast<int32_t>(std::floor(med_m + 0.5));
    if (nactive[s] > 0 && med_v > 0) {
      sc.live[s] = 1;
      sig.push_back(std::sqrt(med_v));
    }
  }
  sc.nlive = static_cast<int>(sig.size());
  PSOUP_CHECK(sc.nlive > 0, "scrunch: no live subband (every subband is killed or has zero variance)");
  sc.sigma_ref = median_of(sig);
  const double t = sigma_out / sc.sigma_ref * 65536.0 + 0.5;
  if (!(t < 2147483648.0))
    sc.mul = 2147483647;
  else if (t < 1.0)
    sc.mul = 1;
  else
    sc.mul = static_cast<int32_t>(std::floor(t));
  return sc;
}

std::vector<ScrunchTier> scrunch_plan(double tsamp, double fch1, double foff, int nchans, double dm_end) {
  PSOUP_CHECK(tsamp > 0 && nchans >= 1 && foff != 0, "scrunch_plan: tsamp, nchans and foff must be non-zero");
  PSOUP_CHECK(std::isfinite(dm_end) && dm_end >= 0, "scrunch_plan: dm_end must be finite and non-negative");
  const double last = fch1 + static_cast<double>(nchans - 1) * foff;
  const double nu = std::min(fch1, last) / 1000.0;
  PSOUP_CHECK(nu > 0, "scrunch_plan: the lowest channel's frequency must be positive");
  const double unit = tsamp * (nu * nu * nu) / (8.3e-6 * std::fabs(foff));
  std::vector<ScrunchTier> tiers;
  for (int k = 0; k <= 6; ++k) {
    ScrunchTier t;
    t.tscrunch = 1 << k;
    t.dm_lo = (k == 0) ? 0.0 : static_cast<double>(1 << k) * unit;
    if (k > 0 && !(t.dm_lo < dm_end)) break;
    const double next = static_cast<double>(2 << k) * unit;
    t.dm_hi = (k == 6 || !(next < dm_end)) ? dm_end : next;
    tiers.push_back(t);
  }
  return tiers;
}

}  // namespace psoup
