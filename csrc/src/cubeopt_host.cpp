// cubeopt, the host steps of psoup/cubeopt.hpp: prepare, the shift tables,
// finish and a host transcription of the search.  No device code; compiled
// with -ffp-contract=off (CMakeLists.txt), so every double expression is
// evaluated as written.
#include <algorithm>
#include <cmath>
#include <limits>
#include <sstream>

#include "psoup/burstcube.hpp"
#include "psoup/cubeopt.hpp"

namespace psoup {

namespace {

constexpr double kC = 299792458.0;
using i128 = __int128;

i128 floordiv(i128 a, i128 b) {  // b > 0
  i128 q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

std::string who(size_t k, const CubeOptInput& in) {
  std::ostringstream s;
  s << "cube opt: candidate " << k << " (period " << in.period << " s, dm " << in.dm << ", acc " << in.acc << ")";
  return s.str();
}

// rint(x) reduced into [0, n); x finite.
int32_t reduced_shift(double x, int n) {
  double r = std::fmod(std::rint(x), static_cast<double>(n));  // exact
  if (r < 0) r += n;
  return static_cast<int32_t>(r);
}

void profile_of(const CubeOptGeom& g, const int32_t* d, const int32_t* sdm, const int32_t* st,
                std::vector<int64_t>& a, std::vector<int64_t>& prof) {
  const int nb = g.nbins;
  if (sdm != nullptr) {
    a.assign(static_cast<size_t>(g.nints) * nb, 0);
    for (int i = 0; i < g.nints; ++i)
      for (int s = 0; s < g.nsub; ++s) {
        const int32_t* row = d + (static_cast<size_t>(i) * g.nsub + s) * nb;
        for (int b = 0; b < nb; ++b) a[static_cast<size_t>(i) * nb + b] += row[(b + sdm[s]) % nb];
      }
  }
  prof.assign(static_cast<size_t>(nb), 0);
  for (int i = 0; i < g.nints; ++i)
    for (int b = 0; b < nb; ++b) prof[static_cast<size_t>(b)] += a[static_cast<size_t>(i) * nb + (b + st[i]) % nb];
}

}  // namespace

void cube_opt_check_grid(const CubeOptGrid& grid) {
  PSOUP_CHECK(grid.ndm >= 1 && grid.ndm <= 256, "cube opt: ndm must be in 1..256");
  PSOUP_CHECK(grid.np >= 1 && grid.np <= 257 && grid.np % 2 == 1, "cube opt: np must be odd and in 1..257");
  PSOUP_CHECK(grid.npd >= 1 && grid.npd <= 129 && grid.npd % 2 == 1, "cube opt: npd must be odd and in 1..129");
  PSOUP_CHECK(std::isfinite(grid.p_step) && std::isfinite(grid.pd_step) && grid.p_step >= 0 && grid.pd_step >= 0,
              "cube opt: p_step and pd_step must be finite and non-negative");
  PSOUP_CHECK(std::isfinite(grid.dm_half_range) && grid.dm_half_range >= 0,
              "cube opt: dm_half_range must be non-negative");
}

CubeOptPrepared cube_opt_prepare(size_t k, const CubeOptGeom& g, const CubeOptGrid& grid, const CubeOptInput& in) {
  PSOUP_CHECK(g.nints >= 1 && g.nsub >= 1 && g.nbins >= 2 && g.nbins <= kern::kOptMaxBins,
              "cube opt: the cubes need nints >= 1, nsub >= 1 and nbins in 2.." << kern::kOptMaxBins);
  const size_t nints = static_cast<size_t>(g.nints), nsub = static_cast<size_t>(g.nsub),
               nbins = static_cast<size_t>(g.nbins);
  const std::string w = who(k, in);
  PSOUP_CHECK(in.nactive.size() == nsub && in.hits.size() == nints * nbins && in.sums.size() == nints * nsub * nbins,
              w << ": the cube has the wrong shape");
  for (size_t j = 0; j < in.hits.size(); ++j)
    PSOUP_CHECK(in.hits[j] > 0, w << ": subint " << j / nbins << " has no sample in bin " << j % nbins
                                  << " (fold fewer bins or subints)");
  PSOUP_CHECK(nints * nbins <= static_cast<size_t>(kern::kOptMaxPlane),
              w << ": nints * nbins = " << nints * nbins << " exceeds " << kern::kOptMaxPlane);
  const uint64_t trials = static_cast<uint64_t>(grid.ndm) * grid.np * grid.npd * nbins;
  PSOUP_CHECK(trials < (uint64_t(1) << 31), w << ": " << trials << " trial bins do not fit 31 bits");
  PSOUP_CHECK(std::isfinite(in.period) && in.period > 0, w << ": the period must be positive");
  PSOUP_CHECK(std::isfinite(in.dm) && std::isfinite(in.acc), w << ": the DM and the acceleration must be finite");

  CubeOptPrepared out;
  out.d.assign(nints * nsub * nbins, 0);
  const i128 lim63 = i128(1) << 63;
  int64_t maxabs = 0;
  size_t nlive = 0;
  for (size_t s = 0; s < nsub; ++s) nlive += in.nactive[s] > 0;
  std::vector<i128> q(nbins);
  i128 mtot = 0, v2 = 0;
  for (size_t i = 0; i < nints; ++i) {
    const int32_t* h = in.hits.data() + i * nbins;
    const i128 href = *std::max_element(h, h + nbins);
    for (size_t s = 0; s < nsub; ++s) {
      const int64_t* sm = in.sums.data() + (i * nsub + s) * nbins;
      i128 tot = 0;
      for (size_t b = 0; b < nbins; ++b) {
        const i128 t = 2 * i128(sm[b]) * href;
        PSOUP_CHECK(t < lim63 && -t < lim63, w << ": 2 * sums * Href does not fit 63 bits");
        q[b] = floordiv(t + h[b], 2 * i128(h[b]));
        tot += q[b];
      }
      if (in.nactive[s] <= 0) continue;
      const i128 base = floordiv(tot, static_cast<i128>(nbins));
      for (size_t b = 0; b < nbins; ++b) {
        const i128 dv = q[b] - base;
        PSOUP_CHECK(dv >= std::numeric_limits<int32_t>::min() && dv <= std::numeric_limits<int32_t>::max(),
                    w << ": a baseline-subtracted value does not fit int32");
        out.d[(i * nsub + s) * nbins + b] = static_cast<int32_t>(dv);
        maxabs = std::max<int64_t>(maxabs, static_cast<int64_t>(dv < 0 ? -dv : dv));
        mtot += dv;
        v2 += dv * dv;
      }
    }
  }
  const i128 bound = i128(maxabs) * static_cast<i128>(nints) * static_cast<i128>(nlive) * static_cast<i128>(nbins / 2);
  PSOUP_CHECK(bound < (i128(1) << 31), w << ": the box sums do not fit int32 (max|d| " << maxabs << ")");
  out.mtot = static_cast<int64_t>(mtot);
  out.v2 = static_cast<int64_t>(v2);
  out.v = static_cast<double>(out.v2) / static_cast<double>(g.nbins);
  return out;
}

CubeOptShifts cube_opt_shifts(const CubeOptGeom& g, const CubeOptGrid& grid, double period, float dm,
                              const std::vector<float>& delays) {
  cube_opt_check_grid(grid);
  PSOUP_CHECK(g.nchans >= 1 && static_cast<int>(delays.size()) == g.nchans, "cube opt: delay table size != nchans");
  PSOUP_CHECK(g.nsub >= 1 && g.nsub <= g.nchans, "cube opt: nsub must be in 1..nchans");
  PSOUP_CHECK(std::isfinite(period) && period > 0 && std::isfinite(dm), "cube opt: bad period or DM");
  CubeOptShifts sh;
  sh.dms = burst_dms(dm, grid.ndm, grid.dm_half_range);
  const int nb = g.nbins;
  // the first and last channel of every subband
  std::vector<int> c0(static_cast<size_t>(g.nsub), -1), c1(static_cast<size_t>(g.nsub), -1);
  for (int c = 0; c < g.nchans; ++c) {
    const size_t s = static_cast<size_t>(static_cast<int64_t>(c) * g.nsub / g.nchans);
    if (c0[s] < 0) c0[s] = c;
    c1[s] = c;
  }
  const double tbp = static_cast<double>(static_cast<float>(g.tsamp)) / period;
  const double dm0 = static_cast<double>(dm);
  sh.sdm.resize(static_cast<size_t>(grid.ndm) * g.nsub);
  for (int kd = 0; kd < grid.ndm; ++kd)
    for (int s = 0; s < g.nsub; ++s) {
      const double dsub = 0.5 * (static_cast<double>(delays[static_cast<size_t>(c0[static_cast<size_t>(s)])]) +
                                 static_cast<double>(delays[static_cast<size_t>(c1[static_cast<size_t>(s)])]));
      const double x = (static_cast<double>(sh.dms[static_cast<size_t>(kd)]) - dm0) * dsub * tbp * nb;
      PSOUP_CHECK(std::isfinite(x), "cube opt: a DM shift is not finite");
      sh.sdm[static_cast<size_t>(kd) * g.nsub + s] = reduced_shift(x, nb);
    }
  sh.st.resize(static_cast<size_t>(grid.np) * grid.npd * g.nints);
  for (int kp = 0; kp < grid.np; ++kp)
    for (int kpd = 0; kpd < grid.npd; ++kpd) {
      const double L = (kp - grid.np / 2) * grid.p_step;
      const double Q = (kpd - grid.npd / 2) * grid.pd_step;
      for (int i = 0; i < g.nints; ++i) {
        const double u = (i + 0.5) / g.nints;
        const double x = L * (u - 0.5) + Q * (4.0 * u * (1.0 - u));
        sh.st[(static_cast<size_t>(kp) * grid.npd + kpd) * g.nints + i] = reduced_shift(x, nb);
      }
    }
  return sh;
}

double cube_opt_snr(double s, int w, int64_t mtot, double v, int nbins) {
  if (!(v > 0)) return 0.0;
  return (s - w * static_cast<double>(mtot) / nbins) / std::sqrt(v * w * (1.0 - static_cast<double>(w) / nbins));
}

CubeOptSearch cube_opt_search_host(const CubeOptGeom& g, const CubeOptGrid& grid, const std::vector<int32_t>& d,
                                   const CubeOptShifts& sh) {
  const int nb = g.nbins, nw = kern::opt_nwidths(nb);
  PSOUP_CHECK(d.size() == static_cast<size_t>(g.nints) * g.nsub * nb, "cube opt: d has the wrong shape");
  CubeOptSearch out;
  const int32_t lo = std::numeric_limits<int32_t>::min();
  out.best_val.assign(static_cast<size_t>(nw), lo);
  out.best_idx.assign(static_cast<size_t>(nw), 0);
  out.centre.assign(static_cast<size_t>(nw), lo);
  out.dmcurve.assign(static_cast<size_t>(nw) * grid.ndm, lo);
  out.ppd.assign(static_cast<size_t>(nw) * grid.np * grid.npd, lo);
  std::vector<int64_t> a, prof, box(static_cast<size_t>(nb)), next(static_cast<size_t>(nb));
  for (int kd = 0; kd < grid.ndm; ++kd)
    for (int kp = 0; kp < grid.np; ++kp)
      for (int kpd = 0; kpd < grid.npd; ++kpd) {
        const size_t t = static_cast<size_t>(kp) * grid.npd + kpd;
        profile_of(g, d.data(), (kp == 0 && kpd == 0) ? sh.sdm.data() + static_cast<size_t>(kd) * g.nsub : nullptr,
                   sh.st.data() + t * g.nints, a, prof);
        box = prof;
        for (int k = 0, w = 1; k < nw; ++k, w *= 2) {
          for (int b = 0; b < nb; ++b) {
            const int32_t v = static_cast<int32_t>(box[static_cast<size_t>(b)]);
            const int32_t idx = static_cast<int32_t>((static_cast<size_t>(kd) * grid.np * grid.npd + t) * nb + b);
            if (v > out.best_val[static_cast<size_t>(k)]) {
              out.best_val[static_cast<size_t>(k)] = v;
              out.best_idx[static_cast<size_t>(k)] = idx;
            }
            int32_t& dc = out.dmcurve[static_cast<size_t>(k) * grid.ndm + kd];
            dc = std::max(dc, v);
            int32_t& pp = out.ppd[static_cast<size_t>(k) * grid.np * grid.npd + t];
            pp = std::max(pp, v);
            if (kd == grid.ndm / 2 && kp == grid.np / 2 && kpd == grid.npd / 2)
              out.centre[static_cast<size_t>(k)] = std::max(out.centre[static_cast<size_t>(k)], v);
          }
          for (int b = 0; b < nb; ++b)
            next[static_cast<size_t>(b)] = box[static_cast<size_t>(b)] + box[static_cast<size_t>((b + w) % nb)];
          box.swap(next);
        }
      }
  return out;
}

CubeOptResult cube_opt_finish(const CubeOptGeom& g, const CubeOptGrid& grid, double period, float acc,
                              const CubeOptPrepared& prep, const CubeOptShifts& sh, const CubeOptSearch& found) {
  const int nb = g.nbins, nw = kern::opt_nwidths(nb);
  PSOUP_CHECK(found.best_val.size() == static_cast<size_t>(nw) && found.best_idx.size() == static_cast<size_t>(nw) &&
                  found.centre.size() == static_cast<size_t>(nw) &&
                  found.dmcurve.size() == static_cast<size_t>(nw) * grid.ndm &&
                  found.ppd.size() == static_cast<size_t>(nw) * grid.np * grid.npd,
              "cube opt: search outputs have the wrong shape");
  CubeOptResult r;
  r.mtot = prep.mtot;
  r.v = prep.v;
  r.dms = sh.dms;
  r.search = found;
  auto best_of = [&](auto value_of, int* which) {
    double best = 0;
    for (int k = 0, w = 1; k < nw; ++k, w *= 2) {
      const double s = cube_opt_snr(static_cast<double>(value_of(k)), w, prep.mtot, prep.v, nb);
      if (k == 0 || s > best) {
        best = s;
        if (which) *which = k;
      }
    }
    return best;
  };
  int kbest = 0;
  r.snr = best_of([&](int k) { return found.best_val[static_cast<size_t>(k)]; }, &kbest);
  r.snr_in = best_of([&](int k) { return found.centre[static_cast<size_t>(k)]; }, nullptr);
  if (sh.dms[0] == 0.f) {
    r.snr_dm0 = best_of([&](int k) { return found.dmcurve[static_cast<size_t>(k) * grid.ndm]; }, nullptr);
  } else {
    r.snr_dm0 = 0;
    r.flags |= 1u;
  }
  const int64_t idx = found.best_idx[static_cast<size_t>(kbest)];
  PSOUP_CHECK(idx >= 0 && idx < static_cast<int64_t>(grid.ndm) * grid.np * grid.npd * nb,
              "cube opt: a best index is out of range");
  r.opt_width = 1u << kbest;
  r.opt_bin = static_cast<uint32_t>(idx % nb);
  const int64_t t = idx / nb;
  r.opt_kpd = static_cast<uint32_t>(t % grid.npd);
  r.opt_kp = static_cast<uint32_t>((t / grid.npd) % grid.np);
  r.opt_kd = static_cast<uint32_t>(t / grid.npd / grid.np);
  r.opt_dm = sh.dms[r.opt_kd];
  const double L = (static_cast<int>(r.opt_kp) - grid.np / 2) * grid.p_step;
  const double Q = (static_cast<int>(r.opt_kpd) - grid.npd / 2) * grid.pd_step;
  const double ts = static_cast<double>(static_cast<float>(g.tsamp));
  const double n = static_cast<double>(g.fold_nsamps);
  const double T = n * ts;
  r.opt_period = 1.0 / (1.0 / period - L / (nb * T));
  r.opt_acc = static_cast<double>(acc) - (8.0 * kC * Q * period) / (nb * ts * ts * n * n);
  std::vector<int64_t> a, prof;
  profile_of(g, prep.d.data(), sh.sdm.data() + static_cast<size_t>(r.opt_kd) * g.nsub,
             sh.st.data() + (static_cast<size_t>(r.opt_kp) * grid.npd + r.opt_kpd) * g.nints, a, prof);
  r.profile.assign(prof.begin(), prof.end());
  return r;
}

}  // namespace psoup
