// burstopt, the host steps of psoup/burstopt.hpp: prepare, the fine DM rows
// and their shifts, finish and a host transcription of the search.  No device
// code; compiled with -ffp-contract=off (CMakeLists.txt), so every double
// expression is evaluated as written.
#include <algorithm>
#include <cmath>
#include <limits>
#include <sstream>

#include "psoup/burstopt.hpp"

namespace psoup {

namespace {

using i128 = __int128;

i128 floordiv(i128 a, i128 b) {  // b > 0
  i128 q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

std::string who(size_t k, const BurstOptInput& in) {
  std::ostringstream s;
  s << "burst opt: candidate " << k << " (sample " << in.sample << ", width " << in.width << ", dm " << in.dm << ")";
  return s.str();
}

bool off_pulse(int k, int ntime) { return k < ntime / 4 || k >= ntime - ntime / 4; }

// Step 1 for the rows of one plane.  Returns max|d|; fits is cleared when a d does not fit int32.
int64_t prepare_rows(int nrows, int ntime, const int32_t* sums, const int32_t* hits, int32_t* d, int32_t* cnt,
                     int64_t* moff, int64_t* v2, bool* fits) {
  int64_t maxabs = 0;
  std::vector<i128> q(static_cast<size_t>(ntime));
  for (int r = 0; r < nrows; ++r) {
    const int32_t* sm = sums + static_cast<size_t>(r) * ntime;
    const int32_t* h = hits + static_cast<size_t>(r) * ntime;
    int32_t* dr = d + static_cast<size_t>(r) * ntime;
    cnt[r] = 0;
    moff[r] = 0;
    v2[r] = 0;
    const i128 href = *std::max_element(h, h + ntime);
    if (href <= 0) continue;
    i128 tot = 0;
    int c = 0;
    for (int k = 0; k < ntime; ++k) {
      if (h[k] <= 0) continue;
      q[static_cast<size_t>(k)] = floordiv(2 * i128(sm[k]) * href + h[k], 2 * i128(h[k]));
      if (off_pulse(k, ntime)) {
        tot += q[static_cast<size_t>(k)];
        ++c;
      }
    }
    if (c == 0) continue;
    cnt[r] = c;
    const i128 base = floordiv(tot, static_cast<i128>(c));
    i128 m = 0, v = 0;
    for (int k = 0; k < ntime; ++k) {
      if (h[k] <= 0) continue;
      const i128 dv = q[static_cast<size_t>(k)] - base;
      if (dv < std::numeric_limits<int32_t>::min() || dv > std::numeric_limits<int32_t>::max()) {
        *fits = false;  // the caller refuses the candidate; the rows' liveness is still wanted
        continue;
      }
      dr[k] = static_cast<int32_t>(dv);
      maxabs = std::max<int64_t>(maxabs, static_cast<int64_t>(dv < 0 ? -dv : dv));
      if (off_pulse(k, ntime)) {
        m += dv;
        v += dv * dv;
      }
    }
    // both fit int64 for every candidate that passes the bounds of the definition
    moff[r] = static_cast<int64_t>(m);
    v2[r] = static_cast<int64_t>(v);
  }
  return maxabs;
}

// P of fine row `sf` (int32 [nsub]) and, with w > 0, band[s] at (bin, w).
void fine_profile(const BurstOptGeom& g, const int32_t* d_ds, const int32_t* sf, std::vector<int64_t>& prof) {
  prof.assign(static_cast<size_t>(g.ntime), 0);
  for (int s = 0; s < g.nsub; ++s) {
    const int32_t* row = d_ds + static_cast<size_t>(s) * g.ntime;
    for (int k = 0; k < g.ntime; ++k) {
      const int64_t x = static_cast<int64_t>(k) + sf[s];
      if (x >= 0 && x < g.ntime) prof[static_cast<size_t>(k)] += row[x];
    }
  }
}

}  // namespace

void burst_opt_check_grid(const BurstOptGrid& grid) {
  PSOUP_CHECK(grid.nfine >= 1 && grid.nfine <= kern::kBoptMaxFine && grid.nfine % 2 == 1,
              "burst opt: nfine must be odd and in 1.." << kern::kBoptMaxFine);
  PSOUP_CHECK(std::isfinite(grid.fine_half_range) && grid.fine_half_range >= 0,
              "burst opt: fine_half_range must be finite and non-negative");
}

BurstOptPrepared burst_opt_prepare(size_t k, const BurstOptGeom& g, const BurstOptInput& in) {
  PSOUP_CHECK(g.ntime >= 1 && g.ntime <= kern::kBoptMaxTime && g.nsub >= 1 && g.ndm >= 1,
              "burst opt: the cutouts need ntime in 1.." << kern::kBoptMaxTime << ", nsub >= 1 and ndm >= 1");
  const size_t nt = static_cast<size_t>(g.ntime), ns = static_cast<size_t>(g.nsub), nd = static_cast<size_t>(g.ndm);
  const std::string w = who(k, in);
  PSOUP_CHECK(in.ds_sums.size() == ns * nt && in.ds_hits.size() == ns * nt && in.dmt_sums.size() == nd * nt &&
                  in.dmt_hits.size() == nd * nt && in.dms.size() == nd,
              w << ": the cutout has the wrong shape");
  PSOUP_CHECK(g.ntime >= 8, w << ": ntime = " << g.ntime << " is below 8");
  PSOUP_CHECK(std::isfinite(in.dm) && in.dm >= 0, w << ": the DM must be finite and non-negative");
  PSOUP_CHECK(in.tscrunch >= 1, w << ": tscrunch must be at least 1");

  BurstOptPrepared out;
  out.d_ds.assign(ns * nt, 0);
  out.d_dmt.assign(nd * nt, 0);
  out.cnt_ds.assign(ns, 0);
  out.cnt_dmt.assign(nd, 0);
  out.moff_ds.assign(ns, 0);
  out.moff_dmt.assign(nd, 0);
  out.v2_ds.assign(ns, 0);
  out.v2_dmt.assign(nd, 0);
  out.mbar_dmt.assign(nd, 0.0);
  bool fits = true;
  const int64_t max_ds = prepare_rows(g.nsub, g.ntime, in.ds_sums.data(), in.ds_hits.data(), out.d_ds.data(),
                                      out.cnt_ds.data(), out.moff_ds.data(), out.v2_ds.data(), &fits);
  int64_t nlive = 0;
  for (size_t s = 0; s < ns; ++s) nlive += out.cnt_ds[s] > 0;
  PSOUP_CHECK(nlive > 0, w << ": no waterfall row is live (no off-pulse bin has samples)");
  PSOUP_CHECK(fits, w << ": a baseline-subtracted value does not fit int32");
  const int64_t max_dmt = prepare_rows(g.ndm, g.ntime, in.dmt_sums.data(), in.dmt_hits.data(), out.d_dmt.data(),
                                       out.cnt_dmt.data(), out.moff_dmt.data(), out.v2_dmt.data(), &fits);
  PSOUP_CHECK(fits, w << ": a baseline-subtracted value does not fit int32");
  const i128 lim = i128(1) << 31;
  PSOUP_CHECK(i128(max_ds) * nlive * (g.ntime / 2) < lim,
              w << ": the waterfall's box sums do not fit int32 (max|d| " << max_ds << ")");
  PSOUP_CHECK(i128(max_dmt) * (g.ntime / 2) < lim,
              w << ": the DM-time plane's box sums do not fit int32 (max|d| " << max_dmt << ")");
  for (size_t s = 0; s < ns; ++s) {
    if (out.cnt_ds[s] == 0) continue;
    out.v = out.v + static_cast<double>(out.v2_ds[s]) / static_cast<double>(out.cnt_ds[s]);
    out.mbar_ds = out.mbar_ds + static_cast<double>(out.moff_ds[s]) / static_cast<double>(out.cnt_ds[s]);
  }
  for (size_t j = 0; j < nd; ++j)
    if (out.cnt_dmt[j] > 0) out.mbar_dmt[j] = static_cast<double>(out.moff_dmt[j]) / static_cast<double>(out.cnt_dmt[j]);
  return out;
}

BurstOptShifts burst_opt_shifts(const BurstOptGeom& g, const BurstOptGrid& grid, float dm, uint32_t f,
                                const std::vector<float>& dms, const std::vector<float>& delays) {
  burst_opt_check_grid(grid);
  PSOUP_CHECK(g.nchans >= 1 && static_cast<int>(delays.size()) == g.nchans, "burst opt: delay table size != nchans");
  PSOUP_CHECK(g.nsub >= 1 && g.nsub <= g.nchans, "burst opt: nsub must be in 1..nchans");
  PSOUP_CHECK(static_cast<int>(dms.size()) == g.ndm && g.ndm >= 1, "burst opt: dms size != ndm");
  PSOUP_CHECK(std::isfinite(dm) && f >= 1, "burst opt: bad DM or tscrunch");
  BurstOptShifts sh;
  const int nf = grid.nfine;
  double half = grid.fine_half_range;
  if (!(half > 0))
    half = g.ndm == 1 ? 0.0
                      : static_cast<double>(dms[static_cast<size_t>(g.ndm / 2)]) -
                            static_cast<double>(dms[static_cast<size_t>(g.ndm / 2 - 1)]);
  const double step = nf == 1 ? 0.0 : half / (nf / 2);
  const double dm0 = static_cast<double>(dm);
  sh.dmf.resize(static_cast<size_t>(nf));
  for (int kf = 0; kf < nf; ++kf)
    sh.dmf[static_cast<size_t>(kf)] = static_cast<float>(std::max(0.0, dm0 + (kf - nf / 2) * step));
  std::vector<int> c0(static_cast<size_t>(g.nsub), -1), c1(static_cast<size_t>(g.nsub), -1);
  for (int c = 0; c < g.nchans; ++c) {
    const size_t s = static_cast<size_t>(static_cast<int64_t>(c) * g.nsub / g.nchans);
    if (c0[s] < 0) c0[s] = c;
    c1[s] = c;
  }
  sh.sf.resize(static_cast<size_t>(nf) * g.nsub);
  const double fd = static_cast<double>(f);
  for (int kf = 0; kf < nf; ++kf)
    for (int s = 0; s < g.nsub; ++s) {
      const double dsub = 0.5 * (static_cast<double>(delays[static_cast<size_t>(c0[static_cast<size_t>(s)])]) +
                                 static_cast<double>(delays[static_cast<size_t>(c1[static_cast<size_t>(s)])]));
      const double x = (static_cast<double>(sh.dmf[static_cast<size_t>(kf)]) - dm0) * dsub / fd;
      PSOUP_CHECK(std::isfinite(x), "burst opt: a DM shift is not finite");
      const double r = std::min(std::max(std::rint(x), -static_cast<double>(g.ntime)), static_cast<double>(g.ntime));
      sh.sf[static_cast<size_t>(kf) * g.nsub + s] = static_cast<int32_t>(r);
    }
  return sh;
}

double burst_opt_snr(double s, int w, double mbar, double v) {
  if (!(v > 0)) return 0.0;
  return (s - w * mbar) / std::sqrt(v * w);
}

BurstOptSearch burst_opt_search_host(const BurstOptGeom& g, int nfine, const std::vector<int32_t>& d_ds,
                                     const std::vector<int32_t>& d_dmt, const std::vector<int32_t>& sf) {
  const int nt = g.ntime, nw = kern::bopt_nwidths(nt), nrows = g.ndm + nfine;
  PSOUP_CHECK(nt >= 2 && d_ds.size() == static_cast<size_t>(g.nsub) * nt &&
                  d_dmt.size() == static_cast<size_t>(g.ndm) * nt && sf.size() == static_cast<size_t>(nfine) * g.nsub,
              "burst opt: the search tables have the wrong shape");
  BurstOptSearch out;
  const int32_t lo = std::numeric_limits<int32_t>::min();
  out.best_val.assign(static_cast<size_t>(2) * nw, lo);
  out.best_idx.assign(static_cast<size_t>(2) * nw, 0);
  out.curve.assign(static_cast<size_t>(nw) * nrows, lo);
  out.curve_bin.assign(static_cast<size_t>(nw) * nrows, 0);
  std::vector<int64_t> box;
  for (int r = 0; r < nrows; ++r) {
    const int plane = r >= g.ndm, rl = plane ? r - g.ndm : r;
    if (plane) {
      fine_profile(g, d_ds.data(), sf.data() + static_cast<size_t>(rl) * g.nsub, box);
    } else {
      box.assign(d_dmt.begin() + static_cast<size_t>(r) * nt, d_dmt.begin() + static_cast<size_t>(r + 1) * nt);
    }
    for (int kw = 0, w = 1; kw < nw; ++kw, w *= 2) {
      int32_t& cv = out.curve[static_cast<size_t>(kw) * nrows + r];
      int32_t& cb = out.curve_bin[static_cast<size_t>(kw) * nrows + r];
      for (int k = 0; k + w <= nt; ++k) {
        const int32_t v = static_cast<int32_t>(box[static_cast<size_t>(k)]);
        if (k == 0 || v > cv) {
          cv = v;
          cb = k;
        }
      }
      int32_t& bv = out.best_val[static_cast<size_t>(plane) * nw + kw];
      if (rl == 0 || cv > bv) {  // rows in ascending order: the first maximum stays
        bv = cv;
        out.best_idx[static_cast<size_t>(plane) * nw + kw] = rl * nt + cb;
      }
      for (int k = 0; k + 2 * w <= nt; ++k) box[static_cast<size_t>(k)] += box[static_cast<size_t>(k + w)];
    }
  }
  return out;
}

BurstOptResult burst_opt_finish(const BurstOptGeom& g, const BurstOptGrid& grid, const BurstOptInput& in,
                                const BurstOptPrepared& prep, const BurstOptShifts& sh, const BurstOptSearch& found) {
  const int nt = g.ntime, nw = kern::bopt_nwidths(nt), nf = grid.nfine, nrows = g.ndm + nf;
  PSOUP_CHECK(found.best_val.size() == static_cast<size_t>(2) * nw && found.best_idx.size() == found.best_val.size() &&
                  found.curve.size() == static_cast<size_t>(nw) * nrows && found.curve_bin.size() == found.curve.size(),
              "burst opt: search outputs have the wrong shape");
  PSOUP_CHECK(prep.d_ds.size() == static_cast<size_t>(g.nsub) * nt && prep.cnt_ds.size() == static_cast<size_t>(g.nsub) &&
                  prep.moff_ds.size() == prep.cnt_ds.size() && prep.mbar_dmt.size() == static_cast<size_t>(g.ndm) &&
                  sh.dmf.size() == static_cast<size_t>(nf) && sh.sf.size() == static_cast<size_t>(nf) * g.nsub &&
                  in.dms.size() == static_cast<size_t>(g.ndm),
              "burst opt: prepared tables have the wrong shape");
  BurstOptResult r;
  r.v = prep.v;
  r.mbar_ds = prep.mbar_ds;
  r.dms = in.dms;
  r.dmf = sh.dmf;
  r.mbar_dmt = prep.mbar_dmt;
  r.search = found;
  auto best_of = [&](auto value_of, auto mbar_of, int* which) {
    double best = 0;
    for (int k = 0, w = 1; k < nw; ++k, w *= 2) {
      const double s = burst_opt_snr(static_cast<double>(value_of(k)), w, mbar_of(k), prep.v);
      if (k == 0 || s > best) {
        best = s;
        if (which) *which = k;
      }
    }
    return best;
  };
  for (int k = 0; k < 2 * nw; ++k) {
    const int64_t rows = k < nw ? g.ndm : nf;
    PSOUP_CHECK(found.best_idx[static_cast<size_t>(k)] >= 0 && found.best_idx[static_cast<size_t>(k)] < rows * nt,
                "burst opt: a best index is out of range");
  }
  // ---- the coarse plane
  int kc = 0;
  r.snr_coarse = best_of([&](int k) { return found.best_val[static_cast<size_t>(k)]; },
                         [&](int k) { return prep.mbar_dmt[static_cast<size_t>(found.best_idx[static_cast<size_t>(k)] / nt)]; },
                         &kc);
  r.coarse_row = static_cast<uint32_t>(found.best_idx[static_cast<size_t>(kc)] / nt);
  r.coarse_bin = static_cast<uint32_t>(found.best_idx[static_cast<size_t>(kc)] % nt);
  r.coarse_dm = in.dms[r.coarse_row];
  r.coarse_width = (1u << kc) * in.tscrunch;
  const size_t jin = static_cast<size_t>(g.ndm / 2);
  r.snr_in = best_of([&](int k) { return found.curve[static_cast<size_t>(k) * nrows + jin]; },
                     [&](int) { return prep.mbar_dmt[jin]; }, nullptr);
  if (in.dms[0] == 0.f) {
    r.snr_dm0 = best_of([&](int k) { return found.curve[static_cast<size_t>(k) * nrows]; },
                        [&](int) { return prep.mbar_dmt[0]; }, nullptr);
  } else {
    r.snr_dm0 = 0;
    r.flags |= 1u;
  }
  // ---- the fine plane
  int kb = 0;
  r.snr = best_of([&](int k) { return found.best_val[static_cast<size_t>(nw + k)]; },
                  [&](int) { return prep.mbar_ds; }, &kb);
  const int32_t idx = found.best_idx[static_cast<size_t>(nw + kb)];
  const int w = 1 << kb;
  r.opt_kf = static_cast<uint32_t>(idx / nt);
  r.opt_bin = static_cast<uint32_t>(idx % nt);
  r.opt_dm = sh.dmf[r.opt_kf];
  r.opt_width = static_cast<uint32_t>(w) * in.tscrunch;
  r.opt_sample = in.t0 + static_cast<int64_t>(r.opt_bin) * static_cast<int64_t>(in.tscrunch);
  const int32_t* sf = sh.sf.data() + static_cast<size_t>(r.opt_kf) * g.nsub;
  std::vector<int64_t> prof;
  fine_profile(g, prep.d_ds.data(), sf, prof);
  r.profile.assign(prof.begin(), prof.end());
  r.band.assign(static_cast<size_t>(g.nsub), 0);
  int nlive = 0, npos = 0;
  for (int s = 0; s < g.nsub; ++s) {
    if (prep.cnt_ds[static_cast<size_t>(s)] == 0) continue;
    const int32_t* row = prep.d_ds.data() + static_cast<size_t>(s) * nt;
    int64_t b = 0;
    for (int i = 0; i < w; ++i) {
      const int64_t x = static_cast<int64_t>(r.opt_bin) + i + sf[s];
      if (x >= 0 && x < nt) b += row[x];
    }
    r.band[static_cast<size_t>(s)] = static_cast<int32_t>(b);
    ++nlive;
    const double mean = static_cast<double>(prep.moff_ds[static_cast<size_t>(s)]) /
                        static_cast<double>(prep.cnt_ds[static_cast<size_t>(s)]);
    if (static_cast<double>(b) - w * mean > 0) ++npos;
  }
  r.frac_pos = nlive > 0 ? static_cast<double>(npos) / static_cast<double>(nlive) : 0.0;
  return r;
}

}  // namespace psoup
