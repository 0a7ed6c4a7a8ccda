// Host unit tests of burstopt's host steps (psoup/burstopt.hpp): prepare on
// hand-made cutouts (empty bins, a dead row, the refusals), the fine DM rows
// and shifts, the host search's tie rule and its non-circular box, and finish
// on a planted pulse.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/burstopt.hpp"

using namespace psoup;

static int g_failed = 0;
#define EXPECT(cond)                                                            \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond << std::endl;      \
      ++g_failed;                                                               \
    }                                                                           \
  } while (0)

namespace {

BurstOptGeom geom(int ntime, int nsub, int ndm, int nchans) {
  BurstOptGeom g;
  g.ntime = ntime;
  g.nsub = nsub;
  g.ndm = ndm;
  g.nchans = nchans;
  g.tsamp = 320e-6;
  g.fch1 = 1510.0;
  g.foff = -1.09;
  return g;
}

BurstOptInput flat_input(const BurstOptGeom& g, int32_t hit, int32_t level) {
  BurstOptInput in;
  in.sample = 1000;
  in.width = 4;
  in.tscrunch = 2;
  in.t0 = 1002 - (g.ntime / 2) * 2;
  in.dm = 100.f;
  in.dms.assign(static_cast<size_t>(g.ndm), 0.f);
  for (int j = 0; j < g.ndm; ++j) in.dms[static_cast<size_t>(j)] = 100.f + (j - g.ndm / 2) * 200.f / g.ndm;
  in.nactive.assign(static_cast<size_t>(g.nsub), 2);
  in.ds_hits.assign(static_cast<size_t>(g.nsub) * g.ntime, hit);
  in.ds_sums.assign(static_cast<size_t>(g.nsub) * g.ntime, level * hit);
  in.dmt_hits.assign(static_cast<size_t>(g.ndm) * g.ntime, hit * g.nsub);
  in.dmt_sums.assign(static_cast<size_t>(g.ndm) * g.ntime, level * hit * g.nsub);
  return in;
}

bool throws_with(const std::string& text, const BurstOptGeom& g, const BurstOptInput& in) {
  try {
    burst_opt_prepare(3, g, in);
  } catch (const std::exception& e) {
    return std::string(e.what()).find(text) != std::string::npos;
  }
  return false;
}

void test_prepare() {
  const BurstOptGeom g = geom(8, 3, 2, 6);
  BurstOptInput in = flat_input(g, 10, 7);
  // off-pulse bins of ntime 8: 0, 1, 6, 7.  Subband 0: bin 1 has half the hits at the same rate, bin 6 is empty,
  // a pulse of 40 in bin 4; subband 1 has no hits at all (killed); subband 2 is flat.
  in.ds_hits[1] = 5;
  in.ds_sums[1] = 35;
  in.ds_hits[6] = 0;
  in.ds_sums[6] = 0;
  in.ds_sums[4] += 40;
  for (int k = 0; k < 8; ++k) in.ds_hits[8 + static_cast<size_t>(k)] = in.ds_sums[8 + static_cast<size_t>(k)] = 0;
  in.nactive[1] = 0;
  const BurstOptPrepared p = burst_opt_prepare(0, g, in);
  // q = 70 in every filled bin but the pulse (110); B = (70 + 70 + 70) // 3 = 70 over the three filled off-pulse bins
  EXPECT(p.cnt_ds[0] == 3 && p.cnt_ds[1] == 0 && p.cnt_ds[2] == 4);
  for (int k = 0; k < 8; ++k) EXPECT(p.d_ds[static_cast<size_t>(k)] == (k == 4 ? 40 : 0));
  for (int k = 0; k < 16; ++k) EXPECT(p.d_ds[8 + static_cast<size_t>(k)] == 0);
  EXPECT(p.moff_ds[0] == 0 && p.v2_ds[0] == 0 && p.v == 0.0 && p.mbar_ds == 0.0);
  EXPECT(p.cnt_dmt[0] == 4 && p.mbar_dmt[0] == 0.0);
  // an off-pulse excess gives Moff and V2: bin 0 of subband 2 at 11 per hit
  in.ds_sums[16] = 110;
  const BurstOptPrepared p2 = burst_opt_prepare(0, g, in);
  // q = 110, 70, 70, 70 over the off-pulse bins: B = 320 // 4 = 80; d = 30, -10, -10, -10 there
  EXPECT(p2.d_ds[16] == 30 && p2.d_ds[17] == -10 && p2.d_ds[19] == -10);
  EXPECT(p2.moff_ds[2] == 0 && p2.v2_ds[2] == 1200 && p2.v == 300.0);
  // refusals name the candidate
  EXPECT(throws_with("candidate 3 ", geom(7, 3, 2, 6), flat_input(geom(7, 3, 2, 6), 10, 7)));
  BurstOptInput bad = in;
  for (size_t i = 0; i < bad.ds_hits.size(); ++i) bad.ds_hits[i] = 0;
  EXPECT(throws_with("candidate 3 ", g, bad));
  bad = in;
  bad.ds_hits[4] = 1;
  bad.ds_sums[4] = 2000000000;  // q = 2e10: d does not fit int32
  EXPECT(throws_with("does not fit int32", g, bad));
  bad = in;
  bad.ds_hits[4] = 10;
  bad.ds_sums[4] = 2000000000;  // d = 2e9 fits, 2e9 x 2 live rows x 4 does not
  EXPECT(throws_with("waterfall's box sums", g, bad));
  bad = in;
  bad.dmt_sums[4] = 2000000000;
  EXPECT(throws_with("DM-time plane's box sums", g, bad));
  bad = in;
  bad.dm = -1.f;
  EXPECT(throws_with("candidate 3 ", g, bad));
}

void test_shifts() {
  const BurstOptGeom g = geom(16, 2, 4, 8);
  BurstOptGrid gr;
  gr.nfine = 5;
  std::vector<float> delays(8);
  for (int c = 0; c < 8; ++c) delays[static_cast<size_t>(c)] = 0.25f * c;
  const std::vector<float> dms = {0.f, 50.f, 100.f, 150.f};
  const BurstOptShifts s = burst_opt_shifts(g, gr, 100.f, 2, dms, delays);
  // the default half range is the spacing of rows 1 and 2, 50: the fine rows step by 25
  EXPECT(s.dmf.size() == 5 && s.dmf[0] == 50.f && s.dmf[2] == 100.f && s.dmf[4] == 150.f);
  for (int sub = 0; sub < 2; ++sub) EXPECT(s.sf[2 * 2 + static_cast<size_t>(sub)] == 0);
  // dsub = 0.5 (0 + 0.75) = 0.375 and 0.5 (1 + 1.75) = 1.375; row 4: rint(50 * 0.375 / 2) = rint(9.375) = 9,
  // rint(50 * 1.375 / 2) = rint(34.375) clamps to ntime = 16; row 0 mirrors them
  EXPECT(s.sf[4 * 2] == 9 && s.sf[4 * 2 + 1] == 16 && s.sf[0] == -9 && s.sf[1] == -16);
  gr.fine_half_range = 8.0;
  EXPECT(burst_opt_shifts(g, gr, 100.f, 2, dms, delays).dmf[4] == 108.f);
  gr.nfine = 1;
  const BurstOptShifts one = burst_opt_shifts(g, gr, 3.f, 2, dms, delays);
  EXPECT(one.dmf.size() == 1 && one.dmf[0] == 3.f && one.sf[0] == 0 && one.sf[1] == 0);
  gr.nfine = 4;
  bool threw = false;
  try {
    burst_opt_check_grid(gr);
  } catch (const std::exception&) {
    threw = true;
  }
  EXPECT(threw);
}

void test_search_and_finish() {
  const BurstOptGeom g = geom(16, 2, 3, 8);
  BurstOptGrid gr;
  gr.nfine = 3;
  const int nw = kern::bopt_nwidths(16), nrows = 6;
  EXPECT(nw == 4 && kern::bopt_nwidths(8) == 3 && kern::bopt_nwidths(9) == 3 && kern::bopt_nwidths(1024) == 10);
  // the tie rule on all-equal negative planes: index 0, and the box does not wrap
  std::vector<int32_t> ds(2 * 16, -3), dmt(3 * 16, -5), sf(3 * 2, 0);
  BurstOptSearch f = burst_opt_search_host(g, 3, ds, dmt, sf);
  for (int k = 0; k < nw; ++k) {
    EXPECT(f.best_idx[static_cast<size_t>(k)] == 0 && f.best_idx[static_cast<size_t>(nw + k)] == 0);
    EXPECT(f.best_val[static_cast<size_t>(k)] == -5 * (1 << k) && f.best_val[static_cast<size_t>(nw + k)] == -6 * (1 << k));
  }
  // a pulse in the last bin is seen by width 1 only at bin 15, by width 8 at bin 8 (the smallest start that holds it)
  std::fill(dmt.begin(), dmt.end(), 0);
  dmt[16 + 15] = 9;
  f = burst_opt_search_host(g, 3, ds, dmt, sf);
  EXPECT(f.best_val[0] == 9 && f.best_idx[0] == 16 + 15 && f.best_idx[3] == 16 + 8);
  EXPECT(f.curve[0 * nrows + 1] == 9 && f.curve_bin[0 * nrows + 1] == 15 && f.curve[0] == 0 && f.curve_bin[0] == 0);
  // a pulse dispersed along fine row 2's shifts is found there at bin 5; a shifted read outside the row gives 0
  std::fill(ds.begin(), ds.end(), 0);
  sf = {-2, -1, 0, 0, 3, 16};
  ds[5 + 3] = 100;
  ds[16 + 0] = 7;  // subband 1 at shift 16 never lands in the window
  f = burst_opt_search_host(g, 3, ds, dmt, sf);
  EXPECT(f.curve[0 * nrows + 3 + 2] == 100 && f.curve_bin[0 * nrows + 3 + 2] == 5);
  EXPECT(f.curve[0 * nrows + 3 + 1] == 100 && f.curve_bin[0 * nrows + 3 + 1] == 8);
  EXPECT(f.best_val[static_cast<size_t>(nw)] == 100 && f.best_idx[static_cast<size_t>(nw)] == 0 * 16 + 10);
  BurstOptInput in = flat_input(g, 1, 1);
  in.dms = {0.f, 100.f, 200.f};
  BurstOptPrepared p;
  p.d_ds = ds;
  p.d_dmt = dmt;
  p.cnt_ds = {8, 8};
  p.cnt_dmt = {8, 8, 8};
  p.moff_ds = {8, 0};
  p.moff_dmt = {0, 16, 0};
  p.v2_ds = {80, 80};
  p.v2_dmt = {0, 0, 0};
  p.v = 20.0;
  p.mbar_ds = 1.0;
  p.mbar_dmt = {0.0, 2.0, 0.0};
  BurstOptShifts sh;
  sh.dmf = {90.f, 100.f, 110.f};
  sh.sf = sf;
  const BurstOptResult r = burst_opt_finish(g, gr, in, p, sh, f);
  // three trials reach 100; the smallest flat index is row 0 (shift -2) at bin 10
  EXPECT(r.opt_kf == 0 && r.opt_bin == 10 && r.opt_dm == 90.f && r.opt_width == 2 && r.profile[10] == 100);
  EXPECT(r.opt_sample == in.t0 + 20 && r.band[0] == 100 && r.band[1] == 0 && r.frac_pos == 0.5);
  EXPECT(std::fabs(r.snr - 99.0 / std::sqrt(20.0)) < 1e-12);
  EXPECT(r.coarse_row == 1 && r.coarse_bin == 15 && r.coarse_dm == 100.f && r.coarse_width == 2 && r.flags == 0);
  EXPECT(std::fabs(r.snr_coarse - 7.0 / std::sqrt(20.0)) < 1e-12 && r.snr_in == r.snr_coarse && r.snr_dm0 == 0.0);
  in.dms[0] = 1.f;
  EXPECT(burst_opt_finish(g, gr, in, p, sh, f).flags == 1);
  EXPECT(burst_opt_snr(10.0, 2, 1.0, 0.0) == 0.0);
}

}  // namespace

int main() {
  test_prepare();
  test_shifts();
  test_search_and_finish();
  if (g_failed) {
    std::cerr << g_failed << " check(s) failed" << std::endl;
    return 1;
  }
  std::cout << "burstopt host unit tests passed" << std::endl;
  return 0;
}
