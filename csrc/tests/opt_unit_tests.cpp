// Host unit tests of cubeopt's host steps (psoup/cubeopt.hpp): prepare on
// hand-made cubes, the shift tables, the host search's tie rule and a planted
// pulse, finish, and the refusals.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/burstcube.hpp"
#include "psoup/cubeopt.hpp"

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

CubeOptGeom geom(int nints, int nsub, int nbins, int nchans) {
  CubeOptGeom g;
  g.nints = nints;
  g.nsub = nsub;
  g.nbins = nbins;
  g.nchans = nchans;
  g.fold_nsamps = 1 << 16;
  g.tsamp = 320e-6;
  g.fch1 = 1510.0;
  g.foff = -1.09;
  return g;
}

CubeOptGrid small_grid(int ndm, int np, int npd) {
  CubeOptGrid gr;
  gr.ndm = ndm;
  gr.np = np;
  gr.npd = npd;
  return gr;
}

CubeOptInput flat_input(const CubeOptGeom& g, int32_t hit, int64_t level) {
  CubeOptInput in;
  in.period = 0.1;
  in.dm = 100.f;
  in.nactive.assign(static_cast<size_t>(g.nsub), 2);
  in.hits.assign(static_cast<size_t>(g.nints) * g.nbins, hit);
  in.sums.assign(static_cast<size_t>(g.nints) * g.nsub * g.nbins, level * hit);
  return in;
}

bool throws_with(const std::string& text, const CubeOptGeom& g, const CubeOptGrid& gr, const CubeOptInput& in) {
  try {
    cube_opt_prepare(3, g, gr, in);
  } catch (const std::exception& e) {
    return std::string(e.what()).find(text) != std::string::npos;
  }
  return false;
}

void test_prepare() {
  const CubeOptGeom g = geom(2, 2, 4, 4);
  const CubeOptGrid gr = small_grid(4, 3, 3);
  CubeOptInput in = flat_input(g, 10, 7);
  // unequal hits: bin 1 of subint 0 has 5 hits and half the sum; its rate is the same
  in.hits[1] = 5;
  in.sums[1] = 35;
  in.sums[4 + 1] = 35;
  // a pulse in subband 0, subint 1, bin 2
  in.sums[(1 * 2 + 0) * 4 + 2] += 40;
  in.nactive[1] = 0;  // subband 1 is dead: d == 0 there
  const CubeOptPrepared p = cube_opt_prepare(0, g, gr, in);
  // q = 70 everywhere but the pulse (110); B of that row = (3 * 70 + 110) // 4 = 80
  for (int b = 0; b < 4; ++b) EXPECT(p.d[static_cast<size_t>(b)] == 0);
  EXPECT(p.d[(1 * 2 + 0) * 4 + 2] == 30 && p.d[(1 * 2 + 0) * 4 + 0] == -10);
  for (int b = 0; b < 4; ++b) EXPECT(p.d[(0 * 2 + 1) * 4 + static_cast<size_t>(b)] == 0);
  EXPECT(p.mtot == 0 && p.v2 == 900 + 300 && p.v == 300.0);
  // refusals name the candidate
  CubeOptInput bad = in;
  bad.hits[3] = 0;
  EXPECT(throws_with("candidate 3 ", g, gr, bad));
  bad = in;
  bad.sums[0] = int64_t(1) << 61;
  EXPECT(throws_with("candidate 3 ", g, gr, bad));
  bad = in;
  bad.sums[0] = int64_t(1) << 40;  // d does not fit int32
  EXPECT(throws_with("candidate 3 ", g, gr, bad));
  bad = in;
  bad.period = 0;
  EXPECT(throws_with("candidate 3 ", g, gr, bad));
  const CubeOptGeom big = geom(65, 1, 256, 4);
  EXPECT(throws_with("candidate 3 ", big, gr, flat_input(big, 1, 1)));
}

void test_shifts() {
  const CubeOptGeom g = geom(4, 2, 16, 8);
  const CubeOptGrid gr = small_grid(4, 5, 3);
  std::vector<float> delays(8);
  for (int c = 0; c < 8; ++c) delays[static_cast<size_t>(c)] = 0.25f * c;
  const CubeOptShifts s = cube_opt_shifts(g, gr, 0.01, 100.f, delays);
  EXPECT(s.dms.size() == 4 && s.dms[0] == 0.f && s.dms[2] == 100.f && s.dms[3] == 150.f);
  for (int sub = 0; sub < 2; ++sub) EXPECT(s.sdm[2 * 2 + static_cast<size_t>(sub)] == 0);  // the candidate's own DM
  for (int32_t v : s.sdm) EXPECT(v >= 0 && v < 16);
  for (int32_t v : s.st) EXPECT(v >= 0 && v < 16);
  // the unshifted trial (kp, kpd) = (2, 1)
  for (int i = 0; i < 4; ++i) EXPECT(s.st[(2 * 3 + 1) * 4 + static_cast<size_t>(i)] == 0);
  // L = 2 bins, Q = 0: rint(2 (u - 0.5)) = rint(-0.75, -0.25, 0.25, 0.75) = -1, 0, 0, 1
  const int32_t* row = s.st.data() + (4 * 3 + 1) * 4;
  EXPECT(row[0] == 15 && row[1] == 0 && row[2] == 0 && row[3] == 1);
  // L = 0, Q = 1: rint(4 u (1 - u)) = rint(0.4375, 0.9375, 0.9375, 0.4375) = 0, 1, 1, 0
  row = s.st.data() + (2 * 3 + 2) * 4;
  EXPECT(row[0] == 0 && row[1] == 1 && row[2] == 1 && row[3] == 0);
  const std::vector<float> dms = burst_dms(30.f, 5, 10.f);
  EXPECT(dms[0] == 22.f && dms[2] == 30.f && dms[4] == 38.f);
}

void test_search_and_finish() {
  const CubeOptGeom g = geom(4, 2, 16, 8);
  const CubeOptGrid gr = small_grid(4, 5, 3);
  std::vector<float> delays(8);
  for (int c = 0; c < 8; ++c) delays[static_cast<size_t>(c)] = 0.9f * c;
  const CubeOptShifts s = cube_opt_shifts(g, gr, 0.01, 100.f, delays);
  const int nw = kern::opt_nwidths(16);
  EXPECT(nw == 4 && kern::opt_nwidths(2) == 1 && kern::opt_nwidths(50) == 5 && kern::opt_nwidths(256) == 8);
  // the tie rule: an all-equal cube gives index 0 for every width
  std::vector<int32_t> d(4 * 2 * 16, 3);
  CubeOptSearch f = cube_opt_search_host(g, gr, d, s);
  for (int k = 0; k < nw; ++k) {
    EXPECT(f.best_idx[static_cast<size_t>(k)] == 0);
    EXPECT(f.best_val[static_cast<size_t>(k)] == 3 * 8 * (1 << k));
    EXPECT(f.centre[static_cast<size_t>(k)] == 3 * 8 * (1 << k));
  }
  // a delta pulse placed along the tables of trial (kd, kp, kpd) = (3, 0, 2) lands at bin 5 of that trial
  const int kd = 3, kp = 0, kpd = 2, bin = 5;
  std::fill(d.begin(), d.end(), 0);
  for (int i = 0; i < 4; ++i)
    for (int sub = 0; sub < 2; ++sub) {
      const int b = (bin + s.st[(static_cast<size_t>(kp) * 3 + kpd) * 4 + i] + s.sdm[kd * 2 + sub]) % 16;
      d[(static_cast<size_t>(i) * 2 + sub) * 16 + b] += 100;
    }
  f = cube_opt_search_host(g, gr, d, s);
  EXPECT(f.best_val[0] == 800);
  EXPECT(f.best_idx[0] == ((kd * 5 + kp) * 3 + kpd) * 16 + bin);
  EXPECT(f.dmcurve[3] == 800 && f.ppd[kp * 3 + kpd] == 800);
  CubeOptPrepared p;
  p.d = d;
  p.mtot = 800;
  p.v2 = 80000;
  p.v = 5000.0;
  const CubeOptResult r = cube_opt_finish(g, gr, 0.01, 0.f, p, s, f);
  EXPECT(r.opt_width == 1 && r.opt_bin == 5 && r.opt_kd == 3 && r.opt_kp == 0 && r.opt_kpd == 2);
  EXPECT(r.opt_dm == 150.f && r.profile[5] == 800 && r.profile[4] == 0);
  EXPECT(r.snr > r.snr_in && r.snr > r.snr_dm0 && r.flags == 0);
  EXPECT(r.opt_period < 0.01 && r.opt_acc < 0);
  EXPECT(cube_opt_snr(10.0, 2, 0, 0.0, 16) == 0.0);
  EXPECT(std::fabs(cube_opt_snr(800.0, 1, 800, 5000.0, 16) - 750.0 / std::sqrt(5000.0 * 15.0 / 16.0)) < 1e-12);
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
  std::cout << "cubeopt host unit tests passed" << std::endl;
  return 0;
}
