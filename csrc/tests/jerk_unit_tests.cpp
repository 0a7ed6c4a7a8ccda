// Host unit tests of jerksearch's host steps (psoup/jerk.hpp): the jerk factor,
// the shift at exact halves, the stationary points and the monotone spans
// between them, the host gather (identity, fixed points, both clamps, the copy
// past n), JerkPlan (zero in the grid, single trial, the 4096 limit), every
// refusal by name, the jerk distillation on a hand-made list and the command
// line.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "psoup/jerk.hpp"

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

template <class F>
bool throws_with(F&& f, const std::string& what) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

std::vector<uint8_t> ramp(size_t n, unsigned seed) {
  std::vector<uint8_t> x(n);
  uint32_t z = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    z = z * 1664525u + 1013904223u;
    x[i] = static_cast<uint8_t>(z >> 24);
  }
  return x;
}

void test_factor_and_shift() {
  EXPECT(jerk_factor(0.f, 64e-6f) == 0.0);
  const float ts = 64e-6f;
  const double jf = jerk_factor(0.1f, ts);
  EXPECT(jf == ((static_cast<double>(0.1f) * ts) * ts) / 1798754748.0);
  // p(2) = 2 * (2 - 2048) * (2 - 4096) = 2^3 * 1023 * 2047: with jf = 2^-4 an exact half
  const double g2 = 2.0 * -2046.0 * -4094.0 / 16.0;
  EXPECT(g2 - std::floor(g2) == 0.5);
  EXPECT(jerk_shift(2, 4096, 0.0625) == static_cast<int64_t>(std::rint(g2)));
  EXPECT(jerk_shift(2, 4096, 0.0625) % 2 == 0);  // half to even
  EXPECT(jerk_shift(0, 4096, 0.0625) == 0 && jerk_shift(2048, 4096, 0.0625) == 0 &&
         jerk_shift(4096, 4096, 0.0625) == 0);
  EXPECT(jerk_shift(5, 4096, -0.0625) == -jerk_shift(5, 4096, 0.0625));
  EXPECT(jerk_freq_factor(0.f, 1 << 20, ts) == 1.0);
  const double T = 1048576.0 * static_cast<double>(ts);
  EXPECT(jerk_freq_factor(2.f, 1 << 20, ts) == 1.0 + ((2.0 * T) * T) / (12.0 * 299792458.0));
}

void test_stationary_and_monotone() {
  for (uint64_t n : {1ull, 2ull, 15ull, 16ull, 17ull, 4101ull, 65539ull, 1ull << 26}) {
    int64_t lo = 0, hi = 0;
    jerk_stationary(n, &lo, &hi);
    EXPECT(lo <= hi && lo >= 0 && hi <= static_cast<int64_t>(n));
    if (n >= 16) {
      const double a = n / 2.0 - n / (2.0 * std::sqrt(3.0)), b = n / 2.0 + n / (2.0 * std::sqrt(3.0));
      EXPECT(std::fabs(static_cast<double>(lo) - a) < 2.0 && std::fabs(static_cast<double>(hi) - b) < 2.0);
    }
  }
  // between the stationary points (a margin of a sample) the shift is monotone
  const uint64_t n = 65539;
  int64_t lo = 0, hi = 0;
  jerk_stationary(n, &lo, &hi);
  const double jf = 40.0 * 12.0 * std::sqrt(3.0) / (65539.0 * 65539.0 * 65539.0);
  bool up = true, down = true, up2 = true;
  for (int64_t i = 1; i < lo - 1; ++i) up = up && jerk_shift(i, n, jf) >= jerk_shift(i - 1, n, jf);
  for (int64_t i = lo + 3; i < hi - 1; ++i) down = down && jerk_shift(i, n, jf) <= jerk_shift(i - 1, n, jf);
  for (int64_t i = hi + 3; i < static_cast<int64_t>(n); ++i) up2 = up2 && jerk_shift(i, n, jf) >= jerk_shift(i - 1, n, jf);
  EXPECT(up && down && up2);
  int64_t mx = 0;
  for (uint64_t i = 0; i < n; ++i) mx = std::max<int64_t>(mx, std::llabs(jerk_shift(i, n, jf)));
  EXPECT(mx >= 39 && mx <= 41);
}

void test_gather() {
  const uint64_t nrow = 4101 + 37, n = 4101, stride = 4352;
  const std::vector<uint8_t> x = ramp(2 * stride, 7);
  // identity: jf = 0 and max|g| < 0.5
  const double small = 0.4 * 12.0 * std::sqrt(3.0) / (4101.0 * 4101.0 * 4101.0);
  std::vector<uint8_t> y(2 * 2 * stride, 0xEE);
  jerk_resample_host(x.data(), stride, 2, nrow, n, {0.0, small}, y.data(), stride);
  bool same = true;
  for (int r = 0; r < 2; ++r)
    for (int k = 0; k < 2; ++k)
      for (uint64_t i = 0; i < nrow; ++i) same = same && y[(r * 2 + k) * stride + i] == x[r * stride + i];
  EXPECT(same);
  EXPECT(y[nrow] == 0xEE);  // nothing past the row
  // a real shift: the definition per sample, the copy past n, the fixed points
  const double jf = 40.0 * 12.0 * std::sqrt(3.0) / (4101.0 * 4101.0 * 4101.0);
  jerk_resample_host(x.data(), stride, 2, nrow, n, {jf, -jf}, y.data(), stride);
  bool ok = true;
  for (uint64_t i = 0; i < nrow; ++i) {
    int64_t j = static_cast<int64_t>(i);
    if (i < n) j = std::min<int64_t>(std::max<int64_t>(j - jerk_shift(i, n, jf), 0), n - 1);
    ok = ok && y[(1 * 2 + 1) * stride + i] == x[stride + static_cast<uint64_t>(j)];
  }
  EXPECT(ok);
  EXPECT(y[0] == x[0] && y[n / 2] == x[n / 2] && y[n - 1] == x[n - 1]);
  // both clamps: jf = 2^-4 at n = 4096 sends most indices outside
  const std::vector<uint8_t> x2 = ramp(4096, 9);
  std::vector<uint8_t> y2(4096);
  jerk_resample_host(x2.data(), 4096, 1, 4096, 4096, {0.0625}, y2.data(), 4096);
  EXPECT(y2[1000] == x2[4095] && y2[3000] == x2[0] && y2[0] == x2[0] && y2[2048] == x2[2048]);
  EXPECT(throws_with([&] { jerk_resample_host(x2.data(), 4096, 1, 4096, 5000, {0.0}, y2.data(), 4096); }, "span"));
  EXPECT(throws_with([&] { jerk_resample_host(x2.data(), 100, 1, 4096, 4096, {0.0}, y2.data(), 4096); }, "stride"));
}

void test_checks() {
  EXPECT(throws_with([] { jerk_check((1ull << 26) + 1, {0.0}); }, "longer than 2^26"));
  jerk_check(1ull << 26, {0.0});
  const double N = 1048576.0;
  jerk_check(1 << 20, {1.79 / (N * N), -1.79 / (N * N)});
  EXPECT(throws_with([&] { jerk_check(1 << 20, {1.81 / (N * N)}); }, "0.9 samples per sample"));
  EXPECT(throws_with([&] { jerk_check(1 << 20, {-1.81 / (N * N)}); }, "0.9 samples per sample"));
  EXPECT(throws_with([] { jerk_check(1024, {std::numeric_limits<double>::infinity()}); }, "non-finite"));
  EXPECT(throws_with([] { jerk_check(1024, {std::nan("")}); }, "non-finite"));
}

void test_plan() {
  const float ts = 64e-6f;
  const uint64_t n = 1ull << 23;
  JerkPlan p(-1.f, 1.f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f);
  const double T = static_cast<double>(n) * static_cast<double>(ts);
  const double w = p.width(30.f);
  EXPECT(w >= 63.9e-6 && w < 1e-3);  // 64 us pulse width, a negligible DM term
  const double st = ((2.0 * w) * std::sqrt(static_cast<double>(1.1f) * 1.1f - 1.0)) *
                    ((72.0 * std::sqrt(3.0)) * 299792458.0) / ((T * T) * T);
  EXPECT(p.step(30.f) == st);
  const std::vector<float> l = p.generate(30.f);
  EXPECT(l.size() % 2 == 1 && l[l.size() / 2] == 0.f);
  EXPECT(l.front() >= -1.f && l.back() <= 1.f && l.front() - st < -1.0 && l.back() + st > 1.0);
  bool grid = true;
  for (size_t i = 1; i < l.size(); ++i) grid = grid && std::fabs((l[i] - l[i - 1]) - st) < 1e-6 * st + 1e-7;
  EXPECT(grid);
  // a range that does not bracket 0 holds no 0
  bool zero = false;
  for (float j : JerkPlan(0.3f, 1.f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f)) zero = zero || j == 0.f;
  EXPECT(!zero);
  // a given step; the grid holds its multiples exactly
  const std::vector<float> g = JerkPlan(0.f, 1.25f, 1.1f, 0.25f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f);
  EXPECT(g.size() == 6 && g[0] == 0.f && g[4] == 1.f && g[5] == 1.25f);
  // start == end: that value alone
  const std::vector<float> one = JerkPlan(0.7f, 0.7f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f).generate(10.f);
  EXPECT(one.size() == 1 && one[0] == 0.7f);
  EXPECT(JerkPlan(0.f, 0.f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f).generate(10.f) == std::vector<float>{0.f});
  // the limits
  EXPECT(JerkPlan(0.f, 4095.f, 1.1f, 1.f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f).size() == 4096);
  EXPECT(throws_with([&] { JerkPlan(0.f, 4096.f, 1.1f, 1.f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f); },
                     "more than 4096 jerk trials"));
  EXPECT(throws_with([&] { JerkPlan(-1e30f, 1e30f, 1.1f, 1e-30f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f); },
                     "more than 4096 jerk trials"));
  EXPECT(throws_with([&] { JerkPlan(0.1f, 0.2f, 1.1f, 1.f, 64.f, n, ts, 1400.f, -0.5f).generate(0.f); }, "no trial"));
  EXPECT(throws_with([&] { JerkPlan(1.f, -1.f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f); }, "jerk_start > jerk_end"));
  EXPECT(throws_with([&] { JerkPlan(0.f, std::numeric_limits<float>::infinity(), 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f); },
                     "non-finite"));
  EXPECT(throws_with([&] { JerkPlan(std::nanf(""), 1.f, 1.1f, 0.f, 64.f, n, ts, 1400.f, -0.5f); }, "non-finite"));
}

JerkCandidate jc(float freq, float acc, float snr, float jerk, int nh = 0) {
  return JerkCandidate{Candidate(10.f, 3, acc, nh, snr, freq), jerk};
}

void test_distill() {
  const float tobs = 536.870912f, tol = 1e-4f;
  const double T = 536.870912;
  const double jw = T * T / (12.0 * 299792458.0);  // 8.0e-5 per m/s^3
  // 0 and 1 differ only in jerk; 2 is outside the plain tolerance of 0 but inside the one widened by its jerk
  // difference; 3 lies equally far off at the same jerk and survives; 4 and 5 are a pair outside the widened
  // tolerance; 6 is related through the acceleration sweep.
  JerkCandidateList in = {
      jc(100.f, 0.f, 50.f, 0.f),   jc(100.f, 0.f, 40.f, 1.f),
      jc(100.02f, 0.f, 30.f, 4.f),  // |df| = 0.02 < 100 (1e-4 + 4 jw) = 0.042
      jc(100.02f, 0.f, 29.f, 0.f),  // 0.02 > 0.01
      jc(200.f, 0.f, 20.f, 0.f),   jc(200.1f, 0.f, 19.f, 2.f),  // 0.1 > 200 (1e-4 + 2 jw) = 0.052
      jc(100.f - 100.f * 5.f * tobs / 299792458.f * 0.5f, 5.f, 10.f, 0.f),
  };
  EXPECT(100.0 * (1e-4 + 4 * jw) > 0.02 && 200.0 * (1e-4 + 2 * jw) < 0.1);
  JerkCandidateList out = jerk_distill(in, tobs, T, tol, true);
  EXPECT(out.size() == 4);
  if (out.size() == 4) {
    EXPECT(out[0].cand.snr == 50.f && out[0].jerk == 0.f && out[0].cand.assoc.size() == 3);
    EXPECT(out[1].cand.snr == 29.f && out[1].cand.assoc.empty());
    EXPECT(out[2].cand.snr == 20.f && out[3].cand.snr == 19.f && out[3].jerk == 2.f);
  }
  EXPECT(jerk_distill(in, tobs, T, tol, false)[0].cand.assoc.empty());
  // one jerk trial: the relation is AccelerationDistiller's, so its survivors pass unchanged and in order
  JerkCandidateList single = {jc(100.f, 0.f, 50.f, 0.5f), jc(100.02f, 0.f, 29.f, 0.5f), jc(200.f, 0.f, 29.f, 0.5f, 1),
                              jc(300.f, 2.f, 12.f, 0.5f)};
  out = jerk_distill(single, tobs, T, tol, true);
  EXPECT(out.size() == 4 && out[1].cand.freq == 100.02f && out[2].cand.nh == 1 && out[3].cand.acc == 2.f);
  EXPECT(jerk_distill({}, tobs, T, tol, true).empty());
}

void test_cli() {
  JerkCmdLineOptions a;
  EXPECT(parse_jerk_cmdline(a, {"jerksearch", "-i", "x.fil"}));
  EXPECT(a.jerk_start == 0.f && a.jerk_end == 0.f && a.jerk_tol == 1.1f && a.jerk_step == 0.f);
  EXPECT(a.search.dm_end == 100.f && a.search.acc_tol == 1.1f && a.search.nharmonics == 4 && a.search.min_snr == 9.f &&
         a.search.limit == 1000 && a.search.npdmp == 0 && a.search.size == 0);
  EXPECT(a.outfilename.find("_jerksearch.output") != std::string::npos);
  JerkCmdLineOptions b;
  EXPECT(parse_jerk_cmdline(b, {"jerksearch", "-i", "x.fil", "-o", "out.txt", "--jerk_start", "-2.5", "--jerk_end=3",
                                "--jerk_tol", "1.2", "--jerk_step", "0.5", "--acc_start", "-5", "--acc_end", "5", "-n",
                                "3", "-m", "7", "--fft_size", "65536", "--npdmp", "4", "--dm_start", "1", "-v"}));
  EXPECT(b.outfilename == "out.txt" && b.jerk_start == -2.5f && b.jerk_end == 3.f && b.jerk_tol == 1.2f &&
         b.jerk_step == 0.5f && b.search.acc_start == -5.f && b.search.nharmonics == 3 && b.search.min_snr == 7.f &&
         b.search.size == 65536u && b.search.npdmp == 4 && b.search.dm_start == 1.f && b.search.verbose);
  JerkCmdLineOptions c;
  EXPECT(parse_jerk_cmdline(c, {"jerksearch", "-i", "x.fil", "--jerk_end", "inf"}) && std::isinf(c.jerk_end));
  JerkCmdLineOptions d;
  EXPECT(!parse_jerk_cmdline(d, {"jerksearch", "-i", "x.fil", "--jerk_end", "1x"}));
  EXPECT(!parse_jerk_cmdline(d, {"jerksearch", "-i", "x.fil", "-t", "2"}));
  EXPECT(!parse_jerk_cmdline(d, {"jerksearch", "-i", "x.fil", "--checkpoint_dir", "ck"}));
  EXPECT(!parse_jerk_cmdline(d, {"jerksearch"}));
}

}  // namespace

int main(int, char**) {
  test_factor_and_shift();
  test_stationary_and_monotone();
  test_gather();
  test_checks();
  test_plan();
  test_distill();
  test_cli();
  std::cout << (g_failed == 0 ? "all jerk unit tests passed; " : "") << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
