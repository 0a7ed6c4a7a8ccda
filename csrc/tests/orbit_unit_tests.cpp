// Host unit tests of orbsearch's host steps (psoup/orbit.hpp): the sine table
// and its symmetries, the quantisation at its edges, the interpolated sine and
// its monotone half turns, the shift and the rule the kernel's wide-load path
// rests on, the host gather (identity, both clamps, the copy past n), every
// refusal by name, the bank parser, the grid, the orbit distillation on a
// hand-made list and the command line.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "psoup/orbit.hpp"

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

void test_table_and_sine() {
  const std::vector<int32_t> t = orbit_sine_table();
  EXPECT(t.size() == 4097);
  EXPECT(t[0] == 0 && t[2048] == 0 && t[4096] == 0 && t[1024] == (1 << 30) && t[3072] == -(1 << 30));
  EXPECT(t[512] == static_cast<int32_t>(std::rint(std::ldexp(std::sqrt(0.5), 30))));
  bool sym = true, mono = true;
  for (int j = 0; j <= 2048; ++j) sym = sym && t[2048 - j] == t[j] && t[2048 + j] == -t[j];
  for (int j = 0; j < 1024; ++j) mono = mono && t[j] < t[j + 1];
  for (int j = 1024; j < 3072; ++j) mono = mono && t[j] > t[j + 1];
  for (int j = 3072; j < 4096; ++j) mono = mono && t[j] < t[j + 1];
  EXPECT(sym && mono);
  // S at the table's own points, at a half step, and the arithmetic shift of a negative slope
  EXPECT(orbit_sine(t.data(), 0) == 0 && orbit_sine(t.data(), 1ull << 62) == (1 << 30));
  EXPECT(orbit_sine(t.data(), 3ull << 62) == -(1 << 30));
  EXPECT(orbit_sine(t.data(), ~0ull) <= 0 && orbit_sine(t.data(), ~0ull) >= t[4095]);
  const int64_t d = static_cast<int64_t>(t[1501]) - t[1500];
  EXPECT(d < 0);
  const int64_t half = orbit_sine(t.data(), (1500ull << 52) | (1ull << 51));
  EXPECT(half == t[1500] + static_cast<int64_t>(std::floor((static_cast<double>(d) * 524288.0 + 524288.0) / 1048576.0)));
  // monotone on each half turn, sampled finely across table steps
  bool up = true, down = true;
  int64_t prev = orbit_sine(t.data(), 3ull << 62);
  for (uint64_t th = (3ull << 62) + (1ull << 40), k = 0; k < (1u << 21); ++k, th += (1ull << 42) + 12345) {
    const int64_t s = orbit_sine(t.data(), th);  // wraps through 0 up to 2^62
    if ((th + (1ull << 62)) >> 63) break;
    up = up && s >= prev;
    prev = s;
  }
  prev = orbit_sine(t.data(), 1ull << 62);
  for (uint64_t th = (1ull << 62) + (1ull << 40); th < (3ull << 62); th += (1ull << 42) + 12345) {
    const int64_t s = orbit_sine(t.data(), th);
    down = down && s <= prev;
    prev = s;
  }
  EXPECT(up && down);
}

void test_quantise() {
  const float ts = 64e-6f;
  const double tsd = ts;
  OrbitQuant q = orbit_quantise(64.0 * tsd, 0.0, 0.0, ts);
  EXPECT(q.W == (1ull << 58) && q.F == 0 && q.Aq == 0);
  q = orbit_quantise(3600.0, 1.5, 0.25, ts);
  EXPECT(q.W == static_cast<uint64_t>(std::rint(std::ldexp(tsd / 3600.0, 64))));
  EXPECT(q.F == (1ull << 62));
  EXPECT(q.Aq == static_cast<int64_t>(std::rint((1.5 / tsd) * 256.0)));
  EXPECT(orbit_quantise(3600.0, 0.0, 0.75, ts).F == (3ull << 62));
  EXPECT(orbit_quantise(3600.0, 0.0, -0.25, ts).F == (3ull << 62));
  EXPECT(orbit_quantise(3600.0, 0.0, -1e-20, ts).F == 0);  // r rounds to 1: taken as 0
  EXPECT(orbit_quantise(3600.0, 0.0, 1.0 - std::ldexp(1.0, -53), ts).F == ~0ull - 2047);
  EXPECT(orbit_quantise(3600.0, 0.0, 7.5, ts).F == (1ull << 63));
  // Aq = 2^30 - 1 is the last one accepted
  const double a_last = (1073741823.0 / 256.0) * tsd;
  EXPECT(orbit_quantise(1e9, a_last, 0.0, ts).Aq == 1073741823);
  EXPECT(throws_with([&] { orbit_quantise(1e9, (1073741824.0 / 256.0) * tsd, 0.0, ts); }, "Aq >= 2^30"));
  EXPECT(throws_with([&] { orbit_quantise(63.9 * tsd, 0.0, 0.0, ts); }, "pb < 64 tsamp"));
  EXPECT(throws_with([&] { orbit_quantise(-5.0, 0.0, 0.0, ts); }, "pb < 64 tsamp"));
  EXPECT(throws_with([&] { orbit_quantise(3600.0, -1e-9, 0.0, ts); }, "a1 < 0"));
  const double inf = std::numeric_limits<double>::infinity();
  EXPECT(throws_with([&] { orbit_quantise(inf, 0.0, 0.0, ts); }, "non-finite"));
  EXPECT(throws_with([&] { orbit_quantise(3600.0, std::nan(""), 0.0, ts); }, "non-finite"));
  EXPECT(throws_with([&] { orbit_quantise(3600.0, 1.0, -inf, ts); }, "non-finite"));
  EXPECT(throws_with([] { orbit_check_quant(OrbitQuant{(1ull << 58) + 1, 0, 0}); }, "pb < 64 tsamp"));
  EXPECT(throws_with([] { orbit_check_quant(OrbitQuant{1, 0, -1}); }, "a1 < 0"));
  EXPECT(throws_with([] { orbit_check_quant(OrbitQuant{1, 0, int64_t{1} << 30}); }, "Aq >= 2^30"));
}

void test_shift_and_lane_rule() {
  const std::vector<int32_t> t = orbit_sine_table();
  const float ts = 320e-6f;
  // amplitude 40 samples, an orbit of 30000 samples, starting at phase 0.37
  const OrbitQuant q = orbit_quantise(30000.0 * static_cast<double>(ts), 40.0 * static_cast<double>(ts), 0.37, ts);
  EXPECT(orbit_shift(t.data(), q, 0) == 0);
  int64_t mn = 0, mx = 0;
  for (uint64_t i = 0; i < 65536; ++i) {
    const int64_t s = orbit_shift(t.data(), q, i);
    mn = std::min(mn, s);
    mx = std::max(mx, s);
    const double want = 40.0 * (std::sin(2.0 * M_PI * (static_cast<double>(i) / 30000.0 + 0.37)) -
                                std::sin(2.0 * M_PI * 0.37));
    if (std::fabs(static_cast<double>(s) - want) > 0.51) ++g_failed;
  }
  EXPECT(mx - mn == 80 || mx - mn == 79 || mx - mn == 81);
  // the kernel's rule: on a 16-sample span with no turning point inside (the top bit of th + 2^62 agrees at its
  // ends), equal end shifts mean one shift throughout; spans with a turning point exist and do break it
  bool rule = true;
  int turning = 0;
  for (const OrbitQuant& u : {q, orbit_quantise(64.0 * static_cast<double>(ts), 1000.0 * static_cast<double>(ts), 0.25, ts),
                              orbit_quantise(5000.0 * static_cast<double>(ts), 1000.0 * static_cast<double>(ts), 0.0, ts)})
    for (uint64_t i0 = 0; i0 < 65536; i0 += 16) {
      const uint64_t th0 = u.F + i0 * u.W, th1 = th0 + 15 * u.W;
      if (((th0 + (1ull << 62)) ^ (th1 + (1ull << 62))) >> 63) {
        ++turning;
        continue;
      }
      const int64_t s0 = orbit_shift(t.data(), u, i0);
      if (s0 != orbit_shift(t.data(), u, i0 + 15)) continue;
      for (uint64_t j = 1; j < 15; ++j) rule = rule && orbit_shift(t.data(), u, i0 + j) == s0;
    }
  EXPECT(rule && turning > 4);
}

void test_gather() {
  const uint64_t nrow = 4101 + 37, n = 4101, stride = 4352;
  const float ts = 320e-6f;
  const double tsd = ts;
  const std::vector<uint8_t> x = ramp(2 * stride, 7);
  const std::vector<int32_t> t = orbit_sine_table();
  // identity: a1 = 0, and an amplitude of 0.2 samples (|s| stays below a half)
  std::vector<uint8_t> y(2 * 2 * stride, 0xEE);
  orbit_resample_host(x.data(), stride, 2, nrow, n, {orbit_quantise(100.0, 0.0, 0.3, ts),
                                                     orbit_quantise(1.0, 0.2 * tsd, 0.3, ts)}, y.data(), stride);
  bool same = true;
  for (int r = 0; r < 2; ++r)
    for (int k = 0; k < 2; ++k)
      for (uint64_t i = 0; i < nrow; ++i) same = same && y[(r * 2 + k) * stride + i] == x[r * stride + i];
  EXPECT(same);
  EXPECT(y[nrow] == 0xEE);  // nothing past the row
  // a real shift: the definition per sample and the copy past n
  const OrbitQuant q = orbit_quantise(1367.0 * tsd, 40.0 * tsd, 0.37, ts);
  orbit_resample_host(x.data(), stride, 2, nrow, n, {q}, y.data(), stride);
  bool ok = true;
  for (uint64_t i = 0; i < nrow; ++i) {
    int64_t j = static_cast<int64_t>(i);
    if (i < n) j = std::min<int64_t>(std::max<int64_t>(j + orbit_shift(t.data(), q, i), 0), n - 1);
    ok = ok && y[stride + i] == x[stride + static_cast<uint64_t>(j)];
  }
  EXPECT(ok && y[0] == x[0]);
  // both clamps: an amplitude of 10 n
  const OrbitQuant big = orbit_quantise(4101.0 * tsd, 41010.0 * tsd, 0.0, ts);
  orbit_resample_host(x.data(), stride, 1, nrow, n, {big}, y.data(), stride);
  EXPECT(y[1000] == x[n - 1] && y[3000] == x[0] && y[0] == x[0]);
  EXPECT(throws_with([&] { orbit_resample_host(x.data(), stride, 1, 4096, 5000, {q}, y.data(), stride); }, "span"));
  EXPECT(throws_with([&] { orbit_resample_host(x.data(), 100, 1, 4096, 4096, {q}, y.data(), stride); }, "stride"));
  EXPECT(throws_with([&] { orbit_resample_host(x.data(), stride, 1, 4096, 4096, {}, y.data(), stride); }, "no templates"));
}

void test_checks() {
  const float ts = 64e-6f;
  const std::vector<OrbitTemplate> one = {{3600.0, 1.0, 0.0}};
  orbit_check(1ull << 26, one, ts);
  EXPECT(throws_with([&] { orbit_check((1ull << 26) + 1, one, ts); }, "longer than 2^26"));
  EXPECT(throws_with([&] { orbit_check(1024, {}, ts); }, "empty bank"));
  EXPECT(throws_with([&] { orbit_check(1024, std::vector<OrbitTemplate>((1u << 20) + 1, one[0]), ts); },
                     "more than 2^20 templates"));
  orbit_check(1024, std::vector<OrbitTemplate>(1u << 10, one[0]), ts);
  // 2 pi a1 / pb: 0.89 passes, 0.91 is refused
  orbit_check(1024, {{100.0, 0.89 * 100.0 / (2.0 * M_PI), 0.0}}, ts);
  EXPECT(throws_with([&] { orbit_check(1024, {{100.0, 0.91 * 100.0 / (2.0 * M_PI), 0.0}}, ts); },
                     "0.9 samples per sample"));
  EXPECT(throws_with([&] { orbit_check(1024, {one[0], {1e-3, 0.0, 0.0}}, ts); }, "pb < 64 tsamp"));
  EXPECT(throws_with([&] { orbit_check(1024, {{3600.0, -1.0, 0.0}}, ts); }, "a1 < 0"));
  EXPECT(throws_with([&] { orbit_check(1024, {{3600.0, 1.0, std::nan("")}}, ts); }, "non-finite"));
  EXPECT(throws_with([&] { orbit_check(1024, {{1e12, 1e9, 0.0}}, ts); }, "Aq >= 2^30"));
  EXPECT(orbit_beta({100.0, 2.0, 0.3}) == ((2.0 * M_PI) * 2.0) / 100.0);
}

void test_bank_and_grid() {
  const std::vector<OrbitTemplate> b = orbit_parse_bank(
      "# pb a1 phase\n3600 1.5 0.25\n\n  7200.5\t0 0.5 extra columns # and a comment\n   # only a comment\n1e3 2e-3 -0.125");
  EXPECT(b.size() == 3);
  if (b.size() == 3) {
    EXPECT((b[0] == OrbitTemplate{3600.0, 1.5, 0.25}));
    EXPECT((b[1] == OrbitTemplate{7200.5, 0.0, 0.5}));
    EXPECT((b[2] == OrbitTemplate{1000.0, 0.002, -0.125}));
  }
  EXPECT(orbit_parse_bank("# nothing\n\n").empty());
  EXPECT(throws_with([] { orbit_parse_bank("3600 1 0\n3600 1\n"); }, "bank line 2 is malformed"));
  EXPECT(throws_with([] { orbit_parse_bank("3600 1 0\n\n# c\n3600 x 0\n"); }, "bank line 4 is malformed"));
  EXPECT(throws_with([] { orbit_parse_bank("3600 1.0.0 0"); }, "bank line 1 is malformed"));
  EXPECT(orbit_parse_bank("inf 1 nan").size() == 1);  // parsed; refused by name in orbit_check

  const std::vector<OrbitTemplate> g = orbit_grid(100.0, 400.0, 3, 0.0, 0.3, 4, 4);
  EXPECT(g.size() == 48);
  if (g.size() == 48) {
    EXPECT((g[0] == OrbitTemplate{100.0, 0.0, 0.0}) && (g[1] == OrbitTemplate{100.0, 0.0, 0.25}));
    EXPECT(g[4].a1 == 0.0 + 0.3 * (1.0 / 3.0) && g[4].ph == 0.0 && g[12].a1 == 0.3);
    EXPECT(g[16].pb == 100.0 * std::pow(4.0, 0.5) && g[32].pb == 400.0 && g[47].ph == 0.75);
  }
  EXPECT(orbit_grid(50.0, 60.0, 1, 0.1, 0.2, 1, 1) == (std::vector<OrbitTemplate>{{50.0, 0.1, 0.0}}));
  EXPECT(throws_with([] { orbit_grid(1.0, 2.0, 0, 0.0, 1.0, 1, 1); }, "at least 1"));
  EXPECT(throws_with([] { orbit_grid(1.0, 2.0, 1025, 0.0, 1.0, 1024, 1); }, "more than 2^20 templates"));
  EXPECT(orbit_grid(1.0, 2.0, 1024, 0.0, 1.0, 1024, 1).size() == (1u << 20));
}

OrbitCandidate oc(float freq, float snr, uint32_t tmpl, int nh = 0) {
  return OrbitCandidate{Candidate(10.f, 3, 0.f, nh, snr, freq), tmpl};
}

void test_distill() {
  const float tol = 1e-4f;
  const std::vector<double> beta = {0.0, 1e-3, 5e-3};
  // 0: the strongest, template 0.  1: the same template, close by: kept (another template is needed).  2: template
  // 1 inside tol + 0 + 1e-3 of 0 and of 1: absorbed by 0 and, still tested, appended to 1 as well.  3: template 1
  // outside it: kept; it absorbs 4 (template 2, inside tol + 1e-3 + 5e-3 of 3, outside tol + 0 + 5e-3 of 0 and 1).
  // 5: equal S/N to 3, far away.
  OrbitCandidateList in = {oc(100.f, 50.f, 0), oc(100.005f, 45.f, 0), oc(100.1f, 40.f, 1), oc(100.2f, 30.f, 1, 1),
                           oc(100.7f, 20.f, 2), oc(300.f, 30.f, 2, 2)};
  OrbitCandidateList out = orbit_distill(in, beta, tol, true);
  EXPECT(out.size() == 4);
  if (out.size() == 4) {
    EXPECT(out[0].cand.snr == 50.f && out[0].tmpl == 0 && out[0].cand.assoc.size() == 1);
    EXPECT(out[1].cand.snr == 45.f && out[1].cand.assoc.size() == 1);
    EXPECT(out[2].cand.nh == 1 && out[2].cand.assoc.size() == 1 && out[2].cand.assoc[0].snr == 20.f);
    EXPECT(out[3].cand.nh == 2 && out[3].tmpl == 2);
  }
  EXPECT(orbit_distill(in, beta, tol, false)[0].cand.assoc.empty());
  // one template: nothing is absorbed, the order is the stable S/N sort
  OrbitCandidateList single = {oc(100.f, 29.f, 1), oc(100.f, 50.f, 1), oc(100.001f, 29.f, 1, 1)};
  out = orbit_distill(single, beta, tol, true);
  EXPECT(out.size() == 3 && out[0].cand.snr == 50.f && out[1].cand.nh == 0 && out[2].cand.nh == 1);
  EXPECT(orbit_distill({}, beta, tol, true).empty());
  EXPECT(throws_with([&] { orbit_distill({oc(1.f, 1.f, 3)}, beta, tol, true); }, "outside the bank"));
}

void test_cli() {
  OrbitCmdLineOptions a;
  EXPECT(parse_orbit_cmdline(a, {"orbsearch", "-i", "x.fil"}));
  EXPECT(a.bankfile.empty() && a.npb == 0 && a.na1 == 0 && a.nphase == 0 && a.pb_start == 0.0);
  EXPECT(a.search.dm_end == 100.f && a.search.acc_tol == 1.1f && a.search.nharmonics == 4 && a.search.min_snr == 9.f &&
         a.search.limit == 1000 && a.search.npdmp == 0 && a.search.size == 0);
  EXPECT(a.outfilename.find("_orbsearch.output") != std::string::npos);
  EXPECT(throws_with([&] { orbit_bank_of(a); }, "exactly one source"));
  OrbitCmdLineOptions b;
  EXPECT(parse_orbit_cmdline(b, {"orbsearch", "-i", "x.fil", "-o", "out.txt", "--pb_start", "3600", "--pb_end=7200",
                                 "--npb", "3", "--a1_start", "0.5", "--a1_end", "1.5", "--na1", "2", "--nphase", "4",
                                 "--acc_start", "-5", "--acc_end", "5", "-n", "3", "-m", "7", "--fft_size", "65536",
                                 "--npdmp", "4", "--dm_start", "1", "-v"}));
  EXPECT(b.outfilename == "out.txt" && b.pb_start == 3600.0 && b.pb_end == 7200.0 && b.npb == 3 && b.a1_start == 0.5 &&
         b.a1_end == 1.5 && b.na1 == 2 && b.nphase == 4 && b.search.acc_start == -5.f && b.search.nharmonics == 3 &&
         b.search.size == 65536u && b.search.npdmp == 4 && b.search.verbose);
  EXPECT(orbit_bank_of(b).size() == 24);
  b.bankfile = "bank.txt";
  EXPECT(throws_with([&] { orbit_bank_of(b); }, "exactly one source"));
  OrbitCmdLineOptions c;
  EXPECT(parse_orbit_cmdline(c, {"orbsearch", "-i", "x.fil", "--pb_end", "inf", "--bankfile", "/nonexistent/bank"}) &&
         std::isinf(c.pb_end));
  EXPECT(throws_with([&] { orbit_bank_of(c); }, "cannot open the bank file"));
  OrbitCmdLineOptions d;
  EXPECT(!parse_orbit_cmdline(d, {"orbsearch", "-i", "x.fil", "--pb_end", "1x"}));
  EXPECT(!parse_orbit_cmdline(d, {"orbsearch", "-i", "x.fil", "-t", "2"}));
  EXPECT(!parse_orbit_cmdline(d, {"orbsearch", "-i", "x.fil", "--checkpoint_dir", "ck"}));
  EXPECT(!parse_orbit_cmdline(d, {"orbsearch"}));
}

}  // namespace

int main(int, char**) {
  test_table_and_sine();
  test_quantise();
  test_shift_and_lane_rule();
  test_gather();
  test_checks();
  test_bank_and_grid();
  test_distill();
  test_cli();
  std::cout << (g_failed == 0 ? "all orbit unit tests passed; " : "") << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
