// Host unit tests of filinject's host steps (psoup/inject.hpp): the injection
// file's parser with its defaults and refusals, the geometry checks, the hash
// on hand-computed values, the profile table, sigma from hand-made block sums
// (full blocks, a short file, zero variance), the tables (delays, widths,
// amplitudes, the A_q limit, killed and dead channels) and the truth numbers.
// No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/inject.hpp"
#include "psoup/plan.hpp"

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

InjectGeometry geom(int nchans = 8, uint64_t nsamps = 10000) {
  InjectGeometry g;
  g.nchans = nchans;
  g.nbits = 8;
  g.nsamps = nsamps;
  g.tsamp = 256e-6;
  g.fch1 = 1500.0;
  g.foff = -2.0;
  return g;
}

void test_parser() {
  const std::vector<InjectSignal> s = inject_parse(
      "# a comment\n"
      "\n"
      "pulsar 0.05 30 0.3   # defaults\n"
      "pulsar 0.1 10 1 0.1 150 0.25 -1.5\n"
      "burst 1.5 100 5\n"
      "  burst 2.5 50 3 0.002 2\n");
  EXPECT(s.size() == 4);
  EXPECT(s[0].kind == InjectKind::Pulsar && s[0].t == 0.05 && s[0].dm == 30 && s[0].amp == 0.3 && s[0].width == 0.05 &&
         s[0].acc == 0 && s[0].phase == 0 && s[0].alpha == 0);
  EXPECT(s[1].width == 0.1 && s[1].acc == 150 && s[1].phase == 0.25 && s[1].alpha == -1.5);
  EXPECT(s[2].kind == InjectKind::Burst && s[2].t == 1.5 && s[2].dm == 100 && s[2].amp == 5 && s[2].width == 0.005 &&
         s[2].alpha == 0);
  EXPECT(s[3].width == 0.002 && s[3].alpha == 2);
  EXPECT(throws_with([] { inject_parse("# nothing\n"); }, "no signal"));
  EXPECT(throws_with([] { inject_parse("quasar 1 2 3\n"); }, "unknown kind"));
  EXPECT(throws_with([] { inject_parse("pulsar 1 2\n"); }, "needs at least"));
  EXPECT(throws_with([] { inject_parse("burst 1 2 3 4 5 6\n"); }, "too many columns"));
  EXPECT(throws_with([] { inject_parse("pulsar 1 2 3x\n"); }, "cannot read column 3"));
  EXPECT(throws_with([] { inject_parse("pulsar 1 2 -3\n"); }, "amp must not be negative"));
  EXPECT(throws_with([] { inject_parse("pulsar 0 2 3\n"); }, "period must be positive"));
  EXPECT(throws_with([] { inject_parse("pulsar 1 2 3 0\n"); }, "duty must be positive"));
  EXPECT(throws_with([] { inject_parse("pulsar 1 2 3 1.5\n"); }, "duty must not exceed 1"));
  EXPECT(throws_with([] { inject_parse("burst 1 2 3 0\n"); }, "width must be positive"));
  EXPECT(throws_with([] { inject_parse("burst 1 -2 3\n"); }, "dm must not be negative"));
  EXPECT(throws_with([] { inject_parse("burst 1 2 inf\n"); }, "not finite"));
  std::string many;
  for (int i = 0; i < 65; ++i) many += "burst 1 2 3\n";
  EXPECT(throws_with([&] { inject_parse(many); }, "more than 64 signals"));
  EXPECT(throws_with([] { inject_read_file("/nonexistent/x.inj"); }, "cannot open the injection file"));
}

void test_geometry() {
  inject_check_geometry(geom());
  InjectGeometry g = geom();
  g.nbits = 16;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "nbits must be 1, 2, 4 or 8"));
  g = geom();
  g.nbits = 2;
  g.nchans = 3;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "multiple of 8"));
  g = geom();
  g.nsamps = 0;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "shorter than one sample"));
  g = geom();
  g.foff = 0;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "foff must not be zero"));
  g = geom();
  g.fch1 = 10;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "frequency must be positive"));
  g = geom();
  g.tsamp = 0;
  EXPECT(throws_with([&] { inject_check_geometry(g); }, "tsamp must be positive"));
}

void test_hash_and_table() {
  // splitmix64 of the states 1, 2 and 3 times the golden constant (seed 0, 1 and 2 at c = t = 0)
  EXPECT(inject_hash(0, 0, 0) == 0xE220A8397B1DCDAFull);
  EXPECT(inject_hash(1, 0, 0) == 0x6E789E6AA1B965F4ull);
  EXPECT(inject_hash(2, 0, 0) == 0x06C45D188009454Full);
  EXPECT(inject_hash(0, 3, 5) == inject_mix(kInjectGolden + ((3ull << 40) | 5ull)));
  const std::vector<uint16_t> T = inject_profile_table();
  EXPECT(T.size() == 1537 && T[0] == 32768 && T[256] == 19875 && T[1536] == 0);
  for (size_t k = 1; k < T.size(); ++k) EXPECT(T[k] <= T[k - 1]);
}

void test_sigma() {
  // two channels, 3 full blocks and a short one: variances 4, 9, 16 -> median 9; channel 1 constant
  const uint64_t n = 4096, nsamps = 3 * n + 100;
  std::vector<uint64_t> S1(8), S2(8);
  const uint64_t d[3] = {2, 3, 4};
  for (int b = 0; b < 3; ++b) {  // n values alternating 100 - d, 100 + d
    S1[b] = n * 100;
    S2[b] = n / 2 * ((100 - d[b]) * (100 - d[b]) + (100 + d[b]) * (100 + d[b]));
    S1[4 + b] = n * 7;
    S2[4 + b] = n * 49;
  }
  S1[3] = 100 * 255;  // the short block is not used
  S2[3] = 100 * 255 * 255;
  S1[7] = 700;
  S2[7] = 4900;
  const std::vector<double> s = inject_sigma(S1, S2, 2, nsamps);
  EXPECT(s[0] == 3.0 && s[1] == 0.0);
  // a file shorter than one block uses its one short block
  const std::vector<double> t = inject_sigma({10 * 100}, {5 * (98 * 98 + 102 * 102)}, 1, 10);
  EXPECT(t[0] == 2.0);
  EXPECT(throws_with([] { inject_sigma({1000}, {10}, 1, 10); }, "S1^2 exceeds"));
  const std::vector<double> u = inject_unit({3.0, 0.0, 2.0}, {1, 1, 0}, 3);
  EXPECT(u[0] == 3.0 && u[1] == 0.0 && u[2] == 0.0);
  const std::vector<double> l = inject_unit({}, {}, 2);
  EXPECT(l[0] == 1.0 && l[1] == 1.0);
}

void test_tables_and_truth() {
  const InjectGeometry g = geom();
  std::vector<InjectSignal> sig = inject_parse("pulsar 0.05 30 0.5\nburst 1.0 100 4 0.004\n");
  std::vector<double> unit(8, 8.0);
  unit[2] = 0.0;
  const InjectTables t = inject_tables(sig, g, unit, true);
  const std::vector<float> D = generate_delay_table(g.nchans, g.tsamp, g.fch1, g.foff);
  EXPECT(t.nsig == 2 && t.nchans == 8 && t.nlive == 7 && t.T.size() == 1537);
  EXPECT(t.sigc[0] == 0.0 && t.sigc[1] == 0.0 && t.sigc[2] == 1.0 / 0.05 && t.sigc[3] == 0.0);
  EXPECT(t.sigc[4] == 1.0 && t.sigc[5] == 1.0 / g.tsamp);
  for (int c = 0; c < 8; ++c) {
    EXPECT(t.delay[c] == 30.0 * static_cast<double>(D[c]));
    EXPECT(t.delay[8 + c] == 100.0 * static_cast<double>(D[c]));
    EXPECT(t.w[c] > 0.05 / 2.3548 && t.inv_w[c] == 256.0 / t.w[c]);
  }
  EXPECT(t.delay[0] == 0.0 && t.delay[7] > 0.0);
  EXPECT(t.A_q[2] == 0 && t.A_q[8 + 2] == 0);
  EXPECT(t.A_q[0] <= 65536u * 4 && t.A_q[0] > 65536u * 3);  // 0.5 x 8 levels, a little less under smearing
  // without smearing the width is the intrinsic one and the amplitude exact
  const InjectTables n = inject_tables(sig, g, unit, false);
  EXPECT(n.w[0] == 0.05 / 2.3548 && n.A_q[0] == 65536u * 4 && n.A_q[8] == 65536u * 32);
  EXPECT(n.w[8] == 0.004 / g.tsamp / 2.3548);
  // the limit
  sig[1].amp = 40;  // 40 x 8 = 320 levels
  EXPECT(throws_with([&] { inject_tables(sig, g, unit, false); }, "A_q >= 2^24"));
  sig[1].amp = 4;
  // truth
  const std::vector<double> sigma(8, 8.0);
  const std::vector<InjectTruth> tr = inject_truth(sig, n, g, unit, sigma);
  EXPECT(tr.size() == 2);
  EXPECT(tr[0].npulses == 52);  // 9999 x 256e-6 / 0.05 = 51.19: pulses 0 .. 51
  EXPECT(tr[0].peak == 4.0 && tr[1].peak == 32.0);
  EXPECT(tr[1].npulses == 1);
  const double ws = n.w[8], want = std::sqrt(7.0 * 16.0 * ws * std::sqrt(3.14159265358979323846));
  EXPECT(std::fabs(tr[1].snr - want) <= 1e-12 * want);
  sig[1].t = 10.0;  // past the end of the file
  const InjectTables m = inject_tables(sig, g, unit, false);
  EXPECT(inject_truth(sig, m, g, unit, sigma)[1].npulses == 0);
  EXPECT(inject_truth(sig, m, g, unit, {})[0].snr == 0.0);
  const std::string text = inject_truth_text(sig, tr, "sigma", 7);
  EXPECT(text.find("units sigma seed 7") != std::string::npos && text.find("\npulsar 0.05") != std::string::npos &&
         text.find("\nburst 10 100 4") != std::string::npos);
}

}  // namespace

int main() {
  test_parser();
  test_geometry();
  test_hash_and_table();
  test_sigma();
  test_tables_and_truth();
  if (g_failed) {
    std::cerr << g_failed << " check(s) failed" << std::endl;
    return 1;
  }
  std::cout << "inject unit tests passed" << std::endl;
  return 0;
}
