// Host unit tests of filscrunch's host steps (psoup/scrunch.hpp): offsets, the
// scale on hand-made tables (medians with odd and even counts, one short
// block, the 128-bit numerator, the clamps of mul) and the plan's tiers.  No
// GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/scrunch.hpp"

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

constexpr uint64_t L = kern::kScrunchStatBlock;

// Sums of a block of `len` values that alternate lo, hi (len even): mean
// (lo + hi) / 2, variance ((hi - lo) / 2)^2.
void two_level(uint64_t len, uint64_t lo, uint64_t hi, uint64_t& s1, uint64_t& s2) {
  s1 = len / 2 * (lo + hi);
  s2 = len / 2 * (lo * lo + hi * hi);
}

template <class F>
bool throws_with(F&& f, const std::string& what) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

void test_params() {
  ScrunchParams p;
  EXPECT(scrunch_check_params(p, 64).nsub == 64);
  p.nsub = 16;
  p.tscrunch = 256;
  EXPECT(scrunch_check_params(p, 64).nsub == 16);
  p.nsub = 24;
  EXPECT(throws_with([&] { scrunch_check_params(p, 64); }, "nsub must divide nchans"));
  p.nsub = 16;
  p.tscrunch = 257;
  EXPECT(throws_with([&] { scrunch_check_params(p, 64); }, "tscrunch must be in 1..256"));
  p.tscrunch = 0;
  EXPECT(throws_with([&] { scrunch_check_params(p, 64); }, "tscrunch must be in 1..256"));
  p.tscrunch = 1;
  p.sigma_out = 0;
  EXPECT(throws_with([&] { scrunch_check_params(p, 64); }, "sigma_out must be positive"));
  p.sigma_out = 16;
  p.dm = -1.f;
  EXPECT(throws_with([&] { scrunch_check_params(p, 64); }, "dm must be"));
}

void test_offsets() {
  // delays 0, 0.5, 1.25, 2, 3.5, 5.25 at DM 2: offsets 0 1 3 4 7 11 (round half up)
  const std::vector<float> d = {0.f, 0.5f, 1.25f, 2.f, 3.5f, 5.25f};
  ScrunchOffsets o = scrunch_offsets(2.f, d, 2);
  EXPECT((o.rel == std::vector<int32_t>{0, 1, 3, 0, 3, 7}) && o.R == 7);
  o = scrunch_offsets(2.f, d, 6);
  EXPECT((o.rel == std::vector<int32_t>(6, 0)) && o.R == 0);
  o = scrunch_offsets(2.f, d, 1);
  EXPECT((o.rel == std::vector<int32_t>{0, 1, 3, 4, 7, 11}) && o.R == 11);
  o = scrunch_offsets(0.f, d, 3);
  EXPECT(o.R == 0);
  EXPECT(throws_with([&] { scrunch_offsets(2.f, d, 4); }, "nsub must divide nchans"));
  const std::vector<float> up = {0.f, -1.f};
  EXPECT(throws_with([&] { scrunch_offsets(2.f, up, 1); }, "foff must be < 0"));
}

void test_scale_medians() {
  // 3 subbands x 5 blocks (odd count), the last block 100 long.  Subband 0:
  // levels 100 +- 8 with one outlier block; 1: 40 +- 2; 2: constant (dead).
  const int nsub = 3;
  const uint64_t nblk = 5, nout = 4 * L + 100;
  std::vector<uint64_t> S1(nsub * nblk), S2(nsub * nblk);
  for (uint64_t b = 0; b < nblk; ++b) {
    const uint64_t len = b + 1 < nblk ? L : 100;
    two_level(len, 92, 108, S1[b], S2[b]);
    two_level(len, 38, 42, S1[nblk + b], S2[nblk + b]);
    two_level(len, 7, 7, S1[2 * nblk + b], S2[2 * nblk + b]);
  }
  two_level(L, 0, 60000, S1[2], S2[2]);  // an outlier block: the medians do not move
  ScrunchScale sc = scrunch_scale(S1, S2, nsub, nout, {4, 4, 4}, 16.0);
  EXPECT((sc.M == std::vector<int32_t>{100, 40, 7}));
  EXPECT((sc.live == std::vector<uint8_t>{1, 1, 0}) && sc.nlive == 2);
  EXPECT(sc.sigma_ref == 5.0);  // median of {8, 2}: the mean of the two
  EXPECT(sc.mul == static_cast<int32_t>(std::floor(16.0 / 5.0 * 65536.0 + 0.5)));
  // a fully killed subband is not live whatever its sums
  sc = scrunch_scale(S1, S2, nsub, nout, {4, 0, 4}, 16.0);
  EXPECT((sc.live == std::vector<uint8_t>{1, 0, 0}) && sc.sigma_ref == 8.0 && sc.mul == 2 * 65536);
  // an even count: 4 blocks with means 10, 20, 30, 41 -> median 25, M = 25; 25.5 rounds up
  std::vector<uint64_t> T1(4), T2(4);
  const uint64_t lev[4] = {10, 20, 30, 41};
  for (int b = 0; b < 4; ++b) two_level(L, lev[b] - 1, lev[b] + 1, T1[b], T2[b]);
  sc = scrunch_scale(T1, T2, 1, 4 * L, {1}, 16.0);
  EXPECT(sc.M[0] == 25 && sc.sigma_ref == 1.0 && sc.mul == 16 * 65536);
  two_level(L, 30, 32, T1[2], T2[2]);  // means 10 20 31 41 -> 25.5 -> 26
  EXPECT(scrunch_scale(T1, T2, 1, 4 * L, {1}, 16.0).M[0] == 26);
  // one short block only
  uint64_t s1, s2;
  two_level(10, 3, 9, s1, s2);
  sc = scrunch_scale({s1}, {s2}, 1, 10, {2}, 16.0);
  EXPECT(sc.M[0] == 6 && sc.sigma_ref == 3.0 && sc.nlive == 1);
  // no live subband
  two_level(10, 5, 5, s1, s2);
  EXPECT(throws_with([&] { scrunch_scale({s1}, {s2}, 1, 10, {2}, 16.0); }, "no live subband"));
  EXPECT(throws_with([&] { scrunch_scale(S1, S2, nsub, nout, {0, 0, 0}, 16.0); }, "no live subband"));
}

void test_scale_wide_numerator() {
  // values near the 2^26 bound: len S2 and S1^2 are about 2^76, far beyond 64
  // bits, and differ by len^2 / 4 * (hi - lo)^2 exactly
  const uint64_t hi = (1ull << 26) - 1, lo = hi - 2;
  uint64_t s1, s2;
  two_level(L, lo, hi, s1, s2);
  ScrunchScale sc = scrunch_scale({s1}, {s2}, 1, L, {1}, 16.0);
  EXPECT(sc.M[0] == static_cast<int32_t>(hi - 1) && sc.sigma_ref == 1.0 && sc.live[0] == 1);
  // a 64-bit product would have wrapped: len * S2 needs more than 64 bits
  EXPECT(s2 > (~0ull) / L);
}

void test_mul_clamps() {
  uint64_t s1, s2;
  two_level(L, 0, 2, s1, s2);  // sigma 1
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 1e-9).mul == 1);
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 1e9).mul == 2147483647);
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 32767.99).mul == 2147482993);  // floor(32767.99 * 65536 + 0.5)
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 32768.0).mul == 2147483647);
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 0.5 / 65536).mul == 1);   // 0.5 + 0.5 = 1
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 0.25 / 65536).mul == 1);  // floor(0.75) = 0, clamped
  EXPECT(scrunch_scale({s1}, {s2}, 1, L, {1}, 1.5 / 65536).mul == 2);
}

void test_plan() {
  // 4096 channels of -400 / 4096 MHz from 1500 MHz, 64 us
  const double tsamp = 64e-6, fch1 = 1500.0, foff = -400.0 / 4096;
  const int nchans = 4096;
  const double nu = (fch1 + 4095 * foff) / 1000.0;
  const double unit = tsamp * (nu * nu * nu) / (8.3e-6 * std::fabs(foff));
  std::vector<ScrunchTier> t = scrunch_plan(tsamp, fch1, foff, nchans, 1e6);
  EXPECT(t.size() == 7);
  for (size_t k = 0; k < t.size(); ++k) {
    EXPECT(t[k].tscrunch == 1 << k);
    EXPECT(t[k].dm_lo == (k == 0 ? 0.0 : static_cast<double>(1 << k) * unit));
    if (k > 0) EXPECT(t[k].dm_lo == t[k - 1].dm_hi);  // contiguous
  }
  EXPECT(t.back().dm_hi == 1e6 && t.back().tscrunch == 64);  // capped at 64
  // a DM range that ends inside the third tier
  t = scrunch_plan(tsamp, fch1, foff, nchans, 5.0 * unit);
  EXPECT(t.size() == 3 && t[2].tscrunch == 4 && t[2].dm_hi == 5.0 * unit && t[1].dm_hi == 4.0 * unit);
  // a range below the first boundary, and one that ends exactly on it
  t = scrunch_plan(tsamp, fch1, foff, nchans, 0.5 * unit);
  EXPECT(t.size() == 1 && t[0].dm_lo == 0.0 && t[0].dm_hi == 0.5 * unit && t[0].tscrunch == 1);
  t = scrunch_plan(tsamp, fch1, foff, nchans, 2.0 * unit);
  EXPECT(t.size() == 1 && t[0].dm_hi == 2.0 * unit);
  t = scrunch_plan(tsamp, fch1, foff, nchans, 0.0);
  EXPECT(t.size() == 1 && t[0].dm_hi == 0.0);
  EXPECT(throws_with([&] { scrunch_plan(tsamp, fch1, foff, nchans, -1.0); }, "dm_end"));
}

}  // namespace

int main() {
  test_params();
  test_offsets();
  test_scale_medians();
  test_scale_wide_numerator();
  test_mul_clamps();
  test_plan();
  std::cout << (g_failed == 0 ? "all scrunch unit tests passed, " : "FAILURES, ") << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
