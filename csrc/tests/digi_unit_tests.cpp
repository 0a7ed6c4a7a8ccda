// Host unit tests of fildigi's host steps (psoup/digi.hpp): parameters, the
// header checks, the scale on hand-made block tables (a single block, odd and
// even counts, blocks without a finite sample, zero variance, a short last
// interval, both scale modes, the quantum's exponent), the band flip and the
// header rewrite.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/digi.hpp"

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

// One channel's block tables, built block by block.
struct Table {
  std::vector<uint32_t> N;
  std::vector<int64_t> S1;
  std::vector<uint64_t> S2;
  std::vector<int32_t> E;
  // n values alternating mean - d, mean + d (n even): mean `mean`, variance d^2
  void two_level(uint32_t n, int64_t mean, int64_t d, int32_t e = 0) {
    N.push_back(n);
    S1.push_back(static_cast<int64_t>(n) * mean);
    S2.push_back(static_cast<uint64_t>(n / 2) * static_cast<uint64_t>((mean - d) * (mean - d) + (mean + d) * (mean + d)));
    E.push_back(e);
  }
  void empty() {
    N.push_back(0);
    S1.push_back(0);
    S2.push_back(0);
    E.push_back(0);
  }
};

void test_params_and_header() {
  DigiParams p;
  digi_check_params(p);
  p.sigma_out = 0;
  EXPECT(throws_with([&] { digi_check_params(p); }, "sigma_out must be positive"));
  p.sigma_out = 16;
  p.rescale_blocks = -1;
  EXPECT(throws_with([&] { digi_check_params(p); }, "rescale_blocks must be non-negative"));
  EXPECT(digi_check_header(8, 0, 1, -1.0, 4) == kern::DigiType::U8);
  EXPECT(digi_check_header(8, 1, 1, 1.0, 4) == kern::DigiType::I8);
  EXPECT(digi_check_header(16, 0, 0, 1.0, 4) == kern::DigiType::U16);
  EXPECT(digi_check_header(32, 0, 1, 1.0, 4) == kern::DigiType::F32);
  for (int nbits : {1, 2, 4, 64})
    EXPECT(throws_with([&] { digi_check_header(nbits, 0, 1, 1.0, 4); }, "nbits must be 8, 16 or 32"));
  EXPECT(throws_with([&] { digi_check_header(8, 0, 2, 1.0, 4); }, "nifs must be 1"));
  EXPECT(throws_with([&] { digi_check_header(8, 0, 1, 0.0, 4); }, "foff must not be zero"));
  DigiCmdLineOptions a;
  a.scale = "file";
  a.rescale_blocks = 3;
  EXPECT(digi_params_from(a).scale == DigiScaleMode::File && digi_params_from(a).rescale_blocks == 3);
  a.scale = "both";
  EXPECT(throws_with([&] { digi_params_from(a); }, "scale must be channel or file"));
  EXPECT(digi_nblk(1) == 1 && digi_nblk(4096) == 1 && digi_nblk(4097) == 2);
  EXPECT(digi_nint(5, 0) == 1 && digi_nint(5, 2) == 3 && digi_nint(4, 2) == 2);
}

void test_scale_medians() {
  // one channel, three blocks of sigma 2, 4, 8 and means 10, 30, 20: the medians are 20 and 16
  Table t;
  t.two_level(4096, 10, 2);
  t.two_level(4096, 30, 4);
  t.two_level(100, 20, 8);
  DigiParams p;
  DigiScale sc = digi_scale(t.N, t.S1, t.S2, t.E, 1, 3, {}, p);
  EXPECT(sc.nint == 1 && sc.live[0] == 1 && sc.nlive == 1 && sc.mean[0] == 20.0 && sc.gain[0] == 16.0 / 4.0);
  EXPECT(sc.gain_min == 4.0 && sc.gain_max == 4.0);
  // an even count: the mean of the two middle values; a block without a finite sample does not count
  t.empty();
  t.two_level(4096, 40, 16);
  sc = digi_scale(t.N, t.S1, t.S2, t.E, 1, 5, {}, p);
  EXPECT(sc.mean[0] == 25.0 && sc.gain[0] == 16.0 / std::sqrt(40.0));
  // a single block; the quantum's exponent scales the mean by 2^E and the variance by 4^E
  Table one;
  one.two_level(64, 3, 1, -10);
  sc = digi_scale(one.N, one.S1, one.S2, one.E, 1, 1, {}, p);
  EXPECT(sc.mean[0] == std::ldexp(3.0, -10) && sc.gain[0] == 16.0 / std::ldexp(1.0, -10));
  // the numerator needs more than 64 bits: q = 2^23 - 1 -/+ 1 over a whole block
  Table big;
  big.two_level(4096, (1 << 23) - 2, 1, 100);
  sc = digi_scale(big.N, big.S1, big.S2, big.E, 1, 1, {}, p);
  EXPECT(sc.mean[0] == std::ldexp(static_cast<double>((1 << 23) - 2), 100) && sc.gain[0] == 16.0 / std::ldexp(1.0, 100));
}

void test_scale_intervals_modes_and_dead() {
  // two channels, five blocks, J = 2: intervals {0, 1}, {2, 3}, {4}
  Table a, b;
  for (int k = 0; k < 5; ++k) a.two_level(4096, 100, 1 << k);  // sigma 1 2 4 8 16
  b.two_level(4096, 7, 3);
  b.two_level(4096, 7, 3);
  b.two_level(4096, 9, 0);  // interval 1: zero variance in both blocks
  b.two_level(4096, 9, 0);
  b.empty();                // interval 2: no finite sample
  Table t = a;
  t.N.insert(t.N.end(), b.N.begin(), b.N.end());
  t.S1.insert(t.S1.end(), b.S1.begin(), b.S1.end());
  t.S2.insert(t.S2.end(), b.S2.begin(), b.S2.end());
  t.E.insert(t.E.end(), b.E.begin(), b.E.end());
  DigiParams p;
  p.rescale_blocks = 2;
  DigiScale sc = digi_scale(t.N, t.S1, t.S2, t.E, 2, 5, {}, p);
  EXPECT(sc.nint == 3 && sc.nlive == 2);
  EXPECT((sc.live == std::vector<uint8_t>{1, 1, 1, 0, 1, 0}));
  EXPECT(sc.gain[0] == 16.0 / std::sqrt(2.5) && sc.gain[2] == 16.0 / std::sqrt(40.0) && sc.gain[4] == 1.0);
  EXPECT(sc.gain[1] == 16.0 / 3.0 && sc.gain[3] == 0.0 && sc.gain[5] == 0.0 && sc.mean[1] == 7.0);
  EXPECT(sc.gain_min == 1.0 && sc.gain_max == 16.0 / std::sqrt(2.5));
  // file mode: one gain per interval from the median sigma of its live channels
  p.scale = DigiScaleMode::File;
  sc = digi_scale(t.N, t.S1, t.S2, t.E, 2, 5, {}, p);
  const double g0 = 16.0 / ((std::sqrt(2.5) + 3.0) / 2.0);
  EXPECT(sc.gain[0] == g0 && sc.gain[1] == g0 && sc.gain[2] == 16.0 / std::sqrt(40.0) && sc.gain[3] == 0.0);
  // a killed channel is not live anywhere; with every channel killed or flat nothing is left
  sc = digi_scale(t.N, t.S1, t.S2, t.E, 2, 5, {0, 1}, p);
  EXPECT(sc.nlive == 1 && (sc.alive == std::vector<int>{0, 1}) && sc.gain[0] == 0.0 && sc.gain[1] == 16.0 / 3.0);
  EXPECT(throws_with([&] { digi_scale(t.N, t.S1, t.S2, t.E, 2, 5, {0, 0}, p); }, "no live channel"));
  Table flat;
  flat.two_level(4096, 5, 0);
  EXPECT(throws_with([&] { digi_scale(flat.N, flat.S1, flat.S2, flat.E, 1, 1, {}, p); }, "no live channel"));
  EXPECT(throws_with([&] { digi_scale(flat.N, flat.S1, flat.S2, flat.E, 1, 2, {}, p); }, "must be [nchans][nblk]"));
}

void test_band_and_header() {
  DigiBand b = digi_band(1200.0, 0.5, 64);
  EXPECT(b.flip && b.fch1 == 1231.5 && b.foff == -0.5);
  b = digi_band(1510.0, -1.09, 64);
  EXPECT(!b.flip && b.fch1 == 1510.0 && b.foff == -1.09);
  SigprocHeader h;
  h.nchans = 64;
  h.nbits = 8;
  h.signed_data = 1;
  h.fch1 = 1200.0;
  h.foff = 0.5;
  h.nsamples = 1000;
  h.ibeam = 3;
  h.keys_present = {"nchans", "nbits", "signed", "fch1", "foff", "nsamples", "ibeam"};
  SigprocHeader o = digi_header(h);
  EXPECT(o.nbits == 8 && o.signed_data == 0 && o.fch1 == 1231.5 && o.foff == -0.5 && o.nsamples == 1000 && o.ibeam == 3);
  EXPECT((o.keys_present == std::vector<std::string>{"nchans", "nbits", "fch1", "foff", "nsamples", "ibeam"}));
  h.nbits = 32;
  h.keys_present = {"nchans", "nbits", "fch1", "foff"};
  o = digi_header(h);
  EXPECT(o.nbits == 8 && o.nsamples == 0);  // derived from the size on reading: not written
}

}  // namespace

int main() {
  test_params_and_header();
  test_scale_medians();
  test_scale_intervals_modes_and_dead();
  test_band_and_header();
  std::cout << (g_failed == 0 ? "all passed, " : "FAILED, ") << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
