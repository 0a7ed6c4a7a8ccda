// Host unit tests of the RFI flagging step (psoup/rfi.hpp): rdiv, rfi_flag on
// hand-made tables, the mask file.  No GPU.  Exit status 0 = all passed.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/rfi.hpp"

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

// Sums of a block of `len` samples that alternate lo, hi (len even).
void two_level(uint64_t len, uint64_t lo, uint64_t hi, uint64_t& s1, uint64_t& s2) {
  s1 = len / 2 * (lo + hi);
  s2 = len / 2 * (lo * lo + hi * hi);
}

void test_rdiv() {
  EXPECT(rfi_rdiv(0, 3) == 0);
  EXPECT(rfi_rdiv(1, 2) == 1);  // halves round up
  EXPECT(rfi_rdiv(1, 3) == 0);
  EXPECT(rfi_rdiv(2, 3) == 1);
  EXPECT(rfi_rdiv(7, 2) == 4);
  EXPECT(rfi_rdiv(10, 4) == 3);
  EXPECT(rfi_rdiv(9, 4) == 2);
  EXPECT(rfi_rdiv(255ll * 65536 * 1000, 65536 * 1000) == 255);
}

void test_flag() {
  // 4 channels x 6 blocks of 256 samples (the last 100 long)
  const int nchans = 4;
  const uint64_t L = 256, nsamps = 5 * 256 + 100, nblk = 6;
  RfiParams p;
  p.block = L;
  p.thresh = 5.0;
  p.chan_frac = 0.5;
  p.block_frac = 0.5;
  std::vector<uint64_t> S1(nchans * nblk), S2(nchans * nblk);
  for (int c = 0; c < nchans; ++c)
    for (uint64_t b = 0; b < nblk; ++b) {
      const uint64_t len = b + 1 < nblk ? L : 100;
      two_level(len, 1, 3, S1[c * nblk + b], S2[c * nblk + b]);  // mean 2, variance 1, MAD 0
    }
  // channel 1, block 2: another mean (MAD 0: any difference flags)
  two_level(L, 2, 4, S1[1 * nblk + 2], S2[1 * nblk + 2]);
  // channel 3: dead
  for (uint64_t b = 0; b < nblk; ++b) {
    const uint64_t len = b + 1 < nblk ? L : 100;
    S1[3 * nblk + b] = 2 * len;
    S2[3 * nblk + b] = 4 * len;
  }
  std::vector<int> kill = {1, 1, 0, 1};  // channel 2 killed
  RfiMask m = rfi_flag(S1, S2, nchans, nsamps, kill, p);
  EXPECT(m.nblk == nblk);
  for (uint64_t b = 0; b < nblk; ++b) {
    EXPECT(m.cell[0 * nblk + b] == (b == 2 ? 1 : 0));  // block 2 is promoted (below)
    EXPECT(m.cell[1 * nblk + b] == (b == 2 ? 1 : 0));
    EXPECT(m.cell[2 * nblk + b] == 1);
    EXPECT(m.cell[3 * nblk + b] == 1);
  }
  // shares: block 2 has channels 1 and 3 flagged of 3 live -> promoted
  EXPECT(m.block_flag[2] == 1);
  EXPECT(m.block_flag[0] == 0);  // 1 of 3
  EXPECT(m.chan_flag[0] == 0 && m.chan_flag[1] == 0 && m.chan_flag[2] == 1 && m.chan_flag[3] == 1);
  EXPECT((m.killmask == std::vector<int>{1, 1, 0, 0}));
  EXPECT(m.fill[0] == 2 && m.fill[1] == 2 && m.fill[2] == 0 && m.fill[3] == 0);
  EXPECT(m.nb[0] == 2 && m.G[0] == 2 && m.nb[2] == 0 && m.G[2] == 0);
}

void test_mask_file(const std::string& dir) {
  RfiParams p;
  p.block = 512;
  p.zero_dm = true;
  std::vector<uint64_t> S1 = {512, 512, 600, 100}, S2 = {1024, 1024, 1400, 100};
  RfiMask m = rfi_flag(S1, S2, 2, 612, {}, p);
  RfiMaskHeader h;
  h.nbits = 2;
  h.tsamp = 64e-6;
  const std::string path = dir + "/rfi_unit.mask";
  write_rfi_mask(path, m, p, h);
  RfiParams p2;
  RfiMaskHeader h2;
  RfiMask r = read_rfi_mask(path, &p2, &h2);
  EXPECT(r.nchans == m.nchans && r.nblk == m.nblk && r.nsamps == m.nsamps && r.block == m.block);
  EXPECT(r.cell == m.cell && r.chan_flag == m.chan_flag && r.block_flag == m.block_flag);
  EXPECT(r.fill == m.fill && r.G == m.G && r.nb == m.nb && r.killmask == m.killmask);
  EXPECT(p2.zero_dm && p2.block == 512 && p2.thresh == p.thresh && h2.nbits == 2 && h2.tsamp == 64e-6);
  std::remove(path.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  try {
    test_rdiv();
    test_flag();
    test_mask_file(dir);
  } catch (const std::exception& e) {
    std::cerr << "exception: " << e.what() << std::endl;
    return 2;
  }
  if (g_failed) {
    std::cerr << g_failed << " check(s) failed" << std::endl;
    return 1;
  }
  std::cout << "rfi unit tests passed" << std::endl;
  return 0;
}
