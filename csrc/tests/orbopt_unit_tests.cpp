// Host unit tests of orbopt's host steps (psoup/orbopt.hpp): the parameter
// ranges, the grid with its default steps, the collapse at a1 = 0 and the sign
// fold, G, hits, the row moments and their refusal, the drift table, the host
// transcriptions of both kernels on hand-checked inputs, the finish with its
// flags, the candidate parser, the bytes of the result file and the command
// line.  No GPU.  Exit status 0 = all passed.
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "psoup/orbopt.hpp"

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

const float kTs = 320e-6f;

template <class F>
bool throws_with(F&& f, const std::string& what) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

std::vector<uint8_t> noise(size_t n, unsigned seed) {
  std::vector<uint8_t> x(n);
  uint32_t z = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    z = z * 1664525u + 1013904223u;
    x[i] = static_cast<uint8_t>(z >> 24);
  }
  return x;
}

OrbOptCandidate cand(double period, double pb, double a1, double ph, float dm = 20.f, float acc = 0.f) {
  OrbOptCandidate c;
  c.period = period;
  c.dm = dm;
  c.acc = acc;
  c.pb = pb;
  c.a1 = a1;
  c.ph = ph;
  return c;
}

void test_params() {
  OrbOptParams p;
  oopt_check_params(p);
  EXPECT(p.nbins == 64 && p.nints == 16 && p.npb == 9 && p.na1 == 9 && p.nphase == 9 && p.np == 33 && p.p_step == 1.0);
  auto bad = [](auto set, const char* what) {
    OrbOptParams q;
    set(q);
    return throws_with([&] { oopt_check_params(q); }, what);
  };
  EXPECT(bad([](OrbOptParams& q) { q.npb = 4; }, "an even count"));
  EXPECT(bad([](OrbOptParams& q) { q.na1 = 0; }, "an even count"));
  EXPECT(bad([](OrbOptParams& q) { q.nphase = 2; }, "an even count"));
  EXPECT(bad([](OrbOptParams& q) { q.np = 34; }, "an even count"));
  EXPECT(bad([](OrbOptParams& q) { q.np = 259; }, "1..257"));
  EXPECT(bad([](OrbOptParams& q) { q.nbins = 1; }, "nbins must be in 2..256"));
  EXPECT(bad([](OrbOptParams& q) { q.nbins = 257; }, "nbins must be in 2..256"));
  EXPECT(bad([](OrbOptParams& q) { q.nints = 65; }, "nints must be in 1..64"));
  EXPECT(bad([](OrbOptParams& q) { q.nints = 64; q.nbins = 256; }, "") == false);  // 16384: the limit itself
  EXPECT(bad([](OrbOptParams& q) { q.npb = 17; q.na1 = 17; q.nphase = 17; }, "more than 4096 templates"));
  // the largest grid the ranges admit, 4095 * 257 * 256 trial bins, is far below 2^31
  EXPECT(bad([](OrbOptParams& q) { q.npb = 15; q.na1 = 21; q.nphase = 13; q.np = 257; q.nbins = 256; q.nints = 1; }, "") == false);
  EXPECT(bad([](OrbOptParams& q) { q.p_step = -1.0; }, "finite and non-negative"));
  EXPECT(bad([](OrbOptParams& q) { q.pb_step = std::numeric_limits<double>::infinity(); }, "finite and non-negative"));
}

void test_grid() {
  OrbOptParams p;
  const uint64_t n = 1u << 17;
  const double ts = static_cast<double>(kTs), P = 0.0101, T = static_cast<double>(n) * ts;
  const OrbOptCandidate c = cand(P, 63.0, 0.0088, 0.72);
  const OrbOptGrid g = oopt_grid(0, p, c, n, kTs);
  EXPECT(g.npb == 9 && g.na1 == 9 && g.nphase == 9 && g.tmpl.size() == 729 && g.quant.size() == 729);
  EXPECT(g.da1 == P / (2.0 * 64.0));
  EXPECT(g.dph == std::min(1.0 / 16.0, P / ((4.0 * M_PI) * 0.0088 * 64.0)));
  EXPECT(g.dpb == std::min(63.0 / 16.0, (63.0 * 63.0 * P) / ((4.0 * M_PI) * 0.0088 * T * 64.0)));
  EXPECT(g.G == static_cast<uint64_t>(std::rint(std::ldexp(ts / P, 64))));
  // the centre is the candidate's own; pb slowest, phase fastest
  EXPECT(g.tmpl[364] == (OrbitTemplate{63.0, 0.0088, 0.72}));
  EXPECT(g.tmpl[365].ph == 0.72 + 1.0 * g.dph && g.tmpl[365].a1 == 0.0088 && g.tmpl[365].pb == 63.0);
  EXPECT(g.tmpl[364 + 9].a1 == 0.0088 + 1.0 * g.da1 && g.tmpl[364 + 81].pb == 63.0 + 1.0 * g.dpb);
  EXPECT(g.tmpl[0].pb == 63.0 + (-4.0) * g.dpb && g.tmpl[0].a1 == 0.0088 + (-4.0) * g.da1);
  const OrbitQuant q = orbit_quantise(63.0, 0.0088, 0.72, kTs);
  EXPECT(g.quant[364].W == q.W && g.quant[364].F == q.F && g.quant[364].Aq == q.Aq);
  // user steps
  p.pb_step = 0.5;
  p.a1_step = 1e-4;
  p.phase_step = 0.01;
  const OrbOptGrid u = oopt_grid(0, p, c, n, kTs);
  EXPECT(u.dpb == 0.5 && u.da1 == 1e-4 && u.dph == 0.01 && u.tmpl[364 + 81 + 9 + 1] == (OrbitTemplate{63.5, 0.0089, 0.73}));
  // a1 = 0: one pb and one phase; the sign fold of the lower half
  OrbOptParams d;
  const OrbOptGrid z = oopt_grid(0, d, cand(P, 63.0, 0.0, 0.25), n, kTs);
  EXPECT(z.npb == 1 && z.nphase == 1 && z.na1 == 9 && z.tmpl.size() == 9 && z.dpb == 0.0 && z.dph == 0.0);
  EXPECT(z.tmpl[4] == (OrbitTemplate{63.0, 0.0, 0.25}));
  EXPECT(z.tmpl[3].a1 == z.da1 && z.tmpl[3].ph == 0.75 && z.tmpl[5].a1 == z.da1 && z.tmpl[5].ph == 0.25);
  EXPECT(z.tmpl[0].a1 == 4.0 * z.da1 && z.tmpl[0].ph == 0.75);
  // a user's pb_step keeps the pb dimension at a1 = 0
  d.pb_step = 1.0;
  EXPECT(oopt_grid(0, d, cand(P, 63.0, 0.0, 0.25), n, kTs).npb == 9);
  // refusals, by candidate
  OrbOptParams r;
  EXPECT(throws_with([&] { oopt_grid(3, r, cand(1.5 * ts, 63.0, 0.0088, 0.72), n, kTs); }, "candidate 3"));
  EXPECT(throws_with([&] { oopt_grid(3, r, cand(1.5 * ts, 63.0, 0.0088, 0.72), n, kTs); }, "below 2 tsamp"));
  EXPECT(throws_with([&] { oopt_grid(0, r, cand(NAN, 63.0, 0.0088, 0.72), n, kTs); }, "below 2 tsamp"));
  EXPECT(throws_with([&] { oopt_grid(1, r, cand(P, 63.0, 0.0088, 0.72, -1.f), n, kTs); }, "non-finite or negative DM"));
  EXPECT(throws_with([&] { oopt_grid(1, r, cand(P, 63.0, 0.0088, 0.72, NAN), n, kTs); }, "non-finite or negative DM"));
  EXPECT(throws_with([&] { oopt_grid(1, r, cand(P, NAN, 0.0088, 0.72), n, kTs); }, "non-finite value"));
  EXPECT(throws_with([&] { oopt_grid(2, r, cand(P, 0.01, 0.0, 0.72), n, kTs); }, "pb < 64 tsamp"));
  EXPECT(throws_with([&] { oopt_grid(2, r, cand(P, 1e9, 2000.0, 0.0), n, kTs); }, "Aq >= 2^30"));
  EXPECT(throws_with([&] { oopt_grid(2, r, cand(P, 100.0, 20.0, 0.0), n, kTs); }, "0.9 samples per sample"));
  EXPECT(throws_with([&] { oopt_grid(2, r, cand(P, 100.0, 20.0, 0.0), n, kTs); }, "candidate 2"));
  EXPECT(throws_with([&] { oopt_grid(0, r, c, (1u << 26) + 1, kTs); }, "longer than 2^26"));
  EXPECT(throws_with([&] { oopt_grid(0, r, c, 0, kTs); }, "empty"));
  // a grid whose edge leaves the admitted range refuses the candidate: pb0 just above 64 tsamp with a user step
  OrbOptParams e;
  e.pb_step = 8.0 * ts;
  EXPECT(throws_with([&] { oopt_grid(5, e, cand(P, 70.0 * ts, 1e-6, 0.0), n, kTs); }, "pb < 64 tsamp"));
}

void test_hits_moments_drift() {
  const uint64_t n = 1000;
  const uint64_t G = static_cast<uint64_t>(std::rint(std::ldexp(1.0 / 2.5, 64)));
  const std::vector<int32_t> h = oopt_hits(G, n, 3, 7);
  EXPECT(h.size() == 21 && std::accumulate(h.begin(), h.end(), 0) == 1000);
  EXPECT(std::accumulate(h.begin(), h.begin() + 7, 0) == 334 && std::accumulate(h.begin() + 14, h.end(), 0) == 333);
  // 17 samples over 16 subints: j(i) = 16 i / 17 reaches every subint, none is empty
  const std::vector<int32_t> e = oopt_hits(G, 17, 16, 2);
  int empty = 0;
  for (int j = 0; j < 16; ++j) empty += e[2 * j] + e[2 * j + 1] == 0;
  EXPECT(std::accumulate(e.begin(), e.end(), 0) == 17 && empty == 0);
  // 5 samples over 16 subints: j(i) = 16 i / 5 = 0, 3, 6, 9, 12; the other 11 subints stay empty
  const std::vector<int32_t> e2 = oopt_hits(G, 5, 16, 2);
  int empty2 = 0;
  for (int j = 0; j < 16; ++j) empty2 += e2[2 * j] + e2[2 * j + 1] == 0;
  EXPECT(std::accumulate(e2.begin(), e2.end(), 0) == 5 && empty2 == 11 && e2[0] + e2[1] == 1 && e2[24] + e2[25] == 1);
  // moments
  const std::vector<uint8_t> x = {1, 2, 3, 4, 250};
  const OrbOptMoments mo = oopt_moments(0, x.data(), 5);
  EXPECT(mo.m == 52 && mo.v1 == 51 * 51 + 50 * 50 + 49 * 49 + 48 * 48 + 198 * 198);
  const std::vector<uint8_t> big((1u << 24), 128);
  EXPECT(throws_with([&] { oopt_moments(7, big.data(), big.size()); }, "candidate 7"));
  EXPECT(throws_with([&] { oopt_moments(7, big.data(), big.size()); }, ">= 2^31"));
  EXPECT(oopt_moments(0, big.data(), big.size() - 1).m == 128);
  // drift table: the centre trial is all zeros; the ends are -/+ L / 2 rounded, reduced
  OrbOptParams p;
  const std::vector<int32_t> st = oopt_drift_table(p);
  EXPECT(st.size() == 33u * 16u);
  bool zero = true;
  for (int j = 0; j < 16; ++j) zero = zero && st[16 * 16 + j] == 0;
  EXPECT(zero);
  EXPECT(st[32 * 16 + 15] == static_cast<int32_t>(std::rint(16.0 * (15.5 / 16 - 0.5))));
  EXPECT(st[32 * 16 + 0] == 64 + static_cast<int32_t>(std::rint(16.0 * (0.5 / 16 - 0.5))));
  for (int32_t v : st) EXPECT(v >= 0 && v < 64);
}

void test_fold_and_search() {
  // the identity template folds the row itself; hits equal the fold of a row of ones
  const uint64_t n = 4101;
  const std::vector<uint8_t> x = noise(n, 3);
  const uint64_t G = static_cast<uint64_t>(std::rint(std::ldexp(1.0 / 64.3, 64)));
  const OrbitQuant ident = orbit_quantise(100.0, 0.0, 0.3, kTs);
  const OrbitQuant moved = orbit_quantise(4101.0 * kTs, 40.0 * kTs, 0.37, kTs);
  const std::vector<int32_t> f = orbopt_fold_host(x.data(), n, G, {ident, moved}, 3, 7);
  EXPECT(f.size() == 2u * 21u);
  std::vector<int64_t> want(21, 0), want2(21, 0);
  const std::vector<int32_t> table = orbit_sine_table();
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t b = (((i * G) >> 32) * 7) >> 32, j = i * 3 / n;
    want[j * 7 + b] += x[i];
    const int64_t s = static_cast<int64_t>(i) + orbit_shift(table.data(), moved, i);
    want2[j * 7 + b] += x[std::min<int64_t>(std::max<int64_t>(s, 0), n - 1)];
  }
  bool same = true, same2 = true, differ = false;
  for (int e = 0; e < 21; ++e) {
    same = same && f[e] == want[e];
    same2 = same2 && f[21 + e] == want2[e];
    differ = differ || want[e] != want2[e];
  }
  EXPECT(same && same2 && differ);
  const std::vector<uint8_t> ones(n, 1);
  const std::vector<int32_t> h = oopt_hits(G, n, 3, 7);
  EXPECT(orbopt_fold_host(ones.data(), n, G, {ident}, 3, 7) == h);
  EXPECT(throws_with([&] { orbopt_fold_host(x.data(), n, G, {}, 3, 7); }, "templates per launch"));
  EXPECT(throws_with([&] { orbopt_fold_host(x.data(), n, G, {OrbitQuant{1, 0, int64_t{1} << 30}}, 3, 7); }, "Aq >= 2^30"));

  // search: a hand-made plane, 2 templates x 2 subints x 8 bins, m = 1 and hits = 1; a pulse that drifts by one bin
  const int K = 2, nints = 2, nbins = 8, np = 3;
  std::vector<int32_t> fold(K * nints * nbins, 0), hits(nints * nbins, 1);
  fold[0 * 16 + 0 * 8 + 2] = 10;  // template 0: bin 2 then bin 3
  fold[0 * 16 + 1 * 8 + 3] = 10;
  fold[1 * 16 + 0 * 8 + 5] = 7;   // template 1: aligned, weaker
  fold[1 * 16 + 1 * 8 + 5] = 7;
  OrbOptParams p;
  p.nbins = nbins;
  p.nints = nints;
  p.npb = 1;
  p.na1 = 1;
  p.nphase = 1;
  p.np = np;
  p.p_step = 4.0;
  const std::vector<int32_t> st = oopt_drift_table(p);  // L = -4, 0, 4: shifts (+1, -1) -> (1, 7); 0; (7, 1)
  EXPECT((st == std::vector<int32_t>{1, 7, 0, 0, 7, 1}));
  const OrbOptSearch s = orbopt_search_host(fold.data(), hits.data(), 1, st.data(), K, nints, nbins, np);
  // d = fold - 1: 9 at the pulse, -1 elsewhere (template 0), 6 and -1 (template 1).  Template 0's pulse drifts by one
  // bin, and the three trials shift the subints by (1, 7), (0, 0) and (7, 1), never by a difference of one: its two
  // pulses never share a bin, so its best single bin is 9 - 1 = 8, first at (k 0, l 0, b 1).  Template 1 is aligned at
  // l = 1: 6 + 6 = 12 at (k 1, l 1, b 5), the overall best and, being (K / 2, np / 2), the centre.
  EXPECT(s.best_val[0] == 12 && s.best_idx[0] == (1 * np + 1) * nbins + 5);
  EXPECT(s.tcurve[0] == 8 && s.tcurve[1] == 12 && s.centre[0] == 12);
  EXPECT(s.msum[0] == 20 - 16 && s.msum[1] == 14 - 16);
  // width 2 at template 0, l 1: bins 2 and 3 adjacent: (9 - 1) + (9 - 1) = 16 at b = 2
  EXPECT(s.best_val[1] == 16 && s.best_idx[1] == (0 * np + 1) * nbins + 2 && s.tcurve[2 + 0] == 16);
  // all-equal planes: ties go to the smallest flat index
  std::vector<int32_t> flat(K * nints * nbins, 5);
  const OrbOptSearch t = orbopt_search_host(flat.data(), hits.data(), 2, st.data(), K, nints, nbins, np);
  EXPECT(t.best_val[0] == 6 && t.best_idx[0] == 0 && t.best_val[2] == 24 && t.best_idx[2] == 0 && t.centre[1] == 12);
  std::vector<int32_t> badst = st;
  badst[1] = 8;
  EXPECT(throws_with([&] { orbopt_search_host(fold.data(), hits.data(), 0, badst.data(), K, nints, nbins, np); },
                     "outside [0, nbins)"));

  // finish on the hand-made search
  OrbOptGrid g;
  g.tmpl = {OrbitTemplate{60.0, 0.01, 0.5}, OrbitTemplate{61.0, 0.01, 0.5}};
  g.quant.resize(2);
  g.npb = 2;  // (not odd: the finish only enumerates)
  OrbOptMoments mo;
  mo.m = 1;
  mo.v1 = 800;
  const OrbOptCandidate c = cand(0.01, 60.0, 0.01, 0.5, 20.f, 0.f);
  const OrbOptResult r = oopt_finish(p, c, g, 100000, kTs, mo, hits, st, s, fold.data() + 16);
  // V = 100; width 1: (12 - 1 * -2 / 8) / sqrt(100 * 1 * 7 / 8); width 2: (16 - 2 * 4 / 8) / sqrt(100 * 2 * 6 / 8)
  const double s1 = (12.0 - 1 * -2.0 / 8) / std::sqrt(100.0 * 1 * (1.0 - 1.0 / 8));
  const double s2 = (16.0 - 2 * 4.0 / 8) / std::sqrt(100.0 * 2 * (1.0 - 2.0 / 8));
  EXPECT(s1 > s2 && r.snr == s1 && r.opt_width == 1 && r.opt_k == 1 && r.opt_l == 1 && r.opt_bin == 5);
  EXPECT(r.opt_pb == 61.0 && r.opt_period == 1.0 / (1.0 / 0.01 - 0.0 / (8 * (100000 * static_cast<double>(kTs)))));
  EXPECT((r.flags & 1u) == 1u && (r.flags & 2u) == 0u);  // template 1 of 2 is a face
  EXPECT(r.profile.size() == 8 && r.fold.size() == 16 && r.hits == hits);
  EXPECT(oopt_finish(p, cand(0.01, 60.0, 0.01, 0.5, 20.f, 5000.f), g, 100000, kTs, mo, hits, st, s, fold.data() + 16).flags & 2u);
  EXPECT(oopt_snr(5.0, 1, 0, 0.0, 8) == 0.0);
}

void test_parser_and_file() {
  const std::string text =
      "# period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx\n"
      "0.0101 20 0 63 0.0088 0.72 99.0099 2 25.1 0 0\n\n"
      "  0.25\t30.5 -1.5 7200.5 0 0.5 # a comment\n";
  const std::vector<OrbOptCandidate> c = oopt_parse_candidates(text);
  EXPECT(c.size() == 2 && c[0].period == 0.0101 && c[0].dm == 20.f && c[0].pb == 63.0 && c[0].a1 == 0.0088 && c[0].ph == 0.72);
  EXPECT(c[1].period == 0.25 && c[1].dm == 30.5f && c[1].acc == -1.5f && c[1].pb == 7200.5 && c[1].a1 == 0.0);
  EXPECT(oopt_parse_candidates("# nothing\n\n").empty());
  EXPECT(throws_with([] { oopt_parse_candidates("0.01 20 0 63 0.0088 0.72\n0.01 20 0 63 0.0088\n"); },
                     "candidate line 2 is malformed"));
  EXPECT(throws_with([] { oopt_parse_candidates("0.01 20 0 63 x 0.72\n"); }, "candidate line 1 is malformed"));
  EXPECT((oopt_dm_list({c[1], c[0], c[1]}) == std::vector<float>{20.f, 30.5f}));
  EXPECT(throws_with([&] { oopt_dm_list({c[0], cand(0.01, 63, 0, 0, -2.f)}); }, "candidate 1"));

  OrbOptFileHeader h;
  h.ncand = 1;
  h.nints = 2;
  h.nbins = 8;
  h.npb = h.na1 = h.nphase = 1;
  h.np = 3;
  h.nw = 3;
  h.n = 1000;
  h.tsamp = 320e-6;
  h.p_step = 1.0;
  OrbOptResult r;
  r.search.best_val = {1, 2, 3};
  r.search.best_idx = {4, 5, 6};
  r.search.centre = {7, 8, 9};
  r.search.tcurve = {1, 2, 3};
  r.search.msum = {-5};
  r.hits.assign(16, 1);
  r.fold.assign(16, 2);
  r.profile.assign(8, 3);
  const std::vector<char> b = oopt_file_bytes(h, {r});
  EXPECT(b.size() == 64 + 160 + 4 * (3 + 3 + 3 + 3) + 8 + 4 * (16 + 16 + 8));
  EXPECT(std::memcmp(b.data(), "PSOOPT01", 8) == 0);
  r.profile.resize(7);
  EXPECT(throws_with([&] { oopt_file_bytes(h, {r}); }, "wrong shape"));
}

void test_cli() {
  OrbOptCmdLineOptions a;
  EXPECT(parse_oopt_cmdline(a, {"orbopt", "-i", "x.fil", "-c", "c.txt"}));
  EXPECT(a.nbins == 64 && a.nints == 16 && a.npb == 9 && a.na1 == 9 && a.nphase == 9 && a.np == 33 && a.p_step == 1.0 &&
         a.limit == 100 && a.size == 0 && a.pb_step == 0.0 && !a.verbose);
  EXPECT(a.outfilename.size() > 12 && a.outfilename.substr(a.outfilename.size() - 12) == "_orbopt.oopt");
  OrbOptCmdLineOptions b;
  EXPECT(parse_oopt_cmdline(b, {"orbopt", "-i", "x.fil", "-c", "c.txt", "-o", "o", "--nbins", "7", "--nints", "3", "--npb",
                                "5", "--na1", "3", "--nphase", "1", "--np", "17", "--p_step", "0.5", "--pb_step", "0.25",
                                "--a1_step", "1e-4", "--phase_step", "0.01", "--limit", "4", "--fft_size", "65536", "-v"}));
  EXPECT(b.outfilename == "o" && b.nbins == 7 && b.nints == 3 && b.npb == 5 && b.na1 == 3 && b.nphase == 1 && b.np == 17 &&
         b.p_step == 0.5 && b.pb_step == 0.25 && b.a1_step == 1e-4 && b.phase_step == 0.01 && b.limit == 4 &&
         b.size == 65536 && b.verbose);
  const OrbOptParams p = oopt_params_of(b);
  EXPECT(p.nbins == 7 && p.np == 17 && p.pb_step == 0.25);
  OrbOptCmdLineOptions c;
  EXPECT(!parse_oopt_cmdline(c, {"orbopt", "-i", "x.fil"}));                           // no candidates
  EXPECT(!parse_oopt_cmdline(c, {"orbopt", "-i", "x.fil", "-c", "c", "-t", "2"}));      // one device
  EXPECT(!parse_oopt_cmdline(c, {"orbopt", "-i", "x.fil", "-c", "c", "--limit", "-1"}));
  EXPECT(!parse_oopt_cmdline(c, {"orbopt", "-i", "x.fil", "-c", "c", "--p_step", "1x"}));
  bool exit_now = false;
  EXPECT(parse_oopt_cmdline(c, {"orbopt", "--help"}, &exit_now) && exit_now);
}

}  // namespace

int main() {
  test_params();
  test_grid();
  test_hits_moments_drift();
  test_fold_and_search();
  test_parser_and_file();
  test_cli();
  std::cout << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
