// Host unit tests of sbsearch's host steps (psoup/sideband.hpp): the segment
// geometry at its edges, the window ownership, the radix plan and the
// digit-reversed read-out, the host transcription of the search against a
// direct double DFT at every size (combs, the pairing, the clip, ties), the
// powers and their fixed summation order, the clustering on hand-made events,
// every refusal by name, the conversions and the command line.  No GPU.  Exit
// status 0 = all passed.
#include <cmath>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "psoup/sideband.hpp"

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

SbGeometry band(int64_t k_lo, int64_t k_hi, int m_lo = 5, int m_hi = 13) {
  SbGeometry g;
  g.k_lo = k_lo;
  g.k_hi = k_hi;
  g.m_lo = m_lo;
  g.m_hi = m_hi;
  for (int m = m_lo; m <= m_hi; ++m) {
    const int64_t n = sb_nseg(k_hi - k_lo, m);
    g.nseg.push_back(n);
    g.seg_stride = std::max(g.seg_stride, n);
    if (n > 0) g.nwin = std::max<int64_t>(g.nwin, (n - 1) / sbk::owned(m) + 1);
  }
  return g;
}

std::vector<float> noise(size_t n, unsigned seed) {  // exponential, mean 1
  std::vector<float> x(n);
  uint32_t z = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    z = z * 1664525u + 1013904223u;
    const double u = (static_cast<double>(z >> 8) + 0.5) / 16777216.0;
    x[i] = static_cast<float>(-std::log(u));
  }
  return x;
}

// The definition's S_j of one segment, in double.
std::vector<double> direct(const float* P, int M, float clip) {
  std::vector<double> S(static_cast<size_t>(M / 2), 0.0);
  for (int j = 0; j < M / 2; ++j) {
    double re = 0.0, im = 0.0;
    for (int i = 0; i < M; ++i) {
      const double x = static_cast<double>(std::fmin(P[i], clip)) - 1.0;
      const double a = -2.0 * M_PI * static_cast<double>((static_cast<int64_t>(i) * j) % M) / M;
      re += x * std::cos(a);
      im += x * std::sin(a);
    }
    S[static_cast<size_t>(j)] = (re * re + im * im) / M;
  }
  return S;
}

void test_geometry() {
  for (int m = 5; m <= 13; ++m) {
    const int64_t M = int64_t(1) << m;
    EXPECT(sb_nseg(M - 1, m) == 0 && sb_nseg(M, m) == 1 && sb_nseg(M + M / 2 - 1, m) == 1 &&
           sb_nseg(M + M / 2, m) == 2 && sb_nseg(0, m) == 0);
  }
  const SbGeometry g = sb_geometry(0.1f, 1100.f, 1u << 17, 0.001f, 5, 13);
  const double T = 131072.0 * static_cast<double>(0.001f);
  EXPECT(g.tobs == T && g.k_lo == static_cast<int64_t>(std::ceil(static_cast<double>(0.1f) * T)) && g.k_hi == 65536);
  EXPECT(g.nseg.size() == 9 && g.nsegs_of(5) == sb_nseg(g.k_hi - g.k_lo, 5) && g.seg_stride == g.nsegs_of(5));
  // the windows own every segment and hold it whole
  for (int64_t b : {int64_t(31), int64_t(32), int64_t(4096), int64_t(8191), int64_t(8192), int64_t(3 * 8192 + 4096 + 611)}) {
    const SbGeometry h = band(37, 37 + b);
    for (int m = 5; m <= 13; ++m) {
      const int64_t n = h.nsegs_of(m), M = int64_t(1) << m;
      if (n == 0) continue;
      const int64_t last = (n - 1) * (M / 2);
      const int64_t w = (n - 1) / sbk::owned(m);
      EXPECT(w < h.nwin && last >= w * kSbHop && last + M <= w * kSbHop + kSbWindow && last + M <= b);
    }
    EXPECT((b < 32) == (h.nwin == 0));
  }
}

void test_plan() {
  for (int m = 5; m <= 13; ++m) {
    int r[5];
    const int nst = sbk::radices(m, r);
    int prod = 1;
    for (int s = 0; s < nst; ++s) prod *= r[s];
    EXPECT(prod == (1 << m) && nst <= 5);
    std::vector<int> seen(static_cast<size_t>(1 << m), 0);
    for (int j = 0; j < (1 << m); ++j) ++seen[static_cast<size_t>(sbk::position(j, m, r, nst))];
    bool perm = true;
    for (int v : seen) perm = perm && v == 1;
    EXPECT(perm);
    EXPECT(sbk::points(m) % (8 * kern::kSbThreads) == 0 || sbk::points(m) / 8 == kern::kSbThreads);
  }
  const std::vector<float2> tw = sb_twiddles();
  EXPECT(tw.size() == 8192 && tw[0].x == 1.f && tw[2048].y == -1.f && tw[4096].x == -1.f && tw[1024].x == -tw[1024].y);
  float S;
  int j;
  sbk::key_split(sbk::key_of(53.5f, 64), &S, &j);
  EXPECT(S == 53.5f && j == 64 && sbk::key_of(2.f, 9) > sbk::key_of(1.f, 3) && sbk::key_of(2.f, 3) > sbk::key_of(2.f, 9));
}

void test_search_against_direct() {
  // an unaligned head, two windows and a bit, every size; all segments of the small band against the direct DFT
  const int64_t k_lo = 37, b = 8192 + 4096 + 611, stride = 12960;
  std::vector<float> P = noise(static_cast<size_t>(stride), 7);
  for (int64_t k = 0; k < stride; ++k)
    if (k < k_lo || k >= k_lo + b) P[static_cast<size_t>(k)] = std::numeric_limits<float>::quiet_NaN();
  P[static_cast<size_t>(k_lo + 5000)] = 1.0e6f;  // clipped
  const SbGeometry g = band(k_lo, k_lo + b);
  SbParams p;
  p.min_power = 12.f;
  const size_t nm = 9, ss = static_cast<size_t>(g.seg_stride);
  std::vector<float> bs(nm * ss, -1.f);
  std::vector<int32_t> bj(nm * ss, -1);
  std::vector<SbEvent> ev;
  sb_search_host(P.data(), static_cast<uint64_t>(stride), 1, g, p, 3, bs.data(), bj.data(), &ev);
  size_t events = 0;
  for (int m = 5; m <= 13; ++m) {
    const int M = 1 << m;
    const int64_t n = g.nsegs_of(m);
    EXPECT(n == sb_nseg(b, m));
    const int64_t step = m <= 7 ? 37 : 1;  // a sample of the many small segments, the ends included
    for (int64_t s = 0; s < n; s += (s + step < n || s == n - 1) ? step : n - 1 - s) {
      const std::vector<double> S = direct(P.data() + k_lo + s * (M / 2), M, p.clip);
      int best = p.j_min;
      for (int j = p.j_min; j < M / 2; ++j)
        if (S[static_cast<size_t>(j)] > S[static_cast<size_t>(best)]) best = j;
      double norm = 0.0;
      for (int i = 0; i < M; ++i) {
        const double x = static_cast<double>(std::fmin(P[static_cast<size_t>(k_lo + s * (M / 2) + i)], p.clip)) - 1.0;
        norm += x * x;
      }
      const double t = 16.0 * std::ldexp(1.0, -24) * m * std::sqrt(norm);
      const size_t o = static_cast<size_t>(m - 5) * ss + static_cast<size_t>(s);
      const int j = bj[o];
      EXPECT(j >= p.j_min && j < M / 2);
      if (j < p.j_min || j >= M / 2) continue;
      const double F = std::sqrt(S[static_cast<size_t>(j)] * M);
      EXPECT(std::fabs(static_cast<double>(bs[o]) - S[static_cast<size_t>(j)]) <= (2.0 * F * t + t * t) / M);
      // the winner is the direct one unless the two are within the bound
      const double Fb = std::sqrt(S[static_cast<size_t>(best)] * M);
      EXPECT(j == best || S[static_cast<size_t>(best)] - S[static_cast<size_t>(j)] <= 2.0 * (2.0 * Fb * t + t * t) / M);
    }
    for (int64_t s = 0; s < n; ++s) events += bs[static_cast<size_t>(m - 5) * ss + static_cast<size_t>(s)] >= p.min_power;
    for (int64_t s = n; s < g.seg_stride; ++s) EXPECT(bs[static_cast<size_t>(m - 5) * ss + static_cast<size_t>(s)] == -1.f);
  }
  EXPECT(ev.size() == events);
  for (const SbEvent& e : ev) {
    const size_t o = static_cast<size_t>(e.m - 5) * ss + static_cast<size_t>(e.seg);
    EXPECT(e.dm_idx == 3 && e.S == bs[o] && e.j == bj[o] && e.S >= p.min_power);
  }
}

void test_combs_and_edges() {
  // x_i = A cos(2 pi j0 i / M) on P = 1: S_j0 = A^2 M / 4; the first segment, the last one and the last a window owns
  for (int m = 5; m <= 13; ++m) {
    const int M = 1 << m;
    const int64_t b = 2 * 8192 + 4096, k_lo = 3;
    const SbGeometry g = band(k_lo, k_lo + b, m, m);
    const int64_t n = g.nsegs_of(m);
    const int64_t owned_last = (m == 13) ? 1 : (4096 - M / 2) / (M / 2);
    for (int64_t seg : {int64_t(0), n - 1, owned_last})
      for (int j0 : {2, M / 2 - 1}) {
        std::vector<float> P(static_cast<size_t>(k_lo + b + 1), 1.0f);
        const double A = 0.5;
        for (int i = 0; i < M; ++i)
          P[static_cast<size_t>(k_lo + seg * (M / 2) + i)] =
              static_cast<float>(1.0 + A * std::cos(2.0 * M_PI * static_cast<double>((static_cast<int64_t>(j0) * i) % M) / M));
        SbParams p;
        p.m_lo = p.m_hi = m;
        std::vector<float> bs(static_cast<size_t>(g.seg_stride), -1.f);
        std::vector<int32_t> bj(static_cast<size_t>(g.seg_stride), -1);
        sb_search_host(P.data(), P.size(), 1, g, p, 0, bs.data(), bj.data(), nullptr);
        const double want = A * A * M / 4.0;
        EXPECT(bj[static_cast<size_t>(seg)] == j0);
        EXPECT(std::fabs(static_cast<double>(bs[static_cast<size_t>(seg)]) - want) <= 1e-4 * want);
      }
  }
  // a band of exactly M bins: one segment; of M - 1: none, nothing written; j_min = M/2 - 1: one admissible j
  const std::vector<float> P = noise(64, 3);
  SbParams p;
  p.m_lo = p.m_hi = 5;
  p.j_min = 15;
  p.min_power = 0.f;
  float bs[2] = {-1.f, -1.f};
  int32_t bj[2] = {-1, -1};
  std::vector<SbEvent> ev;
  SbGeometry g = band(7, 39, 5, 5);
  g.seg_stride = 1;
  sb_search_host(P.data(), 64, 1, g, p, 0, bs, bj, &ev);
  EXPECT(g.nsegs_of(5) == 1 && g.nwin == 1 && bj[0] == 15 && bs[0] >= 0.f && bs[1] == -1.f && ev.size() == 1);
  bs[0] = -1.f;
  ev.clear();
  SbGeometry h = band(7, 38, 5, 5);
  h.seg_stride = 1;
  sb_search_host(P.data(), 64, 1, h, p, 0, bs, bj, &ev);
  EXPECT(h.nsegs_of(5) == 0 && h.nwin == 0 && bs[0] == -1.f && ev.empty());
  // a flat segment: every S is 0 and the lowest admissible j wins the tie
  std::vector<float> flat(64, 1.0f);
  p.j_min = 2;
  sb_search_host(flat.data(), 64, 1, g, p, 0, bs, bj, nullptr);
  EXPECT(bs[0] == 0.f && bj[0] == 2);
}

void test_power() {
  const int64_t k_lo = 11, k_hi = 11 + 4096 + 777;
  const uint64_t nb = 5000;
  std::vector<float> re = noise(2 * nb, 1), im = noise(2 * nb, 2);
  std::vector<float2> spec(2 * nb);
  for (size_t i = 0; i < spec.size(); ++i) spec[i] = make_float2(re[i] - 1.f, im[i] - 1.f);
  std::vector<uint32_t> mask((nb + 31) / 32, 0u);
  for (int64_t k = 100; k < 140; ++k) mask[static_cast<size_t>(k >> 5)] |= 1u << (k & 31);
  mask[0] |= 1u;  // outside the band
  EXPECT(sb_unzapped(mask, k_lo, k_hi) == static_cast<uint64_t>(k_hi - k_lo - 40) && sb_unzapped({}, k_lo, k_hi) == 4873);
  std::vector<double> mu(2);
  std::vector<float> P(2 * nb, -5.f);
  sb_power_host(spec.data(), nb, 2, mask, k_lo, k_hi, mu.data(), P.data(), nb);
  for (int r = 0; r < 2; ++r) {
    long double sum = 0;
    for (int64_t k = k_lo; k < k_hi; ++k)
      if (k < 100 || k >= 140) {
        const float2 v = spec[static_cast<size_t>(r) * nb + static_cast<size_t>(k)];
        sum += static_cast<long double>(v.x) * v.x + static_cast<long double>(v.y) * v.y;
      }
    const double want = static_cast<double>(sum / (k_hi - k_lo - 40));
    EXPECT(std::fabs(mu[static_cast<size_t>(r)] - want) <= 1e-12 * want);
    bool ok = P[static_cast<size_t>(r) * nb + 10] == -5.f && P[static_cast<size_t>(r) * nb + static_cast<size_t>(k_hi)] == -5.f;
    double mean = 0.0;
    for (int64_t k = k_lo; k < k_hi; ++k) {
      const float v = P[static_cast<size_t>(r) * nb + static_cast<size_t>(k)];
      if (k >= 100 && k < 140) ok = ok && v == 1.0f;
      else mean += v;
    }
    EXPECT(ok && std::fabs(mean / (k_hi - k_lo - 40) - 1.0) < 1e-6);
  }
  EXPECT(throws_with([&] {
    std::vector<uint32_t> all((nb + 31) / 32, 0xFFFFFFFFu);
    sb_power_host(spec.data(), nb, 1, all, k_lo, k_hi, mu.data(), P.data(), nb);
  }, "no unzapped bin"));
}

void test_cluster() {
  auto E = [](int dm, int m, int seg, int j, float S) { return SbEvent{dm, m, seg, j, S}; };
  // the issue's example: M = 1024 j = 64 and its third harmonic at M = 2048 (j = 384), overlapping, other DMs
  {
    const auto c = sb_cluster({E(2, 11, 24, 384, 40.f), E(1, 10, 48, 64, 53.f), E(3, 10, 49, 64, 35.f), E(0, 10, 48, 65, 31.f)});
    EXPECT(c.size() == 1 && c[0].ev.m == 10 && c[0].ev.j == 64 && c[0].ev.dm_idx == 1 && c[0].members == 4 &&
           c[0].dm_lo == 0 && c[0].dm_hi == 3);
  }
  // no overlap: |c - c0| = (M + M0) / 2 still overlaps, one more half segment does not
  {
    const auto a = sb_cluster({E(0, 10, 10, 64, 50.f), E(0, 10, 12, 64, 40.f)});
    const auto b = sb_cluster({E(0, 10, 10, 64, 50.f), E(0, 10, 13, 64, 40.f)});
    EXPECT(a.size() == 1 && b.size() == 2 && b[0].ev.S == 50.f && b[1].members == 1);
  }
  // the harmonic relations r = 1..4 both ways, and r = 5 neither way (same size: |r j - j0| <= r + 1)
  for (int r = 1; r <= 5; ++r) {
    const auto up = sb_cluster({E(0, 12, 0, 40, 50.f), E(0, 12, 0, 40 * r, 40.f)});
    const auto down = sb_cluster({E(0, 12, 0, 40 * r, 50.f), E(0, 12, 0, 40, 40.f)});
    EXPECT(up.size() == (r <= 4 ? 1u : 2u) && down.size() == (r <= 4 ? 1u : 2u));
  }
  // the tolerance: r j within r + 1 of j0 at equal sizes
  EXPECT(sb_cluster({E(0, 12, 0, 400, 50.f), E(0, 12, 0, 402, 40.f)}).size() == 1);
  EXPECT(sb_cluster({E(0, 12, 0, 400, 50.f), E(0, 12, 0, 403, 40.f)}).size() == 2);
  EXPECT(sb_cluster({E(0, 12, 0, 400, 50.f), E(0, 12, 0, 201, 40.f)}).size() == 1);   // |2 x 201 - 400| = 2 <= 3
  EXPECT(sb_cluster({E(0, 12, 0, 401, 50.f), E(0, 12, 0, 199, 40.f)}).size() == 1);   // |2 x 199 - 401| = 3 <= 3
  EXPECT(sb_cluster({E(0, 12, 0, 1001, 50.f), E(0, 12, 0, 337, 40.f)}).size() == 2);  // r = 3: 10 > 4; no other r
  // ties in S: dm_idx, then m, then seg decide who leads; absorbed by the FIRST accepted candidate that fits
  {
    const auto c = sb_cluster({E(5, 10, 3, 64, 40.f), E(4, 10, 3, 64, 40.f), E(4, 9, 6, 32, 40.f), E(4, 9, 5, 32, 40.f)});
    EXPECT(c.size() == 1 && c[0].ev.dm_idx == 4 && c[0].ev.m == 9 && c[0].ev.seg == 5 && c[0].members == 4 &&
           c[0].dm_lo == 4 && c[0].dm_hi == 5);
    const auto d = sb_cluster({E(0, 10, 0, 100, 60.f), E(0, 10, 0, 300, 50.f), E(0, 10, 0, 299, 45.f)});
    EXPECT(d.size() == 1 && d[0].members == 3);
    const auto e = sb_cluster({E(0, 10, 0, 100, 60.f), E(0, 10, 0, 107, 50.f), E(0, 10, 0, 214, 45.f)});
    EXPECT(e.size() == 2 && e[0].members == 1 && e[1].members == 2 && e[1].ev.j == 107);
  }
  EXPECT(sb_cluster({}).empty());
}

void test_refusals_and_values() {
  SbParams p;
  const uint64_t n = 1u << 17;
  sb_check(p, 0.1f, 1100.f, n, 0.001f);
  EXPECT(throws_with([&] { sb_check(p, 0.1f, 1100.f, (1ull << 26) + 2, 0.001f); }, "above 2^26"));
  auto with = [&](int lo, int hi, int jm, float clip) {
    SbParams q;
    q.m_lo = lo; q.m_hi = hi; q.j_min = jm; q.clip = clip;
    return q;
  };
  EXPECT(throws_with([&] { sb_check(with(4, 13, 2, 32.f), 0.1f, 1100.f, n, 0.001f); }, "m_min is below 5"));
  EXPECT(throws_with([&] { sb_check(with(5, 14, 2, 32.f), 0.1f, 1100.f, n, 0.001f); }, "m_max is above 13"));
  EXPECT(throws_with([&] { sb_check(with(9, 8, 2, 32.f), 0.1f, 1100.f, n, 0.001f); }, "m_min is above m_max"));
  EXPECT(throws_with([&] { sb_check(with(5, 13, 0, 32.f), 0.1f, 1100.f, n, 0.001f); }, "j_min is outside"));
  EXPECT(throws_with([&] { sb_check(with(5, 13, 16, 32.f), 0.1f, 1100.f, n, 0.001f); }, "j_min is outside"));
  sb_check(with(5, 13, 15, 32.f), 0.1f, 1100.f, n, 0.001f);
  sb_check(with(6, 13, 31, 32.f), 0.1f, 1100.f, n, 0.001f);
  EXPECT(throws_with([&] { sb_check(with(5, 13, 2, 1.0f), 0.1f, 1100.f, n, 0.001f); }, "clip must be above 1"));
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  EXPECT(throws_with([&] { sb_check(with(5, 13, 2, inf), 0.1f, 1100.f, n, 0.001f); }, "non-finite"));
  EXPECT(throws_with([&] { sb_check(p, nan, 1100.f, n, 0.001f); }, "non-finite"));
  EXPECT(throws_with([&] { sb_check(p, 0.1f, inf, n, 0.001f); }, "non-finite"));
  // 10 Hz .. 10.2 Hz of 131 s: 26 bins
  EXPECT(throws_with([&] { sb_check(p, 10.f, 10.2f, n, 0.001f); }, "shorter than 2^m_min"));
  sb_check(p, 10.f, 10.3f, n, 0.001f);
  EXPECT(throws_with([&] { sb_check(p, 20.f, 10.f, n, 0.001f); }, "shorter than 2^m_min"));

  const SbGeometry g = sb_geometry(0.1f, 1100.f, n, 0.001f, 5, 13);
  const SbEvent e{2, 10, 11, 64, 53.f};
  EXPECT(sb_event_pb(g, e) == 64.0 * g.tobs / 1024.0 && sb_event_pb_res(g, e) == g.tobs / 1024.0);
  EXPECT(sb_event_freq(g, e) == static_cast<double>(g.k_lo + 11 * 512 + 512) / g.tobs &&
         sb_event_freq_half_width(g, e) == 512.0 / g.tobs);
}

void test_cmdline() {
  SbCmdLineOptions a;
  bool exit_now = false;
  EXPECT(parse_sb_cmdline(a, {"sbsearch", "-i", "x.fil"}, &exit_now) && !exit_now);
  EXPECT(a.search.infilename == "x.fil" && a.min_power == 30.f && a.m_min == 5 && a.m_max == 13 && a.j_min == 2 &&
         a.clip == 32.f && a.search.max_num_threads == 1 && a.search.min_freq == 0.1f && a.search.max_freq == 1100.f &&
         a.search.dm_end == 100.f && a.search.limit == 1000 && a.outfilename.find("_sbsearch.output") != std::string::npos);
  SbCmdLineOptions b;
  EXPECT(parse_sb_cmdline(b, {"sbsearch", "-i", "x.fil", "-o", "o.txt", "--min_power", "25", "--m_min", "6", "--m_max",
                              "12", "--j_min", "3", "--clip", "1e9", "--min_freq", "1", "--max_freq", "400",
                              "--dm_start", "5", "--dm_end", "9", "--fft_size", "65536", "--limit", "7", "-z", "z.txt",
                              "-k", "k.txt", "--dedisp_kernel", "direct", "-v"}));
  EXPECT(b.outfilename == "o.txt" && b.min_power == 25.f && b.m_min == 6 && b.m_max == 12 && b.j_min == 3 &&
         b.clip == 1e9f && b.search.min_freq == 1.f && b.search.max_freq == 400.f && b.search.dm_start == 5.f &&
         b.search.dm_end == 9.f && b.search.size == 65536u && b.search.limit == 7 && b.search.zapfilename == "z.txt" &&
         b.search.killfilename == "k.txt" && b.search.dedisp_kernel == "direct" && b.search.verbose);
  SbCmdLineOptions c;
  EXPECT(parse_sb_cmdline(c, {"sbsearch", "-i", "x.fil", "--clip", "inf"}) && std::isinf(c.clip));  // refused by the setup
  SbCmdLineOptions d;
  EXPECT(!parse_sb_cmdline(d, {"sbsearch", "-i", "x.fil", "-t", "2"}));
  EXPECT(!parse_sb_cmdline(d, {"sbsearch"}));
  EXPECT(!parse_sb_cmdline(d, {"sbsearch", "-i", "x.fil", "--acc_start", "1"}));
  EXPECT(!parse_sb_cmdline(d, {"sbsearch", "-i", "x.fil", "--clip", "abc"}));
}

}  // namespace

int main() {
  test_geometry();
  test_plan();
  test_search_against_direct();
  test_combs_and_edges();
  test_power();
  test_cluster();
  test_refusals_and_values();
  test_cmdline();
  if (g_failed) {
    std::cerr << g_failed << " check(s) failed" << std::endl;
    return 1;
  }
  std::cout << "sideband unit tests: all passed" << std::endl;
  return 0;
}
