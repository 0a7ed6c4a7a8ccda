// sbsearch, host side: the geometry, the checks, the clustering, the
// conversions, the host transcriptions of sb_power and sb_search and the output
// text.  No device code.  See psoup/sideband.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <sstream>

#include "psoup/sideband.hpp"

namespace psoup {

// ------------------------------------------------------------- geometry ----
int64_t sb_nseg(int64_t band, int m) {
  const int64_t M = int64_t(1) << m;
  if (band < M) return 0;
  return (band - M) / (M / 2) + 1;
}

SbGeometry sb_geometry(float min_freq, float max_freq, uint64_t fft_size, float tsamp, int m_lo, int m_hi) {
  SbGeometry g;
  g.fft_size = fft_size;
  g.tobs = static_cast<double>(fft_size) * static_cast<double>(tsamp);
  g.m_lo = m_lo;
  g.m_hi = m_hi;
  const double lo = std::ceil(static_cast<double>(min_freq) * g.tobs);
  const double hi = std::floor(static_cast<double>(max_freq) * g.tobs);
  const double top = static_cast<double>(fft_size / 2);
  g.k_lo = static_cast<int64_t>(std::min(std::max(lo, 0.0), top));
  g.k_hi = static_cast<int64_t>(std::min(std::max(hi, 0.0), top));
  if (g.k_hi < g.k_lo) g.k_hi = g.k_lo;
  const int64_t band = g.k_hi - g.k_lo;
  g.nranges = static_cast<int>((band + kSbRange - 1) / kSbRange);
  for (int m = m_lo; m <= m_hi; ++m) {
    const int64_t n = sb_nseg(band, m);
    g.nseg.push_back(n);
    g.seg_stride = std::max(g.seg_stride, n);
    if (n > 0) g.nwin = std::max<int64_t>(g.nwin, (n - 1) / sbk::owned(m) + 1);
  }
  return g;
}

void sb_check(const SbParams& p, float min_freq, float max_freq, uint64_t fft_size, float tsamp) {
  PSOUP_CHECK(std::isfinite(min_freq) && std::isfinite(max_freq) && std::isfinite(tsamp) && std::isfinite(p.clip) &&
                  std::isfinite(p.min_power),
              "sideband: a non-finite value");
  PSOUP_CHECK(tsamp > 0.f && min_freq >= 0.f, "sideband: tsamp must be positive and min_freq non-negative");
  PSOUP_CHECK(fft_size >= 2 && fft_size <= kSbMaxSpan, "sideband: the span is above 2^26 samples (or below 2)");
  PSOUP_CHECK(p.m_lo >= kSbMinM, "sideband: m_min is below 5");
  PSOUP_CHECK(p.m_hi <= kSbMaxM, "sideband: m_max is above 13");
  PSOUP_CHECK(p.m_lo <= p.m_hi, "sideband: m_min is above m_max");
  PSOUP_CHECK(p.j_min >= 1 && p.j_min < (1 << p.m_lo) / 2, "sideband: j_min is outside [1, 2^m_min / 2)");
  PSOUP_CHECK(p.clip > 1.0f, "sideband: clip must be above 1");
  const SbGeometry g = sb_geometry(min_freq, max_freq, fft_size, tsamp, p.m_lo, p.m_hi);
  PSOUP_CHECK(g.k_hi - g.k_lo >= (int64_t(1) << p.m_lo),
              "sideband: the band [k_lo, k_hi) = [" << g.k_lo << ", " << g.k_hi << ") is shorter than 2^m_min");
}

uint64_t sb_unzapped(const std::vector<uint32_t>& mask, int64_t k_lo, int64_t k_hi) {
  uint64_t n = 0;
  for (int64_t k = k_lo; k < k_hi; ++k) {
    const size_t w = static_cast<size_t>(k >> 5);
    const bool z = w < mask.size() && ((mask[w] >> (k & 31)) & 1u) != 0;
    n += z ? 0 : 1;
  }
  return n;
}

std::vector<float2> sb_twiddles() {
  std::vector<float2> t(static_cast<size_t>(kSbTwiddles));
  for (int k = 0; k < kSbTwiddles; ++k) {
    const double a = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(kSbTwiddles);
    t[static_cast<size_t>(k)] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
  }
  // the quarter turns exactly
  t[0] = make_float2(1.f, 0.f);
  t[kSbTwiddles / 4] = make_float2(0.f, -1.f);
  t[kSbTwiddles / 2] = make_float2(-1.f, 0.f);
  t[3 * kSbTwiddles / 4] = make_float2(0.f, 1.f);
  return t;
}

// ---------------------------------------------------------- conversions ----
double sb_event_freq(const SbGeometry& g, const SbEvent& e) {
  const int64_t half = int64_t(1) << (e.m - 1);
  return static_cast<double>(g.k_lo + static_cast<int64_t>(e.seg) * half + half) / g.tobs;
}
double sb_event_freq_half_width(const SbGeometry& g, const SbEvent& e) {
  return static_cast<double>(int64_t(1) << (e.m - 1)) / g.tobs;
}
double sb_event_pb(const SbGeometry& g, const SbEvent& e) {
  return static_cast<double>(e.j) * g.tobs / static_cast<double>(int64_t(1) << e.m);
}
double sb_event_pb_res(const SbGeometry& g, const SbEvent& e) {
  return g.tobs / static_cast<double>(int64_t(1) << e.m);
}

// ------------------------------------------------------------ clustering ----
namespace {
bool sb_related(const SbEvent& e, const SbEvent& c0) {
  const int64_t M = int64_t(1) << e.m, M0 = int64_t(1) << c0.m;
  const int64_t c = static_cast<int64_t>(e.seg) * (M / 2) + M / 2;
  const int64_t cc = static_cast<int64_t>(c0.seg) * (M0 / 2) + M0 / 2;
  if (std::llabs(c - cc) > (M + M0) / 2) return false;
  const int64_t j = e.j, j0 = c0.j;
  for (int64_t r = 1; r <= 4; ++r) {
    if (std::llabs(r * j * M0 - j0 * M) <= r * M0 + M) return true;
    if (std::llabs(j * M0 - r * j0 * M) <= M0 + r * M) return true;
  }
  return false;
}
}  // namespace

std::vector<SbCandidate> sb_cluster(std::vector<SbEvent> events) {
  for (const SbEvent& e : events)
    PSOUP_CHECK(e.m >= 1 && e.m <= 30 && e.seg >= 0 && e.j >= 0, "sb_cluster: an event outside the definition");
  std::sort(events.begin(), events.end(), [](const SbEvent& a, const SbEvent& b) {
    if (a.S != b.S) return a.S > b.S;
    if (a.dm_idx != b.dm_idx) return a.dm_idx < b.dm_idx;
    if (a.m != b.m) return a.m < b.m;
    return a.seg < b.seg;
  });
  std::vector<SbCandidate> out;
  for (const SbEvent& e : events) {
    bool absorbed = false;
    for (SbCandidate& c : out) {
      if (!sb_related(e, c.ev)) continue;
      ++c.members;
      c.dm_lo = std::min(c.dm_lo, e.dm_idx);
      c.dm_hi = std::max(c.dm_hi, e.dm_idx);
      absorbed = true;
      break;
    }
    if (!absorbed) out.push_back(SbCandidate{e, 1, e.dm_idx, e.dm_idx});
  }
  return out;
}

// --------------------------------------------------- host transcriptions ----
void sb_power_host(const float2* spec, uint64_t spec_stride, int nrows, const std::vector<uint32_t>& zapmask,
                   int64_t k_lo, int64_t k_hi, double* mu, float* P, uint64_t stride) {
  PSOUP_CHECK(k_lo >= 0 && k_lo < k_hi && static_cast<uint64_t>(k_hi) <= spec_stride &&
                  static_cast<uint64_t>(k_hi) <= stride,
              "sb_power: the band is empty or passes a row");
  auto zapped = [&](int64_t k) {
    const size_t w = static_cast<size_t>(k >> 5);
    return w < zapmask.size() && ((zapmask[w] >> (k & 31)) & 1u) != 0;
  };
  auto power = [](float2 v) {
    return static_cast<double>(v.x) * static_cast<double>(v.x) + static_cast<double>(v.y) * static_cast<double>(v.y);
  };
  const uint64_t count = sb_unzapped(zapmask, k_lo, k_hi);
  PSOUP_CHECK(count >= 1, "sideband: the band has no unzapped bin");
  const int64_t band = k_hi - k_lo;
  const int nranges = static_cast<int>((band + kSbRange - 1) / kSbRange);
  for (int r = 0; r < nrows; ++r) {
    const float2* row = spec + static_cast<uint64_t>(r) * spec_stride;
    double sum = 0.0;
    for (int q = 0; q < nranges; ++q) {
      double a[kSbRangeLanes];
      for (int t = 0; t < kSbRangeLanes; ++t) {
        double acc = 0.0;
        for (int u = 0; u < kSbRange / kSbRangeLanes; ++u) {
          const int64_t k = k_lo + static_cast<int64_t>(q) * kSbRange + t + kSbRangeLanes * u;
          if (k < k_hi && !zapped(k)) acc += power(row[k]);
        }
        a[t] = acc;
      }
      for (int s = kSbRangeLanes / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) a[t] += a[t + s];
      sum += a[0];
    }
    mu[r] = sum / static_cast<double>(count);
    for (int64_t k = k_lo; k < k_hi; ++k)
      P[static_cast<uint64_t>(r) * stride + k] = zapped(k) ? 1.0f : static_cast<float>(power(row[k]) / mu[r]);
  }
}

void sb_search_host(const float* P, uint64_t stride, int nrows, const SbGeometry& g, const SbParams& p, int dm0,
                    float* best_S, int32_t* best_j, std::vector<SbEvent>* events) {
  PSOUP_CHECK(p.m_lo >= kSbMinM && p.m_hi <= kSbMaxM && p.m_lo <= p.m_hi && g.m_lo == p.m_lo && g.m_hi == p.m_hi,
              "sb_search: the sizes are outside 5..13 or not the geometry's");
  PSOUP_CHECK(p.j_min >= 1 && p.j_min < (1 << p.m_lo) / 2, "sb_search: j_min outside [1, 2^m_lo / 2)");
  PSOUP_CHECK(p.clip > 1.0f, "sb_search: clip must be above 1");
  PSOUP_CHECK(static_cast<uint64_t>(g.k_hi) <= stride, "sb_search: the band passes a row");
  const std::vector<float2> tw = sb_twiddles();
  std::vector<float> win(static_cast<size_t>(kSbWindow));
  std::vector<float2> buf(static_cast<size_t>(kSbWindow));
  std::vector<unsigned long long> segkey(static_cast<size_t>(kSbWindow >> kSbMinM));
  const int nm = p.m_hi - p.m_lo + 1;
  for (int row = 0; row < nrows; ++row)
    for (int w = 0; w < g.nwin; ++w) {
      const int64_t g0 = g.k_lo + static_cast<int64_t>(w) * kSbHop;
      const int64_t gend = std::min<int64_t>(g0 + kSbWindow, g.k_hi);
      const float* prow = P + static_cast<uint64_t>(row) * stride;
      bool hot = false;
      for (int i = 0; i < kSbWindow; ++i) {
        const float v = (g0 + i < gend) ? prow[g0 + i] : 1.0f;
        win[static_cast<size_t>(i)] = std::fmin(v, p.clip) - 1.0f;
        hot = hot || win[static_cast<size_t>(i)] > kSbPairLimit;
      }
      for (int m = p.m_lo; m <= p.m_hi; ++m) {
        const int nsl = sbk::owned(m);
        const int64_t nseg = g.nsegs_of(m), s0 = static_cast<int64_t>(w) * nsl;
        if (s0 >= nseg) continue;
        int r[5];
        const int nst = sbk::radices(m, r);
        const int npoints = sbk::points(m);
        std::fill(segkey.begin(), segkey.end(), 0ull);
        for (int ps = 0; ps < sbk::passes(m, hot); ++ps) {
        const int sel = sbk::pass_sel(m, hot, ps);
        for (int e = 0; e < npoints; ++e) buf[static_cast<size_t>(e)] = sbk::load_elem(win.data(), m, e, sel);
        int L = 1 << m;
        for (int s = 0; s < nst; ++s) {
          for (int b = 0; b < npoints / r[s]; ++b) {
            if (r[s] == 8) sbk::butterfly<8>(buf.data(), tw.data(), m, L, b);
            else if (r[s] == 4) sbk::butterfly<4>(buf.data(), tw.data(), m, L, b);
            else sbk::butterfly<2>(buf.data(), tw.data(), m, L, b);
          }
          L /= r[s];
        }
        const int half = 1 << (m - 1);
        const int nitems = (m == kSbMaxM) ? half : npoints / 2;
        for (int it = 0; it < nitems; ++it) {
          int c, j;
          float sa, sb;
          sbk::item(buf.data(), m, r, nst, it, &c, &j, &sa, &sb);
          if (j < p.j_min) continue;
          const size_t ia = (m == kSbMaxM) ? 0 : static_cast<size_t>(2 * c + (sel == 2 ? 1 : 0));
          segkey[ia] = std::max(segkey[ia], sbk::key_of(sa, j));
          if (m != kSbMaxM && sel == 0) segkey[ia + 1] = std::max(segkey[ia + 1], sbk::key_of(sb, j));
        }
        }  // passes
        for (int t = 0; t < nsl && s0 + t < nseg; ++t) {
          float S;
          int j;
          sbk::key_split(segkey[static_cast<size_t>(t)], &S, &j);
          const int64_t seg = s0 + t;
          if (best_S != nullptr) {
            const uint64_t o = (static_cast<uint64_t>(row) * nm + (m - p.m_lo)) * g.seg_stride + seg;
            best_S[o] = S;
            best_j[o] = j;
          }
          if (events != nullptr && S >= p.min_power)
            events->push_back(SbEvent{dm0 + row, m, static_cast<int32_t>(seg), j, S});
        }
      }
    }
}

// ---------------------------------------------------------------- output ----
std::string sb_output_text(const SbCmdLineOptions& args, const SbSetup& setup, const std::vector<SbCandidate>& cands) {
  const SbGeometry& g = setup.geom;
  std::ostringstream os;
  char line[512];
  os << "# sbsearch: sideband (phase-modulation) search\n";
  os << "# input " << args.search.infilename << "\n";
  std::snprintf(line, sizeof(line), "# fft_size %llu tsamp %.9g T %.9g\n", static_cast<unsigned long long>(g.fft_size),
                static_cast<double>(setup.search.search.tsamp), g.tobs);
  os << line;
  std::snprintf(line, sizeof(line), "# min_freq %.9g max_freq %.9g k_lo %lld k_hi %lld unzapped %llu\n",
                static_cast<double>(setup.search.search.min_freq), static_cast<double>(setup.search.search.max_freq),
                static_cast<long long>(g.k_lo), static_cast<long long>(g.k_hi),
                static_cast<unsigned long long>(setup.unzapped));
  os << line;
  std::snprintf(line, sizeof(line), "# min_power %.9g m_min %d m_max %d j_min %d clip %.9g\n",
                static_cast<double>(setup.params.min_power), setup.params.m_lo, setup.params.m_hi, setup.params.j_min,
                static_cast<double>(setup.params.clip));
  os << line;
  os << "# dm trials " << setup.search.dm_list.size() << "\n";
  for (int m = g.m_lo; m <= g.m_hi; ++m)
    os << "# M " << (1 << m) << " segments " << g.nsegs_of(m) << "\n";
  os << "# freq_hz freq_half_width_hz pb_s pb_res_s power M j dm dm_idx members dm_idx_lo dm_idx_hi\n";
  for (const SbCandidate& c : cands) {
    const SbEvent& e = c.ev;
    const size_t d = static_cast<size_t>(e.dm_idx);
    const double dm = d < setup.search.dm_list.size() ? static_cast<double>(setup.search.dm_list[d]) : 0.0;
    std::snprintf(line, sizeof(line), "%.9f %.9f %.9f %.9f %.4f %d %d %.6f %d %d %d %d\n", sb_event_freq(g, e),
                  sb_event_freq_half_width(g, e), sb_event_pb(g, e), sb_event_pb_res(g, e), static_cast<double>(e.S),
                  1 << e.m, e.j, dm, e.dm_idx, c.members, c.dm_lo, c.dm_hi);
    os << line;
  }
  return os.str();
}

}  // namespace psoup
