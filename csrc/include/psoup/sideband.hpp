// sbsearch: the sideband (phase-modulation) search for orbits shorter than the
// observation (Ransom, Cordes & Eikenberry 2003, section 4).  A pulsar whose
// orbit fits several times into the span T spreads its power over a comb of
// sidebands around bin f T, spaced T / pb bins apart; a short FFT of the
// *powers* of that stretch of spectrum peaks at j = M pb / T.  The kernels in
// csrc/kernels/sideband.hip, the host steps (geometry, checks, clustering, the
// conversions, a host transcription of both kernels, the output text) in
// csrc/src/sideband_host.cpp, SidebandSearcher and the file pipeline in
// csrc/src/sideband.cpp, CLI bin/sbsearch (csrc/apps/sb_main.cpp).
//
// Definition.  Per DM trial:
//
// 1. Series.  The dedispersed row goes through the Whitener (zap list applied)
//    and a forward real FFT of fft_size points: X[0 .. fft_size / 2].
//    T = (double)fft_size * (double)tsamp, tsamp the float32 the engine uses.
//
// 2. Powers.  k_lo = ceil((double)min_freq T), k_hi = min(floor((double)max_freq
//    T), fft_size / 2).  The power of a bin is p[k] = (double)re * re + (double)im
//    * im.  mu is the mean of p over the bins of [k_lo, k_hi) that are not
//    zapped, summed in double in a fixed order: the band is cut into ranges of
//    4096 bins from k_lo; in a range, lane t < 256 adds its bins k_lo + 4096 r +
//    t + 256 u, u = 0 .. 15 ascending, and the 256 lane sums are folded by
//    halving (a[t] += a[t + s], s = 128, 64 .. 1); the range sums are added in
//    ascending r by one thread, and divided by the count of bins summed.
//    P[k] = (float)(p[k] / mu); a zapped bin is exactly 1.
//
// 3. Secondary spectra.  For every m in [m_lo, m_hi] (5 and 13), M = 2^m, and
//    every segment s < nseg_m: the segment starts at bin k_lo + s M / 2,
//    nseg_m = floor((k_hi - k_lo - M) / (M / 2)) + 1, 0 when the band is
//    shorter than M.  x_i = min(P[start + i], clip) - 1, F_j = sum_i x_i
//    exp(-2 pi i i j / M), S_j = |F_j|^2 / M for j_min <= j < M / 2.
//
// 4. Event.  Per (DM, m, segment) the largest S_j, the lowest j on a tie, is
//    recorded as {dm_idx, m, seg, j, S} when S >= min_power.  It means: a
//    pulsar frequency within (start + M/2 +- M/2) / T, pb = j T / M to T / M.
//
// 5. Candidates (host).  Events sorted by descending S, ties by ascending
//    dm_idx, m, seg.  With c = seg M/2 + M/2 the segment centre (bins from
//    k_lo), an event is absorbed by the first accepted candidate (M0, c0, j0)
//    for which |c - c0| <= (M + M0) / 2 and, for some integer r in 1..4,
//        |r pb - pb0| <= r T/M + T/M0    or    |pb - r pb0| <= T/M + r T/M0.
//    The period conditions are evaluated exactly, multiplied through by
//    M M0 / T: |r j M0 - j0 M| <= r M0 + M or |j M0 - r j0 M| <= M0 + r M.
//    There is no DM condition; a candidate counts its members and keeps the
//    range of their dm_idx.  An event nobody absorbs becomes a candidate.
//
// Float arithmetic of the kernel (the tests bound it, they do not pin it): the
// twiddles exp(-2 pi i k / 8192) are computed in double on the host and rounded
// once; two real segments ride one complex transform (one by one in a window
// that holds an x above 64, sbk::passes); the butterflies are radix 8 with one
// leading radix-2 or radix-4 pass.
//
// Refused by name before any device work: a span fft_size above 2^26; m_lo < 5,
// m_hi > 13, m_lo > m_hi; j_min < 1 or j_min >= 2^m_lo / 2; clip <= 1; a
// non-finite value; a band [k_lo, k_hi) shorter than 2^m_lo; a band with no
// unzapped bin; -t other than 1.
//
// Caveats.  The segments are not windowed and j is whole: a peak between two j
// loses up to the usual scalloping.  The powers are normalised by one mean
// over the whole band, not locally.  clip lowers very bright sidebands (and
// keeps one interference bin from lifting every j of every size covering it).
// One device only: -t N, multi-rank runs and checkpoints are not supported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "psoup/cli.hpp"
#include "psoup/common.hpp"
#include "psoup/engine.hpp"
#include "psoup/pipeline.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// One event of the definition (20 bytes, the kernel's record).
struct SbEvent {
  int32_t dm_idx = 0;
  int32_t m = 0;
  int32_t seg = 0;
  int32_t j = 0;
  float S = 0.f;
};

constexpr int kSbMinM = 5, kSbMaxM = 13;
constexpr int kSbWindow = 1 << kSbMaxM;    // bins a workgroup stages
constexpr int kSbHop = kSbWindow / 2;      // bins between windows
constexpr int kSbTwiddles = kSbWindow;     // entries of the twiddle table
constexpr int kSbRange = 4096;             // bins per partial sum of mu
constexpr int kSbRangeLanes = 256;
constexpr float kSbPairLimit = 64.f;       // x above this in a window: its segments are transformed one by one
constexpr uint64_t kSbMaxSpan = 1ull << 26;

// ---- arithmetic shared by the kernel and its host transcription ----------
// (plain float operations; the host runs them one "thread" after the other)
namespace sbk {

// The radices of an M = 2^m point transform, the small one first; returns their count.
__host__ __device__ inline int radices(int m, int* r) {
  int n = 0;
  if (m % 3 == 1) r[n++] = 2;
  if (m % 3 == 2) r[n++] = 4;
  for (int i = 0; i < m / 3; ++i) r[n++] = 8;
  return n;
}

// Where frequency j of a transform lies after the in-place passes.
__host__ __device__ inline int position(int j, int m, const int* r, int nst) {
  int stride = 1 << m, pos = 0;
  for (int s = 0; s < nst; ++s) {
    stride /= r[s];
    pos += (j % r[s]) * stride;
    j /= r[s];
  }
  return pos;
}

// Complex points a workgroup transforms at size m: pairs of real segments.
__host__ __device__ inline int points(int m) { return m == kSbMaxM ? kSbWindow : kSbWindow / 2; }
// Segments of size m a window owns (those starting in its first half).
__host__ __device__ inline int owned(int m) { return m == kSbMaxM ? 1 : kSbWindow >> m; }

// Element e of the transforms' input.  sel 0: segment 2c in the real part and
// segment 2c + 1 in the imaginary part of transform c (the window itself at
// m = 13).  sel 1 / 2: segment 2c / 2c + 1 alone, the imaginary part zero.
__host__ __device__ inline float2 load_elem(const float* win, int m, int e, int sel) {
  if (m == kSbMaxM || sel == 1) return make_float2(win[e], 0.f);
  if (sel == 2) return make_float2(win[e + (1 << (m - 1))], 0.f);
  return make_float2(win[e], win[e + (1 << (m - 1))]);
}
// Passes over a window at size m, and the `sel` of pass i: two segments ride
// one transform only in a window that holds no x above kSbPairLimit.  A
// segment's rounding error scales with the norm of the whole complex input, so
// beside a partner of 10^6 (possible only with clip raised far above its
// default) a quiet segment would leave the bound its own norm gives.
__host__ __device__ inline int passes(int m, bool hot) { return (hot && m != kSbMaxM) ? 2 : 1; }
__host__ __device__ inline int pass_sel(int m, bool hot, int i) { return (hot && m != kSbMaxM) ? 1 + i : 0; }

__host__ __device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__host__ __device__ inline float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__host__ __device__ inline float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // * -i

__host__ __device__ inline void dft2(float2* x) {
  const float2 t = x[0];
  x[0] = cadd(t, x[1]);
  x[1] = csub(t, x[1]);
}
__host__ __device__ inline void dft4(float2& x0, float2& x1, float2& x2, float2& x3) {
  const float2 s0 = cadd(x0, x2), d0 = csub(x0, x2);
  const float2 s1 = cadd(x1, x3), e1 = mul_mi(csub(x1, x3));
  x0 = cadd(s0, s1);
  x2 = csub(s0, s1);
  x1 = cadd(d0, e1);
  x3 = csub(d0, e1);
}
__host__ __device__ inline void dft8(float2* a) {
  const float h = 0.70710678118654752440f;
  float2 b0 = cadd(a[0], a[4]), b1 = cadd(a[1], a[5]), b2 = cadd(a[2], a[6]), b3 = cadd(a[3], a[7]);
  float2 c0 = csub(a[0], a[4]), c1 = csub(a[1], a[5]), c2 = csub(a[2], a[6]), c3 = csub(a[3], a[7]);
  c1 = make_float2((c1.x + c1.y) * h, (c1.y - c1.x) * h);    // * W8
  c2 = mul_mi(c2);                                           // * W8^2
  c3 = make_float2((c3.y - c3.x) * h, (-c3.x - c3.y) * h);   // * W8^3
  dft4(b0, b1, b2, b3);
  dft4(c0, c1, c2, c3);
  a[0] = b0; a[1] = c0; a[2] = b1; a[3] = c1; a[4] = b2; a[5] = c2; a[6] = b3; a[7] = c3;
}

// Butterfly b of a decimation-in-frequency pass of radix R over sub-transforms
// of length L, in place: its R points, their DFT, the twiddles W_L^(q u).
template <int R>
__host__ __device__ inline void butterfly(float2* buf, const float2* tw, int m, int L, int b) {
  const int per = (1 << m) / R;      // butterflies of one transform
  const int c = b / per, bb = b - c * per;
  const int sub = L / R;
  const int block = bb / sub, q = bb - block * sub;
  float2* p = buf + (c << m) + block * L + q;
  float2 x[R];
#pragma unroll
  for (int t = 0; t < R; ++t) x[t] = p[t * sub];
  if (R == 2) dft2(x);
  if (R == 4) dft4(x[0], x[1], x[2], x[3]);
  if (R == 8) dft8(x);
  const int step = q * (kSbTwiddles / L);
  p[0] = x[0];
#pragma unroll
  for (int u = 1; u < R; ++u) p[u * sub] = cmul(x[u], tw[(step * u) & (kSbTwiddles - 1)]);
}

// Item `it` of the read-out at size m: transform c, frequency j; the powers of
// the two real segments that rode it (sb unused at m = 13).
__host__ __device__ inline void item(const float2* buf, int m, const int* r, int nst, int it, int* c, int* j,
                                     float* sa, float* sb) {
  const int half = 1 << (m - 1), M = 1 << m;
  *c = it / half;
  *j = it - *c * half;
  const float2* z = buf + (*c << m);
  const float2 a = z[position(*j, m, r, nst)];
  const float2 b = z[position((M - *j) & (M - 1), m, r, nst)];
  const float ar = a.x + b.x, ai = a.y - b.y;   // 2 F of the real part's segment
  const float br = a.y + b.y, bi = a.x - b.x;   // 2 |F| of the imaginary part's (up to a unit factor)
  const float scale = 0.25f / static_cast<float>(M);
  *sa = (ar * ar + ai * ai) * scale;
  *sb = (br * br + bi * bi) * scale;
}

// The largest S with the lowest j wins: S >= 0, so its bits order as it does.
__host__ __device__ inline unsigned long long key_of(float S, int j) {
  union {
    float f;
    uint32_t u;
  } v;
  v.f = S;
  return (static_cast<unsigned long long>(v.u) << 32) | static_cast<unsigned long long>(0xFFFFFFFFu - (uint32_t)j);
}
__host__ __device__ inline void key_split(unsigned long long key, float* S, int* j) {
  union {
    float f;
    uint32_t u;
  } v;
  v.u = static_cast<uint32_t>(key >> 32);
  *S = v.f;
  *j = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFu));
}

}  // namespace sbk

// ------------------------------------------------------------ geometry ----
struct SbParams {
  int m_lo = 5, m_hi = 13;
  int j_min = 2;
  float clip = 32.f;
  float min_power = 30.f;
};

struct SbGeometry {
  uint64_t fft_size = 0;
  double tobs = 0.0;            // T
  int64_t k_lo = 0, k_hi = 0;
  int m_lo = 5, m_hi = 13;
  std::vector<int64_t> nseg;    // per m - m_lo
  int64_t seg_stride = 0;       // the largest nseg: row length of the dense outputs
  int nwin = 0;                 // windows per row
  int nranges = 0;              // partial sums of mu per row
  int64_t nsegs_of(int m) const { return nseg[static_cast<size_t>(m - m_lo)]; }
};
// Segments of size M in a band of `band` bins.
int64_t sb_nseg(int64_t band, int m);
// The definition's T, k_lo, k_hi and the segment counts.  No refusals (sb_check).
SbGeometry sb_geometry(float min_freq, float max_freq, uint64_t fft_size, float tsamp, int m_lo, int m_hi);
// Every refusal of the definition that follows from the numbers alone, by name.
void sb_check(const SbParams& p, float min_freq, float max_freq, uint64_t fft_size, float tsamp);
// The bins of [k_lo, k_hi) a zap mask (build_zap_mask's bits, empty: none) leaves.
uint64_t sb_unzapped(const std::vector<uint32_t>& mask, int64_t k_lo, int64_t k_hi);
// exp(-2 pi i k / 8192), k < 8192: computed in double, rounded once.
std::vector<float2> sb_twiddles();

// The conversions of an event.
double sb_event_freq(const SbGeometry& g, const SbEvent& e);        // centre of its window, Hz
double sb_event_freq_half_width(const SbGeometry& g, const SbEvent& e);
double sb_event_pb(const SbGeometry& g, const SbEvent& e);          // j T / M
double sb_event_pb_res(const SbGeometry& g, const SbEvent& e);      // T / M

// A candidate: its strongest event, the members it absorbed (itself included)
// and the range of their dm_idx.
struct SbCandidate {
  SbEvent ev;
  int32_t members = 1;
  int32_t dm_lo = 0, dm_hi = 0;
};
// The definition's step 5.
std::vector<SbCandidate> sb_cluster(std::vector<SbEvent> events);

// Host transcriptions of the kernels (the same arithmetic, one thread after
// the other).  spec [nrows][spec_stride], P [nrows][stride], mu [nrows].
void sb_power_host(const float2* spec, uint64_t spec_stride, int nrows, const std::vector<uint32_t>& zapmask,
                   int64_t k_lo, int64_t k_hi, double* mu, float* P, uint64_t stride);
// best_S / best_j [nrows][m_hi - m_lo + 1][seg_stride] (may be null; untouched
// past nseg_m); events of S >= min_power are appended in (row, window, m, seg)
// order with dm_idx = dm0 + row.
void sb_search_host(const float* P, uint64_t stride, int nrows, const SbGeometry& g, const SbParams& p, int dm0,
                    float* best_S, int32_t* best_j, std::vector<SbEvent>* events);

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kSbThreads = 512;

// Step 2.  spec [nrows][spec_stride] float2, zapmask build_zap_mask's bits or
// null, count the unzapped bins of the band (sb_unzapped, > 0).  partials
// [nrows][nranges] double scratch; mu [nrows] double and P [nrows][stride]
// float32 out, P written on [k_lo, k_hi) only.  k_hi <= min(spec_stride, stride).
void sb_power(const float2* spec, uint64_t spec_stride, int nrows, const uint32_t* zapmask, int64_t k_lo,
              int64_t k_hi, uint64_t count, double* partials, double* mu, float* P, uint64_t stride, hipStream_t s);

// Steps 3 and 4.  P [nrows][stride] (16-byte aligned, stride a multiple of 4,
// read on [k_lo, k_hi) only), tw sb_twiddles() on the device.  best_S / best_j
// as in sb_search_host (null: not written).  Events are appended at
// events[atomicAdd(count, ..)]: *count (zeroed by the caller) may pass
// `capacity`, nothing is written at or past it.  nrows <= 65535.
void sb_search(const float* P, uint64_t stride, int nrows, const SbGeometry& g, const SbParams& p, int dm0,
               const float2* tw, float* best_S, int32_t* best_j, SbEvent* events, uint32_t capacity,
               uint32_t* count, hipStream_t s);

}  // namespace kern

// ------------------------------------------------------------- options ----
struct SbCmdLineOptions {
  CmdLineOptions search;    // peasoup's options of the same names and defaults
  std::string outfilename;  // -o
  float min_power = 30.f;   // --min_power
  int m_min = 5;            // --m_min
  int m_max = 13;           // --m_max
  int j_min = 2;            // --j_min
  float clip = 32.f;        // --clip
};
// "%Y-%m-%d-%H:%M_sbsearch.output" in UTC.
std::string default_sb_output_filename();
bool parse_sb_cmdline(SbCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// --------------------------------------------------------------- setup ----
struct SbSetup {
  SearchSetup search;   // the plain search's setup for the same options
  uint64_t nrow = 0;    // samples of a dedispersed row
  SbParams params;
  SbGeometry geom;
  std::vector<uint32_t> zapmask;  // empty: no zap list
  uint64_t unzapped = 0;          // bins of the band mu averages
};
// Everything that follows from the options and the header; every refusal of
// the definition is raised here, before any device work.
SbSetup make_sb_setup(const SbCmdLineOptions& args, const SigprocHeader& hdr);

// ------------------------------------------------------------ searcher ----
// One device.  Works per DM chunk: dedisperse, whiten_batch, the forward FFT
// of every row, sb_power, sb_search, events to the host; a chunk whose events
// passed the buffer is run again with a buffer that holds them.
class SidebandSearcher {
 public:
  SidebandSearcher(const SbSetup& setup, const DeviceFilterbank& fb, hipStream_t stream, uint32_t capacity = 1u << 16);
  // The events of DMs [d0, d1) (d1 < 0: all), sorted by (dm_idx, m, seg).
  std::vector<SbEvent> search(int d0 = 0, int d1 = -1);
  // The float32 P rows [d1 - d0][power_stride()] and mu of DMs [d0, d1), for tests and diagnostics.
  std::vector<float> power_rows(int d0, int d1, std::vector<double>* mu = nullptr);
  uint64_t power_stride() const { return pstride_; }
  uint64_t reruns() const { return reruns_; }

 private:
  void powers(int c0, int c1);
  const SbSetup& setup_;
  const DeviceFilterbank& fb_;
  hipStream_t stream_;
  std::unique_ptr<Dedisperser> dd_;
  std::unique_ptr<Whitener> wh_;
  uint64_t rstride_ = 0, pstride_ = 0, nb_ = 0;
  int chunk_ = 1;
  DeviceBuffer<uint8_t> rows_;
  DeviceBuffer<float> series_, P_, stats_;
  DeviceBuffer<float2> spec_, tw_;
  DeviceBuffer<uint32_t> zap_, count_;
  DeviceBuffer<double> partials_, mu_;
  DeviceBuffer<SbEvent> events_;
  uint32_t capacity_ = 0;
  uint64_t reruns_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct SbRun {
  std::vector<SbCandidate> candidates;  // final, sorted, limited
  uint64_t events = 0;
  SbSetup setup;
  std::map<std::string, double> timers;  // reading/searching/total (s)
};
SbRun run_sb_pipeline(const SbCmdLineOptions& args);
// The text of the output file: the commented header, then one line per
// candidate `freq_hz freq_half_width_hz pb_s pb_res_s power M j dm dm_idx
// members dm_idx_lo dm_idx_hi`.
std::string sb_output_text(const SbCmdLineOptions& args, const SbSetup& setup, const std::vector<SbCandidate>& cands);
// Writes it to a temporary file and renames it to args.outfilename.
void write_sb_output(const SbCmdLineOptions& args, const SbSetup& setup, const std::vector<SbCandidate>& cands);

}  // namespace psoup
