// Burst cutouts: candidate readers, BurstCutter (the launch plan), pipeline
// and the cutout file.  See psoup/burstcube.hpp.
#include "psoup/burstcube.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "psoup/plan.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// ----------------------------------------------------------- definition ----
int burst_tscrunch(uint32_t width, int tscrunch) {
  if (tscrunch > 0) return tscrunch;
  return static_cast<int>(std::min<uint32_t>(std::max<uint32_t>(1u, width / 2), 1u << 30));
}

int64_t burst_t0(uint64_t sample, uint32_t width, int f, int ntime) {
  const int64_t tc = static_cast<int64_t>(sample) + static_cast<int64_t>(width / 2);
  return tc - static_cast<int64_t>(ntime / 2) * f;
}

// burst_dms: burst_dms.cpp (host only; cubeopt shares it)

// ----------------------------------------------------------- candidates ----
namespace {

// The numeric columns of every data line of a text table ('#' and blank
// lines skipped), at most `limit` lines; fewer than `need` numbers on a line
// is an error naming it.
std::vector<std::vector<double>> read_table(const std::string& path, int limit, size_t need, const char* what) {
  std::ifstream in(path);
  PSOUP_CHECK(in.good(), "cannot open " << path);
  std::vector<std::vector<double>> rows;
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t first = line.find_first_not_of(" \t\r\n");
    if (first == std::string::npos || line[first] == '#') continue;
    if (limit >= 0 && rows.size() >= static_cast<size_t>(limit)) break;
    std::istringstream ss(line);
    std::vector<double> v;
    double x;
    while (v.size() < need + 1 && ss >> x) v.push_back(x);
    bool ok = v.size() >= need;
    for (size_t i = 0; ok && i < need; ++i) ok = std::isfinite(v[i]);
    if (!ok) PSOUP_THROW(path << ": line " << lineno << " is not '" << what << "': '" << line << "'");
    rows.push_back(v);
  }
  return rows;
}

BurstCandidate make_candidate(const std::string& path, size_t idx, double sample, double width, double dm, double snr) {
  PSOUP_CHECK(sample >= 0 && sample < 1.8e19 && width >= 0 && width < 4.0e9 && sample == std::floor(sample) &&
                  width == std::floor(width),
              path << ": candidate " << idx << ": sample and width must be non-negative integers");
  BurstCandidate c;
  c.sample = static_cast<uint64_t>(sample);
  c.width = static_cast<uint32_t>(width);
  c.dm = static_cast<float>(dm);
  c.snr = static_cast<float>(snr);
  return c;
}

}  // namespace

std::vector<BurstCandidate> read_burst_candfile(const std::string& path, int limit) {
  std::vector<BurstCandidate> out;
  for (const std::vector<double>& v : read_table(path, limit, 3, "sample width dm [snr]"))
    out.push_back(make_candidate(path, out.size(), v[0], v[1], v[2], v.size() > 3 ? v[3] : 0.0));
  return out;
}

std::vector<BurstCandidate> read_sp_output(const std::string& path, int limit) {
  std::vector<BurstCandidate> out;
  for (const std::vector<double>& v : read_table(path, limit, 6, "snr sample time_s width dm_idx dm ..."))
    out.push_back(make_candidate(path, out.size(), v[1], v[3], v[5], v[0]));
  return out;
}

// --------------------------------------------------------------- cutter ----
BurstCutter::BurstCutter(const DeviceFilterbank& fb, const BurstParams& p, hipStream_t stream, size_t batch_bytes)
    : x_(fb.data()),
      stride_(fb.stride()),
      row_valid_(fb.geometry().nsamps),
      nchans_(fb.geometry().nchans),
      bias_(fb.geometry().bias),
      delays_(fb.geometry().delays),
      p_(p),
      stream_(stream),
      batch_bytes_(batch_bytes) {
  init(fb.geometry().killmask);
}

BurstCutter::BurstCutter(const int8_t* d_chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias,
                         const std::vector<float>& delays, const std::vector<int>& killmask, const BurstParams& p,
                         hipStream_t stream, size_t batch_bytes)
    : x_(d_chan_major),
      stride_(stride),
      row_valid_(row_valid),
      nchans_(nchans),
      bias_(bias),
      delays_(delays),
      p_(p),
      stream_(stream),
      batch_bytes_(batch_bytes) {
  init(killmask);
}

BurstCutter::~BurstCutter() { (void)hipStreamSynchronize(stream_); }

void BurstCutter::init(const std::vector<int>& killmask) {
  PSOUP_CHECK(nchans_ >= 1, "burst cube: no channels");
  PSOUP_CHECK(x_ != nullptr && row_valid_ >= 1 && row_valid_ <= stride_ && stride_ % 16 == 0 &&
                  stride_ < (uint64_t(1) << 40),
              "burst cube: rows need a stride that is a multiple of 16 and at least their valid length");
  PSOUP_CHECK(bias_ >= 0 && bias_ <= 128, "burst cube: bias must be in 0..128");
  PSOUP_CHECK(delays_.empty() || static_cast<int>(delays_.size()) == nchans_, "burst cube: delay table size != nchans");
  PSOUP_CHECK(killmask.empty() || static_cast<int>(killmask.size()) == nchans_, "burst cube: killmask size != nchans");
  PSOUP_CHECK(p_.ntime >= 1 && p_.ntime <= 1024, "burst cube: ntime must be in 1..1024");
  PSOUP_CHECK(p_.ndm >= 1 && p_.ndm <= 1024, "burst cube: ndm must be in 1..1024");
  PSOUP_CHECK(p_.nsub >= 1 && p_.nsub <= nchans_, "burst cube: nsub must be in 1..nchans");
  PSOUP_CHECK(p_.tscrunch >= 0 && p_.tscrunch <= kern::kBurstMaxF,
              "burst cube: tscrunch must be in 0.." << kern::kBurstMaxF);
  PSOUP_CHECK(std::isfinite(p_.dm_half_range) && p_.dm_half_range >= 0, "burst cube: dm_half_range must be >= 0");
  // the unkilled channels in ascending order and each subband's range of them
  sub_first_.assign(static_cast<size_t>(p_.nsub) + 1, 0);
  nactive_.assign(static_cast<size_t>(p_.nsub), 0);
  for (int c = 0; c < nchans_; ++c) {
    if (!killmask.empty() && killmask[static_cast<size_t>(c)] == 0) continue;
    const int s = static_cast<int>(static_cast<int64_t>(c) * p_.nsub / nchans_);
    nactive_[static_cast<size_t>(s)] += 1;
    active_.push_back(c);
  }
  for (int s = 0; s < p_.nsub; ++s)
    sub_first_[static_cast<size_t>(s) + 1] = sub_first_[static_cast<size_t>(s)] + nactive_[static_cast<size_t>(s)];
  nactive_total_ = static_cast<int>(active_.size());
  d_active_.resize(std::max<size_t>(1, active_.size()));
  if (!active_.empty()) {
    PSOUP_HIP_CHECK(hipMemcpyAsync(d_active_.data(), active_.data(), active_.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  }
}

size_t BurstCutter::bytes_per_candidate() const {
  const size_t rows = static_cast<size_t>(p_.nsub) + p_.ndm;
  // sums and hits; the rows' relative offsets and the (first, spread) pair of
  // every (tile, channel) at one row per tile; the tiles; the job
  return 2 * rows * p_.ntime * sizeof(int32_t) +
         3 * (static_cast<size_t>(p_.ndm) + 1) * nchans_ * sizeof(int32_t) + rows * sizeof(kern::BurstTile) +
         sizeof(kern::BurstJob);
}

int BurstCutter::batch_size() const {
  // table indices stay below 2^30
  const size_t table = (static_cast<size_t>(p_.ndm) + 1) * nchans_;
  const size_t cap = std::max<size_t>(1, std::min<size_t>(65535, (size_t(1) << 30) / table));
  return static_cast<int>(std::min(std::max<size_t>(1, batch_bytes_ / bytes_per_candidate()), cap));
}

void BurstCutter::check_job(size_t i, int64_t t0, int f) const {
  PSOUP_CHECK(f >= 1, "burst cube: candidate " << i << ": " << f << " samples per time bin");
  // the 32-bit bound of the definition first, then what the kernel's window holds
  PSOUP_CHECK(255ull * static_cast<uint64_t>(f) * static_cast<uint64_t>(std::max(1, nactive_total_)) <
                  (uint64_t(1) << 31),
              "burst cube: candidate " << i << ": 255 x " << f << " samples x " << nactive_total_
                                       << " channels overflow the 32-bit sums; set a smaller tscrunch");
  PSOUP_CHECK(f <= kern::kBurstMaxF, "burst cube: candidate " << i << ": " << f << " samples per time bin; at most "
                                                              << kern::kBurstMaxF
                                                              << " are supported (set tscrunch)");
  PSOUP_CHECK(t0 > -(int64_t(1) << 61) && t0 < (int64_t(1) << 61),
              "burst cube: candidate " << i << ": first sample out of range");
}

void BurstCutter::launch(const int32_t* h_ds, const int32_t* h_dmt, const int64_t* t0, const int* f, int ncand,
                         size_t first, int32_t* d_sums, int32_t* d_hits) {
  using kern::kBurstMaxOut;
  using kern::kBurstMaxRows;
  using kern::kBurstThreads;
  using kern::kBurstWindow;
  const int nch = nchans_, ndm = p_.ndm, nsub = p_.nsub, ntime = p_.ntime, na = nactive_total_;
  std::vector<kern::BurstJob> jobs(static_cast<size_t>(ncand));
  std::vector<kern::BurstTile> tiles;
  std::vector<int32_t> rel, win;
  std::vector<int64_t> mn(static_cast<size_t>(na)), mx(static_cast<size_t>(na));
  int bin_tiles = 1;
  uint64_t single = 0;
  for (int i = 0; i < ncand; ++i) {
    const int32_t* ds = h_ds + static_cast<size_t>(i) * nch;
    const int32_t* dmt = h_dmt + static_cast<size_t>(i) * ndm * nch;
    check_job(first + i, t0[i], f[i]);
    for (size_t e = 0; e < static_cast<size_t>(ndm + 1) * nch; ++e) {
      const int32_t o = e < static_cast<size_t>(nch) ? ds[e] : dmt[e - nch];
      PSOUP_CHECK(o > -(1 << 30) && o < (1 << 30), "burst cube: candidate " << (first + i) << ": sample offset " << o
                                                                            << " out of range");
    }
    // Outputs a workgroup can hold, and how they are shared between rows and
    // bins: with s samples between adjacent rows' windows, R rows x B bins
    // load about f / R + s / B bytes per output byte, least at R / B = f / s.
    const int lg = kern::burst_lanes_log2(f[i]);
    const int cap = (kBurstThreads >> lg) * kBurstMaxOut;
    const int bmax = std::max(1, std::min({ntime, (kBurstWindow / 2) / f[i], cap}));
    double s = 0;
    if (ndm > 1 && na > 0) {
      for (int ci = 0; ci < na; ++ci) {
        const int c = active_[static_cast<size_t>(ci)];
        s += std::fabs(static_cast<double>(dmt[static_cast<size_t>(ndm - 1) * nch + c]) - dmt[c]);
      }
      s /= static_cast<double>(na) * (ndm - 1);
    }
    s = std::max(s, 0.25);
    const int rcap = std::min({kBurstMaxRows, ndm, cap});
    const int rt = std::max(1, std::min(rcap, static_cast<int>(std::sqrt(static_cast<double>(cap) * f[i] / s))));
    const int B = std::max(1, std::min(bmax, cap / rt));
    const int rmax = std::max(1, std::min(rcap, cap / B));
    const int64_t room = kBurstWindow - 15 - static_cast<int64_t>(B) * f[i];  // the largest spread that fits
    PSOUP_CHECK(room >= 0 && B * f[i] < 65536 && rmax * B <= cap, "burst cube: bad tile plan");
    kern::BurstJob& J = jobs[static_cast<size_t>(i)];
    J.t0 = t0[i];
    J.f = f[i];
    J.bins_per_tile = B;
    J.lanes_log2 = lg;
    bin_tiles = std::max(bin_tiles, (ntime + B - 1) / B);
    // the waterfall: one tile per subband, its own channels
    for (int sb = 0; sb < nsub; ++sb) {
      kern::BurstTile T;
      T.cand = i;
      T.row0 = sb;
      T.nrows = 1;
      T.ia = sub_first_[static_cast<size_t>(sb)];
      T.ie = sub_first_[static_cast<size_t>(sb) + 1];
      T.rel0 = static_cast<uint32_t>(rel.size());
      T.win0 = static_cast<uint32_t>(win.size() / 2);
      for (int ci = T.ia; ci < T.ie; ++ci) {
        rel.push_back(0);
        win.push_back(ds[active_[static_cast<size_t>(ci)]]);
        win.push_back(0);
      }
      tiles.push_back(T);
    }
    // the DM-time plane: runs of rows, every unkilled channel; a run grows
    // while every channel's union window fits
    for (int j0 = 0; j0 < ndm;) {
      for (int ci = 0; ci < na; ++ci)
        mn[static_cast<size_t>(ci)] = mx[static_cast<size_t>(ci)] =
            dmt[static_cast<size_t>(j0) * nch + active_[static_cast<size_t>(ci)]];
      int nr = 1;
      while (nr < rmax && j0 + nr < ndm) {
        const int32_t* row = dmt + static_cast<size_t>(j0 + nr) * nch;
        bool fits = true;
        for (int ci = 0; fits && ci < na; ++ci) {
          const int64_t o = row[active_[static_cast<size_t>(ci)]];
          fits = std::max(mx[static_cast<size_t>(ci)], o) - std::min(mn[static_cast<size_t>(ci)], o) <= room;
        }
        if (!fits) break;
        for (int ci = 0; ci < na; ++ci) {
          const int64_t o = row[active_[static_cast<size_t>(ci)]];
          mn[static_cast<size_t>(ci)] = std::min(mn[static_cast<size_t>(ci)], o);
          mx[static_cast<size_t>(ci)] = std::max(mx[static_cast<size_t>(ci)], o);
        }
        ++nr;
      }
      kern::BurstTile T;
      T.cand = i;
      T.row0 = nsub + j0;
      T.nrows = nr;
      T.ia = 0;
      T.ie = na;
      T.rel0 = static_cast<uint32_t>(rel.size());
      T.win0 = static_cast<uint32_t>(win.size() / 2);
      for (int ci = 0; ci < na; ++ci) {
        const int c = active_[static_cast<size_t>(ci)];
        for (int r = 0; r < nr; ++r)
          rel.push_back(static_cast<int32_t>(dmt[static_cast<size_t>(j0 + r) * nch + c] - mn[static_cast<size_t>(ci)]));
        win.push_back(static_cast<int32_t>(mn[static_cast<size_t>(ci)]));
        win.push_back(static_cast<int32_t>(mx[static_cast<size_t>(ci)] - mn[static_cast<size_t>(ci)]));
      }
      tiles.push_back(T);
      single += nr == 1;
      j0 += nr;
    }
    PSOUP_CHECK(rel.size() < (size_t(1) << 31) && win.size() < (size_t(1) << 31), "burst cube: batch too large");
  }
  // what the kernel relies on, once more over the finished tables
  for (const kern::BurstTile& T : tiles) {
    const kern::BurstJob& J = jobs[static_cast<size_t>(T.cand)];
    const int nper = (T.nrows * std::min(J.bins_per_tile, ntime) + (kBurstThreads >> J.lanes_log2) - 1) /
                     (kBurstThreads >> J.lanes_log2);
    PSOUP_CHECK(T.cand >= 0 && T.cand < ncand && T.nrows >= 1 && T.nrows <= kBurstMaxRows && T.row0 >= 0 &&
                    T.row0 + T.nrows <= nsub + ndm && T.ia >= 0 && T.ia <= T.ie && T.ie <= na && nper <= kBurstMaxOut,
                "burst cube: bad tile");
    PSOUP_CHECK(static_cast<size_t>(T.rel0) + static_cast<size_t>(T.ie - T.ia) * T.nrows <= rel.size() &&
                    2 * (static_cast<size_t>(T.win0) + (T.ie - T.ia)) <= win.size(),
                "burst cube: tile tables out of range");
    for (int q = 0; q < T.ie - T.ia; ++q) {
      const int32_t spread = win[2 * (static_cast<size_t>(T.win0) + q) + 1];
      PSOUP_CHECK(spread >= 0 && static_cast<int64_t>(J.bins_per_tile) * J.f + spread + 15 <= kBurstWindow,
                  "burst cube: a tile's window exceeds the staged bytes");
      for (int r = 0; r < T.nrows; ++r) {
        const int32_t v = rel[static_cast<size_t>(T.rel0) + static_cast<size_t>(q) * T.nrows + r];
        PSOUP_CHECK(v >= 0 && v <= spread, "burst cube: a row's offset lies outside its tile's window");
      }
    }
  }
  d_jobs_.resize(jobs.size());
  d_tiles_.resize(tiles.size());
  d_rel_.resize(std::max<size_t>(1, rel.size()));
  d_win_.resize(std::max<size_t>(1, win.size()));
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_jobs_.data(), jobs.data(), jobs.size() * sizeof(kern::BurstJob),
                                 hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_tiles_.data(), tiles.data(), tiles.size() * sizeof(kern::BurstTile),
                                 hipMemcpyHostToDevice, stream_));
  if (!rel.empty())
    PSOUP_HIP_CHECK(hipMemcpyAsync(d_rel_.data(), rel.data(), rel.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                   stream_));
  if (!win.empty())
    PSOUP_HIP_CHECK(hipMemcpyAsync(d_win_.data(), win.data(), win.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                   stream_));
  kern::BurstGeom g;
  g.nchans = nch;
  g.stride = stride_;
  g.nsamps = row_valid_;
  g.bias = bias_;
  g.ntime = ntime;
  g.nrows = nsub + ndm;
  kern::burst_cube(x_, g, d_active_.data(), d_tiles_.data(), static_cast<uint32_t>(tiles.size()), d_jobs_.data(),
                   d_rel_.data(), d_win_.data(), bin_tiles, d_sums, d_hits, stream_);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // the host tables go out of scope
  ++nbatches_;
  ntiles_ += tiles.size();
  nsingle_ += single;
}

std::vector<BurstResult> BurstCutter::cut(const std::vector<BurstCandidate>& cands) {
  PSOUP_CHECK(static_cast<int>(delays_.size()) == nchans_, "burst cube: no delay table");
  const size_t nc = cands.size();
  const size_t nch = static_cast<size_t>(nchans_), ndm = static_cast<size_t>(p_.ndm);
  std::vector<BurstResult> out(nc);
  std::vector<int64_t> t0(nc);
  std::vector<int> f(nc);
  float dmax = 0.f;
  for (float d : delays_) dmax = std::max(dmax, std::fabs(d));
  for (size_t i = 0; i < nc; ++i) {
    const BurstCandidate& c = cands[i];
    std::ostringstream who;
    who << "burst cube: candidate " << i << " (sample " << c.sample << ", width " << c.width << ", dm " << c.dm << ")";
    PSOUP_CHECK(c.sample < row_valid_, who.str() << ": the sample lies past the " << row_valid_
                                                 << " samples of the filterbank");
    PSOUP_CHECK(c.width >= 1, who.str() << ": the width must be at least 1");
    PSOUP_CHECK(std::isfinite(c.dm) && c.dm >= 0, who.str() << ": the DM must be non-negative");
    f[i] = burst_tscrunch(c.width, p_.tscrunch);
    t0[i] = burst_t0(c.sample, c.width, f[i], p_.ntime);
    check_job(i, t0[i], f[i]);
    out[i].dms = burst_dms(c.dm, p_.ndm, p_.dm_half_range);
    PSOUP_CHECK(static_cast<double>(out[i].dms.back()) * dmax < 1.0e9,
                who.str() << ": the dispersion delay overflows the sample offsets");
    out[i].tscrunch = static_cast<uint32_t>(f[i]);
    out[i].t0 = t0[i];
    out[i].nactive = nactive_;
  }
  const size_t rows = static_cast<size_t>(p_.nsub) + ndm, nt = static_cast<size_t>(p_.ntime);
  const size_t bs = static_cast<size_t>(batch_size());
  std::vector<int32_t> ds, dmt, hs, hh;
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    ds.resize(nb * nch);
    dmt.resize(nb * ndm * nch);
    for (size_t i = 0; i < nb; ++i) {
      for (size_t c = 0; c < nch; ++c) ds[i * nch + c] = dm_delay_samples(cands[b0 + i].dm, delays_[c]);
      for (size_t j = 0; j < ndm; ++j)
        for (size_t c = 0; c < nch; ++c)
          dmt[(i * ndm + j) * nch + c] = dm_delay_samples(out[b0 + i].dms[j], delays_[c]);
    }
    d_sums_.resize(nb * rows * nt);
    d_hits_.resize(nb * rows * nt);
    launch(ds.data(), dmt.data(), t0.data() + b0, f.data() + b0, static_cast<int>(nb), b0, d_sums_.data(),
           d_hits_.data());
    hs.resize(nb * rows * nt);
    hh.resize(nb * rows * nt);
    PSOUP_HIP_CHECK(hipMemcpyAsync(hs.data(), d_sums_.data(), hs.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   stream_));
    PSOUP_HIP_CHECK(hipMemcpyAsync(hh.data(), d_hits_.data(), hh.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
    const size_t nds = static_cast<size_t>(p_.nsub) * nt;
    for (size_t i = 0; i < nb; ++i) {
      BurstResult& r = out[b0 + i];
      const int32_t* s = hs.data() + i * rows * nt;
      const int32_t* h = hh.data() + i * rows * nt;
      r.ds_sums.assign(s, s + nds);
      r.ds_hits.assign(h, h + nds);
      r.dmt_sums.assign(s + nds, s + rows * nt);
      r.dmt_hits.assign(h + nds, h + rows * nt);
    }
  }
  return out;
}

void BurstCutter::cut_offsets(const int32_t* h_ds_offsets, const int32_t* h_dmt_offsets, const std::vector<int64_t>& t0,
                              const std::vector<int>& f, int32_t* d_sums, int32_t* d_hits) {
  const size_t nc = t0.size();
  PSOUP_CHECK(f.size() == nc, "burst cube: t0 and f differ in length");
  const size_t nch = static_cast<size_t>(nchans_), ndm = static_cast<size_t>(p_.ndm);
  for (size_t i = 0; i < nc; ++i) {
    check_job(i, t0[i], f[i]);
    for (size_t e = 0; e < (ndm + 1) * nch; ++e) {
      const int32_t o = e < nch ? h_ds_offsets[i * nch + e] : h_dmt_offsets[i * ndm * nch + e - nch];
      PSOUP_CHECK(o > -(1 << 30) && o < (1 << 30), "burst cube: candidate " << i << ": sample offset " << o
                                                                            << " out of range");
    }
  }
  const size_t per = (static_cast<size_t>(p_.nsub) + ndm) * p_.ntime;
  const size_t bs = static_cast<size_t>(batch_size());
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    launch(h_ds_offsets + b0 * nch, h_dmt_offsets + b0 * ndm * nch, t0.data() + b0, f.data() + b0,
           static_cast<int>(nb), b0, d_sums + b0 * per, d_hits + b0 * per);
  }
}

// ------------------------------------------------------------ pipeline ----
BurstRun run_burst_pipeline(const BurstCubeCmdLineOptions& args) {
  BurstRun run;
  Stopwatch t_total, t_read, t_cut;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  PSOUP_CHECK(args.spfilename.empty() != args.candfilename.empty(),
              "burstcube: give exactly one of --spfile and --candfile");
  run.candidates = args.spfilename.empty() ? read_burst_candfile(args.candfilename, args.limit)
                                           : read_sp_output(args.spfilename, args.limit);
  PSOUP_CHECK(!run.candidates.empty(), "burstcube: no candidates");
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  // DM rows may sweep past the end of the file: the geometry is that of DM 0
  DedispGeometry geom = DedispGeometry::make(hdr, fb.nsamps(), {0.f}, kill);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  PSOUP_HIP_CHECK(hipSetDevice(0));
  Stream stream;
  DeviceFilterbank dfb(geom, stream.get());
  load_filterbank_fanout({&dfb}, {0}, fb);
  t_read.stop();
  BurstParams p;
  p.ntime = args.ntime;
  p.ndm = args.ndm;
  p.nsub = std::min(args.nsub, hdr.nchans);
  p.tscrunch = args.tscrunch;
  p.dm_half_range = args.dm_half_range;
  t_cut.start();
  BurstCutter cutter(dfb, p, stream.get());
  run.cutouts = cutter.cut(run.candidates);
  t_cut.stop();
  log_verbose("burst cube: " + std::to_string(run.candidates.size()) + " candidates, " +
              std::to_string(cutter.tiles()) + " row tiles (" + std::to_string(cutter.single_row_tiles()) +
              " DM tiles of one row), " + std::to_string(cutter.batches()) + " launches");
  BurstFileHeader& h = run.header;
  h.ncand = static_cast<uint32_t>(run.candidates.size());
  h.ntime = static_cast<uint32_t>(p.ntime);
  h.nsub = static_cast<uint32_t>(p.nsub);
  h.ndm = static_cast<uint32_t>(p.ndm);
  h.nchans = static_cast<uint32_t>(hdr.nchans);
  h.nbits = static_cast<uint32_t>(hdr.nbits);
  h.nsamps = fb.nsamps();
  h.tsamp = hdr.tsamp;
  h.fch1 = hdr.fch1;
  h.foff = hdr.foff;
  write_burst_file(args.outfilename, h, run.candidates, run.cutouts);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["cutting"] = t_cut.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

namespace {
template <class T>
void put(std::vector<char>& b, const T& v) {
  static_assert(std::is_trivially_copyable<T>::value, "put: plain values");
  const char* p = reinterpret_cast<const char*>(&v);  // gfx950 hosts are little-endian
  b.insert(b.end(), p, p + sizeof(T));
}
template <class T>
bool put_all(FILE* fo, const std::vector<T>& v) {
  return std::fwrite(v.data(), sizeof(T), v.size(), fo) == v.size();
}
}  // namespace

void write_burst_file(const std::string& path, const BurstFileHeader& h, const std::vector<BurstCandidate>& cands,
                      const std::vector<BurstResult>& cutouts) {
  PSOUP_CHECK(cands.size() == cutouts.size() && cands.size() == h.ncand, "burst file: candidate count mismatch");
  const size_t nds = static_cast<size_t>(h.nsub) * h.ntime, ndmt = static_cast<size_t>(h.ndm) * h.ntime;
  for (size_t i = 0; i < cutouts.size(); ++i) {
    const BurstResult& r = cutouts[i];
    PSOUP_CHECK(r.dms.size() == h.ndm && r.nactive.size() == h.nsub && r.ds_sums.size() == nds &&
                    r.ds_hits.size() == nds && r.dmt_sums.size() == ndmt && r.dmt_hits.size() == ndmt,
                "burst file: candidate " << i << " has the wrong shape");
  }
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open burst output " << tmp);
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'B', 'R', 'S', 'T', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  put(b, h.ncand);
  put(b, h.ntime);
  put(b, h.nsub);
  put(b, h.ndm);
  put(b, h.nchans);
  put(b, h.nbits);
  put(b, h.nsamps);
  put(b, h.tsamp);
  put(b, h.fch1);
  put(b, h.foff);
  bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  for (size_t i = 0; ok && i < cands.size(); ++i) {
    const BurstResult& r = cutouts[i];
    b.clear();
    put(b, cands[i].sample);
    put(b, cands[i].width);
    put(b, r.tscrunch);
    put(b, r.t0);
    put(b, cands[i].dm);
    put(b, cands[i].snr);
    ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size() && put_all(fo, r.dms) && put_all(fo, r.nactive) &&
         put_all(fo, r.ds_sums) && put_all(fo, r.ds_hits) && put_all(fo, r.dmt_sums) && put_all(fo, r.dmt_hits);
  }
  ok = (std::fclose(fo) == 0) && ok;
  if (!ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write burst output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace psoup
