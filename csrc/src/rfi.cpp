// RFI excision, host side: the flagging step on the table of block sums, the
// mask file and the killfile writer.  No device code here (the native unit
// tests link this file alone).  See psoup/rfi.hpp.
#include "psoup/rfi.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace psoup {

void rfi_check_params(const RfiParams& p) {
  PSOUP_CHECK(p.block >= 256 && p.block <= 65536 && p.block % 256 == 0,
              "rfi block must be a multiple of 256 in [256, 65536], got " << p.block);
  PSOUP_CHECK(std::isfinite(p.thresh) && p.thresh >= 0, "rfi thresh must be finite and non-negative");
  PSOUP_CHECK(std::isfinite(p.chan_frac) && p.chan_frac >= 0 && std::isfinite(p.block_frac) && p.block_frac >= 0,
              "rfi chan_frac / block_frac must be finite and non-negative");
}

RfiParams rfi_params_from(const RfiCmdLineOptions& a) {
  RfiParams p;
  PSOUP_CHECK(a.rfi_block > 0, "--rfi_block must be positive");
  p.block = static_cast<uint64_t>(a.rfi_block);
  p.thresh = a.rfi_thresh;
  p.chan_frac = a.rfi_chan_frac;
  p.block_frac = a.rfi_block_frac;
  p.zero_dm = a.zero_dm;
  rfi_check_params(p);
  return p;
}

uint64_t RfiMask::flagged_cells() const {
  uint64_t n = 0;
  for (uint8_t f : cell) n += f;
  return n;
}
uint64_t RfiMask::flagged_chans() const {
  uint64_t n = 0;
  for (uint8_t f : chan_flag) n += f;
  return n;
}
uint64_t RfiMask::flagged_blocks() const {
  uint64_t n = 0;
  for (uint8_t f : block_flag) n += f;
  return n;
}

namespace {

// numpy.median: the mean of the two middle values for an even count
double median_of(std::vector<double> v) {
  const size_t n = v.size();
  std::sort(v.begin(), v.end());
  return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

// flags |x - med| > (thresh * 1.4826) * MAD, or x != med where MAD is 0
void flag_outliers(const std::vector<double>& x, double thresh, double* med_out, uint8_t* flags, size_t step) {
  const double med = median_of(x);
  std::vector<double> dev(x.size());
  for (size_t i = 0; i < x.size(); ++i) dev[i] = std::fabs(x[i] - med);
  const double mad = median_of(dev);
  const double k = thresh * 1.4826;
  const double s = k * mad;
  for (size_t i = 0; i < x.size(); ++i) {
    const bool f = (mad == 0.0) ? (x[i] != med) : (dev[i] > s);
    if (f) flags[i * step] = 1;
  }
  *med_out = med;
}

}  // namespace

RfiMask rfi_flag(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nchans, uint64_t nsamps,
                 const std::vector<int>& killmask, const RfiParams& p) {
  rfi_check_params(p);
  PSOUP_CHECK(nchans > 0 && nsamps > 0, "rfi_flag: empty table");
  const uint64_t L = p.block;
  const size_t nblk = static_cast<size_t>((nsamps + L - 1) / L);
  const size_t nc = static_cast<size_t>(nchans);
  PSOUP_CHECK(S1.size() == nc * nblk && S2.size() == nc * nblk, "rfi_flag: S1 / S2 must be [nchans][nblk]");
  PSOUP_CHECK(killmask.empty() || killmask.size() == nc, "rfi_flag: killmask size != nchans");
  RfiMask m;
  m.nchans = nchans;
  m.nblk = nblk;
  m.nsamps = nsamps;
  m.block = L;
  std::vector<int64_t> len(nblk, static_cast<int64_t>(L));
  len[nblk - 1] = static_cast<int64_t>(nsamps - (nblk - 1) * L);
  std::vector<uint8_t> live(nc, 1);
  size_t nlive = 0;
  for (size_t c = 0; c < nc; ++c) {
    if (!killmask.empty() && killmask[c] == 0) live[c] = 0;
    nlive += live[c];
  }
  // cell flags before promotion
  std::vector<uint8_t> pre(nc * nblk, 0);
  std::vector<double> mean(nblk), var(nblk);
  for (size_t c = 0; c < nc; ++c) {
    uint8_t* row = pre.data() + c * nblk;
    if (!live[c]) {
      std::fill(row, row + nblk, 1);
      continue;
    }
    for (size_t b = 0; b < nblk; ++b) {
      const int64_t s1 = static_cast<int64_t>(S1[c * nblk + b]), s2 = static_cast<int64_t>(S2[c * nblk + b]);
      const int64_t n = len[b];
      mean[b] = static_cast<double>(s1) / static_cast<double>(n);
      var[b] = static_cast<double>(n * s2 - s1 * s1) / static_cast<double>(n * n);
    }
    double med_m = 0, med_v = 0;
    flag_outliers(mean, p.thresh, &med_m, row, 1);
    flag_outliers(var, p.thresh, &med_v, row, 1);
    if (med_v == 0.0) std::fill(row, row + nblk, 1);  // dead channel
  }
  // promotion, from the flags as they stand
  m.chan_flag.assign(nc, 0);
  m.block_flag.assign(nblk, 0);
  for (size_t c = 0; c < nc; ++c) {
    if (!live[c]) {
      m.chan_flag[c] = 1;
      continue;
    }
    uint64_t n = 0;
    for (size_t b = 0; b < nblk; ++b) n += pre[c * nblk + b];
    if (static_cast<double>(n) / static_cast<double>(nblk) > p.chan_frac) m.chan_flag[c] = 1;
  }
  if (nlive > 0)
    for (size_t b = 0; b < nblk; ++b) {
      uint64_t n = 0;
      for (size_t c = 0; c < nc; ++c) n += live[c] ? pre[c * nblk + b] : 0;
      if (static_cast<double>(n) / static_cast<double>(nlive) > p.block_frac) m.block_flag[b] = 1;
    }
  m.cell.assign(nc * nblk, 0);
  for (size_t c = 0; c < nc; ++c)
    for (size_t b = 0; b < nblk; ++b)
      m.cell[c * nblk + b] = (pre[c * nblk + b] | m.chan_flag[c] | m.block_flag[b]) ? 1 : 0;
  // fill values, output killmask
  m.fill.assign(nc, 0);
  m.killmask.assign(nc, 1);
  for (size_t c = 0; c < nc; ++c) {
    int64_t a = 0, n = 0;
    for (size_t b = 0; b < nblk; ++b)
      if (!m.cell[c * nblk + b]) {
        a += static_cast<int64_t>(S1[c * nblk + b]);
        n += len[b];
      }
    if (n > 0) m.fill[c] = static_cast<int32_t>(rfi_rdiv(a, n));
    if (n == 0 || !live[c]) m.killmask[c] = 0;
  }
  m.G.assign(nblk, 0);
  m.nb.assign(nblk, 0);
  for (size_t b = 0; b < nblk; ++b) {
    int64_t a = 0, n = 0;
    for (size_t c = 0; c < nc; ++c)
      if (!m.cell[c * nblk + b]) {
        a += m.fill[c];
        n += 1;
      }
    m.nb[b] = static_cast<int32_t>(n);
    if (n > 0) m.G[b] = static_cast<int32_t>(rfi_rdiv(a, n));
  }
  return m;
}

// ------------------------------------------------------------ mask file ----
namespace {

template <class T>
void put(std::vector<char>& b, T v) {
  const char* p = reinterpret_cast<const char*>(&v);
  b.insert(b.end(), p, p + sizeof(T));
}

template <class T>
T get(const std::vector<char>& b, size_t& off) {
  PSOUP_CHECK(off + sizeof(T) <= b.size(), "rfi mask file truncated");
  T v;
  std::memcpy(&v, b.data() + off, sizeof(T));
  off += sizeof(T);
  return v;
}

void write_atomically(const std::string& path, const std::vector<char>& b) {
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open output " << tmp);
  const bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  if (std::fclose(fo) != 0 || !ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace

void write_rfi_mask(const std::string& path, const RfiMask& m, const RfiParams& p, const RfiMaskHeader& h) {
  const size_t nc = static_cast<size_t>(m.nchans), nblk = static_cast<size_t>(m.nblk);
  PSOUP_CHECK(m.chan_flag.size() == nc && m.block_flag.size() == nblk && m.cell.size() == nc * nblk &&
                  m.fill.size() == nc && m.G.size() == nblk,
              "rfi mask: inconsistent sizes");
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'M', 'A', 'S', 'K', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  put<uint32_t>(b, static_cast<uint32_t>(m.nchans));
  put<uint32_t>(b, static_cast<uint32_t>(m.nblk));
  put<uint32_t>(b, h.nbits);
  put<uint32_t>(b, p.zero_dm ? 1u : 0u);
  put<uint64_t>(b, m.nsamps);
  put<uint64_t>(b, m.block);
  put<double>(b, h.tsamp);
  put<double>(b, p.thresh);
  put<double>(b, p.chan_frac);
  put<double>(b, p.block_frac);
  b.insert(b.end(), m.chan_flag.begin(), m.chan_flag.end());
  b.insert(b.end(), m.block_flag.begin(), m.block_flag.end());
  b.insert(b.end(), m.cell.begin(), m.cell.end());
  for (int32_t v : m.fill) put<int32_t>(b, v);
  for (int32_t v : m.G) put<int32_t>(b, v);
  write_atomically(path, b);
}

RfiMask read_rfi_mask(const std::string& path, RfiParams* p, RfiMaskHeader* h) {
  std::ifstream in(path, std::ios::binary);
  PSOUP_CHECK(static_cast<bool>(in), "cannot open rfi mask " << path);
  std::vector<char> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  PSOUP_CHECK(b.size() >= 8 && std::memcmp(b.data(), "PSMASK01", 8) == 0, path << " is not an rfi mask file");
  size_t off = 8;
  RfiMask m;
  RfiParams pp;
  RfiMaskHeader hh;
  m.nchans = static_cast<int>(get<uint32_t>(b, off));
  m.nblk = get<uint32_t>(b, off);
  hh.nbits = get<uint32_t>(b, off);
  pp.zero_dm = get<uint32_t>(b, off) != 0;
  m.nsamps = get<uint64_t>(b, off);
  m.block = get<uint64_t>(b, off);
  pp.block = m.block;
  hh.tsamp = get<double>(b, off);
  pp.thresh = get<double>(b, off);
  pp.chan_frac = get<double>(b, off);
  pp.block_frac = get<double>(b, off);
  const size_t nc = static_cast<size_t>(m.nchans), nblk = static_cast<size_t>(m.nblk);
  PSOUP_CHECK(m.nchans > 0 && nblk > 0 && b.size() == off + nc + nblk + nc * nblk + 4 * nc + 4 * nblk,
              "rfi mask file " << path << " has the wrong size");
  auto bytes = [&](size_t n) {
    std::vector<uint8_t> v(b.begin() + static_cast<std::ptrdiff_t>(off), b.begin() + static_cast<std::ptrdiff_t>(off + n));
    off += n;
    return v;
  };
  m.chan_flag = bytes(nc);
  m.block_flag = bytes(nblk);
  m.cell = bytes(nc * nblk);
  m.fill.resize(nc);
  for (size_t c = 0; c < nc; ++c) m.fill[c] = get<int32_t>(b, off);
  m.G.resize(nblk);
  for (size_t i = 0; i < nblk; ++i) m.G[i] = get<int32_t>(b, off);
  // derived: n_b and the killmask (a channel without an unflagged cell)
  m.nb.assign(nblk, 0);
  m.killmask.assign(nc, 0);
  for (size_t c = 0; c < nc; ++c)
    for (size_t i = 0; i < nblk; ++i)
      if (!m.cell[c * nblk + i]) {
        m.nb[i] += 1;
        m.killmask[c] = 1;
      }
  if (p) *p = pp;
  if (h) *h = hh;
  return m;
}

void write_killfile(const std::string& path, const std::vector<int>& killmask) {
  std::vector<char> b;
  for (int k : killmask) {
    b.push_back(k ? '1' : '0');
    b.push_back('\n');
  }
  write_atomically(path, b);
}

std::string rfi_summary_comment(const RfiMask& m, const RfiParams& p) {
  char buf[512];
  const double share = m.cell.empty() ? 0.0 : static_cast<double>(m.flagged_cells()) / static_cast<double>(m.cell.size());
  std::snprintf(buf, sizeof(buf),
                "# rfi: flagged_channels: %llu of %d  flagged_blocks: %llu of %llu  flagged_cell_share: %.6f\n"
                "# rfi: block: %llu  thresh: %g  chan_frac: %g  block_frac: %g  zero_dm: %d\n",
                static_cast<unsigned long long>(m.flagged_chans()), m.nchans,
                static_cast<unsigned long long>(m.flagged_blocks()), static_cast<unsigned long long>(m.nblk), share,
                static_cast<unsigned long long>(p.block), p.thresh, p.chan_frac, p.block_frac, p.zero_dm ? 1 : 0);
  return std::string(buf);
}

}  // namespace psoup
