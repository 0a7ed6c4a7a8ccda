// burstopt: BurstOptimiser, the burst-file reader, the pipeline and the result
// file.  See psoup/burstopt.hpp.
#include "psoup/burstopt.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "psoup/plan.hpp"

namespace psoup {

// ------------------------------------------------------------ optimiser ----
BurstOptimiser::BurstOptimiser(const BurstOptGeom& g, const BurstOptGrid& grid, hipStream_t stream,
                               size_t batch_bytes)
    : g_(g), grid_(grid), stream_(stream), batch_bytes_(batch_bytes) {
  burst_opt_check_grid(grid_);
  PSOUP_CHECK(g_.ntime >= 2 && g_.ntime <= kern::kBoptMaxTime && g_.nsub >= 1 && g_.ndm >= 1 && g_.ndm <= 65536,
              "burst opt: the cutouts need ntime in 2.." << kern::kBoptMaxTime << ", nsub >= 1 and ndm in 1..65536");
  dims_.ntime = g_.ntime;
  dims_.nsub = g_.nsub;
  dims_.ndm = g_.ndm;
  dims_.nfine = grid_.nfine;
  dims_.nw = kern::bopt_nwidths(g_.ntime);
}

BurstOptimiser::~BurstOptimiser() { (void)hipStreamSynchronize(stream_); }

size_t BurstOptimiser::bytes_per_candidate() const {
  const size_t nw = static_cast<size_t>(dims_.nw), nt = static_cast<size_t>(g_.ntime);
  const size_t rows = static_cast<size_t>(g_.ndm) + grid_.nfine;
  const size_t in = (static_cast<size_t>(g_.nsub) + g_.ndm) * nt + static_cast<size_t>(grid_.nfine) * g_.nsub;
  const size_t out = nw * (4 + 2 * rows);
  return (in + out) * sizeof(int32_t) + 2 * nw * sizeof(uint64_t);
}

int BurstOptimiser::batch_size() const {
  return static_cast<int>(std::min<size_t>(std::max<size_t>(1, batch_bytes_ / bytes_per_candidate()), 65535));
}

std::vector<BurstOptSearch> BurstOptimiser::search(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* sf,
                                                   size_t ncand) {
  const size_t nw = static_cast<size_t>(dims_.nw), nt = static_cast<size_t>(g_.ntime);
  const size_t rows = static_cast<size_t>(g_.ndm) + grid_.nfine;
  const size_t nds = static_cast<size_t>(g_.nsub) * nt, ndmt = static_cast<size_t>(g_.ndm) * nt;
  const size_t nsf = static_cast<size_t>(grid_.nfine) * g_.nsub;
  for (size_t c = 0; c < ncand; ++c)
    for (size_t j = 0; j < nsf; ++j)
      PSOUP_CHECK(sf[c * nsf + j] >= -g_.ntime && sf[c * nsf + j] <= g_.ntime,
                  "burst opt: candidate " << c << " has a shift outside [-ntime, ntime]");
  std::vector<BurstOptSearch> out(ncand);
  const size_t bs = static_cast<size_t>(batch_size());
  DeviceBuffer<int32_t> b_ds, b_dmt, b_sf, b_val, b_idx, b_curve, b_bin;
  DeviceBuffer<uint64_t> b_keys;
  for (size_t b0 = 0; b0 < ncand; b0 += bs) {
    const size_t nb = std::min(bs, ncand - b0);
    b_ds.resize(nb * nds);
    b_dmt.resize(nb * ndmt);
    b_sf.resize(nb * nsf);
    b_keys.resize(nb * 2 * nw);
    b_val.resize(nb * 2 * nw);
    b_idx.resize(nb * 2 * nw);
    b_curve.resize(nb * nw * rows);
    b_bin.resize(nb * nw * rows);
    PSOUP_HIP_CHECK(
        hipMemcpyAsync(b_ds.data(), d_ds + b0 * nds, nb * nds * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    PSOUP_HIP_CHECK(
        hipMemcpyAsync(b_dmt.data(), d_dmt + b0 * ndmt, nb * ndmt * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    PSOUP_HIP_CHECK(
        hipMemcpyAsync(b_sf.data(), sf + b0 * nsf, nb * nsf * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    kern::burst_search(b_ds.data(), b_dmt.data(), b_sf.data(), dims_, static_cast<int>(nb), b_keys.data(),
                       b_val.data(), b_idx.data(), b_curve.data(), b_bin.data(), stream_);
    ++nbatches_;
    std::vector<int32_t> val(nb * 2 * nw), idx(nb * 2 * nw), curve(nb * nw * rows), bin(nb * nw * rows);
    auto fetch = [&](std::vector<int32_t>& h, const DeviceBuffer<int32_t>& dev) {
      PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), dev.data(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    };
    fetch(val, b_val);
    fetch(idx, b_idx);
    fetch(curve, b_curve);
    fetch(bin, b_bin);
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < nb; ++i) {
      BurstOptSearch& r = out[b0 + i];
      r.best_val.assign(val.begin() + i * 2 * nw, val.begin() + (i + 1) * 2 * nw);
      r.best_idx.assign(idx.begin() + i * 2 * nw, idx.begin() + (i + 1) * 2 * nw);
      r.curve.assign(curve.begin() + i * nw * rows, curve.begin() + (i + 1) * nw * rows);
      r.curve_bin.assign(bin.begin() + i * nw * rows, bin.begin() + (i + 1) * nw * rows);
    }
  }
  return out;
}

void BurstOptimiser::search_device(const int32_t* d_ds, const int32_t* d_dmt, const int32_t* d_sf, size_t ncand,
                                   int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_curve, int32_t* d_curve_bin) {
  const size_t nw = static_cast<size_t>(dims_.nw), nt = static_cast<size_t>(g_.ntime);
  const size_t rows = static_cast<size_t>(g_.ndm) + grid_.nfine;
  const size_t nds = static_cast<size_t>(g_.nsub) * nt, ndmt = static_cast<size_t>(g_.ndm) * nt;
  const size_t nsf = static_cast<size_t>(grid_.nfine) * g_.nsub;
  const size_t most = 65535;  // candidates of one launch (grid y)
  d_keys_.resize(std::min(ncand, most) * 2 * nw);
  for (size_t b0 = 0; b0 < ncand; b0 += most) {
    const size_t nb = std::min(most, ncand - b0);
    kern::burst_search(d_ds + b0 * nds, d_dmt + b0 * ndmt, d_sf + b0 * nsf, dims_, static_cast<int>(nb),
                       d_keys_.data(), d_best_val + b0 * 2 * nw, d_best_idx + b0 * 2 * nw, d_curve + b0 * nw * rows,
                       d_curve_bin + b0 * nw * rows, stream_);
    ++nbatches_;
  }
}

std::vector<BurstOptResult> BurstOptimiser::optimise(const std::vector<BurstOptInput>& cands,
                                                     const std::vector<float>& delays) {
  const size_t nc = cands.size(), nt = static_cast<size_t>(g_.ntime);
  const size_t nds = static_cast<size_t>(g_.nsub) * nt, ndmt = static_cast<size_t>(g_.ndm) * nt;
  const size_t nsf = static_cast<size_t>(grid_.nfine) * g_.nsub;
  // every candidate is validated (and its tables built) before the first launch
  std::vector<BurstOptPrepared> prep(nc);
  std::vector<BurstOptShifts> shifts(nc);
  for (size_t i = 0; i < nc; ++i) {
    prep[i] = burst_opt_prepare(i, g_, cands[i]);
    shifts[i] = burst_opt_shifts(g_, grid_, cands[i].dm, cands[i].tscrunch, cands[i].dms, delays);
  }
  std::vector<BurstOptResult> out(nc);
  const size_t bs = static_cast<size_t>(batch_size());
  std::vector<int32_t> ds, dmt, sf;
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    ds.resize(nb * nds);
    dmt.resize(nb * ndmt);
    sf.resize(nb * nsf);
    for (size_t i = 0; i < nb; ++i) {
      std::copy(prep[b0 + i].d_ds.begin(), prep[b0 + i].d_ds.end(), ds.begin() + i * nds);
      std::copy(prep[b0 + i].d_dmt.begin(), prep[b0 + i].d_dmt.end(), dmt.begin() + i * ndmt);
      std::copy(shifts[b0 + i].sf.begin(), shifts[b0 + i].sf.end(), sf.begin() + i * nsf);
    }
    const std::vector<BurstOptSearch> found = search(ds.data(), dmt.data(), sf.data(), nb);
    for (size_t i = 0; i < nb; ++i)
      out[b0 + i] = burst_opt_finish(g_, grid_, cands[b0 + i], prep[b0 + i], shifts[b0 + i], found[i]);
  }
  return out;
}

// ----------------------------------------------------------- burst file ----
namespace {
template <class T>
T take(const std::vector<char>& b, size_t& o) {
  T v;
  std::memcpy(&v, b.data() + o, sizeof(T));  // gfx950 hosts are little-endian
  o += sizeof(T);
  return v;
}

template <class T>
void put(std::vector<char>& b, const T& v) {
  static_assert(std::is_trivially_copyable<T>::value, "put: plain values");
  const char* p = reinterpret_cast<const char*>(&v);
  b.insert(b.end(), p, p + sizeof(T));
}

template <class T>
void put_all(std::vector<char>& b, const std::vector<T>& v) {
  const char* p = reinterpret_cast<const char*>(v.data());
  b.insert(b.end(), p, p + v.size() * sizeof(T));
}

template <class T>
void take_all(const std::vector<char>& b, size_t& o, std::vector<T>& v, size_t n) {
  v.resize(n);
  std::memcpy(v.data(), b.data() + o, n * sizeof(T));
  o += n * sizeof(T);
}
}  // namespace

BurstFile read_burst_file(const std::string& path, int limit) {
  std::ifstream in(path, std::ios::binary);
  PSOUP_CHECK(in.good(), "cannot open burst file " << path);
  std::vector<char> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  PSOUP_CHECK(b.size() >= 64 && std::memcmp(b.data(), "PSBRST01", 8) == 0, path << ": not a burst-cutout file");
  size_t o = 8;
  BurstFile f;
  const uint32_t ncand = take<uint32_t>(b, o);
  f.geom.ntime = static_cast<int>(take<uint32_t>(b, o));
  f.geom.nsub = static_cast<int>(take<uint32_t>(b, o));
  f.geom.ndm = static_cast<int>(take<uint32_t>(b, o));
  f.geom.nchans = static_cast<int>(take<uint32_t>(b, o));
  f.nbits = take<uint32_t>(b, o);
  f.nsamps = take<uint64_t>(b, o);
  f.geom.tsamp = take<double>(b, o);
  f.geom.fch1 = take<double>(b, o);
  f.geom.foff = take<double>(b, o);
  PSOUP_CHECK(f.geom.ntime >= 1 && f.geom.ntime <= 65536 && f.geom.nsub >= 1 && f.geom.nsub <= 65536 &&
                  f.geom.ndm >= 1 && f.geom.ndm <= 65536,
              path << ": bad cutout dimensions");
  const size_t nt = static_cast<size_t>(f.geom.ntime), ns = static_cast<size_t>(f.geom.nsub),
               nd = static_cast<size_t>(f.geom.ndm);
  const size_t rec = 32 + 4 * nd + 4 * ns + 8 * (ns + nd) * nt;
  // no product of header fields: a hostile count cannot wrap round to the file's size
  PSOUP_CHECK((b.size() - 64) % rec == 0 && static_cast<size_t>(ncand) == (b.size() - 64) / rec,
              path << ": truncated burst-cutout file");
  size_t take_n = ncand;
  if (limit >= 0) take_n = std::min<size_t>(take_n, static_cast<size_t>(limit));
  f.candidates.resize(take_n);
  for (size_t i = 0; i < take_n; ++i) {
    BurstOptInput& c = f.candidates[i];
    o = 64 + i * rec;
    c.sample = take<uint64_t>(b, o);
    c.width = take<uint32_t>(b, o);
    c.tscrunch = take<uint32_t>(b, o);
    c.t0 = take<int64_t>(b, o);
    c.dm = take<float>(b, o);
    c.snr = take<float>(b, o);
    take_all(b, o, c.dms, nd);
    take_all(b, o, c.nactive, ns);
    take_all(b, o, c.ds_sums, ns * nt);
    take_all(b, o, c.ds_hits, ns * nt);
    take_all(b, o, c.dmt_sums, nd * nt);
    take_all(b, o, c.dmt_hits, nd * nt);
  }
  return f;
}

// ------------------------------------------------------------ pipeline ----
BurstOptRun run_bopt_pipeline(const BurstOptCmdLineOptions& args) {
  BurstOptRun run;
  Stopwatch t_total, t_read, t_search;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  BurstFile f = read_burst_file(args.infilename, args.limit);
  t_read.stop();
  PSOUP_CHECK(!f.candidates.empty(), "burstopt: no candidates");
  BurstOptGrid grid;
  grid.nfine = args.nfine;
  grid.fine_half_range = args.fine_half_range;
  const std::vector<float> delays = generate_delay_table(f.geom.nchans, f.geom.tsamp, f.geom.fch1, f.geom.foff);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  PSOUP_HIP_CHECK(hipSetDevice(0));
  Stream stream;
  t_search.start();
  BurstOptimiser opt(f.geom, grid, stream.get());
  run.results = opt.optimise(f.candidates, delays);
  t_search.stop();
  log_verbose("burst opt: " + std::to_string(f.candidates.size()) + " candidates, " +
              std::to_string(f.geom.ndm + grid.nfine) + " rows each, " + std::to_string(opt.batches()) + " launches");
  BoptFileHeader& h = run.header;
  h.ncand = static_cast<uint32_t>(f.candidates.size());
  h.ntime = static_cast<uint32_t>(f.geom.ntime);
  h.nsub = static_cast<uint32_t>(f.geom.nsub);
  h.ndm = static_cast<uint32_t>(f.geom.ndm);
  h.nchans = static_cast<uint32_t>(f.geom.nchans);
  h.nbits = f.nbits;
  h.nfine = static_cast<uint32_t>(grid.nfine);
  h.nw = static_cast<uint32_t>(opt.nwidths());
  h.nsamps = f.nsamps;
  h.tsamp = f.geom.tsamp;
  h.fch1 = f.geom.fch1;
  h.foff = f.geom.foff;
  h.fine_half_range = grid.fine_half_range;
  run.candidates.resize(f.candidates.size());
  for (size_t i = 0; i < f.candidates.size(); ++i) {
    const BurstOptInput& c = f.candidates[i];
    BurstOptInput& k = run.candidates[i];
    k.sample = c.sample;
    k.width = c.width;
    k.tscrunch = c.tscrunch;
    k.t0 = c.t0;
    k.dm = c.dm;
    k.snr = c.snr;
  }
  write_bopt_file(args.outfilename, h, run.candidates, run.results);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

void write_bopt_file(const std::string& path, const BoptFileHeader& h, const std::vector<BurstOptInput>& cands,
                     const std::vector<BurstOptResult>& results) {
  PSOUP_CHECK(cands.size() == results.size() && cands.size() == h.ncand, "bopt file: candidate count mismatch");
  const size_t nw = h.nw, rows = static_cast<size_t>(h.ndm) + h.nfine;
  for (size_t i = 0; i < results.size(); ++i) {
    const BurstOptResult& r = results[i];
    PSOUP_CHECK(r.dms.size() == h.ndm && r.dmf.size() == h.nfine && r.mbar_dmt.size() == h.ndm &&
                    r.search.best_val.size() == 2 * nw && r.search.best_idx.size() == 2 * nw &&
                    r.search.curve.size() == nw * rows && r.search.curve_bin.size() == nw * rows &&
                    r.band.size() == h.nsub && r.profile.size() == h.ntime,
                "bopt file: candidate " << i << " has the wrong shape");
  }
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open bopt output " << tmp);
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'B', 'O', 'P', 'T', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  for (uint32_t v : {h.ncand, h.ntime, h.nsub, h.ndm, h.nchans, h.nbits, h.nfine, h.nw}) put(b, v);
  put(b, h.nsamps);
  for (double v : {h.tsamp, h.fch1, h.foff, h.fine_half_range}) put(b, v);
  bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  for (size_t i = 0; ok && i < cands.size(); ++i) {
    const BurstOptResult& r = results[i];
    const BurstOptInput& c = cands[i];
    b.clear();
    put(b, c.sample);
    put(b, c.width);
    put(b, c.tscrunch);
    put(b, c.t0);
    put(b, c.dm);
    put(b, c.snr);
    for (double v : {r.snr, r.snr_coarse, r.snr_in, r.snr_dm0, r.frac_pos, r.v, r.mbar_ds}) put(b, v);
    put(b, r.opt_sample);
    put(b, r.opt_dm);
    put(b, r.coarse_dm);
    for (uint32_t v : {r.opt_width, r.opt_kf, r.opt_bin, r.coarse_row, r.coarse_width, r.coarse_bin, r.flags, uint32_t(0)})
      put(b, v);
    put_all(b, r.dms);
    put_all(b, r.dmf);
    put_all(b, r.mbar_dmt);
    put_all(b, r.search.best_val);
    put_all(b, r.search.best_idx);
    put_all(b, r.search.curve);
    put_all(b, r.search.curve_bin);
    put_all(b, r.band);
    put_all(b, r.profile);
    ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  }
  ok = (std::fclose(fo) == 0) && ok;
  if (!ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write bopt output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace psoup
