// cubeopt: CubeOptimiser, the cube-file reader, the pipeline and the result
// file.  See psoup/cubeopt.hpp.
#include "psoup/cubeopt.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "psoup/plan.hpp"

namespace psoup {

// ------------------------------------------------------------ optimiser ----
CubeOptimiser::CubeOptimiser(const CubeOptGeom& g, const CubeOptGrid& grid, hipStream_t stream, size_t batch_bytes)
    : g_(g), grid_(grid), stream_(stream), batch_bytes_(batch_bytes) {
  cube_opt_check_grid(grid_);
  PSOUP_CHECK(g_.nints >= 1 && g_.nsub >= 1 && g_.nbins >= 2 && g_.nbins <= kern::kOptMaxBins,
              "cube opt: the cubes need nints >= 1, nsub >= 1 and nbins in 2.." << kern::kOptMaxBins);
  dims_.nints = g_.nints;
  dims_.nsub = g_.nsub;
  dims_.nbins = g_.nbins;
  dims_.ndm = grid_.ndm;
  dims_.np = grid_.np;
  dims_.npd = grid_.npd;
  dims_.nw = kern::opt_nwidths(g_.nbins);
}

CubeOptimiser::~CubeOptimiser() { (void)hipStreamSynchronize(stream_); }

size_t CubeOptimiser::bytes_per_candidate() const {
  const size_t nw = static_cast<size_t>(dims_.nw), ntr = static_cast<size_t>(grid_.np) * grid_.npd;
  const size_t in = static_cast<size_t>(g_.nints) * g_.nsub * g_.nbins + static_cast<size_t>(grid_.ndm) * g_.nsub +
                    ntr * g_.nints;
  const size_t out = nw * (3 + grid_.ndm + ntr);
  return (in + out) * sizeof(int32_t) + nw * sizeof(uint64_t);
}

int CubeOptimiser::batch_size() const {
  return static_cast<int>(std::min<size_t>(std::max<size_t>(1, batch_bytes_ / bytes_per_candidate()), 65535));
}

std::vector<CubeOptSearch> CubeOptimiser::search(const int32_t* d, const int32_t* sdm, const int32_t* st,
                                                 size_t ncand) {
  const size_t nw = static_cast<size_t>(dims_.nw), ntr = static_cast<size_t>(grid_.np) * grid_.npd;
  const size_t nd = static_cast<size_t>(g_.nints) * g_.nsub * g_.nbins;
  const size_t nsdm = static_cast<size_t>(grid_.ndm) * g_.nsub, nst = ntr * g_.nints;
  PSOUP_CHECK(static_cast<size_t>(g_.nints) * g_.nbins <= static_cast<size_t>(kern::kOptMaxPlane),
              "cube opt: nints * nbins exceeds " << kern::kOptMaxPlane);
  PSOUP_CHECK(static_cast<uint64_t>(grid_.ndm) * ntr * g_.nbins < (uint64_t(1) << 31),
              "cube opt: the trial bins do not fit 31 bits");
  // the kernel indexes with the shifts: every one must lie in [0, nbins)
  for (size_t c = 0; c < ncand; ++c) {
    for (size_t j = 0; j < nsdm; ++j)
      PSOUP_CHECK(sdm[c * nsdm + j] >= 0 && sdm[c * nsdm + j] < g_.nbins,
                  "cube opt: candidate " << c << " has a DM shift outside [0, nbins)");
    for (size_t j = 0; j < nst; ++j)
      PSOUP_CHECK(st[c * nst + j] >= 0 && st[c * nst + j] < g_.nbins,
                  "cube opt: candidate " << c << " has a subint shift outside [0, nbins)");
  }
  std::vector<CubeOptSearch> out(ncand);
  const size_t bs = static_cast<size_t>(batch_size());
  DeviceBuffer<int32_t> d_d, d_sdm, d_st, d_val, d_idx, d_centre, d_dmc, d_ppd;
  DeviceBuffer<uint64_t> d_keys;
  for (size_t b0 = 0; b0 < ncand; b0 += bs) {
    const size_t nb = std::min(bs, ncand - b0);
    d_d.resize(nb * nd);
    d_sdm.resize(nb * nsdm);
    d_st.resize(nb * nst);
    d_keys.resize(nb * nw);
    d_val.resize(nb * nw);
    d_idx.resize(nb * nw);
    d_centre.resize(nb * nw);
    d_dmc.resize(nb * nw * grid_.ndm);
    d_ppd.resize(nb * nw * ntr);
    PSOUP_HIP_CHECK(hipMemcpyAsync(d_d.data(), d + b0 * nd, nb * nd * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    PSOUP_HIP_CHECK(
        hipMemcpyAsync(d_sdm.data(), sdm + b0 * nsdm, nb * nsdm * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    PSOUP_HIP_CHECK(
        hipMemcpyAsync(d_st.data(), st + b0 * nst, nb * nst * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    kern::cube_search(d_d.data(), d_sdm.data(), d_st.data(), dims_, static_cast<int>(nb), d_keys.data(), d_val.data(),
                      d_idx.data(), d_dmc.data(), d_ppd.data(), d_centre.data(), stream_);
    ++nbatches_;
    std::vector<int32_t> val(nb * nw), idx(nb * nw), cen(nb * nw), dmc(nb * nw * grid_.ndm), ppd(nb * nw * ntr);
    auto fetch = [&](std::vector<int32_t>& h, const DeviceBuffer<int32_t>& dev) {
      PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), dev.data(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    };
    fetch(val, d_val);
    fetch(idx, d_idx);
    fetch(cen, d_centre);
    fetch(dmc, d_dmc);
    fetch(ppd, d_ppd);
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < nb; ++i) {
      CubeOptSearch& r = out[b0 + i];
      r.best_val.assign(val.begin() + i * nw, val.begin() + (i + 1) * nw);
      r.best_idx.assign(idx.begin() + i * nw, idx.begin() + (i + 1) * nw);
      r.centre.assign(cen.begin() + i * nw, cen.begin() + (i + 1) * nw);
      r.dmcurve.assign(dmc.begin() + i * nw * grid_.ndm, dmc.begin() + (i + 1) * nw * grid_.ndm);
      r.ppd.assign(ppd.begin() + i * nw * ntr, ppd.begin() + (i + 1) * nw * ntr);
    }
  }
  return out;
}

void CubeOptimiser::search_device(const int32_t* d_d, const int32_t* d_sdm, const int32_t* d_st, size_t ncand,
                                  int32_t* d_best_val, int32_t* d_best_idx, int32_t* d_dmcurve, int32_t* d_ppd,
                                  int32_t* d_centre) {
  const size_t nw = static_cast<size_t>(dims_.nw), ntr = static_cast<size_t>(grid_.np) * grid_.npd;
  const size_t nd = static_cast<size_t>(g_.nints) * g_.nsub * g_.nbins;
  const size_t nsdm = static_cast<size_t>(grid_.ndm) * g_.nsub, nst = ntr * g_.nints;
  const size_t most = 65535;  // candidates of one launch (grid z)
  d_keys_.resize(std::min(ncand, most) * nw);
  for (size_t b0 = 0; b0 < ncand; b0 += most) {
    const size_t nb = std::min(most, ncand - b0);
    kern::cube_search(d_d + b0 * nd, d_sdm + b0 * nsdm, d_st + b0 * nst, dims_, static_cast<int>(nb), d_keys_.data(),
                      d_best_val + b0 * nw, d_best_idx + b0 * nw, d_dmcurve + b0 * nw * grid_.ndm,
                      d_ppd + b0 * nw * ntr, d_centre + b0 * nw, stream_);
    ++nbatches_;
  }
}

std::vector<CubeOptResult> CubeOptimiser::optimise(const std::vector<CubeOptInput>& cands,
                                                   const std::vector<float>& delays) {
  const size_t nc = cands.size();
  const size_t nd = static_cast<size_t>(g_.nints) * g_.nsub * g_.nbins;
  const size_t nsdm = static_cast<size_t>(grid_.ndm) * g_.nsub;
  const size_t nst = static_cast<size_t>(grid_.np) * grid_.npd * g_.nints;
  // every candidate is validated (and its tables built) before the first launch
  std::vector<CubeOptPrepared> prep(nc);
  std::vector<CubeOptShifts> shifts(nc);
  for (size_t i = 0; i < nc; ++i) {
    prep[i] = cube_opt_prepare(i, g_, grid_, cands[i]);
    shifts[i] = cube_opt_shifts(g_, grid_, cands[i].period, cands[i].dm, delays);
  }
  std::vector<CubeOptResult> out(nc);
  const size_t bs = static_cast<size_t>(batch_size());
  std::vector<int32_t> d, sdm, st;
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    d.resize(nb * nd);
    sdm.resize(nb * nsdm);
    st.resize(nb * nst);
    for (size_t i = 0; i < nb; ++i) {
      std::copy(prep[b0 + i].d.begin(), prep[b0 + i].d.end(), d.begin() + i * nd);
      std::copy(shifts[b0 + i].sdm.begin(), shifts[b0 + i].sdm.end(), sdm.begin() + i * nsdm);
      std::copy(shifts[b0 + i].st.begin(), shifts[b0 + i].st.end(), st.begin() + i * nst);
    }
    const std::vector<CubeOptSearch> found = search(d.data(), sdm.data(), st.data(), nb);
    for (size_t i = 0; i < nb; ++i)
      out[b0 + i] = cube_opt_finish(g_, grid_, cands[b0 + i].period, cands[b0 + i].acc, prep[b0 + i], shifts[b0 + i],
                                    found[i]);
  }
  return out;
}

// ------------------------------------------------------------ cube file ----
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
}  // namespace

CubeFile read_cube_file(const std::string& path, int limit) {
  std::ifstream in(path, std::ios::binary);
  PSOUP_CHECK(in.good(), "cannot open cube file " << path);
  std::vector<char> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  PSOUP_CHECK(b.size() >= 64 && std::memcmp(b.data(), "PSCUBE01", 8) == 0, path << ": not a fold-cube file");
  size_t o = 8;
  CubeFile f;
  const uint32_t ncand = take<uint32_t>(b, o);
  f.geom.nints = static_cast<int>(take<uint32_t>(b, o));
  f.geom.nsub = static_cast<int>(take<uint32_t>(b, o));
  f.geom.nbins = static_cast<int>(take<uint32_t>(b, o));
  f.geom.nchans = static_cast<int>(take<uint32_t>(b, o));
  f.nbits = take<uint32_t>(b, o);
  f.geom.fold_nsamps = take<uint64_t>(b, o);
  f.geom.tsamp = take<double>(b, o);
  f.geom.fch1 = take<double>(b, o);
  f.geom.foff = take<double>(b, o);
  PSOUP_CHECK(f.geom.nints >= 1 && f.geom.nints <= 65536 && f.geom.nsub >= 1 && f.geom.nsub <= 65536 &&
                  f.geom.nbins >= 1 && f.geom.nbins <= 65536,
              path << ": bad cube dimensions");
  const size_t ni = static_cast<size_t>(f.geom.nints), ns = static_cast<size_t>(f.geom.nsub),
               nb = static_cast<size_t>(f.geom.nbins);
  const size_t rec = 16 + 4 * ns + 4 * ni * nb + 8 * ni * ns * nb;
  // no product of header fields: a hostile count cannot wrap round to the file's size
  PSOUP_CHECK((b.size() - 64) % rec == 0 && static_cast<size_t>(ncand) == (b.size() - 64) / rec,
              path << ": truncated fold-cube file");
  size_t take_n = ncand;
  if (limit >= 0) take_n = std::min<size_t>(take_n, static_cast<size_t>(limit));
  f.candidates.resize(take_n);
  for (size_t i = 0; i < take_n; ++i) {
    CubeOptInput& c = f.candidates[i];
    o = 64 + i * rec;
    c.period = take<double>(b, o);
    c.dm = take<float>(b, o);
    c.acc = take<float>(b, o);
    c.nactive.resize(ns);
    c.hits.resize(ni * nb);
    c.sums.resize(ni * ns * nb);
    std::memcpy(c.nactive.data(), b.data() + o, 4 * ns);
    o += 4 * ns;
    std::memcpy(c.hits.data(), b.data() + o, 4 * ni * nb);
    o += 4 * ni * nb;
    std::memcpy(c.sums.data(), b.data() + o, 8 * ni * ns * nb);
  }
  return f;
}

// ------------------------------------------------------------ pipeline ----
CubeOptRun run_opt_pipeline(const CubeOptCmdLineOptions& args) {
  CubeOptRun run;
  Stopwatch t_total, t_read, t_search;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  CubeFile f = read_cube_file(args.infilename, args.limit);
  t_read.stop();
  PSOUP_CHECK(!f.candidates.empty(), "cubeopt: no candidates");
  CubeOptGrid grid;
  grid.ndm = args.ndm;
  grid.dm_half_range = args.dm_half_range;
  grid.np = args.np;
  grid.p_step = args.p_step;
  grid.npd = args.npd;
  grid.pd_step = args.pd_step;
  const std::vector<float> delays = generate_delay_table(f.geom.nchans, f.geom.tsamp, f.geom.fch1, f.geom.foff);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  PSOUP_HIP_CHECK(hipSetDevice(0));
  Stream stream;
  t_search.start();
  CubeOptimiser opt(f.geom, grid, stream.get());
  run.results = opt.optimise(f.candidates, delays);
  t_search.stop();
  log_verbose("cube opt: " + std::to_string(f.candidates.size()) + " candidates, " +
              std::to_string(static_cast<uint64_t>(grid.ndm) * grid.np * grid.npd) + " trials each, " +
              std::to_string(opt.batches()) + " launches");
  OptFileHeader& h = run.header;
  h.ncand = static_cast<uint32_t>(f.candidates.size());
  h.nints = static_cast<uint32_t>(f.geom.nints);
  h.nsub = static_cast<uint32_t>(f.geom.nsub);
  h.nbins = static_cast<uint32_t>(f.geom.nbins);
  h.nchans = static_cast<uint32_t>(f.geom.nchans);
  h.ndm = static_cast<uint32_t>(grid.ndm);
  h.np = static_cast<uint32_t>(grid.np);
  h.npd = static_cast<uint32_t>(grid.npd);
  h.nw = static_cast<uint32_t>(opt.nwidths());
  h.fold_nsamps = f.geom.fold_nsamps;
  h.tsamp = f.geom.tsamp;
  h.fch1 = f.geom.fch1;
  h.foff = f.geom.foff;
  h.p_step = grid.p_step;
  h.pd_step = grid.pd_step;
  h.dm_half_range = static_cast<double>(grid.dm_half_range);
  run.candidates.resize(f.candidates.size());
  for (size_t i = 0; i < f.candidates.size(); ++i) {
    run.candidates[i].period = f.candidates[i].period;
    run.candidates[i].dm = f.candidates[i].dm;
    run.candidates[i].acc = f.candidates[i].acc;
  }
  write_opt_file(args.outfilename, h, run.candidates, run.results);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

void write_opt_file(const std::string& path, const OptFileHeader& h, const std::vector<CubeOptInput>& cands,
                    const std::vector<CubeOptResult>& results) {
  PSOUP_CHECK(cands.size() == results.size() && cands.size() == h.ncand, "opt file: candidate count mismatch");
  const size_t nw = h.nw, ntr = static_cast<size_t>(h.np) * h.npd;
  for (size_t i = 0; i < results.size(); ++i) {
    const CubeOptResult& r = results[i];
    PSOUP_CHECK(r.dms.size() == h.ndm && r.search.best_val.size() == nw && r.search.best_idx.size() == nw &&
                    r.search.centre.size() == nw && r.search.dmcurve.size() == nw * h.ndm &&
                    r.search.ppd.size() == nw * ntr && r.profile.size() == h.nbins,
                "opt file: candidate " << i << " has the wrong shape");
  }
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open opt output " << tmp);
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'O', 'P', 'T', '0', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  for (uint32_t v : {h.ncand, h.nints, h.nsub, h.nbins, h.nchans, h.ndm, h.np, h.npd, h.nw, uint32_t(0)}) put(b, v);
  put(b, h.fold_nsamps);
  for (double v : {h.tsamp, h.fch1, h.foff, h.p_step, h.pd_step, h.dm_half_range}) put(b, v);
  bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  for (size_t i = 0; ok && i < cands.size(); ++i) {
    const CubeOptResult& r = results[i];
    b.clear();
    put(b, cands[i].period);
    put(b, cands[i].dm);
    put(b, cands[i].acc);
    for (double v : {r.snr, r.snr_in, r.snr_dm0, r.opt_period, r.opt_acc}) put(b, v);
    put(b, r.opt_dm);
    for (uint32_t v : {r.opt_width, r.opt_bin, r.opt_kd, r.opt_kp, r.opt_kpd, r.flags, uint32_t(0)}) put(b, v);
    put(b, r.mtot);
    put(b, r.v);
    put_all(b, r.dms);
    put_all(b, r.search.best_val);
    put_all(b, r.search.best_idx);
    put_all(b, r.search.centre);
    put_all(b, r.search.dmcurve);
    put_all(b, r.search.ppd);
    put_all(b, r.profile);
    ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  }
  ok = (std::fclose(fo) == 0) && ok;
  if (!ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write opt output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace psoup
