// Filterbank fold cubes: candidate list, CubeFolder, pipeline and the cube
// file.  See psoup/foldcube.hpp.
#include "psoup/foldcube.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "psoup/plan.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

namespace {
constexpr double kC = 299792458.0;
}

// ----------------------------------------------------------- candidates ----
std::vector<CubeCandidate> read_cube_candfile(const std::string& path, int limit) {
  std::ifstream in(path);
  PSOUP_CHECK(in.good(), "cannot open candidate file " << path);
  std::vector<CubeCandidate> out;
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t first = line.find_first_not_of(" \t\r\n");
    if (first == std::string::npos || line[first] == '#') continue;
    if (limit >= 0 && out.size() >= static_cast<size_t>(limit)) break;
    std::istringstream ss(line);
    CubeCandidate c;
    double dm = 0, acc = 0;
    ss >> c.period >> dm >> acc;
    if (ss.fail() || !std::isfinite(c.period) || !std::isfinite(dm) || !std::isfinite(acc))
      PSOUP_THROW("candidate file " << path << ": line " << lineno << " is not 'period_s dm acc': '" << line << "'");
    c.dm = static_cast<float>(dm);
    c.acc = static_cast<float>(acc);
    out.push_back(c);
  }
  return out;
}

uint64_t default_fold_nsamps(const DedispGeometry& g) {
  int64_t max_off = 0;
  for (float dm : g.dm_list)
    for (float d : g.delays) max_off = std::max<int64_t>(max_off, dm_delay_samples(dm, d));
  PSOUP_CHECK(static_cast<uint64_t>(max_off) < g.nsamps, "the largest dispersion delay exceeds the observation");
  return prev_power_of_two(g.nsamps - static_cast<uint64_t>(max_off));
}

// --------------------------------------------------------------- folder ----
CubeFolder::CubeFolder(const DeviceFilterbank& fb, const CubeParams& p, hipStream_t stream, size_t batch_bytes)
    : x_(fb.data()),
      stride_(fb.stride()),
      row_valid_(fb.geometry().nsamps),
      nchans_(fb.geometry().nchans),
      bias_(fb.geometry().bias),
      tsamp_(static_cast<float>(fb.geometry().tsamp)),
      delays_(fb.geometry().delays),
      p_(p),
      stream_(stream),
      batch_bytes_(batch_bytes) {
  init(fb.geometry().killmask);
}

CubeFolder::CubeFolder(const int8_t* d_chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias,
                       double tsamp, const std::vector<float>& delays, const std::vector<int>& killmask,
                       const CubeParams& p, hipStream_t stream, size_t batch_bytes)
    : x_(d_chan_major),
      stride_(stride),
      row_valid_(row_valid),
      nchans_(nchans),
      bias_(bias),
      tsamp_(static_cast<float>(tsamp)),
      delays_(delays),
      p_(p),
      stream_(stream),
      batch_bytes_(batch_bytes) {
  init(killmask);
}

CubeFolder::~CubeFolder() { (void)hipStreamSynchronize(stream_); }

void CubeFolder::init(const std::vector<int>& killmask) {
  PSOUP_CHECK(nchans_ >= 1, "fold cube: no channels");
  PSOUP_CHECK(x_ != nullptr && row_valid_ <= stride_, "fold cube: rows shorter than their valid length");
  PSOUP_CHECK(delays_.empty() || static_cast<int>(delays_.size()) == nchans_, "fold cube: delay table size != nchans");
  PSOUP_CHECK(killmask.empty() || static_cast<int>(killmask.size()) == nchans_, "fold cube: killmask size != nchans");
  PSOUP_CHECK(tsamp_ > 0, "fold cube: tsamp must be positive");
  PSOUP_CHECK(p_.nints >= 1 && p_.nints <= 256, "fold cube: nints must be in 1..256");
  PSOUP_CHECK(p_.nbins >= 2 && p_.nbins <= 256, "fold cube: nbins must be in 2..256");
  PSOUP_CHECK(p_.nsub >= 1 && p_.nsub <= nchans_, "fold cube: nsub must be in 1..nchans");
  PSOUP_CHECK(p_.fold_nsamps >= static_cast<uint64_t>(p_.nints) && p_.fold_nsamps <= row_valid_ &&
                  p_.fold_nsamps < (uint64_t(1) << 31),
              "fold cube: fold_nsamps " << p_.fold_nsamps << " must be in [nints, min(nsamps, 2^31))");
  // the unkilled channels in ascending order and each subband's range of them
  std::vector<int32_t> active, sub_first(static_cast<size_t>(p_.nsub) + 1, 0);
  nactive_.assign(static_cast<size_t>(p_.nsub), 0);
  for (int c = 0; c < nchans_; ++c) {
    if (!killmask.empty() && killmask[static_cast<size_t>(c)] == 0) continue;
    const int s = static_cast<int>(static_cast<int64_t>(c) * p_.nsub / nchans_);
    nactive_[static_cast<size_t>(s)] += 1;
    active.push_back(c);
  }
  for (int s = 0; s < p_.nsub; ++s) {
    sub_first[static_cast<size_t>(s) + 1] = sub_first[static_cast<size_t>(s)] + nactive_[static_cast<size_t>(s)];
    max_sub_channels_ = std::max(max_sub_channels_, nactive_[static_cast<size_t>(s)]);
  }
  d_active_.resize(std::max<size_t>(1, active.size()));
  d_sub_first_.resize(sub_first.size());
  if (!active.empty())
    PSOUP_HIP_CHECK(hipMemcpyAsync(d_active_.data(), active.data(), active.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_sub_first_.data(), sub_first.data(), sub_first.size() * sizeof(int32_t),
                                 hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // the host tables go out of scope
}

int CubeFolder::batch_size() const {
  const size_t cube = static_cast<size_t>(p_.nints) * p_.nbins;
  const size_t per = cube * p_.nsub * sizeof(int64_t) + cube * sizeof(int32_t) +
                     static_cast<size_t>(nchans_) * sizeof(int32_t) + sizeof(kern::CubeJob);
  return static_cast<int>(std::min<size_t>(std::max<size_t>(1, batch_bytes_ / per), 65535));
}

kern::CubeJob CubeFolder::job_of(double period, float acc) const {
  kern::CubeJob j;
  j.tsamp_by_period = static_cast<double>(tsamp_) / period;
  j.af = (static_cast<double>(acc) * tsamp_) / (2 * kC);
  return j;
}

void CubeFolder::check_candidate(size_t i, const CubeCandidate& c, const int32_t* off) const {
  std::ostringstream who;
  who << "fold cube: candidate " << i << " (period " << c.period << " s, dm " << c.dm << ", acc " << c.acc << ")";
  PSOUP_CHECK(std::isfinite(c.period) && c.period > 0, who.str() << ": the period must be positive");
  PSOUP_CHECK(std::isfinite(c.dm) && c.dm >= 0, who.str() << ": the DM must be non-negative");
  PSOUP_CHECK(std::isfinite(c.acc), who.str() << ": the acceleration must be finite");
  int64_t lo = 0, hi = 0;
  for (int ch = 0; ch < nchans_; ++ch) {
    lo = std::min<int64_t>(lo, off[ch]);
    hi = std::max<int64_t>(hi, off[ch]);
  }
  PSOUP_CHECK(lo >= 0, who.str() << ": negative sample offset");
  PSOUP_CHECK(static_cast<uint64_t>(hi) + p_.fold_nsamps <= row_valid_,
              who.str() << ": largest offset " << hi << " + fold_nsamps " << p_.fold_nsamps << " exceeds the "
                        << row_valid_ << " samples of the filterbank");
  // a tile's source window must fit the staged window (foldcube.hpp)
  const double slope = std::fabs(job_of(c.period, c.acc).af) * static_cast<double>(p_.fold_nsamps);
  PSOUP_CHECK(slope <= kern::kCubeMaxSlope,
              who.str() << ": the acceleration stretches the series by more than " << kern::kCubeMaxSlope);
}

void CubeFolder::launch(const int32_t* h_off, const kern::CubeJob* h_jobs, int ncand, int64_t* d_sums,
                        int32_t* d_hits) {
  kern::CubeGeom g;
  g.nchans = nchans_;
  g.stride = stride_;
  g.bias = bias_;
  g.nints = p_.nints;
  g.nsub = p_.nsub;
  g.nbins = p_.nbins;
  g.n = p_.fold_nsamps;
  const kern::CubePlan plan = kern::cube_plan(g, ncand, max_sub_channels_);
  const size_t cube = static_cast<size_t>(p_.nints) * p_.nbins;
  d_off_.resize(static_cast<size_t>(ncand) * nchans_);
  d_jobs_.resize(static_cast<size_t>(ncand));
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_off_.data(), h_off, d_off_.bytes(), hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_jobs_.data(), h_jobs, d_jobs_.bytes(), hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipMemsetAsync(d_sums, 0, cube * p_.nsub * ncand * sizeof(int64_t), stream_));
  PSOUP_HIP_CHECK(hipMemsetAsync(d_hits, 0, cube * ncand * sizeof(int32_t), stream_));
  kern::fold_cube(x_, g, d_active_.data(), d_sub_first_.data(), d_off_.data(), d_jobs_.data(), ncand, plan, d_sums,
                  d_hits, stream_);
  ++nbatches_;
}

std::vector<CubeResult> CubeFolder::fold(const std::vector<CubeCandidate>& cands) {
  PSOUP_CHECK(static_cast<int>(delays_.size()) == nchans_, "fold cube: no delay table");
  const size_t nc = cands.size();
  std::vector<int32_t> off(nc * static_cast<size_t>(nchans_));
  std::vector<kern::CubeJob> jobs(nc);
  for (size_t i = 0; i < nc; ++i) {
    int32_t* o = off.data() + i * static_cast<size_t>(nchans_);
    const bool dm_ok = std::isfinite(cands[i].dm) && cands[i].dm >= 0;
    for (int ch = 0; ch < nchans_; ++ch)
      o[ch] = dm_ok ? dm_delay_samples(cands[i].dm, delays_[static_cast<size_t>(ch)]) : 0;
    check_candidate(i, cands[i], o);
    jobs[i] = job_of(cands[i].period, cands[i].acc);
  }
  std::vector<CubeResult> out(nc);
  const size_t cube = static_cast<size_t>(p_.nints) * p_.nbins;
  const size_t bs = static_cast<size_t>(batch_size());
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    d_sums_.resize(nb * cube * p_.nsub);
    d_hits_.resize(nb * cube);
    launch(off.data() + b0 * static_cast<size_t>(nchans_), jobs.data() + b0, static_cast<int>(nb), d_sums_.data(),
           d_hits_.data());
    std::vector<int64_t> hs(nb * cube * p_.nsub);
    std::vector<int32_t> hh(nb * cube);
    PSOUP_HIP_CHECK(hipMemcpyAsync(hs.data(), d_sums_.data(), hs.size() * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   stream_));
    PSOUP_HIP_CHECK(hipMemcpyAsync(hh.data(), d_hits_.data(), hh.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < nb; ++i) {
      CubeResult& r = out[b0 + i];
      r.nactive = nactive_;
      r.hits.assign(hh.begin() + i * cube, hh.begin() + (i + 1) * cube);
      r.sums.assign(hs.begin() + i * cube * p_.nsub, hs.begin() + (i + 1) * cube * p_.nsub);
    }
  }
  return out;
}

void CubeFolder::fold_offsets(const int32_t* h_offsets, const std::vector<double>& periods,
                              const std::vector<float>& accs, int64_t* d_sums, int32_t* d_hits) {
  const size_t nc = periods.size();
  PSOUP_CHECK(accs.size() == nc, "fold cube: periods and accelerations differ in length");
  std::vector<kern::CubeJob> jobs(nc);
  for (size_t i = 0; i < nc; ++i) {
    CubeCandidate c;
    c.period = periods[i];
    c.acc = accs[i];
    check_candidate(i, c, h_offsets + i * static_cast<size_t>(nchans_));
    jobs[i] = job_of(periods[i], accs[i]);
  }
  const size_t cube = static_cast<size_t>(p_.nints) * p_.nbins;
  const size_t bs = static_cast<size_t>(batch_size());
  for (size_t b0 = 0; b0 < nc; b0 += bs) {
    const size_t nb = std::min(bs, nc - b0);
    launch(h_offsets + b0 * static_cast<size_t>(nchans_), jobs.data() + b0, static_cast<int>(nb),
           d_sums + b0 * cube * p_.nsub, d_hits + b0 * cube);
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // the offset table is reused by the next batch
  }
}

// ------------------------------------------------------------ pipeline ----
CubeRun run_cube_pipeline(const FoldCubeCmdLineOptions& args) {
  PSOUP_CHECK(!args.candfilename.empty(), "foldcube: --candfile is required (--overview is read by "
                                          "python -m peasoup_amd cube)");
  return run_cube_pipeline(args, read_cube_candfile(args.candfilename, args.limit));
}

CubeRun run_cube_pipeline(const FoldCubeCmdLineOptions& args, const std::vector<CubeCandidate>& cands_in) {
  CubeRun run;
  Stopwatch t_total, t_read, t_fold;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  run.candidates = cands_in;
  if (args.limit >= 0 && run.candidates.size() > static_cast<size_t>(args.limit))
    run.candidates.resize(static_cast<size_t>(args.limit));
  PSOUP_CHECK(!run.candidates.empty(), "foldcube: no candidates");
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  // the geometry of the largest-DM candidate (also checks that it fits)
  float dm_max = 0.f;
  for (size_t i = 0; i < run.candidates.size(); ++i) {
    const CubeCandidate& c = run.candidates[i];
    PSOUP_CHECK(std::isfinite(c.dm) && c.dm >= 0,
                "fold cube: candidate " << i << " (period " << c.period << " s, dm " << c.dm
                                        << "): the DM must be non-negative");
    dm_max = std::max(dm_max, c.dm);
  }
  DedispGeometry geom = DedispGeometry::make(hdr, fb.nsamps(), {dm_max}, kill);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  PSOUP_HIP_CHECK(hipSetDevice(0));
  Stream stream;
  DeviceFilterbank dfb(geom, stream.get());
  load_filterbank_fanout({&dfb}, {0}, fb);
  t_read.stop();
  CubeParams p;
  p.nints = args.nints;
  p.nbins = args.nbins;
  p.nsub = std::min(args.nsub, hdr.nchans);
  p.fold_nsamps = args.fold_nsamps ? args.fold_nsamps : default_fold_nsamps(geom);
  t_fold.start();
  CubeFolder folder(dfb, p, stream.get());
  run.cubes = folder.fold(run.candidates);
  t_fold.stop();
  log_verbose("fold cube: " + std::to_string(run.candidates.size()) + " candidates, " +
              std::to_string(p.fold_nsamps) + " samples, " + std::to_string(folder.batches()) + " launches");
  CubeFileHeader& h = run.header;
  h.ncand = static_cast<uint32_t>(run.candidates.size());
  h.nints = static_cast<uint32_t>(p.nints);
  h.nsub = static_cast<uint32_t>(p.nsub);
  h.nbins = static_cast<uint32_t>(p.nbins);
  h.nchans = static_cast<uint32_t>(hdr.nchans);
  h.nbits = static_cast<uint32_t>(hdr.nbits);
  h.fold_nsamps = p.fold_nsamps;
  h.tsamp = hdr.tsamp;
  h.fch1 = hdr.fch1;
  h.foff = hdr.foff;
  write_cube_file(args.outfilename, h, run.candidates, run.cubes);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["folding"] = t_fold.get_time();
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
}  // namespace

void write_cube_file(const std::string& path, const CubeFileHeader& h, const std::vector<CubeCandidate>& cands,
                     const std::vector<CubeResult>& cubes) {
  PSOUP_CHECK(cands.size() == cubes.size() && cands.size() == h.ncand, "cube file: candidate count mismatch");
  const size_t cube = static_cast<size_t>(h.nints) * h.nbins;
  for (size_t i = 0; i < cubes.size(); ++i)
    PSOUP_CHECK(cubes[i].nactive.size() == h.nsub && cubes[i].hits.size() == cube &&
                    cubes[i].sums.size() == cube * h.nsub,
                "cube file: candidate " << i << " has the wrong shape");
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open cube output " << tmp);
  std::vector<char> b;
  const char magic[8] = {'P', 'S', 'C', 'U', 'B', 'E', '0', '1'};
  b.insert(b.end(), magic, magic + 8);
  put(b, h.ncand);
  put(b, h.nints);
  put(b, h.nsub);
  put(b, h.nbins);
  put(b, h.nchans);
  put(b, h.nbits);
  put(b, h.fold_nsamps);
  put(b, h.tsamp);
  put(b, h.fch1);
  put(b, h.foff);
  bool ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size();
  for (size_t i = 0; ok && i < cands.size(); ++i) {
    const CubeResult& r = cubes[i];
    b.clear();
    put(b, cands[i].period);
    put(b, cands[i].dm);
    put(b, cands[i].acc);
    ok = std::fwrite(b.data(), 1, b.size(), fo) == b.size() &&
         std::fwrite(r.nactive.data(), sizeof(int32_t), r.nactive.size(), fo) == r.nactive.size() &&
         std::fwrite(r.hits.data(), sizeof(int32_t), r.hits.size(), fo) == r.hits.size() &&
         std::fwrite(r.sums.data(), sizeof(int64_t), r.sums.size(), fo) == r.sums.size();
  }
  ok = (std::fclose(fo) == 0) && ok;
  if (!ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write cube output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace psoup
