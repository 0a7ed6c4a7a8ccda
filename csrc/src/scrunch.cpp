// filscrunch, device side: the Scruncher (sums -> host scale -> requantise,
// in time chunks) and the file pipeline.  See psoup/scrunch.hpp.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

#include "psoup/engine.hpp"
#include "psoup/kernels.hpp"
#include "psoup/rfi.hpp"
#include "psoup/scrunch.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

namespace {

constexpr uint64_t kL = kern::kScrunchStatBlock;

// the unkilled channels and the subbands' runs of them
void active_tables(int nchans, int nsub, const std::vector<int>& killmask, std::vector<int32_t>& active,
                   std::vector<int32_t>& sub_first, std::vector<int32_t>& nactive) {
  PSOUP_CHECK(killmask.empty() || static_cast<int>(killmask.size()) == nchans, "scrunch: killmask size != nchans");
  const int w = nchans / nsub;
  active.clear();
  sub_first.assign(static_cast<size_t>(nsub) + 1, 0);
  nactive.assign(static_cast<size_t>(nsub), 0);
  for (int c = 0; c < nchans; ++c) {
    if (c % w == 0) sub_first[static_cast<size_t>(c / w)] = static_cast<int32_t>(active.size());
    if (killmask.empty() || killmask[static_cast<size_t>(c)] != 0) {
      active.push_back(c);
      nactive[static_cast<size_t>(c / w)] += 1;
    }
  }
  sub_first[static_cast<size_t>(nsub)] = static_cast<int32_t>(active.size());
}

struct DeviceTables {
  DeviceBuffer<int32_t> tab;  // active | sub_first | rel
  const int32_t *active = nullptr, *sub_first = nullptr, *rel = nullptr;
  void upload(const std::vector<int32_t>& a, const std::vector<int32_t>& sf, const std::vector<int32_t>& r,
              hipStream_t s) {
    std::vector<int32_t> h;
    h.reserve(a.size() + 1 + sf.size() + r.size());
    h.insert(h.end(), a.begin(), a.end());
    if (a.empty()) h.push_back(0);  // never read: keeps the table non-empty
    const size_t o1 = h.size();
    h.insert(h.end(), sf.begin(), sf.end());
    const size_t o2 = h.size();
    h.insert(h.end(), r.begin(), r.end());
    tab.resize(h.size());
    PSOUP_HIP_CHECK(hipMemcpyAsync(tab.data(), h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PSOUP_HIP_CHECK(hipStreamSynchronize(s));  // h is pageable and goes out of scope
    active = tab.data();
    sub_first = tab.data() + o1;
    rel = tab.data() + o2;
  }
};

void check_reads(const std::vector<int32_t>& rel, int f, uint64_t nout, uint64_t nsamps) {
  int32_t R = 0;
  for (int32_t r : rel) {
    PSOUP_CHECK(r >= 0, "scrunch: negative offset");
    R = std::max(R, r);
  }
  PSOUP_CHECK(nout >= 1 && static_cast<uint64_t>(f) * nout + static_cast<uint64_t>(R) <= nsamps,
              "scrunch: the outputs read past the rows (f nout + R > nsamps)");
}

void write_atomically(const std::string& path, const std::string& head, const std::vector<uint8_t>& data) {
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open output " << tmp);
  const bool ok = std::fwrite(head.data(), 1, head.size(), fo) == head.size() &&
                  std::fwrite(data.data(), 1, data.size(), fo) == data.size();
  if (std::fclose(fo) != 0 || !ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

}  // namespace

// ------------------------------------------------------------ scruncher ----
Scruncher::Scruncher(const int8_t* d_rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias,
                     double foff, const std::vector<float>& delays, const std::vector<int>& killmask,
                     const ScrunchParams& p, hipStream_t stream, size_t budget_bytes)
    : x_(d_rows), stride_(stride), nsamps_(nsamps), nchans_(nchans), nbits_(nbits), bias_(bias), stream_(stream) {
  PSOUP_CHECK(foff < 0, "scrunch: foff must be negative (channels in descending frequency), got " << foff);
  PSOUP_CHECK(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8, "scrunch: nbits must be 1/2/4/8");
  p_ = scrunch_check_params(p, nchans);
  PSOUP_CHECK(static_cast<int>(delays.size()) == nchans, "scrunch: delays size != nchans");
  PSOUP_CHECK((stride & 15) == 0 && (reinterpret_cast<uintptr_t>(d_rows) & 15) == 0 && stride >= nsamps,
              "scrunch: rows must be 16-byte aligned with a stride that is a multiple of 16 and >= nsamps");
  off_ = scrunch_offsets(p_.dm, delays, p_.nsub);
  const uint64_t f = static_cast<uint64_t>(p_.tscrunch);
  nout_ = nsamps > static_cast<uint64_t>(off_.R) ? (nsamps - static_cast<uint64_t>(off_.R)) / f : 0;
  PSOUP_CHECK(nout_ >= 1, "scrunch: nout < 1: " << nsamps << " samples hold no output at tscrunch " << f
                                                << " with a spread of " << off_.R << " samples inside a subband");
  active_tables(nchans, p_.nsub, killmask, active_, sub_first_, nactive_);
  const int64_t most = *std::max_element(nactive_.begin(), nactive_.end());
  PSOUP_CHECK(most > 0, "scrunch: no live subband (every channel is killed)");
  const int64_t V = (int64_t(1) << nbits) - 1;
  PSOUP_CHECK(V * static_cast<int64_t>(f) * most < (int64_t(1) << 26),
              "scrunch: 2^26 bound: V f nactive = " << V << " x " << f << " x " << most << " >= 2^26");
  // chunks: whole statistics blocks, at least one
  const uint64_t per_out = 4ull * static_cast<uint64_t>(p_.nsub);
  chunk_ = std::max<uint64_t>(kL, static_cast<uint64_t>(budget_bytes) / per_out / kL * kL);
}

ScrunchResult Scruncher::run(int8_t* d_y, uint64_t y_stride) {
  PSOUP_CHECK((y_stride & 15) == 0 && (reinterpret_cast<uintptr_t>(d_y) & 15) == 0 && y_stride >= nout_,
              "scrunch: y must be 16-byte aligned with a stride that is a multiple of 16 and >= nout");
  const int nsub = p_.nsub, f = p_.tscrunch;
  const size_t ns = static_cast<size_t>(nsub);
  ScrunchResult res;
  res.nout = nout_;
  res.nblk = (nout_ + kL - 1) / kL;
  res.R = off_.R;
  res.nsub = nsub;
  res.rel = off_.rel;
  res.nactive = nactive_;
  const size_t ncell = ns * static_cast<size_t>(res.nblk);
  const uint64_t nchunks = (nout_ + chunk_ - 1) / chunk_;
  res.chunks = static_cast<int>(nchunks);
  const uint64_t a_stride = (std::min(chunk_, nout_) + 15) / 16 * 16;

  DeviceTables t;
  t.upload(active_, sub_first_, off_.rel, stream_);
  DeviceBuffer<int32_t> A(ns * a_stride);
  DeviceBuffer<uint64_t> S(4 * ncell);  // S1 | S2 of the first pass, then of the second
  S.zero_async(stream_);
  auto sums_of = [&](uint64_t u0, uint64_t* s1, uint64_t* s2) {
    const uint64_t count = std::min(chunk_, nout_ - u0);
    kern::scrunch_sums(x_, stride_, nsamps_, bias_, f, t.active, t.sub_first, t.rel, nsub, u0, count, A.data(),
                       a_stride, s1, s2, res.nblk, stream_);
    ++nlaunch_;
    return count;
  };
  // pass 1: the block sums
  for (uint64_t u0 = 0; u0 < nout_; u0 += chunk_) sums_of(u0, S.data(), S.data() + ncell);
  res.S1.resize(ncell);
  res.S2.resize(ncell);
  PSOUP_HIP_CHECK(
      hipMemcpyAsync(res.S1.data(), S.data(), ncell * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(
      hipMemcpyAsync(res.S2.data(), S.data() + ncell, ncell * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  res.scale = scrunch_scale(res.S1, res.S2, nsub, nout_, nactive_, p_.sigma_out);
  res.killmask.assign(ns, 0);
  for (size_t s = 0; s < ns; ++s) res.killmask[s] = res.scale.live[s] ? 1 : 0;
  // pass 2: requantise, from the sums kept (one chunk) or formed again
  DeviceBuffer<int32_t> dM(ns);
  DeviceBuffer<uint8_t> dlive(ns);
  PSOUP_HIP_CHECK(hipMemcpyAsync(dM.data(), res.scale.M.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(dlive.data(), res.scale.live.data(), ns, hipMemcpyHostToDevice, stream_));
  for (uint64_t u0 = 0; u0 < nout_; u0 += chunk_) {
    uint64_t count = std::min(chunk_, nout_ - u0);
    if (nchunks > 1) count = sums_of(u0, S.data() + 2 * ncell, S.data() + 3 * ncell);
    kern::scrunch_quant(A.data(), a_stride, nsub, count, dM.data(), dlive.data(), res.scale.mul, d_y + u0, y_stride,
                        stream_);
    ++nlaunch_;
  }
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  return res;
}

void Scruncher::sums(const int8_t* d_rows, uint64_t stride, uint64_t nsamps, int nchans, int bias, int f, int nsub,
                     const std::vector<int32_t>& rel, const std::vector<int>& killmask, uint64_t nout, int32_t* d_A,
                     uint64_t a_stride, uint64_t* d_S1, uint64_t* d_S2, hipStream_t stream) {
  PSOUP_CHECK(nchans >= 1 && nsub >= 1 && nchans % nsub == 0, "scrunch sums: nsub must divide nchans");
  PSOUP_CHECK(static_cast<int>(rel.size()) == nchans, "scrunch sums: rel size != nchans");
  PSOUP_CHECK(f >= 1 && f <= kern::kScrunchMaxF, "scrunch sums: tscrunch must be in 1.." << kern::kScrunchMaxF);
  check_reads(rel, f, nout, nsamps);
  std::vector<int32_t> active, sub_first, nactive;
  active_tables(nchans, nsub, killmask, active, sub_first, nactive);
  const int64_t most = *std::max_element(nactive.begin(), nactive.end());
  PSOUP_CHECK(255 * static_cast<int64_t>(f) * most < (int64_t(1) << 31), "scrunch sums: the sums overflow int32");
  DeviceTables t;
  t.upload(active, sub_first, rel, stream);
  const uint64_t nblk = (nout + kL - 1) / kL;
  const size_t ncell = static_cast<size_t>(nsub) * static_cast<size_t>(nblk);
  PSOUP_HIP_CHECK(hipMemsetAsync(d_S1, 0, ncell * sizeof(uint64_t), stream));
  PSOUP_HIP_CHECK(hipMemsetAsync(d_S2, 0, ncell * sizeof(uint64_t), stream));
  kern::scrunch_sums(d_rows, stride, nsamps, bias, f, t.active, t.sub_first, t.rel, nsub, 0, nout, d_A, a_stride, d_S1,
                     d_S2, nblk, stream);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream));
}

void Scruncher::quant(const int32_t* d_A, uint64_t a_stride, int nsub, uint64_t nout, const std::vector<int32_t>& M,
                      const std::vector<uint8_t>& live, int32_t mul, int8_t* d_y, uint64_t y_stride,
                      hipStream_t stream) {
  const size_t ns = static_cast<size_t>(nsub);
  PSOUP_CHECK(nsub >= 1 && M.size() == ns && live.size() == ns, "scrunch quant: M and live must be [nsub]");
  DeviceBuffer<int32_t> dM(ns);
  DeviceBuffer<uint8_t> dlive(ns);
  PSOUP_HIP_CHECK(hipMemcpyAsync(dM.data(), M.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PSOUP_HIP_CHECK(hipMemcpyAsync(dlive.data(), live.data(), ns, hipMemcpyHostToDevice, stream));
  kern::scrunch_quant(d_A, a_stride, nsub, nout, dM.data(), dlive.data(), mul, d_y, y_stride, stream);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------ pipeline ----
ScrunchRun run_scrunch_pipeline(const ScrunchCmdLineOptions& args) {
  ScrunchRun run;
  Stopwatch t_total, t_read, t_work, t_write;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  const uint64_t nsamps = fb.nsamps();
  const uint64_t bytes = nsamps * fb.bytes_per_sample();
  PSOUP_CHECK(nsamps > 0 && bytes <= fb.data_bytes(), "filscrunch: empty or truncated filterbank");
  PSOUP_CHECK(hdr.foff < 0, "scrunch: foff must be negative (channels in descending frequency), got " << hdr.foff);
  const ScrunchParams p = scrunch_check_params(scrunch_params_from(args), hdr.nchans);
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  Stream stream;
  const std::vector<float> delays = generate_delay_table(hdr.nchans, hdr.tsamp, hdr.fch1, hdr.foff);
  const int bias = (hdr.nbits == 8) ? 128 : 0;  // DedispGeometry's
  const uint64_t stride = (nsamps + 255) / 256 * 256;
  DeviceBuffer<int8_t> rows(stride * static_cast<uint64_t>(hdr.nchans));
  {
    DeviceBuffer<uint8_t> d_packed(bytes);
    staged_upload(
        bytes, 64ull << 20, [&](uint64_t off, uint64_t n, uint8_t* dst) { fb.read_data(off, n, dst); },
        d_packed.data(), stream.get());
    kern::unpack_transpose(d_packed.data(), nsamps, hdr.nchans, hdr.nbits, rows.data(), stride, bias, stream.get());
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream.get()));
  }
  t_read.stop();
  t_work.start();
  Scruncher scr(rows.data(), stride, nsamps, hdr.nchans, hdr.nbits, bias, hdr.foff, delays, kill, p, stream.get());
  const uint64_t nout = scr.nout();
  PSOUP_CHECK(nout <= 2147483647ull, "filscrunch: too many output samples for a SIGPROC header");
  const uint64_t y_stride = (nout + 255) / 256 * 256;
  DeviceBuffer<int8_t> y(y_stride * static_cast<uint64_t>(p.nsub));
  run.result = scr.run(y.data(), y_stride);
  const uint64_t out_bytes = nout * static_cast<uint64_t>(p.nsub);
  DeviceBuffer<uint8_t> d_out(out_bytes);
  kern::pack_transpose(y.data(), y_stride, nout, p.nsub, 8, 128, d_out.data(), stream.get());
  std::vector<uint8_t> data(out_bytes);
  PSOUP_HIP_CHECK(hipMemcpyAsync(data.data(), d_out.data(), out_bytes, hipMemcpyDeviceToHost, stream.get()));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream.get()));
  t_work.stop();
  t_write.start();
  SigprocHeader oh = hdr;
  const int w = hdr.nchans / p.nsub;
  oh.nchans = p.nsub;
  oh.foff = static_cast<double>(w) * hdr.foff;
  oh.tsamp = static_cast<double>(p.tscrunch) * hdr.tsamp;
  oh.nbits = 8;
  oh.nsamples = hdr.has("nsamples") ? static_cast<int>(nout) : 0;
  oh.refdm = static_cast<double>(p.dm);
  std::ostringstream head;
  write_header(head, oh);
  write_atomically(args.outfilename, head.str(), data);
  if (!args.killoutfilename.empty()) write_killfile(args.killoutfilename, run.result.killmask);
  t_write.stop();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["scrunching"] = t_work.get_time();
  run.timers["writing"] = t_write.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
