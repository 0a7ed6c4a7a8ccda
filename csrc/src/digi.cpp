// fildigi, device side: the raw reader, the Digitiser (block sums -> host
// scale -> requantise, in time chunks) and the file pipeline.  See
// psoup/digi.hpp.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "psoup/digi.hpp"
#include "psoup/engine.hpp"
#include "psoup/rfi.hpp"

namespace psoup {

namespace {

constexpr uint64_t kL = kern::kDigiStatBlock;

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

// {mean, gain} [nint][nchans] for the device
std::vector<double2> quant_table(const std::vector<double>& mean, const std::vector<double>& gain) {
  std::vector<double2> t(mean.size());
  for (size_t i = 0; i < t.size(); ++i) t[i] = make_double2(mean[i], gain[i]);
  return t;
}

}  // namespace

// ---------------------------------------------------------------- reader ----
RawFilterbank RawFilterbank::from_file(const std::string& filename) {
  RawFilterbank fb;
  fb.hdr_ = read_header_file(filename);
  const SigprocHeader& h = fb.hdr_;
  fb.type_ = digi_check_header(h.nbits, h.signed_data, h.nifs, h.foff, h.nchans);
  int fd = ::open(filename.c_str(), O_RDONLY);
  if (fd < 0) PSOUP_THROW("cannot open " << filename);
  struct stat st;
  if (fstat(fd, &st) != 0) {
    ::close(fd);
    PSOUP_THROW("cannot stat " << filename);
  }
  const uint64_t file_size = static_cast<uint64_t>(st.st_size);
  const uint64_t bps = fb.bytes_per_sample();
  const uint64_t avail = file_size > h.size ? (file_size - h.size) / bps : 0;
  fb.nsamps_ = h.nsamples > 0 ? std::min<uint64_t>(static_cast<uint64_t>(h.nsamples), avail) : avail;
  if (fb.nsamps_ < 1) {
    ::close(fd);
    PSOUP_THROW("digi: " << filename << " is shorter than one sample");
  }
  void* map = ::mmap(nullptr, file_size, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (map == MAP_FAILED) PSOUP_THROW("mmap failed for " << filename);
  ::madvise(map, file_size, MADV_SEQUENTIAL);
  fb.owner_ = std::shared_ptr<void>(map, [file_size](void* p) { ::munmap(p, file_size); });
  fb.data_ = static_cast<const uint8_t*>(map) + h.size;
  return fb;
}

// ------------------------------------------------------------- digitiser ----
Digitiser::Digitiser(const void* h_x, kern::DigiType type, uint64_t nsamps, int nchans, double foff,
                     const std::vector<int>& killmask, const DigiParams& p, hipStream_t stream, size_t budget_bytes)
    : x_(static_cast<const uint8_t*>(h_x)), type_(type), nsamps_(nsamps), nchans_(nchans), kill_(killmask), p_(p),
      stream_(stream) {
  digi_check_params(p);
  PSOUP_CHECK(static_cast<int>(type) >= 0 && static_cast<int>(type) <= 3, "digi: bad sample type");
  PSOUP_CHECK(nchans >= 1, "digi: no channels");
  PSOUP_CHECK(std::isfinite(foff) && foff != 0, "digi: foff must not be zero");
  PSOUP_CHECK(nsamps >= 1 && h_x != nullptr, "digi: the input is shorter than one sample");
  PSOUP_CHECK(killmask.empty() || static_cast<int>(killmask.size()) == nchans, "digi: killmask size != nchans");
  PSOUP_CHECK(killmask.empty() || std::any_of(killmask.begin(), killmask.end(), [](int k) { return k != 0; }),
              "digi: no live channel (every channel is killed)");
  flip_ = foff > 0;
  // chunks: whole statistics blocks, at least one
  const uint64_t per_row = static_cast<uint64_t>(nchans) * static_cast<uint64_t>(kern::digi_type_bytes(type) + 1);
  chunk_ = std::max<uint64_t>(kL, static_cast<uint64_t>(budget_bytes) / per_row / kL * kL);
  chunk_ = std::min<uint64_t>(chunk_, 65535 * kL);  // the sums' grid
}

DigiResult Digitiser::run(uint8_t* h_y) {
  PSOUP_CHECK(h_y != nullptr, "digi: no output buffer");
  const size_t nc = static_cast<size_t>(nchans_);
  const uint64_t esz = static_cast<uint64_t>(kern::digi_type_bytes(type_));
  const uint64_t row = static_cast<uint64_t>(nchans_) * esz;
  DigiResult res;
  res.nsamps = nsamps_;
  res.nchans = nchans_;
  res.nblk = digi_nblk(nsamps_);
  res.flip = flip_;
  const size_t ncell = nc * static_cast<size_t>(res.nblk);
  const uint64_t nchunks = (nsamps_ + chunk_ - 1) / chunk_;
  res.chunks = static_cast<int>(nchunks);
  const uint64_t rows = std::min(chunk_, nsamps_);

  DeviceBuffer<uint8_t> dx(rows * row);
  DeviceBuffer<uint8_t> dy((rows * static_cast<uint64_t>(nchans_) + 15) / 16 * 16);
  DeviceBuffer<uint32_t> dN(ncell);
  DeviceBuffer<int64_t> dS1(ncell);
  DeviceBuffer<uint64_t> dS2(ncell);
  DeviceBuffer<int32_t> dE(ncell);
  auto upload = [&](uint64_t t0, uint64_t count) {
    const uint8_t* src = x_ + t0 * row;
    staged_upload(
        count * row, 64ull << 20, [&](uint64_t off, uint64_t n, uint8_t* dst) { std::memcpy(dst, src + off, n); },
        dx.data(), stream_);
  };
  // pass 1: the block sums
  for (uint64_t t0 = 0; t0 < nsamps_; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps_ - t0);
    upload(t0, count);
    kern::digi_block_sums(dx.data(), type_, count, nchans_, t0, dN.data(), dS1.data(), dS2.data(), dE.data(), res.nblk,
                          stream_);
    ++nlaunch_;
    if (nchunks > 1) PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // dx is uploaded over next
  }
  res.N.resize(ncell);
  res.S1.resize(ncell);
  res.S2.resize(ncell);
  res.E.resize(ncell);
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.N.data(), dN.data(), ncell * 4, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.S1.data(), dS1.data(), ncell * 8, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.S2.data(), dS2.data(), ncell * 8, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.E.data(), dE.data(), ncell * 4, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  res.nbad.assign(nc, nsamps_);
  for (size_t c = 0; c < nc; ++c)
    for (size_t b = 0; b < res.nblk; ++b) res.nbad[c] -= res.N[c * res.nblk + b];
  res.scale = digi_scale(res.N, res.S1, res.S2, res.E, nchans_, res.nblk, kill_, p_);
  res.killmask.assign(nc, 0);
  for (size_t c = 0; c < nc; ++c) res.killmask[flip_ ? nc - 1 - c : c] = res.scale.alive[c];
  // pass 2: requantise, from the resident input (one chunk) or uploaded again
  const std::vector<double2> tab = quant_table(res.scale.mean, res.scale.gain);
  DeviceBuffer<double2> dtab(tab.size());
  DeviceBuffer<unsigned long long> dclip(1);
  PSOUP_HIP_CHECK(hipMemcpyAsync(dtab.data(), tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice, stream_));
  dclip.zero_async(stream_);
  for (uint64_t t0 = 0; t0 < nsamps_; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps_ - t0);
    if (nchunks > 1) upload(t0, count);
    kern::digi_quant(dx.data(), type_, count, nchans_, t0, p_.rescale_blocks, res.scale.nint, dtab.data(), flip_,
                     dy.data(), dclip.data(), stream_);
    ++nlaunch_;
    PSOUP_HIP_CHECK(hipMemcpyAsync(h_y + t0 * static_cast<uint64_t>(nchans_), dy.data(),
                                   count * static_cast<uint64_t>(nchans_), hipMemcpyDeviceToHost, stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  unsigned long long nclip = 0;
  PSOUP_HIP_CHECK(hipMemcpyAsync(&nclip, dclip.data(), sizeof(nclip), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  res.nclip = nclip;
  return res;
}

void Digitiser::sums(const void* d_x, kern::DigiType type, uint64_t nsamps, int nchans, uint32_t* d_N, int64_t* d_S1,
                     uint64_t* d_S2, int32_t* d_E, hipStream_t stream) {
  PSOUP_CHECK(nsamps >= 1 && nchans >= 1, "digi sums: empty input");
  const uint64_t nblk = digi_nblk(nsamps);
  const uint64_t step = 65535 * kL;
  for (uint64_t t0 = 0; t0 < nsamps; t0 += step) {
    const uint64_t count = std::min(step, nsamps - t0);
    const uint8_t* p = static_cast<const uint8_t*>(d_x) +
                       t0 * static_cast<uint64_t>(nchans) * static_cast<uint64_t>(kern::digi_type_bytes(type));
    kern::digi_block_sums(p, type, count, nchans, t0, d_N, d_S1, d_S2, d_E, nblk, stream);
  }
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream));
}

uint64_t Digitiser::quant(const void* d_x, kern::DigiType type, uint64_t nsamps, int nchans, int J,
                          const std::vector<double>& mean, const std::vector<double>& gain, bool flip, uint8_t* d_y,
                          hipStream_t stream) {
  PSOUP_CHECK(nsamps >= 1 && nchans >= 1 && J >= 0, "digi quant: bad shape");
  const int nint = digi_nint(digi_nblk(nsamps), J);
  const size_t want = static_cast<size_t>(nint) * static_cast<size_t>(nchans);
  PSOUP_CHECK(mean.size() == want && gain.size() == want, "digi quant: mean and gain must be [nint][nchans]");
  const std::vector<double2> tab = quant_table(mean, gain);
  DeviceBuffer<double2> dtab(tab.size());
  DeviceBuffer<unsigned long long> dclip(1);
  PSOUP_HIP_CHECK(hipMemcpyAsync(dtab.data(), tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice, stream));
  dclip.zero_async(stream);
  kern::digi_quant(d_x, type, nsamps, nchans, 0, J, nint, dtab.data(), flip, d_y, dclip.data(), stream);
  unsigned long long nclip = 0;
  PSOUP_HIP_CHECK(hipMemcpyAsync(&nclip, dclip.data(), sizeof(nclip), hipMemcpyDeviceToHost, stream));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream));
  return nclip;
}

// ------------------------------------------------------------ pipeline ----
DigiRun run_digi_pipeline(const DigiCmdLineOptions& args) {
  DigiRun run;
  Stopwatch t_total, t_read, t_work, t_write;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  const DigiParams p = digi_params_from(args);
  digi_check_params(p);
  RawFilterbank fb = RawFilterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  t_read.stop();
  t_work.start();
  PSOUP_CHECK(fb.nsamps() <= 2147483647ull, "fildigi: too many samples for a SIGPROC header");
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  Stream stream;
  Digitiser dig(fb.data(), fb.type(), fb.nsamps(), hdr.nchans, hdr.foff, kill, p, stream.get());
  std::vector<uint8_t> data(fb.nsamps() * static_cast<uint64_t>(hdr.nchans));
  run.result = dig.run(data.data());
  t_work.stop();
  t_write.start();
  SigprocHeader oh = digi_header(hdr);
  if (oh.nsamples != 0) oh.nsamples = static_cast<int>(fb.nsamps());
  std::ostringstream head;
  write_header(head, oh);
  write_atomically(args.outfilename, head.str(), data);
  if (!args.killoutfilename.empty()) write_killfile(args.killoutfilename, run.result.killmask);
  t_write.stop();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["digitising"] = t_work.get_time();
  run.timers["writing"] = t_write.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
