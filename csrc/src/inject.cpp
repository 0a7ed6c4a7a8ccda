// filinject, device side: the Injector (block sums -> host tables -> the
// injection kernel, in time chunks) and the file pipeline.  See
// psoup/inject.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "psoup/engine.hpp"
#include "psoup/inject.hpp"
#include "psoup/kernels.hpp"
#include "psoup/rfi.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

namespace {

constexpr uint64_t kL = kern::kInjectStatBlock;

// The tables on the device.
struct DeviceTables {
  DeviceBuffer<double> sigc, delay, inv_w;
  DeviceBuffer<uint32_t> A_q;
  DeviceBuffer<uint16_t> T;
  DeviceBuffer<unsigned long long> counters;  // nclip, then touched[nsig]
  int nsig = 0;
  DeviceTables(const InjectTables& t, hipStream_t s)
      : sigc(t.sigc.size()), delay(t.delay.size()), inv_w(t.inv_w.size()), A_q(t.A_q.size()), T(t.T.size()),
        counters(1 + static_cast<size_t>(t.nsig)), nsig(t.nsig) {
    const size_t want = static_cast<size_t>(t.nsig) * static_cast<size_t>(t.nchans);
    PSOUP_CHECK(t.nsig >= 1 && t.nsig <= kern::kInjectMaxSignals && t.nchans >= 1 &&
                    t.sigc.size() == static_cast<size_t>(t.nsig) * kern::kInjectSigDoubles && t.delay.size() == want &&
                    t.inv_w.size() == want && t.A_q.size() == want &&
                    t.T.size() == static_cast<size_t>(kern::kInjectTableLen),
                "inject: inconsistent tables");
    for (uint32_t a : t.A_q) PSOUP_CHECK(a < (1u << 24), "inject: the amplitude reaches 256 levels (A_q >= 2^24)");
    for (double w : t.inv_w) PSOUP_CHECK(std::isfinite(w) && w > 0, "inject: inv_w must be positive");
    for (double d : t.delay) PSOUP_CHECK(std::isfinite(d), "inject: a delay is not finite");
    for (double k : t.sigc) PSOUP_CHECK(std::isfinite(k), "inject: a signal constant is not finite");
    PSOUP_CHECK(std::isfinite(t.tsamp) && t.tsamp > 0, "inject: tsamp must be positive");
    PSOUP_HIP_CHECK(hipMemcpyAsync(sigc.data(), t.sigc.data(), t.sigc.size() * 8, hipMemcpyHostToDevice, s));
    PSOUP_HIP_CHECK(hipMemcpyAsync(delay.data(), t.delay.data(), want * 8, hipMemcpyHostToDevice, s));
    PSOUP_HIP_CHECK(hipMemcpyAsync(inv_w.data(), t.inv_w.data(), want * 8, hipMemcpyHostToDevice, s));
    PSOUP_HIP_CHECK(hipMemcpyAsync(A_q.data(), t.A_q.data(), want * 4, hipMemcpyHostToDevice, s));
    PSOUP_HIP_CHECK(hipMemcpyAsync(T.data(), t.T.data(), t.T.size() * 2, hipMemcpyHostToDevice, s));
    counters.zero_async(s);
    PSOUP_HIP_CHECK(hipStreamSynchronize(s));  // the host vectors may go away
  }
  void launch(int8_t* rows, uint64_t stride, uint64_t count, int nchans, int nbits, int bias, uint64_t t0,
              double tsamp, uint64_t seed, hipStream_t s) {
    kern::inject(rows, stride, count, nchans, nbits, bias, t0, nsig, sigc.data(), tsamp, delay.data(), inv_w.data(),
                 A_q.data(), T.data(), inject_seed_mul(seed), counters.data(), counters.data() + 1, s);
  }
  // nclip; touched[nsig] into *touched.  Synchronises.
  uint64_t read(std::vector<uint64_t>* touched, hipStream_t s) {
    std::vector<unsigned long long> h(1 + static_cast<size_t>(nsig));
    PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), counters.data(), h.size() * 8, hipMemcpyDeviceToHost, s));
    PSOUP_HIP_CHECK(hipStreamSynchronize(s));
    if (touched) touched->assign(h.begin() + 1, h.end());
    return h[0];
  }
};

}  // namespace

Injector::Injector(const uint8_t* h_packed, const InjectGeometry& g, const std::vector<InjectSignal>& signals,
                   const std::vector<int>& killmask, bool sigma_units, bool smear, uint64_t seed, hipStream_t stream,
                   size_t budget_bytes)
    : x_(h_packed), g_(g), signals_(signals), kill_(killmask), sigma_units_(sigma_units), smear_(smear), seed_(seed),
      stream_(stream) {
  inject_check_signals(signals);
  inject_check_geometry(g);
  PSOUP_CHECK(h_packed != nullptr, "inject: no input");
  PSOUP_CHECK(killmask.empty() || static_cast<int>(killmask.size()) == g.nchans, "inject: killmask size != nchans");
  // chunks: whole statistics blocks, at least one; per sample the packed bytes and the rows
  const uint64_t per = static_cast<uint64_t>(g.nchans) * static_cast<uint64_t>(g.nbits) / 8 +
                       static_cast<uint64_t>(g.nchans);
  chunk_ = std::max<uint64_t>(kL, static_cast<uint64_t>(budget_bytes) / per / kL * kL);
  chunk_ = std::min<uint64_t>(chunk_, (1ull << 30));
}

InjectResult Injector::run(uint8_t* h_out) {
  PSOUP_CHECK(h_out != nullptr, "inject: no output buffer");
  const int nchans = g_.nchans, nbits = g_.nbits;
  const size_t nc = static_cast<size_t>(nchans);
  const uint64_t nsamps = g_.nsamps;
  const uint64_t bps = static_cast<uint64_t>(nchans) * static_cast<uint64_t>(nbits) / 8;
  const int bias = (nbits == 8) ? 128 : 0;  // DedispGeometry's
  const uint64_t nchunks = (nsamps + chunk_ - 1) / chunk_;
  const uint64_t rows_n = std::min(chunk_, nsamps);
  const uint64_t stride = (rows_n + 255) / 256 * 256;
  InjectResult res;
  res.nsamps = nsamps;
  res.nchans = nchans;
  res.chunks = static_cast<int>(nchunks);

  DeviceBuffer<uint8_t> d_packed(rows_n * bps);
  DeviceBuffer<int8_t> d_rows(stride * static_cast<uint64_t>(nchans));
  bool resident = false;  // the one chunk is uploaded and unpacked
  auto load = [&](uint64_t t0, uint64_t count) {
    if (resident) return;
    const uint8_t* src = x_ + t0 * bps;
    staged_upload(
        count * bps, 64ull << 20, [&](uint64_t off, uint64_t n, uint8_t* dst) { std::memcpy(dst, src + off, n); },
        d_packed.data(), stream_);
    kern::unpack_transpose(d_packed.data(), count, nchans, nbits, d_rows.data(), stride, bias, stream_);
    resident = nchunks == 1;
  };
  // pass 1: the block sums (sigma units only)
  if (sigma_units_) {
    const uint64_t nblk = (nsamps + kL - 1) / kL;
    std::vector<uint64_t> S1(nc * nblk), S2(nc * nblk), h;
    DeviceBuffer<uint64_t> d_sums;
    for (uint64_t t0 = 0; t0 < nsamps; t0 += chunk_) {
      const uint64_t count = std::min(chunk_, nsamps - t0);
      const uint64_t nb = (count + kL - 1) / kL, b0 = t0 / kL;
      load(t0, count);
      d_sums.resize(2 * nc * nb);
      kern::rfi_block_sums(d_rows.data(), stride, nchans, count, kL, bias, d_sums.data(), d_sums.data() + nc * nb,
                           stream_);
      h.resize(2 * nc * nb);
      PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), d_sums.data(), h.size() * 8, hipMemcpyDeviceToHost, stream_));
      PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
      for (size_t c = 0; c < nc; ++c)
        for (uint64_t b = 0; b < nb; ++b) {
          S1[c * nblk + b0 + b] = h[c * nb + b];
          S2[c * nblk + b0 + b] = h[nc * nb + c * nb + b];
        }
    }
    res.sigma = inject_sigma(S1, S2, nchans, nsamps);
  }
  const std::vector<double> unit = inject_unit(res.sigma, kill_, nchans);
  res.tables = inject_tables(signals_, g_, unit, smear_);
  res.nlive = res.tables.nlive;
  res.truth = inject_truth(signals_, res.tables, g_, unit, res.sigma);
  // pass 2: the injection, on the resident rows (one chunk) or uploaded again
  DeviceTables dt(res.tables, stream_);
  for (uint64_t t0 = 0; t0 < nsamps; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps - t0);
    load(t0, count);
    dt.launch(d_rows.data(), stride, count, nchans, nbits, bias, t0, g_.tsamp, seed_, stream_);
    kern::pack_transpose(d_rows.data(), stride, count, nchans, nbits, bias, d_packed.data(), stream_);
    PSOUP_HIP_CHECK(hipMemcpyAsync(h_out + t0 * bps, d_packed.data(), count * bps, hipMemcpyDeviceToHost, stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  res.nclip = dt.read(&res.touched, stream_);
  return res;
}

uint64_t Injector::apply(int8_t* d_rows, uint64_t stride, uint64_t count, int nbits, int bias, uint64_t t0,
                         const InjectTables& tab, uint64_t seed, std::vector<uint64_t>* touched, hipStream_t stream) {
  DeviceTables dt(tab, stream);
  dt.launch(d_rows, stride, count, tab.nchans, nbits, bias, t0, tab.tsamp, seed, stream);
  return dt.read(touched, stream);
}

// ------------------------------------------------------------ pipeline ----
InjectRun run_inject_pipeline(const InjectCmdLineOptions& args) {
  InjectRun run;
  Stopwatch t_total, t_read, t_work, t_write;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  PSOUP_CHECK(args.units == "sigma" || args.units == "level", "inject: units must be sigma or level, got " << args.units);
  PSOUP_CHECK(!args.injfilename.empty(), "inject: no injection file (--injfile)");
  run.signals = inject_read_file(args.injfilename);
  Filterbank fb = Filterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  InjectGeometry g;
  g.nchans = hdr.nchans;
  g.nbits = hdr.nbits;
  g.nsamps = fb.nsamps();
  g.tsamp = hdr.tsamp;
  g.fch1 = hdr.fch1;
  g.foff = hdr.foff;
  inject_check_geometry(g);
  const uint64_t bytes = g.nsamps * fb.bytes_per_sample();
  PSOUP_CHECK(bytes <= fb.data_bytes(), "filinject: truncated filterbank");
  std::vector<int> kill;
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  t_read.stop();
  t_work.start();
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  Stream stream;
  Injector inj(fb.data(), g, run.signals, kill, args.units == "sigma", !args.no_smear, args.seed, stream.get());
  std::vector<uint8_t> data(bytes);
  run.result = inj.run(data.data());
  t_work.stop();
  t_write.start();
  // the header bytes verbatim, then the data block
  std::vector<char> head(static_cast<size_t>(hdr.size));
  {
    std::ifstream in(args.infilename, std::ios::binary);
    PSOUP_CHECK(static_cast<bool>(in.read(head.data(), static_cast<std::streamsize>(head.size()))),
                "cannot read the header of " << args.infilename);
  }
  const std::string tmp = args.outfilename + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open output " << tmp);
  const bool ok = std::fwrite(head.data(), 1, head.size(), fo) == head.size() &&
                  std::fwrite(data.data(), 1, data.size(), fo) == data.size();
  if (std::fclose(fo) != 0 || !ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), args.outfilename.c_str()) == 0,
              "cannot rename " << tmp << " to " << args.outfilename);
  if (!args.truthfilename.empty()) {
    const std::string ttmp = args.truthfilename + ".tmp";
    {
      std::ofstream out(ttmp);
      PSOUP_CHECK(static_cast<bool>(out), "cannot open output " << ttmp);
      out << inject_truth_text(run.signals, run.result.truth, args.units, args.seed);
      PSOUP_CHECK(static_cast<bool>(out.flush()), "cannot write output " << ttmp);
    }
    PSOUP_CHECK(std::rename(ttmp.c_str(), args.truthfilename.c_str()) == 0,
                "cannot rename " << ttmp << " to " << args.truthfilename);
  }
  t_write.stop();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["injecting"] = t_work.get_time();
  run.timers["writing"] = t_write.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
