// Single-pulse search: width ladder, event clustering, engine, pipeline and
// the spsearch output.  See psoup/singlepulse.hpp.
#include "psoup/singlepulse.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <exception>
#include <iostream>
#include <mutex>
#include <thread>

#include "psoup/engine.hpp"
#include "psoup/pipeline.hpp"
#include "psoup/plan.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

std::vector<int> sp_widths(uint64_t n, int wmax) {
  std::vector<int> w;
  const uint64_t lim = std::min<uint64_t>(wmax > 0 ? static_cast<uint64_t>(wmax) : 0, n / 2);
  for (uint64_t v = 1; v <= lim && v <= (uint64_t(1) << 30); v <<= 1) w.push_back(static_cast<int>(v));
  return w;
}

uint64_t sp_baseline_samples(const SpParams& p, uint64_t n) {
  uint64_t b = p.baseline_samples;
  if (b == 0) b = static_cast<uint64_t>(std::ceil(p.baseline_s / p.tsamp));
  return std::min<uint64_t>(std::max<uint64_t>(b, 64), n);
}

namespace {

bool event_order(const SpEvent& a, const SpEvent& b) {
  if (a.dm_idx != b.dm_idx) return a.dm_idx < b.dm_idx;
  if (a.width_log2 != b.width_log2) return a.width_log2 < b.width_log2;
  return a.sample < b.sample;
}

}  // namespace

SpCandidateList sp_cluster(const std::vector<SpEvent>& events, const std::vector<float>& dm_list,
                           double band_delay_per_dm, double tsamp) {
  PSOUP_CHECK(tsamp > 0, "sp_cluster: tsamp");
  std::vector<SpEvent> ev(events);
  for (const SpEvent& e : ev)
    PSOUP_CHECK(e.dm_idx >= 0 && static_cast<size_t>(e.dm_idx) < dm_list.size() && e.width_log2 >= 0 &&
                    e.width_log2 < 31,
                "sp_cluster: event outside the DM list or width ladder");
  std::sort(ev.begin(), ev.end(), [](const SpEvent& a, const SpEvent& b) {
    if (a.snr != b.snr) return a.snr > b.snr;
    return event_order(a, b);
  });
  SpCandidateList out;
  // twice the boxcar centre, an integer: 2 sample + w
  std::vector<int64_t> centre2;
  for (const SpEvent& e : ev) {
    const int64_t w = int64_t(1) << e.width_log2;
    const int64_t c2 = 2 * static_cast<int64_t>(e.sample) + w;
    const double dm = static_cast<double>(dm_list[static_cast<size_t>(e.dm_idx)]);
    const uint64_t last = static_cast<uint64_t>(e.sample) + static_cast<uint64_t>(w) - 1;
    bool absorbed = false;
    for (size_t c = 0; c < out.size(); ++c) {
      SpCandidate& k = out[c];
      const double slack = std::fabs(dm - static_cast<double>(k.dm)) * band_delay_per_dm / tsamp;
      const double reach = 0.5 * static_cast<double>(w + k.width) + slack;
      const double dist = 0.5 * static_cast<double>(std::llabs(c2 - centre2[c]));
      if (dist <= reach) {
        k.members += 1;
        k.first_sample = std::min<uint64_t>(k.first_sample, e.sample);
        k.last_sample = std::max<uint64_t>(k.last_sample, last);
        k.dm_idx_lo = std::min(k.dm_idx_lo, e.dm_idx);
        k.dm_idx_hi = std::max(k.dm_idx_hi, e.dm_idx);
        absorbed = true;
        break;
      }
    }
    if (absorbed) continue;
    SpCandidate k;
    k.sample = e.sample;
    k.width = static_cast<int>(w);
    k.time_s = 0.5 * static_cast<double>(c2) * tsamp;
    k.snr = e.snr;
    k.dm = dm_list[static_cast<size_t>(e.dm_idx)];
    k.dm_idx = e.dm_idx;
    k.members = 1;
    k.first_sample = e.sample;
    k.last_sample = last;
    k.dm_idx_lo = k.dm_idx_hi = e.dm_idx;
    out.push_back(k);
    centre2.push_back(c2);
  }
  return out;
}

// --------------------------------------------------------------- engine ----
SinglePulseEngine::SinglePulseEngine(const SpParams& p, uint64_t nsamps, hipStream_t stream)
    : p_(p), n_(nsamps), stream_(stream) {
  PSOUP_CHECK(n_ >= 64 && n_ < (uint64_t(1) << 32), "single pulse: series length must be in [64, 2^32)");
  PSOUP_CHECK(p_.boxcar_max >= 4 && p_.boxcar_max <= (1 << kern::kSpMaxLog2),
              "single pulse: boxcar_max must be in [4, " << (1 << kern::kSpMaxLog2) << "]");
  PSOUP_CHECK(p_.tsamp > 0 && std::isfinite(p_.min_snr), "single pulse: bad parameters");
  widths_ = sp_widths(n_, p_.boxcar_max);
  kmax_ = static_cast<int>(widths_.size()) - 1;
  baseline_ = sp_baseline_samples(p_, n_);
  nblk_ = (n_ + baseline_ - 1) / baseline_;
  cap_ = std::max<uint32_t>(1, p_.capacity);
}

SinglePulseEngine::~SinglePulseEngine() { (void)hipStreamSynchronize(stream_); }

std::vector<SpEvent> SinglePulseEngine::search_block(const uint8_t* d_rows, uint64_t row_stride, int ndm, int dm_idx0,
                                                     float* d_best_snr, uint32_t* d_best_arg) {
  PSOUP_CHECK(ndm > 0, "single pulse: empty trial block");
  hipStream_t s = stream_;
  const size_t nd = static_cast<size_t>(ndm);
  if (means_.size() < nd * nblk_) means_.resize(nd * nblk_);
  if (partials_.size() < nd * kern::kSpSigmaParts) partials_.resize(nd * kern::kSpSigmaParts);
  if (d_count_.size() < 1) d_count_.resize(1);
  kern::sp_block_means(d_rows, row_stride, ndm, n_, baseline_, means_.data(), s);
  kern::sp_sigma(d_rows, row_stride, ndm, n_, baseline_, means_.data(), partials_.data(), s);
  // The record count may exceed the buffer (the kernel stops writing at its
  // capacity): grow it to the count and search the block again, so the
  // events never depend on the initial capacity.
  uint32_t count = 0;
  for (int attempt = 0;; ++attempt) {
    if (d_events_.size() < cap_) d_events_.resize(cap_);
    PSOUP_HIP_CHECK(hipMemsetAsync(d_count_.data(), 0, sizeof(uint32_t), s));
    kern::sp_search(d_rows, row_stride, ndm, n_, baseline_, means_.data(), partials_.data(), kmax_, p_.min_snr,
                    dm_idx0, d_events_.data(), d_count_.data(), cap_, d_best_snr, d_best_arg, s);
    PSOUP_HIP_CHECK(hipMemcpyAsync(&count, d_count_.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PSOUP_HIP_CHECK(hipStreamSynchronize(s));
    if (count <= cap_) break;
    PSOUP_CHECK(attempt < 2, "single pulse: record buffer overflow persists");
    cap_ = count;  // the search is deterministic: the same count again
    ++nreruns_;
  }
  std::vector<SpEvent> ev(count);
  if (count) PSOUP_HIP_CHECK(hipMemcpy(ev.data(), d_events_.data(), count * sizeof(SpEvent), hipMemcpyDeviceToHost));
  std::sort(ev.begin(), ev.end(), event_order);
  nevents_ += count;
  return ev;
}

// ------------------------------------------------------------ pipeline ----
SpParams sp_params_from(const SpCmdLineOptions& a, double tsamp) {
  SpParams p;
  p.tsamp = tsamp;
  p.min_snr = a.min_snr;
  p.boxcar_max = a.boxcar_max;
  p.baseline_s = a.baseline;
  return p;
}

RfiParams sp_rfi_params(const SpCmdLineOptions& a) {
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

SpResult run_sp_pipeline(const SpCmdLineOptions& args) {
  SpResult res;
  Stopwatch t_total, t_read;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  t_read.stop();
  const SigprocHeader& hdr = fb.header();
  res.dm_list = generate_dm_list(args.dm_start, args.dm_end, hdr.tsamp, args.dm_pulse_width, hdr.fch1, hdr.foff,
                                 hdr.nchans, args.dm_tol);
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  const int ndev = device_count();
  PSOUP_CHECK(ndev > 0, "no HIP devices visible");
  const int ngpu = std::max(1, std::min(ndev, args.max_num_threads));
  for (int i = 0; i < ngpu; ++i) res.devices.push_back(i);
  // --rfi: the packed bytes are cleaned once on device 0 (unpack, block sums,
  // flags, apply, pack) and the flagged channels join the killmask before the
  // geometry is made.  Device 0 unpacks the cleaned bytes where they lie; the
  // other devices get the same bytes from a host copy.
  const bool rfi = args.rfi || args.zero_dm;
  DeviceBuffer<uint8_t> d_clean;
  std::vector<uint8_t> h_clean;
  if (rfi) {
    const RfiParams rp = sp_rfi_params(args);
    const uint64_t bytes = fb.nsamps() * fb.bytes_per_sample();
    PSOUP_CHECK(fb.nsamps() > 0 && bytes <= fb.data_bytes(), "spsearch: empty or truncated filterbank");
    PSOUP_HIP_CHECK(hipSetDevice(0));
    Stream cs;
    d_clean.resize(bytes);
    staged_upload(
        bytes, 64ull << 20, [&](uint64_t off, uint64_t n, uint8_t* dst) { fb.read_data(off, n, dst); }, d_clean.data(),
        cs.get());
    PSOUP_HIP_CHECK(hipStreamSynchronize(cs.get()));
    RfiCleaner cleaner(rp, cs.get());
    const RfiMask mask = cleaner.clean_packed(d_clean.data(), hdr.nchans, fb.nsamps(), hdr.nbits, kill);
    for (size_t c = 0; c < kill.size(); ++c) kill[c] = (kill[c] != 0 && mask.killmask[c] != 0) ? 1 : 0;
    res.rfi_comment = rfi_summary_comment(mask, rp);
    if (!args.rfi_maskfilename.empty()) {
      RfiMaskHeader mh;
      mh.nbits = static_cast<uint32_t>(hdr.nbits);
      mh.tsamp = hdr.tsamp;
      write_rfi_mask(args.rfi_maskfilename, mask, rp, mh);
    }
    if (ngpu > 1) {
      h_clean.resize(bytes);
      PSOUP_HIP_CHECK(hipMemcpy(h_clean.data(), d_clean.data(), bytes, hipMemcpyDeviceToHost));
    }
  }
  DedispGeometry geom = DedispGeometry::make(hdr, fb.nsamps(), res.dm_list, kill);
  res.nsamps = geom.out_nsamps;
  res.tsamp = hdr.tsamp;
  const SpParams sp = sp_params_from(args, hdr.tsamp);
  res.widths = sp_widths(res.nsamps, sp.boxcar_max);
  res.baseline = sp_baseline_samples(sp, res.nsamps);
  const DedispKernel dk = parse_dedisp_kernel(args.dedisp_kernel);
  const int ndm = static_cast<int>(res.dm_list.size());
  const int chunk = Dedisperser::kTileDms;
  std::atomic<int> next{0}, done{0};
  std::atomic<uint64_t> nevents{0}, nreruns{0};
  std::mutex mu;
  std::exception_ptr err;
  std::vector<SpEvent> all;
  std::vector<double> dedisp_s(static_cast<size_t>(ngpu), 0.0), search_s(static_cast<size_t>(ngpu), 0.0);
  ProgressBar progress("Single-pulse search over DM trials");
  if (args.progress_bar) progress.start();
  Stopwatch t_search;
  t_search.start();
  auto worker = [&](int dev) {
    try {
      PSOUP_HIP_CHECK(hipSetDevice(dev));
      Stream stream, side;
      DeviceFilterbank dfb(geom, stream.get());
      if (!rfi) {
        load_filterbank_fanout({&dfb}, {dev}, fb);
      } else if (dev == 0) {
        dfb.load_packed_device(d_clean.data());
        PSOUP_HIP_CHECK(hipStreamSynchronize(stream.get()));
      } else {
        load_filterbank_fanout({&dfb}, {dev}, h_clean.data());
      }
      Dedisperser dd(dfb, stream.get());
      dd.warm();  // every table up front: no upload lands between the two streams' work
      PSOUP_HIP_CHECK(hipStreamSynchronize(stream.get()));
      SinglePulseEngine eng(sp, geom.out_nsamps, stream.get());
      const uint64_t rs = Dedisperser::row_stride(geom.out_nsamps);
      // two trial buffers: chunk k + 1 is dedispersed on the side stream
      // while chunk k is searched on the main one
      DeviceBuffer<uint8_t> trials[2] = {DeviceBuffer<uint8_t>(rs * static_cast<uint64_t>(chunk)),
                                         DeviceBuffer<uint8_t>(rs * static_cast<uint64_t>(chunk))};
      Event ready[2];
      Stopwatch wd, ws;
      auto issue = [&](int slot) -> int {  // next chunk's dedispersion; returns its first DM (or -1)
        const int d0 = next.fetch_add(chunk);
        if (d0 >= ndm) return -1;
        wd.start();
        dd.run(d0, std::min(ndm, d0 + chunk), trials[slot].data(), rs, dk, side.get());
        ready[slot].record(side.get());
        wd.stop();
        return d0;
      };
      int slot = 0;
      int d0 = issue(slot);
      while (d0 >= 0) {
        const int d1 = std::min(ndm, d0 + chunk);
        // search_block(k - 1) has synchronised: the other buffer is free
        const int nd0 = issue(slot ^ 1);
        ws.start();
        PSOUP_HIP_CHECK(hipStreamWaitEvent(stream.get(), ready[slot].get(), 0));
        std::vector<SpEvent> ev = eng.search_block(trials[slot].data(), rs, d1 - d0, d0);
        ws.stop();
        log_verbose("single pulse DMs [" + std::to_string(d0) + ", " + std::to_string(d1) + "): " +
                    std::to_string(ev.size()) + " events");
        {
          std::lock_guard<std::mutex> lk(mu);
          all.insert(all.end(), ev.begin(), ev.end());
        }
        const int dn = done.fetch_add(d1 - d0) + (d1 - d0);
        if (args.progress_bar) progress.set(static_cast<double>(dn) / ndm);
        d0 = nd0;
        slot ^= 1;
      }
      PSOUP_HIP_CHECK(hipStreamSynchronize(side.get()));
      nevents += eng.events();
      nreruns += eng.reruns();
      dedisp_s[static_cast<size_t>(dev)] = wd.get_time();
      search_s[static_cast<size_t>(dev)] = ws.get_time();
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!err) err = std::current_exception();
      next.store(ndm + 1000000);
    }
  };
  std::vector<std::thread> th;
  for (int d = 0; d < ngpu; ++d) th.emplace_back(worker, d);
  for (auto& t : th) t.join();
  t_search.stop();
  if (args.progress_bar) progress.stop();
  if (err) std::rethrow_exception(err);
  // deterministic order before the cross-DM clustering
  std::sort(all.begin(), all.end(), event_order);
  const double band_delay = geom.delays.empty() ? 0.0 : static_cast<double>(geom.delays.back()) * hdr.tsamp;
  res.candidates = sp_cluster(all, res.dm_list, band_delay, hdr.tsamp);
  if (args.limit >= 0 && res.candidates.size() > static_cast<size_t>(args.limit))
    res.candidates.resize(static_cast<size_t>(args.limit));
  res.events = nevents.load();
  res.reruns = nreruns.load();
  t_total.stop();
  res.timers["reading"] = t_read.get_time();
  res.timers["dedispersion"] = *std::max_element(dedisp_s.begin(), dedisp_s.end());
  res.timers["searching"] = t_search.get_time();
  res.timers["total"] = t_total.get_time();
  return res;
}

void write_sp_output(const std::string& path, const SpCmdLineOptions& args, const SpResult& res) {
  FILE* fo = std::fopen(path.c_str(), "w");
  PSOUP_CHECK(fo != nullptr, "cannot open single-pulse output " << path);
  std::fprintf(fo, "# peasoup_amd single-pulse search (spsearch)\n# input: %s\n", args.infilename.c_str());
  std::fprintf(fo, "# dm_trials: %zu (%.3f..%.3f)  nsamps: %llu  tsamp: %.9g s  widths: 1..%d  baseline: %llu samples\n",
               res.dm_list.size(), res.dm_list.empty() ? 0.0 : res.dm_list.front(),
               res.dm_list.empty() ? 0.0 : res.dm_list.back(), static_cast<unsigned long long>(res.nsamps), res.tsamp,
               res.widths.empty() ? 0 : res.widths.back(), static_cast<unsigned long long>(res.baseline));
  std::fprintf(fo, "# events: %llu  min_snr: %g  searching: %.3f s  total: %.3f s\n",
               static_cast<unsigned long long>(res.events), static_cast<double>(args.min_snr),
               res.timers.count("searching") ? res.timers.at("searching") : 0.0,
               res.timers.count("total") ? res.timers.at("total") : 0.0);
  if (!res.rfi_comment.empty()) std::fputs(res.rfi_comment.c_str(), fo);
  std::fprintf(fo, "#%8s %12s %16s %7s %7s %10s %8s %12s %12s %7s %7s\n", "snr", "sample", "time_s", "width", "dm_idx",
               "dm", "members", "first_sample", "last_sample", "dm_lo", "dm_hi");
  for (const SpCandidate& c : res.candidates)
    std::fprintf(fo, "%9.3f %12llu %16.9f %7d %7d %10.4f %8d %12llu %12llu %7d %7d\n", static_cast<double>(c.snr),
                 static_cast<unsigned long long>(c.sample), c.time_s, c.width, c.dm_idx, static_cast<double>(c.dm),
                 c.members, static_cast<unsigned long long>(c.first_sample),
                 static_cast<unsigned long long>(c.last_sample), c.dm_idx_lo, c.dm_idx_hi);
  std::fclose(fo);
}

}  // namespace psoup
