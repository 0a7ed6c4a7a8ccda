// sbsearch, device side: the setup (with every refusal), SidebandSearcher (per
// DM chunk: dedisperse, whiten, forward FFT, sb_power, sb_search, events to the
// host, again with a larger buffer where they passed it) and the file pipeline.
// See psoup/sideband.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>

#include "psoup/sideband.hpp"

namespace psoup {

// ---------------------------------------------------------------- setup ----
SbSetup make_sb_setup(const SbCmdLineOptions& args, const SigprocHeader& hdr) {
  PSOUP_CHECK(args.search.max_num_threads == 1,
              "sideband: sbsearch runs on one device (-t 1); multi-GPU runs and checkpoints are not supported");
  SbSetup s;
  s.params.m_lo = args.m_min;
  s.params.m_hi = args.m_max;
  s.params.j_min = args.j_min;
  s.params.clip = args.clip;
  s.params.min_power = args.min_power;
  PSOUP_CHECK(std::isfinite(args.search.min_freq) && std::isfinite(args.search.max_freq) &&
                  std::isfinite(args.search.dm_start) && std::isfinite(args.search.dm_end) &&
                  std::isfinite(args.search.dm_tol) && std::isfinite(args.search.dm_pulse_width) &&
                  std::isfinite(args.clip) && std::isfinite(args.min_power),
              "sideband: a non-finite value");
  s.search = make_search_setup(args.search, hdr);
  const DedispGeometry g = DedispGeometry::make(hdr, s.search.nsamps, s.search.dm_list, s.search.killmask);
  s.nrow = g.out_nsamps;
  PSOUP_CHECK(s.nrow >= 1, "sideband: the dedispersed series is empty");
  const SearchParams& sp = s.search.search;
  sb_check(s.params, sp.min_freq, sp.max_freq, s.search.fft_size, sp.tsamp);
  s.geom = sb_geometry(sp.min_freq, sp.max_freq, s.search.fft_size, sp.tsamp, s.params.m_lo, s.params.m_hi);
  if (!sp.zap_freqs.empty()) {
    // the whitener's mask: its bin width is the float32 1 / (float32 fft_size x tsamp)
    const float tobs = static_cast<float>(static_cast<float>(s.search.fft_size) * sp.tsamp);
    s.zapmask = build_zap_mask(sp.zap_freqs, sp.zap_widths, static_cast<float>(1.0 / tobs), s.search.fft_size / 2 + 1);
  }
  s.unzapped = sb_unzapped(s.zapmask, s.geom.k_lo, s.geom.k_hi);
  PSOUP_CHECK(s.unzapped >= 1, "sideband: the band has no unzapped bin");
  return s;
}

// ------------------------------------------------------------- searcher ----
SidebandSearcher::SidebandSearcher(const SbSetup& setup, const DeviceFilterbank& fb, hipStream_t stream,
                                   uint32_t capacity)
    : setup_(setup), fb_(fb), stream_(stream), capacity_(std::max<uint32_t>(capacity, 1u)) {
  PSOUP_CHECK(fb.geometry().out_nsamps == setup.nrow && fb.geometry().dm_list.size() == setup.search.dm_list.size(),
              "sideband: the resident filterbank does not belong to this setup");
  const uint64_t n = setup.search.fft_size;
  dd_ = std::make_unique<Dedisperser>(fb, stream);
  dd_->warm();
  wh_ = std::make_unique<Whitener>(n, setup.search.search.tsamp, stream);
  rstride_ = Dedisperser::row_stride(setup.nrow);
  nb_ = n / 2 + 1;
  pstride_ = (nb_ + 3) / 4 * 4;
  const size_t ndm = setup.search.dm_list.size();
  chunk_ = static_cast<int>(std::min<size_t>(std::max<size_t>(ndm, 1), static_cast<size_t>(Dedisperser::kTileDms)));
  const size_t C = static_cast<size_t>(chunk_);
  rows_.resize(rstride_ * C);
  series_.resize(n * C);
  spec_.resize(nb_ * C);
  P_.resize(pstride_ * C);
  stats_.resize(4 * C);
  partials_.resize(static_cast<size_t>(std::max(setup.geom.nranges, 1)) * C);
  mu_.resize(C);
  count_.resize(1);
  events_.resize(capacity_);
  wh_->reserve_batch(chunk_);
  const std::vector<float2> tw = sb_twiddles();
  tw_.resize(tw.size());
  PSOUP_HIP_CHECK(hipMemcpyAsync(tw_.data(), tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, stream_));
  if (!setup.zapmask.empty()) {
    zap_.resize(setup.zapmask.size());
    PSOUP_HIP_CHECK(hipMemcpyAsync(zap_.data(), setup.zapmask.data(), setup.zapmask.size() * sizeof(uint32_t),
                                   hipMemcpyHostToDevice, stream_));
  }
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
}

void SidebandSearcher::powers(int c0, int c1) {
  const int cnt = c1 - c0;
  const uint64_t n = setup_.search.fft_size;
  const SearchParams& sp = setup_.search.search;
  const uint32_t* zap = setup_.zapmask.empty() ? nullptr : zap_.data();
  dd_->run(c0, c1, rows_.data(), rstride_, setup_.search.dedisp_kernel, stream_);
  wh_->whiten_batch(rows_.data(), rstride_, setup_.nrow, cnt, series_.data(), n, zap, stats_.data(),
                    sp.boundary_5_freq, sp.boundary_25_freq);
  for (int b = 0; b < cnt; ++b)
    wh_->forward(series_.data() + static_cast<uint64_t>(b) * n, spec_.data() + static_cast<uint64_t>(b) * nb_);
  kern::sb_power(spec_.data(), nb_, cnt, zap, setup_.geom.k_lo, setup_.geom.k_hi, setup_.unzapped, partials_.data(),
                 mu_.data(), P_.data(), pstride_, stream_);
}

std::vector<SbEvent> SidebandSearcher::search(int d0, int d1) {
  const int ndm = static_cast<int>(setup_.search.dm_list.size());
  if (d1 < 0) d1 = ndm;
  PSOUP_CHECK(d0 >= 0 && d0 <= d1 && d1 <= ndm, "sideband: DM range outside the list");
  std::vector<SbEvent> out;
  for (int c0 = d0; c0 < d1; c0 += chunk_) {
    const int c1 = std::min(d1, c0 + chunk_), cnt = c1 - c0;
    powers(c0, c1);
    for (;;) {
      count_.zero_async(stream_);
      kern::sb_search(P_.data(), pstride_, cnt, setup_.geom, setup_.params, c0, tw_.data(), nullptr, nullptr,
                      events_.data(), capacity_, count_.data(), stream_);
      uint32_t found = 0;
      PSOUP_HIP_CHECK(hipMemcpyAsync(&found, count_.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
      PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
      if (found > capacity_) {
        // the buffer held only the first `capacity_`: the chunk again, with room for all
        capacity_ = found;
        events_.resize(capacity_);
        ++reruns_;
        continue;
      }
      const size_t at = out.size();
      out.resize(at + found);
      if (found != 0) {
        PSOUP_HIP_CHECK(hipMemcpyAsync(out.data() + at, events_.data(), static_cast<size_t>(found) * sizeof(SbEvent),
                                       hipMemcpyDeviceToHost, stream_));
        PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
      }
      break;
    }
  }
  // the append order of the kernel is not fixed: a fixed order for the caller
  std::sort(out.begin(), out.end(), [](const SbEvent& a, const SbEvent& b) {
    if (a.dm_idx != b.dm_idx) return a.dm_idx < b.dm_idx;
    if (a.m != b.m) return a.m < b.m;
    return a.seg < b.seg;
  });
  return out;
}

std::vector<float> SidebandSearcher::power_rows(int d0, int d1, std::vector<double>* mu) {
  const int ndm = static_cast<int>(setup_.search.dm_list.size());
  PSOUP_CHECK(d0 >= 0 && d0 <= d1 && d1 <= ndm, "sideband: DM range outside the list");
  std::vector<float> out(static_cast<size_t>(d1 - d0) * pstride_, 0.f);
  if (mu) mu->assign(static_cast<size_t>(d1 - d0), 0.0);
  for (int c0 = d0; c0 < d1; c0 += chunk_) {
    const int c1 = std::min(d1, c0 + chunk_), cnt = c1 - c0;
    // rows outside the band are never written by sb_power: zero them for the copy
    P_.zero_async(stream_);
    powers(c0, c1);
    PSOUP_HIP_CHECK(hipMemcpyAsync(out.data() + static_cast<size_t>(c0 - d0) * pstride_, P_.data(),
                                   static_cast<size_t>(cnt) * pstride_ * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (mu)
      PSOUP_HIP_CHECK(hipMemcpyAsync(mu->data() + (c0 - d0), mu_.data(), static_cast<size_t>(cnt) * sizeof(double),
                                     hipMemcpyDeviceToHost, stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  return out;
}

// ------------------------------------------------------------- pipeline ----
SbRun run_sb_pipeline(const SbCmdLineOptions& args) {
  SbRun run;
  Stopwatch t_total, t_read, t_search;
  t_total.start();
  if (args.search.verbose) set_log_level(LogLevel::Verbose);
  // every refusal, from the header alone, before the data is read and before any device work
  run.setup = make_sb_setup(args, read_header_file(args.search.infilename));
  const SbSetup& setup = run.setup;
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.search.infilename);
  t_read.stop();
  PSOUP_CHECK(fb.nsamps() * fb.bytes_per_sample() <= fb.data_bytes(), "sbsearch: truncated filterbank");
  log_verbose("sbsearch: " + std::to_string(setup.search.dm_list.size()) + " DM trials, band [" +
              std::to_string(setup.geom.k_lo) + ", " + std::to_string(setup.geom.k_hi) + "), " +
              std::to_string(setup.geom.nwin) + " windows per row");
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  t_search.start();
  Stream stream;
  const DedispGeometry geom =
      DedispGeometry::make(fb.header(), fb.nsamps(), setup.search.dm_list, setup.search.killmask);
  DeviceFilterbank dfb(geom, stream.get());
  dfb.load_packed_host(fb.data());
  SidebandSearcher ss(setup, dfb, stream.get());
  std::vector<SbEvent> events = ss.search();
  run.events = events.size();
  std::vector<SbCandidate> cands = sb_cluster(std::move(events));
  t_search.stop();
  cands.resize(std::min(static_cast<size_t>(std::max(args.search.limit, 0)), cands.size()));
  run.candidates = std::move(cands);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

void write_sb_output(const SbCmdLineOptions& args, const SbSetup& setup, const std::vector<SbCandidate>& cands) {
  const std::string tmp = args.outfilename + ".tmp";
  {
    std::ofstream out(tmp);
    PSOUP_CHECK(static_cast<bool>(out), "cannot open output " << tmp);
    out << sb_output_text(args, setup, cands);
    if (!out.flush()) {
      out.close();
      std::remove(tmp.c_str());
      PSOUP_THROW("cannot write output " << tmp);
    }
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), args.outfilename.c_str()) == 0,
              "cannot rename " << tmp << " to " << args.outfilename);
}

}  // namespace psoup
