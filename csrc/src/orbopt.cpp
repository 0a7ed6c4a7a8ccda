// orbopt, device side: OrbitOptimiser (validate every candidate, then per batch
// dedisperse the batch's DMs, fold on the template grids, search, copy the
// optimum planes back and finish) and the file pipeline.  See psoup/orbopt.hpp.
#include "psoup/orbopt.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

#include "psoup/plan.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// ------------------------------------------------------------ optimiser ----
OrbitOptimiser::OrbitOptimiser(const OrbOptParams& p, const DeviceFilterbank& fb, uint64_t fft_size, hipStream_t stream,
                               size_t batch_bytes)
    : p_(p), fb_(fb), stream_(stream), batch_bytes_(batch_bytes), d_table_(static_cast<size_t>(kern::kOrbitTable)) {
  oopt_check_params(p_);
  nrow_ = fb.geometry().out_nsamps;
  PSOUP_CHECK(nrow_ >= 1, "orbopt: the dedispersed series is empty");
  PSOUP_CHECK(fft_size >= 1, "orbopt: fft_size must be at least 1");
  n_ = std::min<uint64_t>(nrow_, fft_size);
  PSOUP_CHECK(n_ <= kOrbitMaxSpan, "orbopt: series longer than 2^26 samples (n = " << n_ << ")");
  tsamp_ = static_cast<float>(fb.geometry().tsamp);
  rstride_ = Dedisperser::row_stride(nrow_);
  dd_ = std::make_unique<Dedisperser>(fb, stream);
  const std::vector<int32_t> table = orbit_sine_table();
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_table_.data(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                 stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
}

OrbitOptimiser::~OrbitOptimiser() { (void)hipStreamSynchronize(stream_); }

std::vector<uint8_t> OrbitOptimiser::row(int d) {
  PSOUP_CHECK(d >= 0 && static_cast<size_t>(d) < fb_.geometry().dm_list.size(), "orbopt: DM index outside the list");
  DeviceBuffer<uint8_t> r(rstride_);
  dd_->run_list({d}, r.data(), rstride_, stream_);
  std::vector<uint8_t> h(nrow_);
  PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), r.data(), nrow_, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  return h;
}

std::vector<OrbOptResult> OrbitOptimiser::optimise(const std::vector<OrbOptCandidate>& cands) {
  const size_t nc = cands.size();
  const std::vector<float>& dms = fb_.geometry().dm_list;
  const size_t plane = static_cast<size_t>(p_.nints) * p_.nbins;
  const size_t nw = static_cast<size_t>(nwidths());
  // every candidate is validated (and its grid built) before the first launch
  std::vector<OrbOptGrid> grids(nc);
  std::vector<int> dm_idx(nc);
  for (size_t i = 0; i < nc; ++i) {
    grids[i] = oopt_grid(i, p_, cands[i], n_, tsamp_);
    const auto it = std::find(dms.begin(), dms.end(), cands[i].dm);
    PSOUP_CHECK(it != dms.end(), "orbopt: candidate " << i << ": its DM " << cands[i].dm
                                                      << " is not in the resident filterbank's list");
    dm_idx[i] = static_cast<int>(it - dms.begin());
  }
  // the row moments of every DM in use: their refusal comes before any fold too
  std::vector<int> used(dm_idx);
  std::sort(used.begin(), used.end());
  used.erase(std::unique(used.begin(), used.end()), used.end());
  std::vector<OrbOptMoments> mom(nc);
  {
    DeviceBuffer<uint8_t> r(rstride_);
    std::vector<uint8_t> h(n_);
    for (int d : used) {
      dd_->run_list({d}, r.data(), rstride_, stream_);
      PSOUP_HIP_CHECK(hipMemcpyAsync(h.data(), r.data(), n_, hipMemcpyDeviceToHost, stream_));
      PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
      bool first = true;
      OrbOptMoments md;
      for (size_t i = 0; i < nc; ++i)
        if (dm_idx[i] == d) {
          if (first) md = oopt_moments(i, h.data(), n_);
          first = false;
          mom[i] = md;
        }
    }
  }
  const std::vector<int32_t> st = oopt_drift_table(p_);
  DeviceBuffer<int32_t> d_st(st.size());
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_st.data(), st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));

  std::vector<OrbOptResult> out(nc);
  // hits depend on G alone (n, nints and nbins are the run's): candidates of one period share them
  std::map<uint64_t, std::vector<int32_t>> hits_of;
  DeviceBuffer<uint8_t> d_rows;
  DeviceBuffer<int32_t> d_rowof, d_m, d_hits, d_fold, d_val, d_idx, d_centre, d_tcurve;
  DeviceBuffer<uint64_t> d_G, d_keys;
  DeviceBuffer<int64_t> d_msum;
  DeviceBuffer<OrbitQuant> d_q;
  for (size_t b0 = 0; b0 < nc;) {
    // a batch: consecutive candidates of one template count, inside the budget
    const size_t K = grids[b0].tmpl.size();
    const size_t per = K * plane * sizeof(int32_t) + rstride_ + K * (sizeof(OrbitQuant) + 8 + 4 * nw) + plane * 4 + 64;
    const size_t most = std::min<size_t>(std::max<size_t>(1, batch_bytes_ / per), 65535);
    size_t nb = 1;
    while (b0 + nb < nc && nb < most && grids[b0 + nb].tmpl.size() == K) ++nb;
    // the batch's rows
    std::vector<int> rows_dm;
    std::vector<int32_t> rowof(nb);
    for (size_t i = 0; i < nb; ++i) {
      const auto it = std::find(rows_dm.begin(), rows_dm.end(), dm_idx[b0 + i]);
      rowof[i] = static_cast<int32_t>(it - rows_dm.begin());
      if (it == rows_dm.end()) rows_dm.push_back(dm_idx[b0 + i]);
    }
    d_rows.resize(rows_dm.size() * rstride_);
    dd_->run_list(rows_dm, d_rows.data(), rstride_, stream_);
    std::vector<uint64_t> G(nb);
    std::vector<int32_t> ms(nb), hits(nb * plane);
    std::vector<OrbitQuant> q(nb * K);
    for (size_t i = 0; i < nb; ++i) {
      const OrbOptGrid& g = grids[b0 + i];
      G[i] = g.G;
      ms[i] = static_cast<int32_t>(mom[b0 + i].m);
      auto hit = hits_of.find(g.G);
      if (hit == hits_of.end()) hit = hits_of.emplace(g.G, oopt_hits(g.G, n_, p_.nints, p_.nbins)).first;
      const std::vector<int32_t>& h = hit->second;
      std::copy(h.begin(), h.end(), hits.begin() + i * plane);
      for (size_t k = 0; k < K; ++k) {
        orbit_check_quant(g.quant[k]);
        q[i * K + k] = g.quant[k];
      }
    }
    d_rowof.resize(nb);
    d_G.resize(nb);
    d_m.resize(nb);
    d_hits.resize(nb * plane);
    d_q.resize(nb * K);
    d_fold.resize(nb * K * plane);
    d_keys.resize(nb * nw);
    d_val.resize(nb * nw);
    d_idx.resize(nb * nw);
    d_centre.resize(nb * nw);
    d_tcurve.resize(nb * nw * K);
    d_msum.resize(nb * K);
    auto up = [&](void* dst, const void* src, size_t bytes) {
      PSOUP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_));
    };
    up(d_rowof.data(), rowof.data(), nb * sizeof(int32_t));
    up(d_G.data(), G.data(), nb * sizeof(uint64_t));
    up(d_m.data(), ms.data(), nb * sizeof(int32_t));
    up(d_hits.data(), hits.data(), hits.size() * sizeof(int32_t));
    up(d_q.data(), q.data(), q.size() * sizeof(OrbitQuant));
    // (pageable sources: the copies have left the host vectors when the calls return)
    kern::orbopt_fold(d_rows.data(), rstride_, rows_dm.size() * rstride_, d_rowof.data(), d_G.data(), d_q.data(),
                      static_cast<int>(nb), static_cast<int>(K), n_, p_.nints, p_.nbins, d_table_.data(), d_fold.data(),
                      stream_);
    kern::orbopt_search(d_fold.data(), d_hits.data(), d_m.data(), d_st.data(), static_cast<int>(nb), static_cast<int>(K),
                        p_.nints, p_.nbins, p_.np, d_keys.data(), d_val.data(), d_idx.data(), d_tcurve.data(),
                        d_centre.data(), d_msum.data(), stream_);
    ++nbatches_;
    std::vector<int32_t> val(nb * nw), idx(nb * nw), cen(nb * nw), tc(nb * nw * K);
    std::vector<int64_t> msum(nb * K);
    auto down = [&](void* dst, const void* src, size_t bytes) {
      PSOUP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_));
    };
    down(val.data(), d_val.data(), val.size() * sizeof(int32_t));
    down(idx.data(), d_idx.data(), idx.size() * sizeof(int32_t));
    down(cen.data(), d_centre.data(), cen.size() * sizeof(int32_t));
    down(tc.data(), d_tcurve.data(), tc.size() * sizeof(int32_t));
    down(msum.data(), d_msum.data(), msum.size() * sizeof(int64_t));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
    std::vector<int32_t> fplane(plane);
    for (size_t i = 0; i < nb; ++i) {
      OrbOptSearch found;
      found.best_val.assign(val.begin() + i * nw, val.begin() + (i + 1) * nw);
      found.best_idx.assign(idx.begin() + i * nw, idx.begin() + (i + 1) * nw);
      found.centre.assign(cen.begin() + i * nw, cen.begin() + (i + 1) * nw);
      found.tcurve.assign(tc.begin() + i * nw * K, tc.begin() + (i + 1) * nw * K);
      found.msum.assign(msum.begin() + i * K, msum.begin() + (i + 1) * K);
      const OrbOptOptimum o = oopt_optimum(p_, grids[b0 + i], mom[b0 + i], found);
      down(fplane.data(), d_fold.data() + (i * K + o.k) * plane, plane * sizeof(int32_t));
      PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
      const std::vector<int32_t> h(hits.begin() + i * plane, hits.begin() + (i + 1) * plane);
      out[b0 + i] = oopt_finish(p_, cands[b0 + i], grids[b0 + i], n_, tsamp_, mom[b0 + i], h, st, found, fplane.data());
    }
    b0 += nb;
  }
  return out;
}

// ------------------------------------------------------------- pipeline ----
OrbOptRun run_orbopt_pipeline(const OrbOptCmdLineOptions& args) {
  OrbOptRun run;
  Stopwatch t_total, t_read, t_search;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  // every refusal that needs no data, before the filterbank is read and before any device work
  PSOUP_CHECK(args.max_num_threads == 1,
              "orbopt: orbopt runs on one device (-t 1); multi-GPU runs are not supported");
  const OrbOptParams p = oopt_params_of(args);
  oopt_check_params(p);
  std::vector<OrbOptCandidate> cands;
  {
    std::ifstream in(args.candfilename);
    PSOUP_CHECK(static_cast<bool>(in), "orbopt: cannot open the candidate file " << args.candfilename);
    std::ostringstream os;
    os << in.rdbuf();
    cands = oopt_parse_candidates(os.str());
  }
  PSOUP_CHECK(!cands.empty(), "orbopt: an empty candidate file (" << args.candfilename << ")");
  if (args.limit >= 0 && cands.size() > static_cast<size_t>(args.limit)) cands.resize(static_cast<size_t>(args.limit));
  PSOUP_CHECK(!cands.empty(), "orbopt: an empty candidate file (--limit 0)");
  const std::vector<float> dm_list = oopt_dm_list(cands);
  const SigprocHeader hdr = read_header_file(args.infilename);
  std::vector<int> killmask(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) killmask = read_killfile(args.killfilename, hdr.nchans);
  const uint64_t nsamps = static_cast<uint64_t>(hdr.nsamples);
  const uint64_t fft_size = args.size == 0 ? prev_power_of_two(nsamps) : args.size;
  {
    const DedispGeometry g0 = DedispGeometry::make(hdr, nsamps, dm_list, killmask);
    PSOUP_CHECK(g0.out_nsamps >= 1, "orbopt: the dedispersed series is empty");
    const uint64_t n = std::min<uint64_t>(g0.out_nsamps, fft_size);
    for (size_t i = 0; i < cands.size(); ++i) oopt_grid(i, p, cands[i], n, static_cast<float>(hdr.tsamp));
  }
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  t_read.stop();
  PSOUP_CHECK(fb.nsamps() * fb.bytes_per_sample() <= fb.data_bytes(), "orbopt: truncated filterbank");
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  PSOUP_HIP_CHECK(hipSetDevice(0));
  t_search.start();
  Stream stream;
  const DedispGeometry geom = DedispGeometry::make(fb.header(), fb.nsamps(), dm_list, killmask);
  DeviceFilterbank dfb(geom, stream.get());
  dfb.load_packed_host(fb.data());
  OrbitOptimiser opt(p, dfb, fft_size, stream.get());
  run.results = opt.optimise(cands);
  t_search.stop();
  log_verbose("orbopt: " + std::to_string(cands.size()) + " candidates at " + std::to_string(dm_list.size()) +
              " DMs, span " + std::to_string(opt.span()) + ", " + std::to_string(opt.batches()) + " batches");
  OrbOptFileHeader& h = run.header;
  h.ncand = static_cast<uint32_t>(cands.size());
  h.nints = static_cast<uint32_t>(p.nints);
  h.nbins = static_cast<uint32_t>(p.nbins);
  h.npb = static_cast<uint32_t>(p.npb);
  h.na1 = static_cast<uint32_t>(p.na1);
  h.nphase = static_cast<uint32_t>(p.nphase);
  h.np = static_cast<uint32_t>(p.np);
  h.nw = static_cast<uint32_t>(opt.nwidths());
  h.n = opt.span();
  h.tsamp = static_cast<double>(opt.tsamp());
  h.p_step = p.p_step;
  write_orbopt_file(args.outfilename, h, run.results);
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
