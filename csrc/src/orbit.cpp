// orbsearch, device side: the setup (with every refusal), OrbitSearcher (per DM
// chunk: dedisperse, resample per group of templates, whiten and search on the
// unchanged engine, orbit-distil per DM), the fold on the re-made DM-template
// rows and the file pipeline.  See psoup/orbit.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "psoup/orbit.hpp"

namespace psoup {

// ---------------------------------------------------------------- setup ----
OrbitSetup make_orbit_setup(const OrbitCmdLineOptions& args, const SigprocHeader& hdr) {
  PSOUP_CHECK(args.search.max_num_threads == 1,
              "orbit: orbsearch runs on one device (-t 1); multi-GPU runs and checkpoints are not supported");
  OrbitSetup s;
  s.bank = orbit_bank_of(args);
  s.search = make_search_setup(args.search, hdr);
  const DedispGeometry g = DedispGeometry::make(hdr, s.search.nsamps, s.search.dm_list, s.search.killmask);
  s.nrow = g.out_nsamps;
  PSOUP_CHECK(s.nrow >= 1, "orbit: the dedispersed series is empty");
  s.span = std::min<uint64_t>(s.nrow, s.search.fft_size);
  const float tsamp = s.search.search.tsamp;
  orbit_check(s.span, s.bank, tsamp);
  for (const OrbitTemplate& t : s.bank) {
    s.quant.push_back(orbit_quantise(t.pb, t.a1, t.ph, tsamp));
    s.beta.push_back(orbit_beta(t));
  }
  return s;
}

// ------------------------------------------------------------- searcher ----
OrbitSearcher::OrbitSearcher(const OrbitSetup& setup, const DeviceFilterbank& fb, hipStream_t stream)
    : setup_(setup), fb_(fb), stream_(stream), d_q_(static_cast<size_t>(kOrbitMaxPerLaunch)),
      d_table_(static_cast<size_t>(kern::kOrbitTable)) {
  PSOUP_CHECK(fb.geometry().out_nsamps == setup.nrow && fb.geometry().dm_list.size() == setup.search.dm_list.size(),
              "orbit: the resident filterbank does not belong to this setup");
  PSOUP_CHECK(!setup.bank.empty() && setup.quant.size() == setup.bank.size(), "orbit: an empty bank");
  dd_ = std::make_unique<Dedisperser>(fb, stream);
  dd_->warm();
  engine_ = std::make_unique<SearchEngine>(setup.search.search, stream);
  rstride_ = Dedisperser::row_stride(setup.nrow);
  const size_t ndm = setup.search.dm_list.size();
  rows_.resize(rstride_ * std::min<size_t>(ndm, static_cast<size_t>(Dedisperser::kTileDms)));
  resampled_.resize(rstride_ * static_cast<size_t>(engine_->max_prepare()));
  const std::vector<int32_t> table = orbit_sine_table();
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_table_.data(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                 stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
}

void OrbitSearcher::resample(const uint8_t* rows, int nrows, size_t k0, int kc, uint8_t* out) {
  PSOUP_CHECK(kc >= 1 && kc <= kOrbitMaxPerLaunch && k0 + static_cast<size_t>(kc) <= setup_.quant.size(),
              "orbit: a template group outside the bank");
  for (int k = 0; k < kc; ++k) orbit_check_quant(setup_.quant[k0 + static_cast<size_t>(k)]);
  // (pageable source: the copy has left the host vector when the call returns)
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_q_.data(), setup_.quant.data() + k0, static_cast<size_t>(kc) * sizeof(OrbitQuant),
                                 hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  kern::orbit_resample(rows, rstride_, nrows, setup_.nrow, setup_.span, d_q_.data(), kc, d_table_.data(), out, rstride_,
                       stream_);
}

OrbitCandidateList OrbitSearcher::search(int d0, int d1) {
  const int ndm = static_cast<int>(setup_.search.dm_list.size());
  if (d1 < 0) d1 = ndm;
  PSOUP_CHECK(d0 >= 0 && d0 <= d1 && d1 <= ndm, "orbit: DM range outside the list");
  const int chunk = Dedisperser::kTileDms;
  const int mp = engine_->max_prepare();
  const size_t K = setup_.bank.size();
  OrbitCandidateList out;
  for (int c0 = d0; c0 < d1; c0 += chunk) {
    const int c1 = std::min(d1, c0 + chunk), cnt = c1 - c0;
    dd_->run(c0, c1, rows_.data(), rstride_, setup_.search.dedisp_kernel, stream_);
    // runs of at most max_prepare rows; the bank is the same at every DM
    for (int r0 = 0; r0 < cnt;) {
      const int r1 = std::min(cnt, r0 + mp), R = r1 - r0;
      const size_t kk = static_cast<size_t>(std::min(std::max(1, mp / R), kOrbitMaxPerLaunch));
      std::vector<OrbitCandidateList> per_dm(static_cast<size_t>(R));
      for (size_t k0 = 0; k0 < K; k0 += kk) {
        const int kc = static_cast<int>(std::min(kk, K - k0));
        resample(rows_.data() + static_cast<uint64_t>(r0) * rstride_, R, k0, kc, resampled_.data());
        engine_->prepare(resampled_.data(), rstride_, setup_.nrow, R * kc);
        std::vector<SearchEngine::Job> jobs;
        for (int r = 0; r < R; ++r)
          for (int k = 0; k < kc; ++k) {
            const int d = c0 + r0 + r;
            const float dm = setup_.search.dm_list[static_cast<size_t>(d)];
            jobs.push_back(SearchEngine::Job{r * kc + k, dm, d, setup_.search.accel_plan.generate(dm)});
            accel_trials_ += jobs.back().accs.size();
            ++template_trials_;
          }
        std::vector<CandidateList> lists = engine_->search_prepared_many(jobs);
        for (int r = 0; r < R; ++r)
          for (int k = 0; k < kc; ++k)
            for (Candidate& c : lists[static_cast<size_t>(r * kc + k)])
              per_dm[static_cast<size_t>(r)].push_back(
                  OrbitCandidate{std::move(c), static_cast<uint32_t>(k0 + static_cast<size_t>(k))});
      }
      for (int r = 0; r < R; ++r) {
        OrbitCandidateList kept = std::move(per_dm[static_cast<size_t>(r)]);
        if (K > 1) kept = orbit_distill(std::move(kept), setup_.beta, setup_.search.search.freq_tol, true);
        for (OrbitCandidate& c : kept) out.push_back(std::move(c));
      }
      r0 = r1;
    }
  }
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

void OrbitSearcher::fold(OrbitCandidateList& cands, int npdmp) {
  if (npdmp <= 0 || cands.empty()) return;
  // the plain search's selection (select_fold_candidates), grouped by DM and template
  std::map<std::pair<int, uint32_t>, std::vector<int>> groups;
  const int count = std::min(npdmp, static_cast<int>(cands.size()));
  for (int i = 0; i < count; ++i) {
    const float p = static_cast<float>(1.0 / cands[static_cast<size_t>(i)].cand.freq);
    if (!(p > 0.001f && p < 10.00f)) continue;
    groups[{cands[static_cast<size_t>(i)].cand.dm_idx, cands[static_cast<size_t>(i)].tmpl}].push_back(i);
  }
  if (!groups.empty()) {
    FoldEngine fe(prev_power_of_two(setup_.nrow), setup_.search.search.tsamp, stream_);
    const size_t B = static_cast<size_t>(std::max(1, fe.max_batch()));
    DeviceBuffer<uint8_t> frows(rstride_ * B);
    std::vector<std::pair<std::pair<int, uint32_t>, std::vector<int>>> glist(groups.begin(), groups.end());
    for (size_t b0 = 0; b0 < glist.size(); b0 += B) {
      const size_t cnt = std::min(B, glist.size() - b0);
      std::vector<std::vector<double>> periods(cnt);
      std::vector<std::vector<float>> accs(cnt);
      for (size_t t = 0; t < cnt; ++t) {
        const auto& grp = glist[b0 + t];
        // the DM-template row, re-made
        dd_->run_list({grp.first.first}, rows_.data(), rstride_, stream_);
        resample(rows_.data(), 1, static_cast<size_t>(grp.first.second), 1, frows.data() + t * rstride_);
        for (int ci : grp.second) {
          periods[t].push_back(static_cast<double>(static_cast<float>(1.0 / cands[static_cast<size_t>(ci)].cand.freq)));
          accs[t].push_back(cands[static_cast<size_t>(ci)].cand.acc);
        }
      }
      std::vector<const uint8_t*> rows;
      for (size_t t = 0; t < cnt; ++t) rows.push_back(frows.data() + t * rstride_);
      auto fr = fe.fold_rows(rows, setup_.nrow, periods, accs);
      for (size_t t = 0; t < cnt; ++t) {
        const auto& grp = glist[b0 + t];
        for (size_t k = 0; k < fr[t].size(); ++k) {
          Candidate& c = cands[static_cast<size_t>(grp.second[k])].cand;
          c.folded_snr = fr[t][k].folded_snr;
          c.set_fold(fr[t][k].fold.data(), FoldEngine::kNbins, FoldEngine::kNints);
          c.opt_period = fr[t][k].opt_period;
        }
      }
    }
  }
  std::stable_sort(cands.begin(), cands.end(), [](const OrbitCandidate& x, const OrbitCandidate& y) {
    return std::max(x.cand.snr, x.cand.folded_snr) > std::max(y.cand.snr, y.cand.folded_snr);
  });
}

// ---------------------------------------------------- global distillation ----
namespace {
void clear_tags(Candidate& c) {
  c.opt_period = 0.0;
  for (Candidate& a : c.assoc) clear_tags(a);
}
}  // namespace

OrbitCandidateList orbit_global_distill(OrbitCandidateList cands, const OrbitCmdLineOptions& args,
                                        const OrbitSetup& setup) {
  // The distillers move whole candidates: until they are folded, opt_period is
  // unused and carries the index of the wrapper record through them.
  std::vector<uint32_t> tmpl(cands.size());
  CandidateList plain;
  plain.reserve(cands.size());
  for (size_t i = 0; i < cands.size(); ++i) {
    tmpl[i] = cands[i].tmpl;
    cands[i].cand.opt_period = static_cast<double>(i);
    plain.push_back(std::move(cands[i].cand));
  }
  stable_sort_by_dm_idx(plain);
  plain = global_distill_and_score(std::move(plain), args.search, setup.search);
  OrbitCandidateList out;
  out.reserve(plain.size());
  for (Candidate& c : plain) {
    const size_t i = static_cast<size_t>(c.opt_period);
    PSOUP_CHECK(i < tmpl.size(), "orbit: a candidate lost its record");
    clear_tags(c);
    out.push_back(OrbitCandidate{std::move(c), tmpl[i]});
  }
  return out;
}

// ------------------------------------------------------------- pipeline ----
OrbitRun run_orbit_pipeline(const OrbitCmdLineOptions& args) {
  OrbitRun run;
  Stopwatch t_total, t_read, t_search, t_fold;
  t_total.start();
  if (args.search.verbose) set_log_level(LogLevel::Verbose);
  // every refusal, from the header alone, before the data is read and before any device work
  run.setup = make_orbit_setup(args, read_header_file(args.search.infilename));
  const OrbitSetup& setup = run.setup;
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.search.infilename);
  t_read.stop();
  PSOUP_CHECK(fb.nsamps() * fb.bytes_per_sample() <= fb.data_bytes(), "orbsearch: truncated filterbank");
  log_verbose("orbsearch: " + std::to_string(setup.search.dm_list.size()) + " DM trials, " +
              std::to_string(setup.bank.size()) + " templates, span " + std::to_string(setup.span));
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  t_search.start();
  Stream stream;
  const DedispGeometry geom =
      DedispGeometry::make(fb.header(), fb.nsamps(), setup.search.dm_list, setup.search.killmask);
  DeviceFilterbank dfb(geom, stream.get());
  dfb.load_packed_host(fb.data());
  OrbitSearcher os(setup, dfb, stream.get());
  OrbitCandidateList cands = os.search();
  cands = orbit_global_distill(std::move(cands), args, setup);
  t_search.stop();
  t_fold.start();
  os.fold(cands, args.search.npdmp);
  t_fold.stop();
  cands.resize(std::min(static_cast<size_t>(std::max(args.search.limit, 0)), cands.size()));
  run.candidates = std::move(cands);
  run.accel_trials = os.accel_trials();
  run.template_trials = os.template_trials();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["folding"] = t_fold.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

void write_orbit_output(const OrbitCmdLineOptions& args, const OrbitSetup& setup, const OrbitCandidateList& cands) {
  const std::string tmp = args.outfilename + ".tmp";
  {
    std::ofstream out(tmp);
    PSOUP_CHECK(static_cast<bool>(out), "cannot open output " << tmp);
    out << orbit_output_text(args, setup, cands);
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
