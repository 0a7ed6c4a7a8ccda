// jerksearch, device side: the setup (with every refusal), JerkSearcher (per DM
// chunk: dedisperse, resample per group of jerk trials, whiten and search on
// the unchanged engine, jerk-distil per DM), the fold on the re-made DM-jerk
// rows and the file pipeline.  See psoup/jerk.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "psoup/jerk.hpp"

namespace psoup {

// ---------------------------------------------------------------- setup ----
JerkSetup make_jerk_setup(const JerkCmdLineOptions& args, const SigprocHeader& hdr) {
  PSOUP_CHECK(std::isfinite(args.jerk_start) && std::isfinite(args.jerk_end) && std::isfinite(args.jerk_tol) &&
                  std::isfinite(args.jerk_step),
              "jerk: a non-finite value (--jerk_start, --jerk_end, --jerk_tol or --jerk_step)");
  PSOUP_CHECK(!(args.jerk_start > args.jerk_end),
              "jerk: jerk_start > jerk_end (" << args.jerk_start << " > " << args.jerk_end << ")");
  PSOUP_CHECK(args.jerk_tol > 1.f || args.jerk_step > 0.f || args.jerk_start == args.jerk_end,
              "jerk: --jerk_tol must be above 1");
  JerkSetup s;
  s.search = make_search_setup(args.search, hdr);
  const DedispGeometry g = DedispGeometry::make(hdr, s.search.nsamps, s.search.dm_list, s.search.killmask);
  s.nrow = g.out_nsamps;
  PSOUP_CHECK(s.nrow >= 1, "jerk: the dedispersed series is empty");
  s.span = std::min<uint64_t>(s.nrow, s.search.fft_size);
  PSOUP_CHECK(s.span <= kJerkMaxSpan, "jerk: series longer than 2^26 samples (n = " << s.span << ")");
  const float tsamp = s.search.search.tsamp;
  s.plan = JerkPlan(args.jerk_start, args.jerk_end, args.jerk_tol, args.jerk_step, args.search.acc_pulse_width, s.span,
                    tsamp, s.search.cfreq, static_cast<float>(hdr.foff),
                    parse_accel_convention(args.search.accel_convention));
  for (float dm : s.search.dm_list) {
    s.jerks.push_back(s.plan.generate(dm));
    std::vector<double> jf;
    for (float j : s.jerks.back()) jf.push_back(jerk_factor(j, tsamp));
    jerk_check(s.span, jf);
    s.total_trials += jf.size();
  }
  return s;
}

// ------------------------------------------------------------- searcher ----
JerkSearcher::JerkSearcher(const JerkSetup& setup, const DeviceFilterbank& fb, hipStream_t stream)
    : setup_(setup), fb_(fb), stream_(stream), d_jf_(static_cast<size_t>(kJerkMaxTrials)) {
  PSOUP_CHECK(fb.geometry().out_nsamps == setup.nrow && fb.geometry().dm_list.size() == setup.search.dm_list.size(),
              "jerk: the resident filterbank does not belong to this setup");
  dd_ = std::make_unique<Dedisperser>(fb, stream);
  dd_->warm();
  engine_ = std::make_unique<SearchEngine>(setup.search.search, stream);
  rstride_ = Dedisperser::row_stride(setup.nrow);
  jerk_stationary(setup.span, &sp0_, &sp1_);
  const size_t ndm = setup.search.dm_list.size();
  rows_.resize(rstride_ * std::min<size_t>(ndm, static_cast<size_t>(Dedisperser::kTileDms)));
  resampled_.resize(rstride_ * static_cast<size_t>(engine_->max_prepare()));
}

void JerkSearcher::resample(const uint8_t* rows, int nrows, const std::vector<float>& jerks, size_t k0, int kc,
                            uint8_t* out) {
  std::vector<double> jf(static_cast<size_t>(kc));
  for (int k = 0; k < kc; ++k) jf[static_cast<size_t>(k)] = jerk_factor(jerks[k0 + static_cast<size_t>(k)],
                                                                         setup_.search.search.tsamp);
  jerk_check(setup_.span, jf);
  // (pageable source: the copy has left the host vector when the call returns)
  PSOUP_HIP_CHECK(hipMemcpyAsync(d_jf_.data(), jf.data(), jf.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  kern::jerk_resample(rows, rstride_, nrows, setup_.nrow, setup_.span, d_jf_.data(), kc, out, rstride_, sp0_, sp1_,
                      stream_);
}

JerkCandidateList JerkSearcher::search(int d0, int d1) {
  const int ndm = static_cast<int>(setup_.search.dm_list.size());
  if (d1 < 0) d1 = ndm;
  PSOUP_CHECK(d0 >= 0 && d0 <= d1 && d1 <= ndm, "jerk: DM range outside the list");
  const int chunk = Dedisperser::kTileDms;
  const int mp = engine_->max_prepare();
  const double span_s = static_cast<double>(setup_.span) * static_cast<double>(setup_.search.search.tsamp);
  JerkCandidateList out;
  for (int c0 = d0; c0 < d1; c0 += chunk) {
    const int c1 = std::min(d1, c0 + chunk), cnt = c1 - c0;
    dd_->run(c0, c1, rows_.data(), rstride_, setup_.search.dedisp_kernel, stream_);
    // runs of rows that share one jerk list, at most max_prepare rows each
    for (int r0 = 0; r0 < cnt;) {
      const std::vector<float>& jl = setup_.jerks[static_cast<size_t>(c0 + r0)];
      int r1 = r0 + 1;
      while (r1 < cnt && r1 - r0 < mp && setup_.jerks[static_cast<size_t>(c0 + r1)] == jl) ++r1;
      const int R = r1 - r0, K = static_cast<int>(jl.size()), kk = std::max(1, mp / R);
      std::vector<JerkCandidateList> per_dm(static_cast<size_t>(R));
      for (int k0 = 0; k0 < K; k0 += kk) {
        const int kc = std::min(kk, K - k0);
        resample(rows_.data() + static_cast<uint64_t>(r0) * rstride_, R, jl, static_cast<size_t>(k0), kc,
                 resampled_.data());
        engine_->prepare(resampled_.data(), rstride_, setup_.nrow, R * kc);
        std::vector<SearchEngine::Job> jobs;
        for (int r = 0; r < R; ++r)
          for (int k = 0; k < kc; ++k) {
            const int d = c0 + r0 + r;
            const float dm = setup_.search.dm_list[static_cast<size_t>(d)];
            jobs.push_back(SearchEngine::Job{r * kc + k, dm, d, setup_.search.accel_plan.generate(dm)});
            accel_trials_ += jobs.back().accs.size();
            ++jerk_trials_;
          }
        std::vector<CandidateList> lists = engine_->search_prepared_many(jobs);
        for (int r = 0; r < R; ++r)
          for (int k = 0; k < kc; ++k)
            for (Candidate& c : lists[static_cast<size_t>(r * kc + k)])
              per_dm[static_cast<size_t>(r)].push_back(JerkCandidate{std::move(c), jl[static_cast<size_t>(k0 + k)]});
      }
      for (int r = 0; r < R; ++r) {
        JerkCandidateList kept = jerk_distill(std::move(per_dm[static_cast<size_t>(r)]), engine_->tobs(), span_s,
                                              setup_.search.search.freq_tol, true);
        for (JerkCandidate& c : kept) out.push_back(std::move(c));
      }
      r0 = r1;
    }
  }
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  return out;
}

void JerkSearcher::fold(JerkCandidateList& cands, int npdmp) {
  if (npdmp <= 0 || cands.empty()) return;
  // the plain search's selection (select_fold_candidates), grouped by DM and jerk
  std::map<std::pair<int, uint32_t>, std::vector<int>> groups;
  const int count = std::min(npdmp, static_cast<int>(cands.size()));
  for (int i = 0; i < count; ++i) {
    const float p = static_cast<float>(1.0 / cands[static_cast<size_t>(i)].cand.freq);
    if (!(p > 0.001f && p < 10.00f)) continue;
    uint32_t jb;
    std::memcpy(&jb, &cands[static_cast<size_t>(i)].jerk, 4);
    groups[{cands[static_cast<size_t>(i)].cand.dm_idx, jb}].push_back(i);
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
        float jerk;
        std::memcpy(&jerk, &grp.first.second, 4);
        // the DM-jerk row, re-made
        dd_->run_list({grp.first.first}, rows_.data(), rstride_, stream_);
        resample(rows_.data(), 1, {jerk}, 0, 1, frows.data() + t * rstride_);
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
  std::stable_sort(cands.begin(), cands.end(), [](const JerkCandidate& x, const JerkCandidate& y) {
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

JerkCandidateList jerk_global_distill(JerkCandidateList cands, const JerkCmdLineOptions& args, const JerkSetup& setup) {
  // The distillers move whole candidates: until they are folded, opt_period is
  // unused and carries the index of the wrapper record through them.
  std::vector<float> jerks(cands.size());
  CandidateList plain;
  plain.reserve(cands.size());
  for (size_t i = 0; i < cands.size(); ++i) {
    jerks[i] = cands[i].jerk;
    cands[i].cand.opt_period = static_cast<double>(i);
    plain.push_back(std::move(cands[i].cand));
  }
  stable_sort_by_dm_idx(plain);
  plain = global_distill_and_score(std::move(plain), args.search, setup.search);
  JerkCandidateList out;
  out.reserve(plain.size());
  for (Candidate& c : plain) {
    const size_t i = static_cast<size_t>(c.opt_period);
    PSOUP_CHECK(i < jerks.size(), "jerk: a candidate lost its record");
    clear_tags(c);
    out.push_back(JerkCandidate{std::move(c), jerks[i]});
  }
  return out;
}

// ------------------------------------------------------------- pipeline ----
JerkRun run_jerk_pipeline(const JerkCmdLineOptions& args) {
  JerkRun run;
  Stopwatch t_total, t_read, t_search, t_fold;
  t_total.start();
  if (args.search.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.search.infilename);
  t_read.stop();
  run.setup = make_jerk_setup(args, fb.header());  // every refusal, before any device work
  const JerkSetup& setup = run.setup;
  PSOUP_CHECK(fb.nsamps() * fb.bytes_per_sample() <= fb.data_bytes(), "jerksearch: truncated filterbank");
  log_verbose("jerksearch: " + std::to_string(setup.search.dm_list.size()) + " DM trials, " +
              std::to_string(setup.total_trials) + " DM-jerk trials, span " + std::to_string(setup.span));
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  t_search.start();
  Stream stream;
  const DedispGeometry geom =
      DedispGeometry::make(fb.header(), fb.nsamps(), setup.search.dm_list, setup.search.killmask);
  DeviceFilterbank dfb(geom, stream.get());
  dfb.load_packed_host(fb.data());
  JerkSearcher js(setup, dfb, stream.get());
  JerkCandidateList cands = js.search();
  cands = jerk_global_distill(std::move(cands), args, setup);
  t_search.stop();
  t_fold.start();
  js.fold(cands, args.search.npdmp);
  t_fold.stop();
  cands.resize(std::min(static_cast<size_t>(std::max(args.search.limit, 0)), cands.size()));
  run.candidates = std::move(cands);
  run.accel_trials = js.accel_trials();
  run.jerk_trials = js.jerk_trials();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["searching"] = t_search.get_time();
  run.timers["folding"] = t_fold.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

void write_jerk_output(const JerkCmdLineOptions& args, const JerkSetup& setup, const JerkCandidateList& cands) {
  const std::string tmp = args.outfilename + ".tmp";
  {
    std::ofstream out(tmp);
    PSOUP_CHECK(static_cast<bool>(out), "cannot open output " << tmp);
    out << jerk_output_text(args, setup, cands);
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
