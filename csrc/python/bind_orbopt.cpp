// pybind11 bindings of orbopt (orbopt.hpp): options, the host steps (no GPU
// needed), both kernels over raw device addresses, OrbitOptimiser over a
// resident filterbank, the pipeline and the writer.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/orbopt.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using U8 = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using I64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using Triple = std::tuple<uint64_t, uint64_t, int64_t>;                    // (W, F, Aq)
using Orbit = std::tuple<double, double, double>;                          // (pb, a1, ph)
using Cand = std::tuple<double, float, float, double, double, double>;     // (period, dm, acc, pb, a1, ph)

template <class T>
py::array_t<T> arr(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  PSOUP_CHECK(static_cast<size_t>(a.size()) == v.size(), "orbopt: array shape mismatch");
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

template <class A>
auto vec(const A& a) {
  using T = typename std::remove_const<typename std::remove_pointer<decltype(a.data())>::type>::type;
  return std::vector<T>(a.data(), a.data() + a.size());
}

OrbOptCandidate cand_of(const Cand& c) {
  OrbOptCandidate o;
  o.period = std::get<0>(c);
  o.dm = std::get<1>(c);
  o.acc = std::get<2>(c);
  o.pb = std::get<3>(c);
  o.a1 = std::get<4>(c);
  o.ph = std::get<5>(c);
  return o;
}

Cand tuple_of(const OrbOptCandidate& c) { return Cand(c.period, c.dm, c.acc, c.pb, c.a1, c.ph); }

std::vector<OrbitQuant> quants(const std::vector<Triple>& q) {
  PSOUP_CHECK(!q.empty() && q.size() <= static_cast<size_t>(kern::kOoptMaxTemplates),
              "orbopt_fold: 1.." << kern::kOoptMaxTemplates << " templates per launch");
  std::vector<OrbitQuant> out;
  for (const Triple& t : q) {
    out.push_back(OrbitQuant{std::get<0>(t), std::get<1>(t), std::get<2>(t)});
    orbit_check_quant(out.back());
  }
  return out;
}

py::dict grid_to_dict(const OrbOptGrid& g) {
  py::dict d;
  d["npb"] = g.npb;
  d["na1"] = g.na1;
  d["nphase"] = g.nphase;
  d["dpb"] = g.dpb;
  d["da1"] = g.da1;
  d["dph"] = g.dph;
  d["G"] = g.G;
  std::vector<Orbit> t;
  std::vector<Triple> q;
  for (const OrbitTemplate& x : g.tmpl) t.emplace_back(x.pb, x.a1, x.ph);
  for (const OrbitQuant& x : g.quant) q.emplace_back(x.W, x.F, x.Aq);
  d["templates"] = t;
  d["quant"] = q;
  return d;
}

py::dict search_to_dict(const OrbOptSearch& s, int nw, int K) {
  py::dict d;
  d["best_val"] = arr(s.best_val, {nw});
  d["best_idx"] = arr(s.best_idx, {nw});
  d["centre"] = arr(s.centre, {nw});
  d["tcurve"] = arr(s.tcurve, {nw, K});
  d["msum"] = arr(s.msum, {K});
  return d;
}

OrbOptSearch search_of(const py::dict& d) {
  OrbOptSearch s;
  s.best_val = vec(d["best_val"].cast<I32>());
  s.best_idx = vec(d["best_idx"].cast<I32>());
  s.centre = vec(d["centre"].cast<I32>());
  s.tcurve = vec(d["tcurve"].cast<I32>());
  s.msum = vec(d["msum"].cast<I64>());
  return s;
}

py::dict result_to_dict(const OrbOptResult& r, int nints, int nbins) {
  const int nw = static_cast<int>(r.search.best_val.size());
  const int K = r.npb * r.na1 * r.nphase;
  py::dict d = search_to_dict(r.search, nw, K);
  d["period"] = r.cand.period;
  d["dm"] = r.cand.dm;
  d["acc"] = r.cand.acc;
  d["pb"] = r.cand.pb;
  d["a1"] = r.cand.a1;
  d["phase"] = r.cand.ph;
  d["npb"] = r.npb;
  d["na1"] = r.na1;
  d["nphase"] = r.nphase;
  d["dpb"] = r.dpb;
  d["da1"] = r.da1;
  d["dph"] = r.dph;
  d["snr"] = r.snr;
  d["snr_in"] = r.snr_in;
  d["opt_period"] = r.opt_period;
  d["opt_pb"] = r.opt_pb;
  d["opt_a1"] = r.opt_a1;
  d["opt_phase"] = r.opt_phase;
  d["opt_width"] = r.opt_width;
  d["opt_bin"] = r.opt_bin;
  d["opt_k"] = r.opt_k;
  d["opt_l"] = r.opt_l;
  d["flags"] = r.flags;
  d["m"] = r.m;
  d["v1"] = r.v1;
  d["hits"] = arr(r.hits, {nints, nbins});
  d["fold"] = arr(r.fold, {nints, nbins});
  d["profile"] = arr(r.profile, {nbins});
  return d;
}

OrbOptResult result_of(const py::dict& d) {
  OrbOptResult r;
  r.search = search_of(d);
  r.cand.period = d["period"].cast<double>();
  r.cand.dm = d["dm"].cast<float>();
  r.cand.acc = d["acc"].cast<float>();
  r.cand.pb = d["pb"].cast<double>();
  r.cand.a1 = d["a1"].cast<double>();
  r.cand.ph = d["phase"].cast<double>();
  r.npb = d["npb"].cast<int>();
  r.na1 = d["na1"].cast<int>();
  r.nphase = d["nphase"].cast<int>();
  r.dpb = d["dpb"].cast<double>();
  r.da1 = d["da1"].cast<double>();
  r.dph = d["dph"].cast<double>();
  r.snr = d["snr"].cast<double>();
  r.snr_in = d["snr_in"].cast<double>();
  r.opt_period = d["opt_period"].cast<double>();
  r.opt_pb = d["opt_pb"].cast<double>();
  r.opt_a1 = d["opt_a1"].cast<double>();
  r.opt_phase = d["opt_phase"].cast<double>();
  r.opt_width = d["opt_width"].cast<uint32_t>();
  r.opt_bin = d["opt_bin"].cast<uint32_t>();
  r.opt_k = d["opt_k"].cast<uint32_t>();
  r.opt_l = d["opt_l"].cast<uint32_t>();
  r.flags = d["flags"].cast<uint32_t>();
  r.m = d["m"].cast<int64_t>();
  r.v1 = d["v1"].cast<int64_t>();
  r.hits = vec(d["hits"].cast<I32>());
  r.fold = vec(d["fold"].cast<I32>());
  r.profile = vec(d["profile"].cast<I32>());
  return r;
}

OrbOptFileHeader header_of(const py::dict& h, size_t ncand) {
  OrbOptFileHeader o;
  o.ncand = static_cast<uint32_t>(ncand);
  o.nints = h["nints"].cast<uint32_t>();
  o.nbins = h["nbins"].cast<uint32_t>();
  o.npb = h["npb"].cast<uint32_t>();
  o.na1 = h["na1"].cast<uint32_t>();
  o.nphase = h["nphase"].cast<uint32_t>();
  o.np = h["np"].cast<uint32_t>();
  o.nw = h["nw"].cast<uint32_t>();
  o.n = h["n"].cast<uint64_t>();
  o.tsamp = h["tsamp"].cast<double>();
  o.p_step = h["p_step"].cast<double>();
  return o;
}

py::dict header_to_dict(const OrbOptFileHeader& h) {
  py::dict d;
  d["ncand"] = h.ncand;
  d["nints"] = h.nints;
  d["nbins"] = h.nbins;
  d["npb"] = h.npb;
  d["na1"] = h.na1;
  d["nphase"] = h.nphase;
  d["np"] = h.np;
  d["nw"] = h.nw;
  d["n"] = h.n;
  d["tsamp"] = h.tsamp;
  d["p_step"] = h.p_step;
  return d;
}

}  // namespace

void bind_orbopt(py::module_& m) {
  py::class_<OrbOptCmdLineOptions>(m, "OrbOptCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &OrbOptCmdLineOptions::infilename)
      .def_readwrite("candfilename", &OrbOptCmdLineOptions::candfilename)
      .def_readwrite("outfilename", &OrbOptCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &OrbOptCmdLineOptions::killfilename)
      .def_readwrite("size", &OrbOptCmdLineOptions::size)
      .def_readwrite("max_num_threads", &OrbOptCmdLineOptions::max_num_threads)
      .def_readwrite("nbins", &OrbOptCmdLineOptions::nbins)
      .def_readwrite("nints", &OrbOptCmdLineOptions::nints)
      .def_readwrite("npb", &OrbOptCmdLineOptions::npb)
      .def_readwrite("na1", &OrbOptCmdLineOptions::na1)
      .def_readwrite("nphase", &OrbOptCmdLineOptions::nphase)
      .def_readwrite("pb_step", &OrbOptCmdLineOptions::pb_step)
      .def_readwrite("a1_step", &OrbOptCmdLineOptions::a1_step)
      .def_readwrite("phase_step", &OrbOptCmdLineOptions::phase_step)
      .def_readwrite("np", &OrbOptCmdLineOptions::np)
      .def_readwrite("p_step", &OrbOptCmdLineOptions::p_step)
      .def_readwrite("limit", &OrbOptCmdLineOptions::limit)
      .def_readwrite("verbose", &OrbOptCmdLineOptions::verbose);
  m.def("parse_oopt_cmdline", [](const std::vector<std::string>& argv) {
    OrbOptCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_oopt_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.attr("OOPT_TILE") = kern::kOoptTile;
  m.attr("OOPT_LANE") = kern::kOoptLane;
  m.attr("OOPT_TILES_PER_GROUP") = kern::kOoptTilesPerGroup;
  m.attr("OOPT_MAX_TEMPLATES") = kern::kOoptMaxTemplates;
  m.def("oopt_nwidths", &kern::oopt_nwidths);

  py::class_<OrbOptParams>(m, "OrbOptParams")
      .def(py::init([](int nbins, int nints, int npb, int na1, int nphase, int np, double p_step, double pb_step,
                       double a1_step, double phase_step) {
             OrbOptParams p;
             p.nbins = nbins;
             p.nints = nints;
             p.npb = npb;
             p.na1 = na1;
             p.nphase = nphase;
             p.np = np;
             p.p_step = p_step;
             p.pb_step = pb_step;
             p.a1_step = a1_step;
             p.phase_step = phase_step;
             return p;
           }),
           py::arg("nbins") = 64, py::arg("nints") = 16, py::arg("npb") = 9, py::arg("na1") = 9, py::arg("nphase") = 9,
           py::arg("np") = 33, py::arg("p_step") = 1.0, py::arg("pb_step") = 0.0, py::arg("a1_step") = 0.0,
           py::arg("phase_step") = 0.0)
      .def_readwrite("nbins", &OrbOptParams::nbins)
      .def_readwrite("nints", &OrbOptParams::nints)
      .def_readwrite("npb", &OrbOptParams::npb)
      .def_readwrite("na1", &OrbOptParams::na1)
      .def_readwrite("nphase", &OrbOptParams::nphase)
      .def_readwrite("np", &OrbOptParams::np)
      .def_readwrite("p_step", &OrbOptParams::p_step)
      .def_readwrite("pb_step", &OrbOptParams::pb_step)
      .def_readwrite("a1_step", &OrbOptParams::a1_step)
      .def_readwrite("phase_step", &OrbOptParams::phase_step);
  m.def("oopt_params_of", &oopt_params_of);

  // ---- the host steps (no GPU)
  m.def("oopt_check_params", &oopt_check_params);
  m.def(
      "oopt_grid",
      [](size_t k, const OrbOptParams& p, const Cand& c, uint64_t n, float tsamp) {
        return grid_to_dict(oopt_grid(k, p, cand_of(c), n, tsamp));
      },
      py::arg("k"), py::arg("params"), py::arg("cand"), py::arg("n"), py::arg("tsamp"));
  m.def(
      "oopt_hits",
      [](uint64_t G, uint64_t n, int nints, int nbins) {
        PSOUP_CHECK(n >= 1 && n <= kOrbitMaxSpan && nints >= 1 && nints <= kern::kOoptMaxInts && nbins >= 2 &&
                        nbins <= kern::kOoptMaxBins,
                    "oopt_hits: bad shape");
        return arr(oopt_hits(G, n, nints, nbins), {nints, nbins});
      },
      py::arg("G"), py::arg("n"), py::arg("nints"), py::arg("nbins"));
  m.def(
      "oopt_moments",
      [](size_t k, const U8& x, uint64_t n) {
        PSOUP_CHECK(x.ndim() == 1 && n >= 1 && static_cast<uint64_t>(x.shape(0)) >= n, "oopt_moments: x shorter than n");
        const OrbOptMoments mo = oopt_moments(k, x.data(), n);
        return py::make_tuple(mo.m, mo.v1);
      },
      py::arg("k"), py::arg("x"), py::arg("n"));
  m.def("oopt_drift_table", [](const OrbOptParams& p) { return arr(oopt_drift_table(p), {p.np, p.nints}); });
  m.def(
      "orbopt_fold_host",
      [](const U8& x, uint64_t n, uint64_t G, const std::vector<Triple>& q, int nints, int nbins) {
        PSOUP_CHECK(x.ndim() == 1 && n >= 1 && static_cast<uint64_t>(x.shape(0)) >= n,
                    "orbopt_fold_host: x shorter than n");
        const std::vector<OrbitQuant> t = quants(q);
        return arr(orbopt_fold_host(x.data(), n, G, t, nints, nbins),
                   {static_cast<py::ssize_t>(t.size()), nints, nbins});
      },
      py::arg("x"), py::arg("n"), py::arg("G"), py::arg("q"), py::arg("nints"), py::arg("nbins"));
  m.def(
      "orbopt_search_host",
      [](const I32& fold, const I32& hits, int32_t mm, const I32& st) {
        PSOUP_CHECK(fold.ndim() == 3 && hits.ndim() == 2 && st.ndim() == 2, "orbopt_search_host: fold [K, nints, "
                    "nbins], hits [nints, nbins], st [np, nints]");
        const int K = static_cast<int>(fold.shape(0)), nints = static_cast<int>(fold.shape(1)),
                  nbins = static_cast<int>(fold.shape(2)), np = static_cast<int>(st.shape(0));
        PSOUP_CHECK(hits.shape(0) == nints && hits.shape(1) == nbins && st.shape(1) == nints && nbins >= 2 &&
                        nbins <= kern::kOoptMaxBins && K >= 1 && np >= 1,
                    "orbopt_search_host: array shapes");
        return search_to_dict(orbopt_search_host(fold.data(), hits.data(), mm, st.data(), K, nints, nbins, np),
                              kern::oopt_nwidths(nbins), K);
      },
      py::arg("fold"), py::arg("hits"), py::arg("m"), py::arg("st"));
  m.def(
      "oopt_finish",
      [](const OrbOptParams& p, const Cand& c, uint64_t n, float tsamp, int64_t mm, int64_t v1, const I32& hits,
         const py::dict& found, const I32& fold_opt) {
        const OrbOptGrid g = oopt_grid(0, p, cand_of(c), n, tsamp);
        OrbOptMoments mo;
        mo.m = mm;
        mo.v1 = v1;
        PSOUP_CHECK(static_cast<size_t>(fold_opt.size()) == static_cast<size_t>(p.nints) * p.nbins,
                    "oopt_finish: fold_opt must be [nints, nbins]");
        return result_to_dict(
            oopt_finish(p, cand_of(c), g, n, tsamp, mo, vec(hits), oopt_drift_table(p), search_of(found), fold_opt.data()),
            p.nints, p.nbins);
      },
      py::arg("params"), py::arg("cand"), py::arg("n"), py::arg("tsamp"), py::arg("m"), py::arg("v1"), py::arg("hits"),
      py::arg("found"), py::arg("fold_opt"));
  m.def("oopt_parse_candidates", [](const std::string& text) {
    std::vector<Cand> out;
    for (const OrbOptCandidate& c : oopt_parse_candidates(text)) out.push_back(tuple_of(c));
    return out;
  });
  m.def("oopt_dm_list", [](const std::vector<Cand>& cands) {
    std::vector<OrbOptCandidate> c;
    for (const Cand& t : cands) c.push_back(cand_of(t));
    return oopt_dm_list(c);
  });

  // ---- the kernels alone: device addresses.  q are the quantised templates [ncand * K] on the host (checked here),
  // q_dev the same records {uint64 W, uint64 F, int64 Aq}, row_of int32 [ncand] and G uint64 [ncand] on the host
  // (row_of checked here) and on the device, table_dev the 4097 int32 of the sine table; the caller keeps them alive
  // until the stream has run the kernel
  m.def(
      "orbopt_fold_raw",
      [](uintptr_t rows, uint64_t row_stride, uint64_t in_bytes, const std::vector<int32_t>& row_of, uintptr_t row_of_dev,
         uintptr_t G_dev, const std::vector<Triple>& q, uintptr_t q_dev, int K, uint64_t n, int nints, int nbins,
         uintptr_t table_dev, uintptr_t fold, uintptr_t s) {
        PSOUP_CHECK(K >= 1 && !row_of.empty() && q.size() == row_of.size() * static_cast<size_t>(K),
                    "orbopt_fold: q must hold ncand * K templates");
        for (const Triple& t : q) orbit_check_quant(OrbitQuant{std::get<0>(t), std::get<1>(t), std::get<2>(t)});
        for (int32_t r : row_of)
          PSOUP_CHECK(r >= 0 && static_cast<uint64_t>(r) * row_stride + n <= in_bytes,
                      "orbopt_fold: a row lies outside the input");
        PSOUP_CHECK(q_dev != 0 && q_dev % 8 == 0 && G_dev != 0 && G_dev % 8 == 0 && row_of_dev != 0 &&
                        row_of_dev % 4 == 0 && table_dev != 0 && table_dev % 4 == 0 && fold != 0 && fold % 4 == 0,
                    "orbopt_fold: a device array is missing or misaligned");
        kern::orbopt_fold(reinterpret_cast<const uint8_t*>(rows), row_stride, in_bytes,
                          reinterpret_cast<const int32_t*>(row_of_dev), reinterpret_cast<const uint64_t*>(G_dev),
                          reinterpret_cast<const OrbitQuant*>(q_dev), static_cast<int>(row_of.size()), K, n, nints, nbins,
                          reinterpret_cast<const int32_t*>(table_dev), reinterpret_cast<int32_t*>(fold),
                          reinterpret_cast<hipStream_t>(s));
      },
      py::arg("rows"), py::arg("row_stride"), py::arg("in_bytes"), py::arg("row_of"), py::arg("row_of_dev"),
      py::arg("G_dev"), py::arg("q"), py::arg("q_dev"), py::arg("K"), py::arg("n"), py::arg("nints"), py::arg("nbins"),
      py::arg("table_dev"), py::arg("fold"), py::arg("stream") = 0);
  // st: the drift table [np][nints] on the host (checked here), st_dev the same on the device
  m.def(
      "orbopt_search_raw",
      [](uintptr_t fold, uintptr_t hits, uintptr_t mm, const std::vector<int32_t>& st, uintptr_t st_dev, int ncand, int K,
         int nints, int nbins, int np, uintptr_t keys, uintptr_t best_val, uintptr_t best_idx, uintptr_t tcurve,
         uintptr_t centre, uintptr_t msum, uintptr_t s) {
        PSOUP_CHECK(np >= 1 && nints >= 1 && st.size() == static_cast<size_t>(np) * nints,
                    "orbopt_search: st must be [np, nints]");
        for (int32_t v : st) PSOUP_CHECK(v >= 0 && v < nbins, "orbopt_search: a drift shift outside [0, nbins)");
        PSOUP_CHECK(keys % 8 == 0 && msum % 8 == 0, "orbopt_search: keys and msum must be 8-byte aligned");
        kern::orbopt_search(reinterpret_cast<const int32_t*>(fold), reinterpret_cast<const int32_t*>(hits),
                            reinterpret_cast<const int32_t*>(mm), reinterpret_cast<const int32_t*>(st_dev), ncand, K,
                            nints, nbins, np, reinterpret_cast<uint64_t*>(keys), reinterpret_cast<int32_t*>(best_val),
                            reinterpret_cast<int32_t*>(best_idx), reinterpret_cast<int32_t*>(tcurve),
                            reinterpret_cast<int32_t*>(centre), reinterpret_cast<int64_t*>(msum),
                            reinterpret_cast<hipStream_t>(s));
      },
      py::arg("fold"), py::arg("hits"), py::arg("m"), py::arg("st"), py::arg("st_dev"), py::arg("ncand"), py::arg("K"),
      py::arg("nints"), py::arg("nbins"), py::arg("np"), py::arg("keys"), py::arg("best_val"), py::arg("best_idx"),
      py::arg("tcurve"), py::arg("centre"), py::arg("msum"), py::arg("stream") = 0);

  // ---- OrbitOptimiser over a resident filterbank
  py::class_<OrbitOptimiser>(m, "OrbitOptimiser")
      .def(py::init([](const OrbOptParams& p, const DeviceFilterbank& fb, uint64_t fft_size, uintptr_t s,
                       size_t batch_bytes) {
             return new OrbitOptimiser(p, fb, fft_size, reinterpret_cast<hipStream_t>(s), batch_bytes);
           }),
           py::arg("params"), py::arg("filterbank"), py::arg("fft_size"), py::arg("stream") = 0,
           py::arg("batch_bytes") = OrbitOptimiser::kDefaultBatchBytes, py::keep_alive<1, 3>())
      .def("optimise",
           [](OrbitOptimiser& o, const std::vector<Cand>& cands) {
             std::vector<OrbOptCandidate> in;
             for (const Cand& c : cands) in.push_back(cand_of(c));
             std::vector<OrbOptResult> res;
             {
               py::gil_scoped_release nogil;
               res = o.optimise(in);
             }
             py::list out;
             for (const OrbOptResult& r : res) out.append(result_to_dict(r, o.params().nints, o.params().nbins));
             return out;
           },
           py::arg("candidates"))
      .def("row",
           [](OrbitOptimiser& o, int d) {
             const std::vector<uint8_t> r = o.row(d);
             return arr(r, {static_cast<py::ssize_t>(r.size())});
           })
      .def_property_readonly("span", &OrbitOptimiser::span)
      .def_property_readonly("nrow", &OrbitOptimiser::nrow)
      .def_property_readonly("tsamp", &OrbitOptimiser::tsamp)
      .def_property_readonly("batches", &OrbitOptimiser::batches)
      .def_property_readonly("nwidths", &OrbitOptimiser::nwidths);

  // ---- the pipeline and the writer
  py::class_<OrbOptRun>(m, "OrbOptRun")
      .def_readonly("timers", &OrbOptRun::timers)
      .def_property_readonly("header", [](const OrbOptRun& r) { return header_to_dict(r.header); })
      .def_property_readonly("ncand", [](const OrbOptRun& r) { return r.results.size(); })
      .def("result", [](const OrbOptRun& r, size_t i) {
        PSOUP_CHECK(i < r.results.size(), "OrbOptRun.result: index out of range");
        return result_to_dict(r.results[i], static_cast<int>(r.header.nints), static_cast<int>(r.header.nbins));
      });
  m.def("run_orbopt_pipeline", [](const OrbOptCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_orbopt_pipeline(a);
  });
  m.def(
      "write_orbopt_file",
      [](const std::string& path, const py::dict& header, const std::vector<py::dict>& records) {
        std::vector<OrbOptResult> results;
        for (const py::dict& d : records) results.push_back(result_of(d));
        write_orbopt_file(path, header_of(header, records.size()), results);
      },
      py::arg("path"), py::arg("header"), py::arg("records"));
  m.def("oopt_verbose_line", [](const py::dict& d) { return oopt_verbose_line(result_of(d)); });
}
