// pybind11 bindings of cubeopt (cubeopt.hpp): options, grid, the host steps
// (which need no GPU), CubeOptimiser, pipeline, reader and writer.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/cubeopt.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using I64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using F32 = py::array_t<float, py::array::c_style | py::array::forcecast>;

template <class T>
py::array_t<T> arr(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  PSOUP_CHECK(static_cast<size_t>(a.size()) == v.size(), "cube opt: array shape mismatch");
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

template <class A>
auto vec(const A& a) {
  using T = typename std::remove_const<typename std::remove_pointer<decltype(a.data())>::type>::type;
  return std::vector<T>(a.data(), a.data() + a.size());
}

CubeOptInput input_of(double period, float dm, float acc, const I32& nactive, const I32& hits, const I64& sums) {
  CubeOptInput in;
  in.period = period;
  in.dm = dm;
  in.acc = acc;
  in.nactive = vec(nactive);
  in.hits = vec(hits);
  in.sums = vec(sums);
  return in;
}

py::dict search_to_dict(const CubeOptSearch& s, int nw, const CubeOptGrid& g) {
  py::dict d;
  d["best_val"] = arr(s.best_val, {nw});
  d["best_idx"] = arr(s.best_idx, {nw});
  d["dmcurve"] = arr(s.dmcurve, {nw, g.ndm});
  d["ppd"] = arr(s.ppd, {nw, g.np, g.npd});
  d["centre"] = arr(s.centre, {nw});
  return d;
}

CubeOptSearch search_of(const py::dict& d) {
  CubeOptSearch s;
  s.best_val = vec(d["best_val"].cast<I32>());
  s.best_idx = vec(d["best_idx"].cast<I32>());
  s.dmcurve = vec(d["dmcurve"].cast<I32>());
  s.ppd = vec(d["ppd"].cast<I32>());
  s.centre = vec(d["centre"].cast<I32>());
  return s;
}

py::dict result_to_dict(const CubeOptResult& r, const CubeOptGrid& g, int nbins) {
  const int nw = static_cast<int>(r.search.best_val.size());
  py::dict d = search_to_dict(r.search, nw, g);
  d["snr"] = r.snr;
  d["snr_in"] = r.snr_in;
  d["snr_dm0"] = r.snr_dm0;
  d["opt_period"] = r.opt_period;
  d["opt_acc"] = r.opt_acc;
  d["opt_dm"] = r.opt_dm;
  d["opt_width"] = r.opt_width;
  d["opt_bin"] = r.opt_bin;
  d["opt_kd"] = r.opt_kd;
  d["opt_kp"] = r.opt_kp;
  d["opt_kpd"] = r.opt_kpd;
  d["flags"] = r.flags;
  d["mtot"] = r.mtot;
  d["v"] = r.v;
  d["dms"] = arr(r.dms, {g.ndm});
  d["profile"] = arr(r.profile, {nbins});
  return d;
}

CubeOptResult result_of(const py::dict& d) {
  CubeOptResult r;
  r.search = search_of(d);
  r.snr = d["snr"].cast<double>();
  r.snr_in = d["snr_in"].cast<double>();
  r.snr_dm0 = d["snr_dm0"].cast<double>();
  r.opt_period = d["opt_period"].cast<double>();
  r.opt_acc = d["opt_acc"].cast<double>();
  r.opt_dm = d["opt_dm"].cast<float>();
  r.opt_width = d["opt_width"].cast<uint32_t>();
  r.opt_bin = d["opt_bin"].cast<uint32_t>();
  r.opt_kd = d["opt_kd"].cast<uint32_t>();
  r.opt_kp = d["opt_kp"].cast<uint32_t>();
  r.opt_kpd = d["opt_kpd"].cast<uint32_t>();
  r.flags = d["flags"].cast<uint32_t>();
  r.mtot = d["mtot"].cast<int64_t>();
  r.v = d["v"].cast<double>();
  r.dms = vec(d["dms"].cast<F32>());
  r.profile = vec(d["profile"].cast<I32>());
  return r;
}

}  // namespace

void bind_opt(py::module_& m) {
  py::class_<CubeOptCmdLineOptions>(m, "CubeOptCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &CubeOptCmdLineOptions::infilename)
      .def_readwrite("outfilename", &CubeOptCmdLineOptions::outfilename)
      .def_readwrite("ndm", &CubeOptCmdLineOptions::ndm)
      .def_readwrite("dm_half_range", &CubeOptCmdLineOptions::dm_half_range)
      .def_readwrite("np", &CubeOptCmdLineOptions::np)
      .def_readwrite("p_step", &CubeOptCmdLineOptions::p_step)
      .def_readwrite("npd", &CubeOptCmdLineOptions::npd)
      .def_readwrite("pd_step", &CubeOptCmdLineOptions::pd_step)
      .def_readwrite("limit", &CubeOptCmdLineOptions::limit)
      .def_readwrite("verbose", &CubeOptCmdLineOptions::verbose);
  m.def("parse_opt_cmdline", [](const std::vector<std::string>& argv) {
    CubeOptCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_opt_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("default_opt_output_filename", &default_opt_output_filename);
  m.def("opt_nwidths", &kern::opt_nwidths);

  py::class_<CubeOptGrid>(m, "CubeOptGrid")
      .def(py::init([](int ndm, float dm_half_range, int np, double p_step, int npd, double pd_step) {
             CubeOptGrid g;
             g.ndm = ndm;
             g.dm_half_range = dm_half_range;
             g.np = np;
             g.p_step = p_step;
             g.npd = npd;
             g.pd_step = pd_step;
             return g;
           }),
           py::arg("ndm") = 64, py::arg("dm_half_range") = 0.f, py::arg("np") = 65, py::arg("p_step") = 1.0,
           py::arg("npd") = 33, py::arg("pd_step") = 1.0)
      .def_readwrite("ndm", &CubeOptGrid::ndm)
      .def_readwrite("dm_half_range", &CubeOptGrid::dm_half_range)
      .def_readwrite("np", &CubeOptGrid::np)
      .def_readwrite("p_step", &CubeOptGrid::p_step)
      .def_readwrite("npd", &CubeOptGrid::npd)
      .def_readwrite("pd_step", &CubeOptGrid::pd_step);

  py::class_<CubeOptGeom>(m, "CubeOptGeom")
      .def(py::init([](int nints, int nsub, int nbins, int nchans, uint64_t fold_nsamps, double tsamp, double fch1,
                       double foff) {
             CubeOptGeom g;
             g.nints = nints;
             g.nsub = nsub;
             g.nbins = nbins;
             g.nchans = nchans;
             g.fold_nsamps = fold_nsamps;
             g.tsamp = tsamp;
             g.fch1 = fch1;
             g.foff = foff;
             return g;
           }),
           py::arg("nints"), py::arg("nsub"), py::arg("nbins"), py::arg("nchans") = 1, py::arg("fold_nsamps") = 1,
           py::arg("tsamp") = 1.0, py::arg("fch1") = 0.0, py::arg("foff") = 0.0)
      .def_readwrite("nints", &CubeOptGeom::nints)
      .def_readwrite("nsub", &CubeOptGeom::nsub)
      .def_readwrite("nbins", &CubeOptGeom::nbins)
      .def_readwrite("nchans", &CubeOptGeom::nchans)
      .def_readwrite("fold_nsamps", &CubeOptGeom::fold_nsamps)
      .def_readwrite("tsamp", &CubeOptGeom::tsamp)
      .def_readwrite("fch1", &CubeOptGeom::fch1)
      .def_readwrite("foff", &CubeOptGeom::foff);

  // ---- the host steps: no GPU
  m.def(
      "cube_opt_prepare",
      [](size_t k, const CubeOptGeom& g, const CubeOptGrid& grid, double period, float dm, float acc,
         const I32& nactive, const I32& hits, const I64& sums) {
        const CubeOptPrepared p = cube_opt_prepare(k, g, grid, input_of(period, dm, acc, nactive, hits, sums));
        py::dict d;
        d["d"] = arr(p.d, {g.nints, g.nsub, g.nbins});
        d["mtot"] = p.mtot;
        d["v2"] = p.v2;
        d["v"] = p.v;
        return d;
      },
      py::arg("k"), py::arg("geom"), py::arg("grid"), py::arg("period"), py::arg("dm"), py::arg("acc"),
      py::arg("nactive"), py::arg("hits"), py::arg("sums"));
  m.def(
      "cube_opt_shifts",
      [](const CubeOptGeom& g, const CubeOptGrid& grid, double period, float dm, const std::vector<float>& delays) {
        const CubeOptShifts s = cube_opt_shifts(g, grid, period, dm, delays);
        py::dict d;
        d["dms"] = arr(s.dms, {grid.ndm});
        d["sdm"] = arr(s.sdm, {grid.ndm, g.nsub});
        d["st"] = arr(s.st, {grid.np, grid.npd, g.nints});
        return d;
      },
      py::arg("geom"), py::arg("grid"), py::arg("period"), py::arg("dm"), py::arg("delays"));
  m.def(
      "cube_opt_search_host",
      [](const CubeOptGeom& g, const CubeOptGrid& grid, const I32& d, const I32& sdm, const I32& st) {
        CubeOptShifts sh;
        sh.sdm = vec(sdm);
        sh.st = vec(st);
        PSOUP_CHECK(sh.sdm.size() == static_cast<size_t>(grid.ndm) * g.nsub &&
                        sh.st.size() == static_cast<size_t>(grid.np) * grid.npd * g.nints,
                    "cube_opt_search_host: table shapes");
        for (int32_t v : sh.sdm) PSOUP_CHECK(v >= 0 && v < g.nbins, "cube_opt_search_host: shift outside [0, nbins)");
        for (int32_t v : sh.st) PSOUP_CHECK(v >= 0 && v < g.nbins, "cube_opt_search_host: shift outside [0, nbins)");
        return search_to_dict(cube_opt_search_host(g, grid, vec(d), sh), kern::opt_nwidths(g.nbins), grid);
      },
      py::arg("geom"), py::arg("grid"), py::arg("d"), py::arg("sdm"), py::arg("st"));
  m.def(
      "cube_opt_finish",
      [](const CubeOptGeom& g, const CubeOptGrid& grid, double period, float acc, const I32& d, int64_t mtot,
         int64_t v2, const F32& dms, const I32& sdm, const I32& st, const py::dict& found) {
        CubeOptPrepared p;
        p.d = vec(d);
        p.mtot = mtot;
        p.v2 = v2;
        p.v = static_cast<double>(v2) / static_cast<double>(g.nbins);
        CubeOptShifts sh;
        sh.dms = vec(dms);
        sh.sdm = vec(sdm);
        sh.st = vec(st);
        PSOUP_CHECK(p.d.size() == static_cast<size_t>(g.nints) * g.nsub * g.nbins &&
                        sh.dms.size() == static_cast<size_t>(grid.ndm) &&
                        sh.sdm.size() == static_cast<size_t>(grid.ndm) * g.nsub &&
                        sh.st.size() == static_cast<size_t>(grid.np) * grid.npd * g.nints,
                    "cube_opt_finish: array shapes");
        for (int32_t v : sh.sdm) PSOUP_CHECK(v >= 0 && v < g.nbins, "cube_opt_finish: shift outside [0, nbins)");
        for (int32_t v : sh.st) PSOUP_CHECK(v >= 0 && v < g.nbins, "cube_opt_finish: shift outside [0, nbins)");
        return result_to_dict(cube_opt_finish(g, grid, period, acc, p, sh, search_of(found)), grid, g.nbins);
      },
      py::arg("geom"), py::arg("grid"), py::arg("period"), py::arg("acc"), py::arg("d"), py::arg("mtot"),
      py::arg("v2"), py::arg("dms"), py::arg("sdm"), py::arg("st"), py::arg("found"));

  // ---- the optimiser
  py::class_<CubeOptimiser>(m, "CubeOptimiser")
      .def(py::init([](const CubeOptGeom& g, const CubeOptGrid& grid, uintptr_t stream, size_t batch_bytes) {
             return new CubeOptimiser(g, grid, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("geom"), py::arg("grid"), py::arg("stream") = 0,
           py::arg("batch_bytes") = CubeOptimiser::kDefaultBatchBytes)
      // candidates: list of dict(period, dm, acc, nactive, hits, sums); list of result dicts
      .def("optimise",
           [](CubeOptimiser& o, const std::vector<py::dict>& cands, const std::vector<float>& delays) {
             std::vector<CubeOptInput> in;
             for (const py::dict& c : cands)
               in.push_back(input_of(c["period"].cast<double>(), c["dm"].cast<float>(), c["acc"].cast<float>(),
                                     c["nactive"].cast<I32>(), c["hits"].cast<I32>(), c["sums"].cast<I64>()));
             std::vector<CubeOptResult> res;
             {
               py::gil_scoped_release nogil;
               res = o.optimise(in, delays);
             }
             py::list out;
             for (const CubeOptResult& r : res) out.append(result_to_dict(r, o.grid(), o.geom().nbins));
             return out;
           },
           py::arg("candidates"), py::arg("delays"))
      // d [ncand, nints, nsub, nbins], sdm [ncand, ndm, nsub], st [ncand, np, npd, nints]
      .def("search",
           [](CubeOptimiser& o, const I32& d, const I32& sdm, const I32& st) {
             const CubeOptGeom& g = o.geom();
             const CubeOptGrid& gr = o.grid();
             PSOUP_CHECK(d.ndim() == 4 && sdm.ndim() == 3 && st.ndim() == 4, "cube search: d [ncand, nints, nsub, "
                         "nbins], sdm [ncand, ndm, nsub], st [ncand, np, npd, nints]");
             const py::ssize_t nc = d.shape(0);
             PSOUP_CHECK(d.shape(1) == g.nints && d.shape(2) == g.nsub && d.shape(3) == g.nbins && sdm.shape(0) == nc &&
                             sdm.shape(1) == gr.ndm && sdm.shape(2) == g.nsub && st.shape(0) == nc &&
                             st.shape(1) == gr.np && st.shape(2) == gr.npd && st.shape(3) == g.nints,
                         "cube search: array shapes do not match the geometry and the grid");
             std::vector<CubeOptSearch> res;
             {
               py::gil_scoped_release nogil;
               res = o.search(d.data(), sdm.data(), st.data(), static_cast<size_t>(nc));
             }
             py::list out;
             for (const CubeOptSearch& s : res) out.append(search_to_dict(s, o.nwidths(), gr));
             return out;
           },
           py::arg("d"), py::arg("sdm"), py::arg("st"))
      // device addresses of int32 tensors; shifts already checked to lie in [0, nbins)
      .def("search_device",
           [](CubeOptimiser& o, uintptr_t d, uintptr_t sdm, uintptr_t st, size_t ncand, uintptr_t best_val,
              uintptr_t best_idx, uintptr_t dmcurve, uintptr_t ppd, uintptr_t centre) {
             py::gil_scoped_release nogil;
             o.search_device(reinterpret_cast<const int32_t*>(d), reinterpret_cast<const int32_t*>(sdm),
                             reinterpret_cast<const int32_t*>(st), ncand, reinterpret_cast<int32_t*>(best_val),
                             reinterpret_cast<int32_t*>(best_idx), reinterpret_cast<int32_t*>(dmcurve),
                             reinterpret_cast<int32_t*>(ppd), reinterpret_cast<int32_t*>(centre));
           },
           py::arg("d"), py::arg("sdm"), py::arg("st"), py::arg("ncand"), py::arg("best_val"), py::arg("best_idx"),
           py::arg("dmcurve"), py::arg("ppd"), py::arg("centre"))
      .def_property_readonly("bytes_per_candidate", &CubeOptimiser::bytes_per_candidate)
      .def_property_readonly("batch_size", &CubeOptimiser::batch_size)
      .def_property_readonly("batches", &CubeOptimiser::batches)
      .def_property_readonly("nwidths", &CubeOptimiser::nwidths);

  py::class_<OptFileHeader>(m, "OptFileHeader")
      .def(py::init<>())
      .def_readwrite("ncand", &OptFileHeader::ncand)
      .def_readwrite("nints", &OptFileHeader::nints)
      .def_readwrite("nsub", &OptFileHeader::nsub)
      .def_readwrite("nbins", &OptFileHeader::nbins)
      .def_readwrite("nchans", &OptFileHeader::nchans)
      .def_readwrite("ndm", &OptFileHeader::ndm)
      .def_readwrite("np", &OptFileHeader::np)
      .def_readwrite("npd", &OptFileHeader::npd)
      .def_readwrite("nw", &OptFileHeader::nw)
      .def_readwrite("fold_nsamps", &OptFileHeader::fold_nsamps)
      .def_readwrite("tsamp", &OptFileHeader::tsamp)
      .def_readwrite("fch1", &OptFileHeader::fch1)
      .def_readwrite("foff", &OptFileHeader::foff)
      .def_readwrite("p_step", &OptFileHeader::p_step)
      .def_readwrite("pd_step", &OptFileHeader::pd_step)
      .def_readwrite("dm_half_range", &OptFileHeader::dm_half_range);

  py::class_<CubeOptRun>(m, "CubeOptRun")
      .def_readonly("header", &CubeOptRun::header)
      .def_readonly("timers", &CubeOptRun::timers)
      .def_property_readonly("ncand", [](const CubeOptRun& r) { return r.results.size(); })
      .def("result", [](const CubeOptRun& r, size_t i) {
        PSOUP_CHECK(i < r.results.size(), "CubeOptRun.result: index out of range");
        CubeOptGrid g;
        g.ndm = static_cast<int>(r.header.ndm);
        g.np = static_cast<int>(r.header.np);
        g.npd = static_cast<int>(r.header.npd);
        py::dict d = result_to_dict(r.results[i], g, static_cast<int>(r.header.nbins));
        d["period"] = r.candidates[i].period;
        d["dm"] = r.candidates[i].dm;
        d["acc"] = r.candidates[i].acc;
        return d;
      });
  m.def("run_opt_pipeline", [](const CubeOptCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_opt_pipeline(a);
  });
  // dict(geom, nbits, candidates: list of dict(period, dm, acc, nactive, hits, sums))
  m.def(
      "read_cube_file",
      [](const std::string& path, int limit) {
        const CubeFile f = read_cube_file(path, limit);
        py::list cands;
        for (const CubeOptInput& c : f.candidates) {
          py::dict d;
          d["period"] = c.period;
          d["dm"] = c.dm;
          d["acc"] = c.acc;
          d["nactive"] = arr(c.nactive, {f.geom.nsub});
          d["hits"] = arr(c.hits, {f.geom.nints, f.geom.nbins});
          d["sums"] = arr(c.sums, {f.geom.nints, f.geom.nsub, f.geom.nbins});
          cands.append(d);
        }
        py::dict out;
        out["geom"] = f.geom;
        out["nbits"] = f.nbits;
        out["candidates"] = cands;
        return out;
      },
      py::arg("path"), py::arg("limit") = -1);
  // Native writer over result dicts (tests compare it with the Python one).
  m.def(
      "write_opt_file",
      [](const std::string& path, const OptFileHeader& h, const std::vector<py::dict>& records) {
        std::vector<CubeOptInput> cands(records.size());
        std::vector<CubeOptResult> results;
        for (size_t i = 0; i < records.size(); ++i) {
          cands[i].period = records[i]["period"].cast<double>();
          cands[i].dm = records[i]["dm"].cast<float>();
          cands[i].acc = records[i]["acc"].cast<float>();
          results.push_back(result_of(records[i]));
        }
        write_opt_file(path, h, cands, results);
      },
      py::arg("path"), py::arg("header"), py::arg("records"));
}
