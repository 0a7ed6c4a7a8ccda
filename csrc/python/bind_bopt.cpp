// pybind11 bindings of burstopt (burstopt.hpp): options, grid, the host steps
// (which need no GPU), BurstOptimiser, pipeline, reader and writer.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/burstopt.hpp"
#include "psoup/common.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using I64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using F32 = py::array_t<float, py::array::c_style | py::array::forcecast>;
using F64 = py::array_t<double, py::array::c_style | py::array::forcecast>;

template <class T>
py::array_t<T> arr(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  PSOUP_CHECK(static_cast<size_t>(a.size()) == v.size(), "burst opt: array shape mismatch");
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

template <class A>
auto vec(const A& a) {
  using T = typename std::remove_const<typename std::remove_pointer<decltype(a.data())>::type>::type;
  return std::vector<T>(a.data(), a.data() + a.size());
}

// The scalars of a cutout (BurstCubeFile.candidate's keys); the input's S/N is "snr".
void scalars_of(const py::dict& c, BurstOptInput& in) {
  in.sample = c["sample"].cast<uint64_t>();
  in.width = c["width"].cast<uint32_t>();
  in.tscrunch = c["tscrunch"].cast<uint32_t>();
  in.t0 = c["t0"].cast<int64_t>();
  in.dm = c["dm"].cast<float>();
  in.snr = c.contains("snr") ? c["snr"].cast<float>() : 0.f;
  in.dms = vec(c["dms"].cast<F32>());
}

BurstOptInput input_of(const py::dict& c) {
  BurstOptInput in;
  scalars_of(c, in);
  in.nactive = vec(c["nactive"].cast<I32>());
  in.ds_sums = vec(c["ds_sums"].cast<I32>());
  in.ds_hits = vec(c["ds_hits"].cast<I32>());
  in.dmt_sums = vec(c["dmt_sums"].cast<I32>());
  in.dmt_hits = vec(c["dmt_hits"].cast<I32>());
  return in;
}

py::dict input_to_dict(const BurstOptInput& c, const BurstOptGeom& g) {
  py::dict d;
  d["sample"] = c.sample;
  d["width"] = c.width;
  d["tscrunch"] = c.tscrunch;
  d["t0"] = c.t0;
  d["dm"] = c.dm;
  d["snr"] = c.snr;
  d["dms"] = arr(c.dms, {g.ndm});
  d["nactive"] = arr(c.nactive, {g.nsub});
  d["ds_sums"] = arr(c.ds_sums, {g.nsub, g.ntime});
  d["ds_hits"] = arr(c.ds_hits, {g.nsub, g.ntime});
  d["dmt_sums"] = arr(c.dmt_sums, {g.ndm, g.ntime});
  d["dmt_hits"] = arr(c.dmt_hits, {g.ndm, g.ntime});
  return d;
}

py::dict prepared_to_dict(const BurstOptPrepared& p, const BurstOptGeom& g) {
  py::dict d;
  d["d_ds"] = arr(p.d_ds, {g.nsub, g.ntime});
  d["d_dmt"] = arr(p.d_dmt, {g.ndm, g.ntime});
  d["cnt_ds"] = arr(p.cnt_ds, {g.nsub});
  d["cnt_dmt"] = arr(p.cnt_dmt, {g.ndm});
  d["moff_ds"] = arr(p.moff_ds, {g.nsub});
  d["moff_dmt"] = arr(p.moff_dmt, {g.ndm});
  d["v2_ds"] = arr(p.v2_ds, {g.nsub});
  d["v2_dmt"] = arr(p.v2_dmt, {g.ndm});
  d["v"] = p.v;
  d["mbar_ds"] = p.mbar_ds;
  d["mbar_dmt"] = arr(p.mbar_dmt, {g.ndm});
  return d;
}

BurstOptPrepared prepared_of(const py::dict& d) {
  BurstOptPrepared p;
  p.d_ds = vec(d["d_ds"].cast<I32>());
  p.d_dmt = vec(d["d_dmt"].cast<I32>());
  p.cnt_ds = vec(d["cnt_ds"].cast<I32>());
  p.cnt_dmt = vec(d["cnt_dmt"].cast<I32>());
  p.moff_ds = vec(d["moff_ds"].cast<I64>());
  p.moff_dmt = vec(d["moff_dmt"].cast<I64>());
  p.v2_ds = vec(d["v2_ds"].cast<I64>());
  p.v2_dmt = vec(d["v2_dmt"].cast<I64>());
  p.v = d["v"].cast<double>();
  p.mbar_ds = d["mbar_ds"].cast<double>();
  p.mbar_dmt = vec(d["mbar_dmt"].cast<F64>());
  return p;
}

py::dict search_to_dict(const BurstOptSearch& s, int nw, int rows) {
  py::dict d;
  d["best_val"] = arr(s.best_val, {2, nw});
  d["best_idx"] = arr(s.best_idx, {2, nw});
  d["curve"] = arr(s.curve, {nw, rows});
  d["curve_bin"] = arr(s.curve_bin, {nw, rows});
  return d;
}

BurstOptSearch search_of(const py::dict& d) {
  BurstOptSearch s;
  s.best_val = vec(d["best_val"].cast<I32>());
  s.best_idx = vec(d["best_idx"].cast<I32>());
  s.curve = vec(d["curve"].cast<I32>());
  s.curve_bin = vec(d["curve_bin"].cast<I32>());
  return s;
}

py::dict result_to_dict(const BurstOptResult& r, int ntime, int nsub) {
  const int ndm = static_cast<int>(r.dms.size()), nfine = static_cast<int>(r.dmf.size());
  const int nw = static_cast<int>(r.search.best_val.size() / 2);
  py::dict d = search_to_dict(r.search, nw, ndm + nfine);
  d["snr"] = r.snr;
  d["snr_coarse"] = r.snr_coarse;
  d["snr_in"] = r.snr_in;
  d["snr_dm0"] = r.snr_dm0;
  d["frac_pos"] = r.frac_pos;
  d["v"] = r.v;
  d["mbar_ds"] = r.mbar_ds;
  d["opt_sample"] = r.opt_sample;
  d["opt_dm"] = r.opt_dm;
  d["coarse_dm"] = r.coarse_dm;
  d["opt_width"] = r.opt_width;
  d["opt_kf"] = r.opt_kf;
  d["opt_bin"] = r.opt_bin;
  d["coarse_row"] = r.coarse_row;
  d["coarse_width"] = r.coarse_width;
  d["coarse_bin"] = r.coarse_bin;
  d["flags"] = r.flags;
  d["dms"] = arr(r.dms, {ndm});
  d["dmf"] = arr(r.dmf, {nfine});
  d["mbar_dmt"] = arr(r.mbar_dmt, {ndm});
  d["band"] = arr(r.band, {nsub});
  d["profile"] = arr(r.profile, {ntime});
  return d;
}

BurstOptResult result_of(const py::dict& d) {
  BurstOptResult r;
  r.search = search_of(d);
  r.snr = d["snr"].cast<double>();
  r.snr_coarse = d["snr_coarse"].cast<double>();
  r.snr_in = d["snr_in"].cast<double>();
  r.snr_dm0 = d["snr_dm0"].cast<double>();
  r.frac_pos = d["frac_pos"].cast<double>();
  r.v = d["v"].cast<double>();
  r.mbar_ds = d["mbar_ds"].cast<double>();
  r.opt_sample = d["opt_sample"].cast<int64_t>();
  r.opt_dm = d["opt_dm"].cast<float>();
  r.coarse_dm = d["coarse_dm"].cast<float>();
  r.opt_width = d["opt_width"].cast<uint32_t>();
  r.opt_kf = d["opt_kf"].cast<uint32_t>();
  r.opt_bin = d["opt_bin"].cast<uint32_t>();
  r.coarse_row = d["coarse_row"].cast<uint32_t>();
  r.coarse_width = d["coarse_width"].cast<uint32_t>();
  r.coarse_bin = d["coarse_bin"].cast<uint32_t>();
  r.flags = d["flags"].cast<uint32_t>();
  r.dms = vec(d["dms"].cast<F32>());
  r.dmf = vec(d["dmf"].cast<F32>());
  r.mbar_dmt = vec(d["mbar_dmt"].cast<F64>());
  r.band = vec(d["band"].cast<I32>());
  r.profile = vec(d["profile"].cast<I32>());
  return r;
}

void add_cand_scalars(py::dict& d, const BurstOptInput& c) {
  d["sample"] = c.sample;
  d["width"] = c.width;
  d["tscrunch"] = c.tscrunch;
  d["t0"] = c.t0;
  d["dm"] = c.dm;
  d["cand_snr"] = c.snr;
}

}  // namespace

void bind_bopt(py::module_& m) {
  py::class_<BurstOptCmdLineOptions>(m, "BurstOptCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &BurstOptCmdLineOptions::infilename)
      .def_readwrite("outfilename", &BurstOptCmdLineOptions::outfilename)
      .def_readwrite("nfine", &BurstOptCmdLineOptions::nfine)
      .def_readwrite("fine_half_range", &BurstOptCmdLineOptions::fine_half_range)
      .def_readwrite("limit", &BurstOptCmdLineOptions::limit)
      .def_readwrite("verbose", &BurstOptCmdLineOptions::verbose);
  m.def("parse_bopt_cmdline", [](const std::vector<std::string>& argv) {
    BurstOptCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_bopt_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("default_bopt_output_filename", &default_bopt_output_filename);
  m.def("bopt_nwidths", &kern::bopt_nwidths);

  py::class_<BurstOptGrid>(m, "BurstOptGrid")
      .def(py::init([](int nfine, double fine_half_range) {
             BurstOptGrid g;
             g.nfine = nfine;
             g.fine_half_range = fine_half_range;
             return g;
           }),
           py::arg("nfine") = 65, py::arg("fine_half_range") = 0.0)
      .def_readwrite("nfine", &BurstOptGrid::nfine)
      .def_readwrite("fine_half_range", &BurstOptGrid::fine_half_range);

  py::class_<BurstOptGeom>(m, "BurstOptGeom")
      .def(py::init([](int ntime, int nsub, int ndm, int nchans, double tsamp, double fch1, double foff) {
             BurstOptGeom g;
             g.ntime = ntime;
             g.nsub = nsub;
             g.ndm = ndm;
             g.nchans = nchans;
             g.tsamp = tsamp;
             g.fch1 = fch1;
             g.foff = foff;
             return g;
           }),
           py::arg("ntime"), py::arg("nsub"), py::arg("ndm"), py::arg("nchans") = 1, py::arg("tsamp") = 1.0,
           py::arg("fch1") = 0.0, py::arg("foff") = 0.0)
      .def_readwrite("ntime", &BurstOptGeom::ntime)
      .def_readwrite("nsub", &BurstOptGeom::nsub)
      .def_readwrite("ndm", &BurstOptGeom::ndm)
      .def_readwrite("nchans", &BurstOptGeom::nchans)
      .def_readwrite("tsamp", &BurstOptGeom::tsamp)
      .def_readwrite("fch1", &BurstOptGeom::fch1)
      .def_readwrite("foff", &BurstOptGeom::foff);

  // ---- the host steps: no GPU
  m.def(
      "burst_opt_prepare",
      [](size_t k, const BurstOptGeom& g, const py::dict& cand) {
        return prepared_to_dict(burst_opt_prepare(k, g, input_of(cand)), g);
      },
      py::arg("k"), py::arg("geom"), py::arg("cand"));
  m.def(
      "burst_opt_shifts",
      [](const BurstOptGeom& g, const BurstOptGrid& grid, float dm, uint32_t f, const F32& dms,
         const std::vector<float>& delays) {
        const BurstOptShifts s = burst_opt_shifts(g, grid, dm, f, vec(dms), delays);
        py::dict d;
        d["dmf"] = arr(s.dmf, {grid.nfine});
        d["sf"] = arr(s.sf, {grid.nfine, g.nsub});
        return d;
      },
      py::arg("geom"), py::arg("grid"), py::arg("dm"), py::arg("tscrunch"), py::arg("dms"), py::arg("delays"));
  m.def(
      "burst_opt_search_host",
      [](const BurstOptGeom& g, const I32& d_ds, const I32& d_dmt, const I32& sf) {
        PSOUP_CHECK(sf.ndim() == 2, "burst_opt_search_host: sf must be [nfine, nsub]");
        const int nfine = static_cast<int>(sf.shape(0));
        return search_to_dict(burst_opt_search_host(g, nfine, vec(d_ds), vec(d_dmt), vec(sf)),
                              kern::bopt_nwidths(g.ntime), g.ndm + nfine);
      },
      py::arg("geom"), py::arg("d_ds"), py::arg("d_dmt"), py::arg("sf"));
  m.def(
      "burst_opt_finish",
      [](const BurstOptGeom& g, const BurstOptGrid& grid, const py::dict& cand, const py::dict& prep,
         const py::dict& shifts, const py::dict& found) {
        BurstOptInput in;
        scalars_of(cand, in);
        BurstOptShifts sh;
        sh.dmf = vec(shifts["dmf"].cast<F32>());
        sh.sf = vec(shifts["sf"].cast<I32>());
        return result_to_dict(burst_opt_finish(g, grid, in, prepared_of(prep), sh, search_of(found)), g.ntime, g.nsub);
      },
      py::arg("geom"), py::arg("grid"), py::arg("cand"), py::arg("prep"), py::arg("shifts"), py::arg("found"));
  m.def("burst_opt_snr", &burst_opt_snr, py::arg("s"), py::arg("w"), py::arg("mbar"), py::arg("v"));

  // ---- the optimiser
  py::class_<BurstOptimiser>(m, "BurstOptimiser")
      .def(py::init([](const BurstOptGeom& g, const BurstOptGrid& grid, uintptr_t stream, size_t batch_bytes) {
             return new BurstOptimiser(g, grid, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("geom"), py::arg("grid"), py::arg("stream") = 0,
           py::arg("batch_bytes") = BurstOptimiser::kDefaultBatchBytes)
      // candidates: list of cutout dicts (BurstCubeFile.candidate's keys); list of result dicts
      .def("optimise",
           [](BurstOptimiser& o, const std::vector<py::dict>& cands, const std::vector<float>& delays) {
             std::vector<BurstOptInput> in;
             for (const py::dict& c : cands) in.push_back(input_of(c));
             std::vector<BurstOptResult> res;
             {
               py::gil_scoped_release nogil;
               res = o.optimise(in, delays);
             }
             py::list out;
             for (size_t i = 0; i < res.size(); ++i) {
               py::dict d = result_to_dict(res[i], o.geom().ntime, o.geom().nsub);
               add_cand_scalars(d, in[i]);
               out.append(d);
             }
             return out;
           },
           py::arg("candidates"), py::arg("delays"))
      // d_ds [ncand, nsub, ntime], d_dmt [ncand, ndm, ntime], sf [ncand, nfine, nsub]
      .def("search",
           [](BurstOptimiser& o, const I32& d_ds, const I32& d_dmt, const I32& sf) {
             const BurstOptGeom& g = o.geom();
             PSOUP_CHECK(d_ds.ndim() == 3 && d_dmt.ndim() == 3 && sf.ndim() == 3,
                         "burst search: d_ds [ncand, nsub, ntime], d_dmt [ncand, ndm, ntime], sf [ncand, nfine, nsub]");
             const py::ssize_t nc = d_ds.shape(0);
             PSOUP_CHECK(d_ds.shape(1) == g.nsub && d_ds.shape(2) == g.ntime && d_dmt.shape(0) == nc &&
                             d_dmt.shape(1) == g.ndm && d_dmt.shape(2) == g.ntime && sf.shape(0) == nc &&
                             sf.shape(1) == o.grid().nfine && sf.shape(2) == g.nsub,
                         "burst search: array shapes do not match the geometry and the grid");
             std::vector<BurstOptSearch> res;
             {
               py::gil_scoped_release nogil;
               res = o.search(d_ds.data(), d_dmt.data(), sf.data(), static_cast<size_t>(nc));
             }
             py::list out;
             for (const BurstOptSearch& s : res) out.append(search_to_dict(s, o.nwidths(), g.ndm + o.grid().nfine));
             return out;
           },
           py::arg("d_ds"), py::arg("d_dmt"), py::arg("sf"))
      // device addresses of int32 tensors
      .def("search_device",
           [](BurstOptimiser& o, uintptr_t d_ds, uintptr_t d_dmt, uintptr_t sf, size_t ncand, uintptr_t best_val,
              uintptr_t best_idx, uintptr_t curve, uintptr_t curve_bin) {
             py::gil_scoped_release nogil;
             o.search_device(reinterpret_cast<const int32_t*>(d_ds), reinterpret_cast<const int32_t*>(d_dmt),
                             reinterpret_cast<const int32_t*>(sf), ncand, reinterpret_cast<int32_t*>(best_val),
                             reinterpret_cast<int32_t*>(best_idx), reinterpret_cast<int32_t*>(curve),
                             reinterpret_cast<int32_t*>(curve_bin));
           },
           py::arg("d_ds"), py::arg("d_dmt"), py::arg("sf"), py::arg("ncand"), py::arg("best_val"),
           py::arg("best_idx"), py::arg("curve"), py::arg("curve_bin"))
      .def_property_readonly("bytes_per_candidate", &BurstOptimiser::bytes_per_candidate)
      .def_property_readonly("batch_size", &BurstOptimiser::batch_size)
      .def_property_readonly("batches", &BurstOptimiser::batches)
      .def_property_readonly("nwidths", &BurstOptimiser::nwidths);

  py::class_<BoptFileHeader>(m, "BoptFileHeader")
      .def(py::init<>())
      .def_readwrite("ncand", &BoptFileHeader::ncand)
      .def_readwrite("ntime", &BoptFileHeader::ntime)
      .def_readwrite("nsub", &BoptFileHeader::nsub)
      .def_readwrite("ndm", &BoptFileHeader::ndm)
      .def_readwrite("nchans", &BoptFileHeader::nchans)
      .def_readwrite("nbits", &BoptFileHeader::nbits)
      .def_readwrite("nfine", &BoptFileHeader::nfine)
      .def_readwrite("nw", &BoptFileHeader::nw)
      .def_readwrite("nsamps", &BoptFileHeader::nsamps)
      .def_readwrite("tsamp", &BoptFileHeader::tsamp)
      .def_readwrite("fch1", &BoptFileHeader::fch1)
      .def_readwrite("foff", &BoptFileHeader::foff)
      .def_readwrite("fine_half_range", &BoptFileHeader::fine_half_range);

  py::class_<BurstOptRun>(m, "BurstOptRun")
      .def_readonly("header", &BurstOptRun::header)
      .def_readonly("timers", &BurstOptRun::timers)
      .def_property_readonly("ncand", [](const BurstOptRun& r) { return r.results.size(); })
      .def("result", [](const BurstOptRun& r, size_t i) {
        PSOUP_CHECK(i < r.results.size(), "BurstOptRun.result: index out of range");
        py::dict d = result_to_dict(r.results[i], static_cast<int>(r.header.ntime), static_cast<int>(r.header.nsub));
        add_cand_scalars(d, r.candidates[i]);
        return d;
      });
  m.def("run_bopt_pipeline", [](const BurstOptCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_bopt_pipeline(a);
  });
  // dict(geom, nbits, nsamps, candidates: list of cutout dicts)
  m.def(
      "read_burst_file",
      [](const std::string& path, int limit) {
        const BurstFile f = read_burst_file(path, limit);
        py::list cands;
        for (const BurstOptInput& c : f.candidates) cands.append(input_to_dict(c, f.geom));
        py::dict out;
        out["geom"] = f.geom;
        out["nbits"] = f.nbits;
        out["nsamps"] = f.nsamps;
        out["candidates"] = cands;
        return out;
      },
      py::arg("path"), py::arg("limit") = -1);
  // Native writer over result dicts (tests compare it with the Python one).
  m.def(
      "write_bopt_file",
      [](const std::string& path, const BoptFileHeader& h, const std::vector<py::dict>& records) {
        std::vector<BurstOptInput> cands(records.size());
        std::vector<BurstOptResult> results;
        for (size_t i = 0; i < records.size(); ++i) {
          const py::dict& r = records[i];
          cands[i].sample = r["sample"].cast<uint64_t>();
          cands[i].width = r["width"].cast<uint32_t>();
          cands[i].tscrunch = r["tscrunch"].cast<uint32_t>();
          cands[i].t0 = r["t0"].cast<int64_t>();
          cands[i].dm = r["dm"].cast<float>();
          cands[i].snr = r["cand_snr"].cast<float>();
          results.push_back(result_of(r));
        }
        write_bopt_file(path, h, cands, results);
      },
      py::arg("path"), py::arg("header"), py::arg("records"));
}
