// pybind11 bindings of the burst cutouts (burstcube.hpp): options, params,
// candidates and their readers, BurstCutter over raw device addresses,
// pipeline, writer.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/burstcube.hpp"
#include "psoup/common.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using i32_array = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

py::array_t<int32_t> plane(const std::vector<int32_t>& v, int rows, int cols) {
  py::array_t<int32_t> a(std::vector<py::ssize_t>{rows, cols});
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(int32_t));
  return a;
}

py::dict result_to_dict(const BurstResult& r, const BurstParams& p) {
  py::array_t<float> dms(std::vector<py::ssize_t>{p.ndm});
  py::array_t<int32_t> na(std::vector<py::ssize_t>{p.nsub});
  std::memcpy(dms.mutable_data(), r.dms.data(), r.dms.size() * sizeof(float));
  std::memcpy(na.mutable_data(), r.nactive.data(), r.nactive.size() * sizeof(int32_t));
  py::dict d;
  d["tscrunch"] = r.tscrunch;
  d["t0"] = r.t0;
  d["dms"] = dms;
  d["nactive"] = na;
  d["ds_sums"] = plane(r.ds_sums, p.nsub, p.ntime);
  d["ds_hits"] = plane(r.ds_hits, p.nsub, p.ntime);
  d["dmt_sums"] = plane(r.dmt_sums, p.ndm, p.ntime);
  d["dmt_hits"] = plane(r.dmt_hits, p.ndm, p.ntime);
  return d;
}

}  // namespace

void bind_burst(py::module_& m) {
  py::class_<BurstCubeCmdLineOptions>(m, "BurstCubeCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &BurstCubeCmdLineOptions::infilename)
      .def_readwrite("outfilename", &BurstCubeCmdLineOptions::outfilename)
      .def_readwrite("spfilename", &BurstCubeCmdLineOptions::spfilename)
      .def_readwrite("candfilename", &BurstCubeCmdLineOptions::candfilename)
      .def_readwrite("killfilename", &BurstCubeCmdLineOptions::killfilename)
      .def_readwrite("ntime", &BurstCubeCmdLineOptions::ntime)
      .def_readwrite("nsub", &BurstCubeCmdLineOptions::nsub)
      .def_readwrite("ndm", &BurstCubeCmdLineOptions::ndm)
      .def_readwrite("tscrunch", &BurstCubeCmdLineOptions::tscrunch)
      .def_readwrite("dm_half_range", &BurstCubeCmdLineOptions::dm_half_range)
      .def_readwrite("limit", &BurstCubeCmdLineOptions::limit)
      .def_readwrite("verbose", &BurstCubeCmdLineOptions::verbose);
  m.def("parse_burst_cmdline", [](const std::vector<std::string>& argv) {
    BurstCubeCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_burst_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("default_burst_output_filename", &default_burst_output_filename);
  // the kernel's tile constants (tests build edge shapes from them)
  m.def("burst_window", []() { return kern::kBurstWindow; });
  m.def("burst_max_rows", []() { return kern::kBurstMaxRows; });
  m.def("burst_max_f", []() { return kern::kBurstMaxF; });
  m.def("burst_tscrunch", &burst_tscrunch, py::arg("width"), py::arg("tscrunch") = 0);
  m.def("burst_t0", &burst_t0, py::arg("sample"), py::arg("width"), py::arg("f"), py::arg("ntime"));
  m.def("burst_dms", [](float dm, int ndm, float half) {
    const std::vector<float> v = burst_dms(dm, ndm, half);
    py::array_t<float> a(std::vector<py::ssize_t>{static_cast<py::ssize_t>(v.size())});
    std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(float));
    return a;
  }, py::arg("dm"), py::arg("ndm"), py::arg("dm_half_range") = 0.f);

  py::class_<BurstParams>(m, "BurstParams")
      .def(py::init<>())
      .def(py::init([](int ntime, int nsub, int ndm, int tscrunch, float dm_half_range) {
             BurstParams p;
             p.ntime = ntime;
             p.nsub = nsub;
             p.ndm = ndm;
             p.tscrunch = tscrunch;
             p.dm_half_range = dm_half_range;
             return p;
           }),
           py::arg("ntime"), py::arg("nsub"), py::arg("ndm"), py::arg("tscrunch") = 0,
           py::arg("dm_half_range") = 0.f)
      .def_readwrite("ntime", &BurstParams::ntime)
      .def_readwrite("nsub", &BurstParams::nsub)
      .def_readwrite("ndm", &BurstParams::ndm)
      .def_readwrite("tscrunch", &BurstParams::tscrunch)
      .def_readwrite("dm_half_range", &BurstParams::dm_half_range);

  py::class_<BurstCandidate>(m, "BurstCandidate")
      .def(py::init<>())
      .def(py::init([](uint64_t sample, uint32_t width, float dm, float snr) {
             BurstCandidate c;
             c.sample = sample;
             c.width = width;
             c.dm = dm;
             c.snr = snr;
             return c;
           }),
           py::arg("sample"), py::arg("width"), py::arg("dm"), py::arg("snr") = 0.f)
      .def_readwrite("sample", &BurstCandidate::sample)
      .def_readwrite("width", &BurstCandidate::width)
      .def_readwrite("dm", &BurstCandidate::dm)
      .def_readwrite("snr", &BurstCandidate::snr);
  m.def("read_burst_candfile", &read_burst_candfile, py::arg("path"), py::arg("limit") = -1);
  m.def("read_sp_output", &read_sp_output, py::arg("path"), py::arg("limit") = -1);

  // chan_major: device address of int8 [nchans][stride]; row_valid samples of
  // each row may be read.
  py::class_<BurstCutter>(m, "BurstCutter")
      .def(py::init([](uintptr_t chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias,
                       const std::vector<float>& delays, const std::vector<int>& killmask, const BurstParams& p,
                       uintptr_t stream, size_t batch_bytes) {
             return new BurstCutter(reinterpret_cast<const int8_t*>(chan_major), stride, row_valid, nchans, bias,
                                    delays, killmask, p, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("chan_major"), py::arg("stride"), py::arg("row_valid"), py::arg("nchans"), py::arg("bias"),
           py::arg("delays"), py::arg("killmask"), py::arg("params"), py::arg("stream") = 0,
           py::arg("batch_bytes") = BurstCutter::kDefaultBatchBytes)
      .def(py::init([](const DeviceFilterbank& fb, const BurstParams& p, uintptr_t stream, size_t batch_bytes) {
             return new BurstCutter(fb, p, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("filterbank"), py::arg("params"), py::arg("stream") = 0,
           py::arg("batch_bytes") = BurstCutter::kDefaultBatchBytes, py::keep_alive<1, 2>())
      // list of dict(tscrunch, t0, dms float32 [ndm], nactive int32 [nsub], ds_sums / ds_hits int32 [nsub,
      // ntime], dmt_sums / dmt_hits int32 [ndm, ntime])
      .def("cut",
           [](BurstCutter& f, const std::vector<BurstCandidate>& cands) {
             std::vector<BurstResult> res;
             {
               py::gil_scoped_release nogil;
               res = f.cut(cands);
             }
             py::list out;
             for (const BurstResult& r : res) out.append(result_to_dict(r, f.params()));
             return out;
           })
      .def("cut_offsets",
           [](BurstCutter& f, i32_array ds_offsets, i32_array dmt_offsets, const std::vector<int64_t>& t0,
              const std::vector<int>& tscrunch, uintptr_t sums, uintptr_t hits) {
             const size_t nc = t0.size();
             PSOUP_CHECK(ds_offsets.ndim() == 2 && static_cast<size_t>(ds_offsets.shape(0)) == nc &&
                             dmt_offsets.ndim() == 3 && static_cast<size_t>(dmt_offsets.shape(0)) == nc &&
                             dmt_offsets.shape(1) == f.params().ndm && dmt_offsets.shape(2) == ds_offsets.shape(1),
                         "cut_offsets: offsets must be [ncand, nchans] and [ncand, ndm, nchans]");
             const int32_t* a = ds_offsets.data();
             const int32_t* b = dmt_offsets.data();
             py::gil_scoped_release nogil;
             f.cut_offsets(a, b, t0, tscrunch, reinterpret_cast<int32_t*>(sums), reinterpret_cast<int32_t*>(hits));
           },
           py::arg("ds_offsets"), py::arg("dmt_offsets"), py::arg("t0"), py::arg("tscrunch"), py::arg("sums"),
           py::arg("hits"))
      .def_property_readonly("nactive", &BurstCutter::nactive)
      .def_property_readonly("bytes_per_candidate", &BurstCutter::bytes_per_candidate)
      .def_property_readonly("batch_size", &BurstCutter::batch_size)
      .def_property_readonly("batches", &BurstCutter::batches)
      .def_property_readonly("tiles", &BurstCutter::tiles)
      .def_property_readonly("single_row_tiles", &BurstCutter::single_row_tiles);

  py::class_<BurstFileHeader>(m, "BurstFileHeader")
      .def(py::init<>())
      .def_readwrite("ncand", &BurstFileHeader::ncand)
      .def_readwrite("ntime", &BurstFileHeader::ntime)
      .def_readwrite("nsub", &BurstFileHeader::nsub)
      .def_readwrite("ndm", &BurstFileHeader::ndm)
      .def_readwrite("nchans", &BurstFileHeader::nchans)
      .def_readwrite("nbits", &BurstFileHeader::nbits)
      .def_readwrite("nsamps", &BurstFileHeader::nsamps)
      .def_readwrite("tsamp", &BurstFileHeader::tsamp)
      .def_readwrite("fch1", &BurstFileHeader::fch1)
      .def_readwrite("foff", &BurstFileHeader::foff);

  py::class_<BurstRun>(m, "BurstRun")
      .def_readonly("header", &BurstRun::header)
      .def_readonly("candidates", &BurstRun::candidates)
      .def_readonly("timers", &BurstRun::timers)
      .def_property_readonly("ncand", [](const BurstRun& r) { return r.candidates.size(); });
  m.def("run_burst_pipeline", [](const BurstCubeCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_burst_pipeline(a);
  });
  // Native writer over NumPy arrays (tests compare it with the Python one):
  // each candidate a dict as BurstCutter.cut returns.
  m.def(
      "write_burst_file",
      [](const std::string& path, const BurstFileHeader& h, const std::vector<BurstCandidate>& cands,
         const std::vector<py::dict>& cutouts) {
        PSOUP_CHECK(cutouts.size() == cands.size(), "write_burst_file: one cutout per candidate");
        std::vector<BurstResult> res(cands.size());
        auto flat = [](const py::handle& o) {
          const i32_array a = py::cast<i32_array>(o);
          return std::vector<int32_t>(a.data(), a.data() + a.size());
        };
        for (size_t i = 0; i < cands.size(); ++i) {
          const py::dict& d = cutouts[i];
          res[i].tscrunch = py::cast<uint32_t>(d["tscrunch"]);
          res[i].t0 = py::cast<int64_t>(d["t0"]);
          const auto dms = py::cast<py::array_t<float, py::array::c_style | py::array::forcecast>>(d["dms"]);
          res[i].dms.assign(dms.data(), dms.data() + dms.size());
          res[i].nactive = flat(d["nactive"]);
          res[i].ds_sums = flat(d["ds_sums"]);
          res[i].ds_hits = flat(d["ds_hits"]);
          res[i].dmt_sums = flat(d["dmt_sums"]);
          res[i].dmt_hits = flat(d["dmt_hits"]);
        }
        write_burst_file(path, h, cands, res);
      },
      py::arg("path"), py::arg("header"), py::arg("candidates"), py::arg("cutouts"));
}
