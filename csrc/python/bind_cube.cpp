// pybind11 bindings of the filterbank fold cubes (foldcube.hpp): options,
// params, candidates, CubeFolder over raw device addresses, pipeline, writer.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/foldcube.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

py::dict result_to_dict(const CubeResult& r, const CubeParams& p) {
  py::array_t<int32_t> na(std::vector<py::ssize_t>{p.nsub});
  py::array_t<int32_t> hits(std::vector<py::ssize_t>{p.nints, p.nbins});
  py::array_t<int64_t> sums(std::vector<py::ssize_t>{p.nints, p.nsub, p.nbins});
  std::memcpy(na.mutable_data(), r.nactive.data(), r.nactive.size() * sizeof(int32_t));
  std::memcpy(hits.mutable_data(), r.hits.data(), r.hits.size() * sizeof(int32_t));
  std::memcpy(sums.mutable_data(), r.sums.data(), r.sums.size() * sizeof(int64_t));
  py::dict d;
  d["nactive"] = na;
  d["hits"] = hits;
  d["sums"] = sums;
  return d;
}

}  // namespace

void bind_cube(py::module_& m) {
  py::class_<FoldCubeCmdLineOptions>(m, "FoldCubeCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &FoldCubeCmdLineOptions::infilename)
      .def_readwrite("outfilename", &FoldCubeCmdLineOptions::outfilename)
      .def_readwrite("candfilename", &FoldCubeCmdLineOptions::candfilename)
      .def_readwrite("overviewfilename", &FoldCubeCmdLineOptions::overviewfilename)
      .def_readwrite("killfilename", &FoldCubeCmdLineOptions::killfilename)
      .def_readwrite("nints", &FoldCubeCmdLineOptions::nints)
      .def_readwrite("nsub", &FoldCubeCmdLineOptions::nsub)
      .def_readwrite("nbins", &FoldCubeCmdLineOptions::nbins)
      .def_readwrite("fold_nsamps", &FoldCubeCmdLineOptions::fold_nsamps)
      .def_readwrite("limit", &FoldCubeCmdLineOptions::limit)
      .def_readwrite("top", &FoldCubeCmdLineOptions::top)
      .def_readwrite("verbose", &FoldCubeCmdLineOptions::verbose);
  m.def("parse_cube_cmdline", [](const std::vector<std::string>& argv) {
    FoldCubeCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_cube_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("default_cube_output_filename", &default_cube_output_filename);
  m.def("cube_tile", []() { return kern::kCubeTile; });

  py::class_<CubeParams>(m, "CubeParams")
      .def(py::init<>())
      .def(py::init([](int nints, int nsub, int nbins, uint64_t fold_nsamps) {
             CubeParams p;
             p.nints = nints;
             p.nsub = nsub;
             p.nbins = nbins;
             p.fold_nsamps = fold_nsamps;
             return p;
           }),
           py::arg("nints"), py::arg("nsub"), py::arg("nbins"), py::arg("fold_nsamps"))
      .def_readwrite("nints", &CubeParams::nints)
      .def_readwrite("nsub", &CubeParams::nsub)
      .def_readwrite("nbins", &CubeParams::nbins)
      .def_readwrite("fold_nsamps", &CubeParams::fold_nsamps);

  py::class_<CubeCandidate>(m, "CubeCandidate")
      .def(py::init<>())
      .def(py::init([](double period, float dm, float acc) {
             CubeCandidate c;
             c.period = period;
             c.dm = dm;
             c.acc = acc;
             return c;
           }),
           py::arg("period"), py::arg("dm"), py::arg("acc") = 0.f)
      .def_readwrite("period", &CubeCandidate::period)
      .def_readwrite("dm", &CubeCandidate::dm)
      .def_readwrite("acc", &CubeCandidate::acc);
  m.def("read_cube_candfile", &read_cube_candfile, py::arg("path"), py::arg("limit") = -1);
  m.def("default_fold_nsamps", &default_fold_nsamps);

  // chan_major: device address of int8 [nchans][stride]; row_valid samples of
  // each row may be folded.
  py::class_<CubeFolder>(m, "CubeFolder")
      .def(py::init([](uintptr_t chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias, double tsamp,
                       const std::vector<float>& delays, const std::vector<int>& killmask, const CubeParams& p,
                       uintptr_t stream, size_t batch_bytes) {
             return new CubeFolder(reinterpret_cast<const int8_t*>(chan_major), stride, row_valid, nchans, bias, tsamp,
                                   delays, killmask, p, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("chan_major"), py::arg("stride"), py::arg("row_valid"), py::arg("nchans"), py::arg("bias"),
           py::arg("tsamp"), py::arg("delays"), py::arg("killmask"), py::arg("params"), py::arg("stream") = 0,
           py::arg("batch_bytes") = CubeFolder::kDefaultBatchBytes)
      .def(py::init([](const DeviceFilterbank& fb, const CubeParams& p, uintptr_t stream, size_t batch_bytes) {
             return new CubeFolder(fb, p, reinterpret_cast<hipStream_t>(stream), batch_bytes);
           }),
           py::arg("filterbank"), py::arg("params"), py::arg("stream") = 0,
           py::arg("batch_bytes") = CubeFolder::kDefaultBatchBytes, py::keep_alive<1, 2>())
      // list of dict(nactive int32 [nsub], hits int32 [nints, nbins], sums int64 [nints, nsub, nbins])
      .def("fold",
           [](CubeFolder& f, const std::vector<CubeCandidate>& cands) {
             std::vector<CubeResult> res;
             {
               py::gil_scoped_release nogil;
               res = f.fold(cands);
             }
             py::list out;
             for (const CubeResult& r : res) out.append(result_to_dict(r, f.params()));
             return out;
           })
      .def("fold_offsets",
           [](CubeFolder& f, py::array_t<int32_t, py::array::c_style | py::array::forcecast> offsets,
              const std::vector<double>& periods, const std::vector<float>& accs, uintptr_t sums, uintptr_t hits) {
             PSOUP_CHECK(offsets.ndim() == 2 && static_cast<size_t>(offsets.shape(0)) == periods.size(),
                         "fold_offsets: offsets must be [ncand, nchans]");
             PSOUP_CHECK(static_cast<size_t>(offsets.shape(1)) * sizeof(int32_t) ==
                             static_cast<size_t>(offsets.strides(0)),
                         "fold_offsets: offsets must be contiguous");
             const int32_t* o = offsets.data();
             py::gil_scoped_release nogil;
             f.fold_offsets(o, periods, accs, reinterpret_cast<int64_t*>(sums), reinterpret_cast<int32_t*>(hits));
           },
           py::arg("offsets"), py::arg("periods"), py::arg("accs"), py::arg("sums"), py::arg("hits"))
      .def_property_readonly("nactive", &CubeFolder::nactive)
      .def_property_readonly("batch_size", &CubeFolder::batch_size)
      .def_property_readonly("batches", &CubeFolder::batches);

  py::class_<CubeFileHeader>(m, "CubeFileHeader")
      .def(py::init<>())
      .def_readwrite("ncand", &CubeFileHeader::ncand)
      .def_readwrite("nints", &CubeFileHeader::nints)
      .def_readwrite("nsub", &CubeFileHeader::nsub)
      .def_readwrite("nbins", &CubeFileHeader::nbins)
      .def_readwrite("nchans", &CubeFileHeader::nchans)
      .def_readwrite("nbits", &CubeFileHeader::nbits)
      .def_readwrite("fold_nsamps", &CubeFileHeader::fold_nsamps)
      .def_readwrite("tsamp", &CubeFileHeader::tsamp)
      .def_readwrite("fch1", &CubeFileHeader::fch1)
      .def_readwrite("foff", &CubeFileHeader::foff);

  py::class_<CubeRun>(m, "CubeRun")
      .def_readonly("header", &CubeRun::header)
      .def_readonly("candidates", &CubeRun::candidates)
      .def_readonly("timers", &CubeRun::timers)
      .def_property_readonly("ncand", [](const CubeRun& r) { return r.candidates.size(); });
  m.def("run_cube_pipeline", [](const FoldCubeCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_cube_pipeline(a);
  });
  m.def("run_cube_pipeline", [](const FoldCubeCmdLineOptions& a, const std::vector<CubeCandidate>& cands) {
    py::gil_scoped_release nogil;
    return run_cube_pipeline(a, cands);
  });
  // Native writer over NumPy arrays (tests compare it with the Python one).
  m.def(
      "write_cube_file",
      [](const std::string& path, const CubeFileHeader& h, const std::vector<CubeCandidate>& cands,
         const std::vector<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>& nactive,
         const std::vector<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>& hits,
         const std::vector<py::array_t<int64_t, py::array::c_style | py::array::forcecast>>& sums) {
        PSOUP_CHECK(nactive.size() == cands.size() && hits.size() == cands.size() && sums.size() == cands.size(),
                    "write_cube_file: one nactive / hits / sums array per candidate");
        std::vector<CubeResult> cubes(cands.size());
        for (size_t i = 0; i < cands.size(); ++i) {
          cubes[i].nactive.assign(nactive[i].data(), nactive[i].data() + nactive[i].size());
          cubes[i].hits.assign(hits[i].data(), hits[i].data() + hits[i].size());
          cubes[i].sums.assign(sums[i].data(), sums[i].data() + sums[i].size());
        }
        write_cube_file(path, h, cands, cubes);
      },
      py::arg("path"), py::arg("header"), py::arg("candidates"), py::arg("nactive"), py::arg("hits"),
      py::arg("sums"));
}
