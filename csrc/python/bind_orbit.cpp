// pybind11 bindings of orbsearch (orbit.hpp): options, the host steps (no GPU
// needed), the kernel alone over raw device addresses, OrbitSearcher over a
// resident filterbank, the global distillation and the output text.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/orbit.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using U8 = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
using Triple = std::tuple<uint64_t, uint64_t, int64_t>;  // (W, F, Aq)
using Orbit = std::tuple<double, double, double>;        // (pb, a1, ph)

// What the raw entries accept: 1..4096 quantised templates inside the definition's ranges.
std::vector<OrbitQuant> quants(const std::vector<Triple>& q) {
  PSOUP_CHECK(!q.empty() && q.size() <= static_cast<size_t>(kOrbitMaxPerLaunch),
              "orbit_resample: 1.." << kOrbitMaxPerLaunch << " templates per launch");
  std::vector<OrbitQuant> out;
  for (const Triple& t : q) {
    out.push_back(OrbitQuant{std::get<0>(t), std::get<1>(t), std::get<2>(t)});
    orbit_check_quant(out.back());
  }
  return out;
}

std::vector<OrbitTemplate> bank_of(const std::vector<Orbit>& b) {
  std::vector<OrbitTemplate> out;
  for (const Orbit& t : b) out.push_back(OrbitTemplate{std::get<0>(t), std::get<1>(t), std::get<2>(t)});
  return out;
}

std::vector<Orbit> tuples_of(const std::vector<OrbitTemplate>& b) {
  std::vector<Orbit> out;
  for (const OrbitTemplate& t : b) out.emplace_back(t.pb, t.a1, t.ph);
  return out;
}

}  // namespace

void bind_orbit(py::module_& m) {
  py::class_<OrbitCmdLineOptions>(m, "OrbitCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("search", &OrbitCmdLineOptions::search)
      .def_readwrite("outfilename", &OrbitCmdLineOptions::outfilename)
      .def_readwrite("bankfile", &OrbitCmdLineOptions::bankfile)
      .def_readwrite("pb_start", &OrbitCmdLineOptions::pb_start)
      .def_readwrite("pb_end", &OrbitCmdLineOptions::pb_end)
      .def_readwrite("npb", &OrbitCmdLineOptions::npb)
      .def_readwrite("a1_start", &OrbitCmdLineOptions::a1_start)
      .def_readwrite("a1_end", &OrbitCmdLineOptions::a1_end)
      .def_readwrite("na1", &OrbitCmdLineOptions::na1)
      .def_readwrite("nphase", &OrbitCmdLineOptions::nphase);
  m.def("parse_orbit_cmdline", [](const std::vector<std::string>& argv) {
    OrbitCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_orbit_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.attr("ORBIT_TILE") = kern::kOrbitTile;
  m.attr("ORBIT_LANE") = kern::kOrbitLane;
  m.attr("ORBIT_TILES_PER_GROUP") = kern::kOrbitTilesPerGroup;
  m.attr("ORBIT_MAX_SPAN") = kOrbitMaxSpan;
  m.attr("ORBIT_MAX_PER_LAUNCH") = kOrbitMaxPerLaunch;
  m.attr("ORBIT_MAX_TEMPLATES") = kOrbitMaxTemplates;

  // ---- the host steps (no GPU)
  m.def("orbit_sine_table", [] {
    const std::vector<int32_t> t = orbit_sine_table();
    py::array_t<int32_t> a(static_cast<py::ssize_t>(t.size()));
    std::memcpy(a.mutable_data(), t.data(), t.size() * sizeof(int32_t));
    return a;
  });
  m.def(
      "orbit_quantise",
      [](double pb, double a1, double ph, float tsamp) {
        const OrbitQuant q = orbit_quantise(pb, a1, ph, tsamp);
        return Triple(q.W, q.F, q.Aq);
      },
      py::arg("pb"), py::arg("a1"), py::arg("ph"), py::arg("tsamp"));
  m.def(
      "orbit_shift",
      [](Triple q, uint64_t i) {
        static const std::vector<int32_t> table = orbit_sine_table();
        const OrbitQuant t{std::get<0>(q), std::get<1>(q), std::get<2>(q)};
        orbit_check_quant(t);
        return orbit_shift(table.data(), t, i);
      },
      py::arg("q"), py::arg("i"));
  m.def(
      "orbit_shifts",
      [](Triple q, uint64_t n) {
        static const std::vector<int32_t> table = orbit_sine_table();
        const OrbitQuant t{std::get<0>(q), std::get<1>(q), std::get<2>(q)};
        orbit_check_quant(t);
        py::array_t<int64_t> s(static_cast<py::ssize_t>(n));
        for (uint64_t i = 0; i < n; ++i) s.mutable_data()[i] = orbit_shift(table.data(), t, i);
        return s;
      },
      py::arg("q"), py::arg("n"));
  m.def("orbit_beta", [](double pb, double a1) { return orbit_beta(OrbitTemplate{pb, a1, 0.0}); });
  m.def(
      "orbit_check", [](uint64_t n, const std::vector<Orbit>& bank, float tsamp) { orbit_check(n, bank_of(bank), tsamp); },
      py::arg("n"), py::arg("bank"), py::arg("tsamp"));
  m.def("orbit_parse_bank", [](const std::string& text) { return tuples_of(orbit_parse_bank(text)); });
  m.def(
      "orbit_grid",
      [](double pb_start, double pb_end, int npb, double a1_start, double a1_end, int na1, int nphase) {
        return tuples_of(orbit_grid(pb_start, pb_end, npb, a1_start, a1_end, na1, nphase));
      },
      py::arg("pb_start"), py::arg("pb_end"), py::arg("npb"), py::arg("a1_start"), py::arg("a1_end"), py::arg("na1"),
      py::arg("nphase"));
  m.def(
      "orbit_resample_host",
      [](U8 x, uint64_t nrow, uint64_t n, const std::vector<Triple>& q, uint64_t out_stride) {
        PSOUP_CHECK(x.ndim() == 2, "orbit_resample_host: x must be [nrows, row_stride]");
        const int nrows = static_cast<int>(x.shape(0));
        const uint64_t row_stride = static_cast<uint64_t>(x.shape(1));
        const std::vector<OrbitQuant> t = quants(q);
        if (out_stride == 0) out_stride = nrow;
        PSOUP_CHECK(out_stride >= nrow && row_stride >= nrow, "orbit_resample: a stride is shorter than the row");
        py::array_t<uint8_t> y({static_cast<py::ssize_t>(nrows), static_cast<py::ssize_t>(t.size()),
                                static_cast<py::ssize_t>(out_stride)});
        std::memset(y.mutable_data(), 0, static_cast<size_t>(y.size()));
        orbit_resample_host(x.data(), row_stride, nrows, nrow, n, t, y.mutable_data(), out_stride);
        return y;
      },
      py::arg("x"), py::arg("nrow"), py::arg("n"), py::arg("q"), py::arg("out_stride") = 0);

  py::class_<OrbitCandidate>(m, "OrbitCandidate")
      .def(py::init<>())
      .def(py::init([](const Candidate& c, uint32_t tmpl) { return OrbitCandidate{c, tmpl}; }), py::arg("cand"),
           py::arg("tmpl"))
      .def_readwrite("cand", &OrbitCandidate::cand)
      .def_readwrite("tmpl", &OrbitCandidate::tmpl);
  m.def("orbit_distill", &orbit_distill, py::arg("cands"), py::arg("beta"), py::arg("tol"),
        py::arg("keep_related") = true);

  py::class_<OrbitSetup>(m, "OrbitSetup")
      .def_readonly("nrow", &OrbitSetup::nrow)
      .def_readonly("span", &OrbitSetup::span)
      .def_readonly("beta", &OrbitSetup::beta)
      .def_property_readonly("bank", [](const OrbitSetup& s) { return tuples_of(s.bank); })
      .def_property_readonly("quant",
                             [](const OrbitSetup& s) {
                               std::vector<Triple> q;
                               for (const OrbitQuant& t : s.quant) q.emplace_back(t.W, t.F, t.Aq);
                               return q;
                             })
      .def_property_readonly("dm_list", [](const OrbitSetup& s) { return s.search.dm_list; })
      .def_property_readonly("killmask", [](const OrbitSetup& s) { return s.search.killmask; })
      .def_property_readonly("fft_size", [](const OrbitSetup& s) { return s.search.fft_size; })
      .def_property_readonly("tsamp", [](const OrbitSetup& s) { return s.search.search.tsamp; })
      .def_property_readonly("nsamps", [](const OrbitSetup& s) { return s.search.nsamps; })
      .def_property_readonly("accel_plan", [](const OrbitSetup& s) { return s.search.accel_plan; })
      .def_property_readonly("search_params", [](const OrbitSetup& s) { return s.search.search; })
      .def_property_readonly("geometry", [](const OrbitSetup& s) {
        return DedispGeometry::make(s.search.header, s.search.nsamps, s.search.dm_list, s.search.killmask);
      });
  // reads the header of args.search.infilename; every refusal is raised here
  m.def("orbit_setup", [](const OrbitCmdLineOptions& a) {
    return make_orbit_setup(a, read_header_file(a.search.infilename));
  });

  // ---- the kernel alone: device addresses; q are the quantised templates on the host (checked here), q_dev the
  // same K records {uint64 W, uint64 F, int64 Aq} and table_dev the 4097 int32 of the sine table on the device, which
  // the caller keeps alive until the stream has run the kernel
  m.def(
      "orbit_resample_raw",
      [](uintptr_t in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, const std::vector<Triple>& q,
         uintptr_t q_dev, uintptr_t table_dev, uintptr_t out, uint64_t out_stride, uintptr_t s) {
        const std::vector<OrbitQuant> t = quants(q);
        PSOUP_CHECK(q_dev != 0 && q_dev % 8 == 0, "orbit_resample: the device templates must be 8-byte aligned");
        PSOUP_CHECK(table_dev != 0 && table_dev % 4 == 0, "orbit_resample: the device table must be 4-byte aligned");
        kern::orbit_resample(reinterpret_cast<const uint8_t*>(in), row_stride, nrows, nrow, n,
                             reinterpret_cast<const OrbitQuant*>(q_dev), static_cast<int>(t.size()),
                             reinterpret_cast<const int32_t*>(table_dev), reinterpret_cast<uint8_t*>(out), out_stride,
                             reinterpret_cast<hipStream_t>(s));
      },
      py::arg("rows"), py::arg("row_stride"), py::arg("nrows"), py::arg("nrow"), py::arg("n"), py::arg("q"),
      py::arg("q_dev"), py::arg("table_dev"), py::arg("out"), py::arg("out_stride"), py::arg("stream") = 0);

  // ---- OrbitSearcher over a resident filterbank
  py::class_<OrbitSearcher>(m, "OrbitSearcher")
      .def(py::init([](const OrbitSetup& setup, const DeviceFilterbank& fb, uintptr_t s) {
             return new OrbitSearcher(setup, fb, reinterpret_cast<hipStream_t>(s));
           }),
           py::arg("setup"), py::arg("filterbank"), py::arg("stream") = 0, py::keep_alive<1, 2>(),
           py::keep_alive<1, 3>())
      .def("search", &OrbitSearcher::search, py::arg("d0") = 0, py::arg("d1") = -1,
           py::call_guard<py::gil_scoped_release>())
      .def("fold",
           [](OrbitSearcher& os, OrbitCandidateList cands, int npdmp) {
             {
               py::gil_scoped_release nogil;
               os.fold(cands, npdmp);
             }
             return cands;
           },
           py::arg("cands"), py::arg("npdmp"))
      .def_property_readonly("accel_trials", &OrbitSearcher::accel_trials)
      .def_property_readonly("template_trials", &OrbitSearcher::template_trials);
  m.def("orbit_global_distill", &orbit_global_distill, py::arg("cands"), py::arg("args"), py::arg("setup"),
        py::call_guard<py::gil_scoped_release>());

  m.def("orbit_output_text", &orbit_output_text);
  m.def("write_orbit_output", &write_orbit_output);
}
