// pybind11 bindings of jerksearch (jerk.hpp): options, the host steps (no GPU
// needed), the kernel alone over raw device addresses, JerkSearcher over a
// resident filterbank, the global distillation and the output text.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <cstring>

#include "psoup/common.hpp"
#include "psoup/jerk.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using U8 = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
using F64 = py::array_t<double, py::array::c_style | py::array::forcecast>;

std::vector<double> factors(const F64& jf) { return std::vector<double>(jf.data(), jf.data() + jf.size()); }

// What the raw kernel entry accepts: finite factors whose shifts stay far
// inside int64 (the driver's stricter rule is jerk_check).
void check_raw_factors(const std::vector<double>& jf, uint64_t n) {
  PSOUP_CHECK(!jf.empty() && jf.size() <= static_cast<size_t>(kJerkMaxTrials),
              "jerk_resample: 1.." << kJerkMaxTrials << " jerk factors");
  PSOUP_CHECK(n >= 1 && n <= kJerkMaxSpan, "jerk: series longer than 2^26 samples");
  const double N = static_cast<double>(n);
  for (double f : jf)
    PSOUP_CHECK(std::isfinite(f) && std::fabs(f) * N * N * N < 4.0e18, "jerk: a non-finite value (jerk factor)");
}

}  // namespace

void bind_jerk(py::module_& m) {
  py::class_<JerkCmdLineOptions>(m, "JerkCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("search", &JerkCmdLineOptions::search)
      .def_readwrite("outfilename", &JerkCmdLineOptions::outfilename)
      .def_readwrite("jerk_start", &JerkCmdLineOptions::jerk_start)
      .def_readwrite("jerk_end", &JerkCmdLineOptions::jerk_end)
      .def_readwrite("jerk_tol", &JerkCmdLineOptions::jerk_tol)
      .def_readwrite("jerk_step", &JerkCmdLineOptions::jerk_step);
  m.def("parse_jerk_cmdline", [](const std::vector<std::string>& argv) {
    JerkCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_jerk_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.attr("JERK_TILE") = kern::kJerkTile;
  m.attr("JERK_LANE") = kern::kJerkLane;
  m.attr("JERK_MAX_SPAN") = kJerkMaxSpan;
  m.attr("JERK_MAX_TRIALS") = kJerkMaxTrials;

  // ---- the host steps (no GPU)
  m.def("jerk_factor", &jerk_factor, py::arg("jerk"), py::arg("tsamp"));
  m.def("jerk_shift", &jerk_shift, py::arg("i"), py::arg("n"), py::arg("jf"));
  m.def("jerk_stationary", [](uint64_t n) {
    int64_t lo = 0, hi = 0;
    jerk_stationary(n, &lo, &hi);
    return py::make_tuple(lo, hi);
  });
  m.def("jerk_freq_factor", &jerk_freq_factor, py::arg("jerk"), py::arg("n"), py::arg("tsamp"));
  m.def("jerk_check", [](uint64_t n, F64 jf) { jerk_check(n, factors(jf)); }, py::arg("n"), py::arg("jf"));
  m.def(
      "jerk_resample_host",
      [](U8 x, uint64_t nrow, uint64_t n, F64 jf, uint64_t out_stride) {
        PSOUP_CHECK(x.ndim() == 2, "jerk_resample_host: x must be [nrows, row_stride]");
        const int nrows = static_cast<int>(x.shape(0));
        const uint64_t row_stride = static_cast<uint64_t>(x.shape(1));
        const std::vector<double> f = factors(jf);
        check_raw_factors(f, n);
        if (out_stride == 0) out_stride = nrow;
        PSOUP_CHECK(out_stride >= nrow && row_stride >= nrow, "jerk_resample: a stride is shorter than the row");
        py::array_t<uint8_t> y({static_cast<py::ssize_t>(nrows), static_cast<py::ssize_t>(f.size()),
                                static_cast<py::ssize_t>(out_stride)});
        std::memset(y.mutable_data(), 0, static_cast<size_t>(y.size()));
        jerk_resample_host(x.data(), row_stride, nrows, nrow, n, f, y.mutable_data(), out_stride);
        return y;
      },
      py::arg("x"), py::arg("nrow"), py::arg("n"), py::arg("jf"), py::arg("out_stride") = 0);

  py::class_<JerkPlan>(m, "JerkPlan")
      .def(py::init<float, float, float, float, float, uint64_t, float, float, float, AccelConvention>(),
           py::arg("jerk_start"), py::arg("jerk_end"), py::arg("tol"), py::arg("step"), py::arg("pulse_width"),
           py::arg("n"), py::arg("tsamp"), py::arg("cfreq"), py::arg("bw"),
           py::arg("convention") = AccelConvention::Legacy)
      .def("width", &JerkPlan::width)
      .def("step", &JerkPlan::step)
      .def("generate", &JerkPlan::generate)
      .def_property_readonly("span", &JerkPlan::span);

  py::class_<JerkCandidate>(m, "JerkCandidate")
      .def(py::init<>())
      .def(py::init([](const Candidate& c, float jerk) { return JerkCandidate{c, jerk}; }), py::arg("cand"),
           py::arg("jerk"))
      .def_readwrite("cand", &JerkCandidate::cand)
      .def_readwrite("jerk", &JerkCandidate::jerk);
  m.def("jerk_distill", &jerk_distill, py::arg("cands"), py::arg("tobs"), py::arg("span_s"), py::arg("tol"),
        py::arg("keep_related") = true);

  py::class_<JerkSetup>(m, "JerkSetup")
      .def_readonly("nrow", &JerkSetup::nrow)
      .def_readonly("span", &JerkSetup::span)
      .def_readonly("plan", &JerkSetup::plan)
      .def_readonly("jerks", &JerkSetup::jerks)
      .def_readonly("total_trials", &JerkSetup::total_trials)
      .def_property_readonly("dm_list", [](const JerkSetup& s) { return s.search.dm_list; })
      .def_property_readonly("killmask", [](const JerkSetup& s) { return s.search.killmask; })
      .def_property_readonly("fft_size", [](const JerkSetup& s) { return s.search.fft_size; })
      .def_property_readonly("tsamp", [](const JerkSetup& s) { return s.search.search.tsamp; })
      .def_property_readonly("nsamps", [](const JerkSetup& s) { return s.search.nsamps; })
      .def_property_readonly("accel_plan", [](const JerkSetup& s) { return s.search.accel_plan; })
      .def_property_readonly("search_params", [](const JerkSetup& s) { return s.search.search; })
      .def_property_readonly("geometry", [](const JerkSetup& s) {
        return DedispGeometry::make(s.search.header, s.search.nsamps, s.search.dm_list, s.search.killmask);
      });
  // reads the header of args.search.infilename; every refusal is raised here
  m.def("jerk_setup", [](const JerkCmdLineOptions& a) {
    return make_jerk_setup(a, read_header_file(a.search.infilename));
  });

  // ---- the kernel alone: device addresses; jf are the factors on the host (checked here), jf_dev the same K
  // doubles on the device, which the caller keeps alive until the stream has run the kernel
  m.def(
      "jerk_resample_raw",
      [](uintptr_t in, uint64_t row_stride, int nrows, uint64_t nrow, uint64_t n, F64 jf, uintptr_t jf_dev,
         uintptr_t out, uint64_t out_stride, uintptr_t s) {
        const std::vector<double> f = factors(jf);
        check_raw_factors(f, n);
        PSOUP_CHECK(jf_dev != 0 && jf_dev % 8 == 0, "jerk_resample: the device factors must be 8-byte aligned");
        int64_t sp0 = 0, sp1 = 0;
        jerk_stationary(n, &sp0, &sp1);
        kern::jerk_resample(reinterpret_cast<const uint8_t*>(in), row_stride, nrows, nrow, n,
                            reinterpret_cast<const double*>(jf_dev), static_cast<int>(f.size()),
                            reinterpret_cast<uint8_t*>(out), out_stride, sp0, sp1, reinterpret_cast<hipStream_t>(s));
      },
      py::arg("rows"), py::arg("row_stride"), py::arg("nrows"), py::arg("nrow"), py::arg("n"), py::arg("jf"),
      py::arg("jf_dev"), py::arg("out"), py::arg("out_stride"), py::arg("stream") = 0);

  // ---- JerkSearcher over a resident filterbank
  py::class_<JerkSearcher>(m, "JerkSearcher")
      .def(py::init([](const JerkSetup& setup, const DeviceFilterbank& fb, uintptr_t s) {
             return new JerkSearcher(setup, fb, reinterpret_cast<hipStream_t>(s));
           }),
           py::arg("setup"), py::arg("filterbank"), py::arg("stream") = 0, py::keep_alive<1, 2>(),
           py::keep_alive<1, 3>())
      .def("search", &JerkSearcher::search, py::arg("d0") = 0, py::arg("d1") = -1,
           py::call_guard<py::gil_scoped_release>())
      .def("fold",
           [](JerkSearcher& js, JerkCandidateList cands, int npdmp) {
             {
               py::gil_scoped_release nogil;
               js.fold(cands, npdmp);
             }
             return cands;
           },
           py::arg("cands"), py::arg("npdmp"))
      .def_property_readonly("accel_trials", &JerkSearcher::accel_trials)
      .def_property_readonly("jerk_trials", &JerkSearcher::jerk_trials);
  m.def("jerk_global_distill", &jerk_global_distill, py::arg("cands"), py::arg("args"), py::arg("setup"),
        py::call_guard<py::gil_scoped_release>());

  m.def("jerk_output_text", &jerk_output_text);
  m.def("write_jerk_output", &write_jerk_output);
}
