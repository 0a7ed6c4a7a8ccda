// pybind11 bindings of the single-pulse search (singlepulse.hpp): options,
// params, candidates, clustering, engine, pipeline, and a self-contained
// kernel driver for numerics tests.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "psoup/common.hpp"
#include "psoup/singlepulse.hpp"

namespace py = pybind11;
using namespace psoup;

void bind_sp(py::module_& m) {
  py::class_<SpCmdLineOptions>(m, "SpCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &SpCmdLineOptions::infilename)
      .def_readwrite("outfilename", &SpCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &SpCmdLineOptions::killfilename)
      .def_readwrite("max_num_threads", &SpCmdLineOptions::max_num_threads)
      .def_readwrite("dm_start", &SpCmdLineOptions::dm_start)
      .def_readwrite("dm_end", &SpCmdLineOptions::dm_end)
      .def_readwrite("dm_tol", &SpCmdLineOptions::dm_tol)
      .def_readwrite("dm_pulse_width", &SpCmdLineOptions::dm_pulse_width)
      .def_readwrite("verbose", &SpCmdLineOptions::verbose)
      .def_readwrite("progress_bar", &SpCmdLineOptions::progress_bar)
      .def_readwrite("min_snr", &SpCmdLineOptions::min_snr)
      .def_readwrite("boxcar_max", &SpCmdLineOptions::boxcar_max)
      .def_readwrite("baseline", &SpCmdLineOptions::baseline)
      .def_readwrite("limit", &SpCmdLineOptions::limit)
      .def_readwrite("dedisp_kernel", &SpCmdLineOptions::dedisp_kernel)
      .def_readwrite("rfi", &SpCmdLineOptions::rfi)
      .def_readwrite("zero_dm", &SpCmdLineOptions::zero_dm)
      .def_readwrite("rfi_block", &SpCmdLineOptions::rfi_block)
      .def_readwrite("rfi_thresh", &SpCmdLineOptions::rfi_thresh)
      .def_readwrite("rfi_chan_frac", &SpCmdLineOptions::rfi_chan_frac)
      .def_readwrite("rfi_block_frac", &SpCmdLineOptions::rfi_block_frac)
      .def_readwrite("rfi_maskfilename", &SpCmdLineOptions::rfi_maskfilename);
  m.def("sp_rfi_params", &sp_rfi_params);
  m.def("parse_sp_cmdline", [](const std::vector<std::string>& argv) {
    SpCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_sp_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("default_sp_output_filename", &default_sp_output_filename);

  py::class_<SpParams>(m, "SpParams")
      .def(py::init<>())
      .def_readwrite("tsamp", &SpParams::tsamp)
      .def_readwrite("min_snr", &SpParams::min_snr)
      .def_readwrite("boxcar_max", &SpParams::boxcar_max)
      .def_readwrite("baseline_s", &SpParams::baseline_s)
      .def_readwrite("baseline_samples", &SpParams::baseline_samples)
      .def_readwrite("capacity", &SpParams::capacity);
  m.def("sp_params_from", &sp_params_from);

  py::class_<SpEvent>(m, "SpEvent")
      .def(py::init<>())
      .def(py::init([](uint32_t sample, int32_t width_log2, float snr, int32_t dm_idx) {
             return SpEvent{sample, width_log2, snr, dm_idx};
           }),
           py::arg("sample"), py::arg("width_log2"), py::arg("snr"), py::arg("dm_idx"))
      .def_readwrite("sample", &SpEvent::sample)
      .def_readwrite("width_log2", &SpEvent::width_log2)
      .def_readwrite("snr", &SpEvent::snr)
      .def_readwrite("dm_idx", &SpEvent::dm_idx)
      .def("astuple", [](const SpEvent& e) { return py::make_tuple(e.dm_idx, e.width_log2, e.sample, e.snr); });

  py::class_<SpCandidate>(m, "SpCandidate")
      .def(py::init<>())
      .def_readwrite("sample", &SpCandidate::sample)
      .def_readwrite("time_s", &SpCandidate::time_s)
      .def_readwrite("width", &SpCandidate::width)
      .def_readwrite("snr", &SpCandidate::snr)
      .def_readwrite("dm", &SpCandidate::dm)
      .def_readwrite("dm_idx", &SpCandidate::dm_idx)
      .def_readwrite("members", &SpCandidate::members)
      .def_readwrite("first_sample", &SpCandidate::first_sample)
      .def_readwrite("last_sample", &SpCandidate::last_sample)
      .def_readwrite("dm_idx_lo", &SpCandidate::dm_idx_lo)
      .def_readwrite("dm_idx_hi", &SpCandidate::dm_idx_hi);

  m.def("sp_widths", &sp_widths);
  m.def("sp_baseline_samples", &sp_baseline_samples);
  m.def("sp_cluster", &sp_cluster, py::arg("events"), py::arg("dm_list"), py::arg("band_delay_per_dm"),
        py::arg("tsamp"));
  m.attr("SP_TILE") = kern::kSpTile;
  m.attr("SP_BLOCK") = kern::kSpBlock;
  m.attr("SP_MAX_LOG2") = kern::kSpMaxLog2;

  py::class_<SinglePulseEngine>(m, "SinglePulseEngine")
      .def(py::init([](const SpParams& p, uint64_t nsamps, uintptr_t stream) {
             return new SinglePulseEngine(p, nsamps, reinterpret_cast<hipStream_t>(stream));
           }),
           py::arg("params"), py::arg("nsamps"), py::arg("stream") = 0)
      .def(
          "search_block",
          [](SinglePulseEngine& e, uintptr_t rows, uint64_t row_stride, int ndm, int dm_idx0, uintptr_t best_snr,
             uintptr_t best_arg) {
            py::gil_scoped_release nogil;
            return e.search_block(reinterpret_cast<const uint8_t*>(rows), row_stride, ndm, dm_idx0,
                                  reinterpret_cast<float*>(best_snr), reinterpret_cast<uint32_t*>(best_arg));
          },
          py::arg("rows"), py::arg("row_stride"), py::arg("ndm"), py::arg("dm_idx0") = 0, py::arg("best_snr") = 0,
          py::arg("best_arg") = 0)
      .def_property_readonly("nsamps", &SinglePulseEngine::nsamps)
      .def_property_readonly("baseline", &SinglePulseEngine::baseline)
      .def_property_readonly("widths", &SinglePulseEngine::widths)
      .def_property_readonly("events", &SinglePulseEngine::events)
      .def_property_readonly("reruns", &SinglePulseEngine::reruns);

  py::class_<SpResult>(m, "SpResult")
      .def(py::init<>())
      .def_readwrite("candidates", &SpResult::candidates)
      .def_readwrite("dm_list", &SpResult::dm_list)
      .def_readwrite("devices", &SpResult::devices)
      .def_readwrite("timers", &SpResult::timers)
      .def_readwrite("nsamps", &SpResult::nsamps)
      .def_readwrite("tsamp", &SpResult::tsamp)
      .def_readwrite("widths", &SpResult::widths)
      .def_readwrite("baseline", &SpResult::baseline)
      .def_readwrite("events", &SpResult::events)
      .def_readwrite("reruns", &SpResult::reruns)
      .def_readwrite("rfi_comment", &SpResult::rfi_comment);
  m.def("run_sp_pipeline", [](const SpCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_sp_pipeline(a);
  });
  m.def("write_sp_output", &write_sp_output);

  // Kernel driver for tests: uploads host rows [ndm, stride] (nsamps samples
  // used of each), searches them as one block on the current device and
  // returns (events, reruns, best_snr, best_arg); the dense arrays
  // [ndm, K + 1, ceil(nsamps / 64)] are None unless dense.
  m.def(
      "sp_search_rows",
      [](py::array_t<uint8_t, py::array::c_style> rows, uint64_t nsamps, const SpParams& params, bool dense,
         int dm_idx0) -> py::tuple {
        PSOUP_CHECK(rows.ndim() == 2, "sp_search_rows: rows must be [ndm, stride]");
        const int ndm = static_cast<int>(rows.shape(0));
        const uint64_t stride = static_cast<uint64_t>(rows.shape(1));
        PSOUP_CHECK(ndm > 0 && stride >= nsamps, "sp_search_rows: stride shorter than nsamps");
        DeviceBuffer<uint8_t> d_rows(static_cast<size_t>(ndm) * stride);
        PSOUP_HIP_CHECK(hipMemcpy(d_rows.data(), rows.data(), d_rows.bytes(), hipMemcpyHostToDevice));
        SinglePulseEngine eng(params, nsamps, nullptr);
        const size_t nk = eng.widths().size(), nb = (nsamps + kern::kSpBlock - 1) / kern::kSpBlock;
        DeviceBuffer<float> d_snr;
        DeviceBuffer<uint32_t> d_arg;
        if (dense) {
          d_snr.resize(ndm * nk * nb);
          d_arg.resize(ndm * nk * nb);
        }
        std::vector<SpEvent> ev =
            eng.search_block(d_rows.data(), stride, ndm, dm_idx0, dense ? d_snr.data() : nullptr,
                             dense ? d_arg.data() : nullptr);
        py::object o_snr = py::none(), o_arg = py::none();
        if (dense) {
          py::array_t<float> a_snr({static_cast<size_t>(ndm), nk, nb});
          py::array_t<uint32_t> a_arg({static_cast<size_t>(ndm), nk, nb});
          PSOUP_HIP_CHECK(hipMemcpy(a_snr.mutable_data(), d_snr.data(), d_snr.bytes(), hipMemcpyDeviceToHost));
          PSOUP_HIP_CHECK(hipMemcpy(a_arg.mutable_data(), d_arg.data(), d_arg.bytes(), hipMemcpyDeviceToHost));
          o_snr = a_snr;
          o_arg = a_arg;
        }
        return py::make_tuple(ev, eng.reruns(), o_snr, o_arg);
      },
      py::arg("rows"), py::arg("nsamps"), py::arg("params"), py::arg("dense") = true, py::arg("dm_idx0") = 0);

  // Trend and sigma driver for tests: the two launches that precede the
  // search, on host rows [ndm, stride].  Returns (means float32 [ndm, nblk],
  // partials float64 [ndm, kSpSigmaParts]): the trend block means and the
  // partial sums of (u - trend)^2, neither of which leaves the engine.
  m.def(
      "sp_trend_sigma_rows",
      [](py::array_t<uint8_t, py::array::c_style> rows, uint64_t nsamps, uint64_t baseline_samples) -> py::tuple {
        PSOUP_CHECK(rows.ndim() == 2, "sp_trend_sigma_rows: rows must be [ndm, stride]");
        const int ndm = static_cast<int>(rows.shape(0));
        const uint64_t stride = static_cast<uint64_t>(rows.shape(1));
        PSOUP_CHECK(ndm > 0 && stride >= nsamps, "sp_trend_sigma_rows: stride shorter than nsamps");
        PSOUP_CHECK(baseline_samples > 0 && baseline_samples <= nsamps, "sp_trend_sigma_rows: trend block length");
        const size_t nblk = (nsamps + baseline_samples - 1) / baseline_samples;
        DeviceBuffer<uint8_t> d_rows(static_cast<size_t>(ndm) * stride);
        PSOUP_HIP_CHECK(hipMemcpy(d_rows.data(), rows.data(), d_rows.bytes(), hipMemcpyHostToDevice));
        DeviceBuffer<float> d_means(static_cast<size_t>(ndm) * nblk);
        DeviceBuffer<double> d_part(static_cast<size_t>(ndm) * kern::kSpSigmaParts);
        kern::sp_block_means(d_rows.data(), stride, ndm, nsamps, baseline_samples, d_means.data(), nullptr);
        kern::sp_sigma(d_rows.data(), stride, ndm, nsamps, baseline_samples, d_means.data(), d_part.data(), nullptr);
        PSOUP_HIP_CHECK(hipStreamSynchronize(nullptr));
        py::array_t<float> a_means({static_cast<size_t>(ndm), nblk});
        py::array_t<double> a_part({static_cast<size_t>(ndm), static_cast<size_t>(kern::kSpSigmaParts)});
        PSOUP_HIP_CHECK(hipMemcpy(a_means.mutable_data(), d_means.data(), d_means.bytes(), hipMemcpyDeviceToHost));
        PSOUP_HIP_CHECK(hipMemcpy(a_part.mutable_data(), d_part.data(), d_part.bytes(), hipMemcpyDeviceToHost));
        return py::make_tuple(a_means, a_part);
      },
      py::arg("rows"), py::arg("nsamps"), py::arg("baseline_samples"));
}
