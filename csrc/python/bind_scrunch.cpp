// pybind11 bindings of filscrunch (scrunch.hpp): options, params, the host
// steps (no GPU needed), Scruncher over raw device addresses, the two kernels
// with explicit tables, the pipeline.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/scrunch.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

template <class T>
py::array_t<T> as_array(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

template <class T>
std::vector<T> to_vector(const py::array_t<T, py::array::c_style | py::array::forcecast>& a) {
  return std::vector<T>(a.data(), a.data() + a.size());
}

using U8 = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using U64 = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;

py::dict scale_dict(const ScrunchScale& sc) {
  py::dict d;
  const py::ssize_t ns = static_cast<py::ssize_t>(sc.M.size());
  d["M"] = as_array(sc.M, {ns});
  d["live"] = as_array(sc.live, {ns});
  d["mul"] = sc.mul;
  d["sigma_ref"] = sc.sigma_ref;
  d["nlive"] = sc.nlive;
  return d;
}

py::dict result_dict(const ScrunchResult& r) {
  py::dict d = scale_dict(r.scale);
  const py::ssize_t ns = r.nsub, nblk = static_cast<py::ssize_t>(r.nblk);
  d["nout"] = r.nout;
  d["nblk"] = r.nblk;
  d["R"] = r.R;
  d["nsub"] = r.nsub;
  d["chunks"] = r.chunks;
  d["rel"] = as_array(r.rel, {static_cast<py::ssize_t>(r.rel.size())});
  d["nactive"] = as_array(r.nactive, {ns});
  d["S1"] = as_array(r.S1, {ns, nblk});
  d["S2"] = as_array(r.S2, {ns, nblk});
  d["killmask"] = r.killmask;
  return d;
}

}  // namespace

void bind_scrunch(py::module_& m) {
  py::class_<ScrunchCmdLineOptions>(m, "ScrunchCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &ScrunchCmdLineOptions::infilename)
      .def_readwrite("outfilename", &ScrunchCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &ScrunchCmdLineOptions::killfilename)
      .def_readwrite("killoutfilename", &ScrunchCmdLineOptions::killoutfilename)
      .def_readwrite("dm", &ScrunchCmdLineOptions::dm)
      .def_readwrite("nsub", &ScrunchCmdLineOptions::nsub)
      .def_readwrite("tscrunch", &ScrunchCmdLineOptions::tscrunch)
      .def_readwrite("sigma_out", &ScrunchCmdLineOptions::sigma_out)
      .def_readwrite("plan", &ScrunchCmdLineOptions::plan)
      .def_readwrite("dm_end", &ScrunchCmdLineOptions::dm_end)
      .def_readwrite("verbose", &ScrunchCmdLineOptions::verbose);
  m.def("parse_scrunch_cmdline", [](const std::vector<std::string>& argv) {
    ScrunchCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_scrunch_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("scrunch_params_from", &scrunch_params_from);
  m.def("scrunch_check_params", &scrunch_check_params, py::arg("params"), py::arg("nchans"));
  m.def("scrunch_tile", []() { return kern::kScrunchTile; });
  m.def("scrunch_tile_at", &kern::scrunch_tile, py::arg("tscrunch"));
  m.def("scrunch_stat_block", []() { return kern::kScrunchStatBlock; });

  py::class_<ScrunchParams>(m, "ScrunchParams")
      .def(py::init<>())
      .def(py::init([](float dm, int nsub, int tscrunch, double sigma_out) {
             ScrunchParams p;
             p.dm = dm;
             p.nsub = nsub;
             p.tscrunch = tscrunch;
             p.sigma_out = sigma_out;
             return p;
           }),
           py::arg("dm") = 0.f, py::arg("nsub") = 0, py::arg("tscrunch") = 1, py::arg("sigma_out") = 16.0)
      .def_readwrite("dm", &ScrunchParams::dm)
      .def_readwrite("nsub", &ScrunchParams::nsub)
      .def_readwrite("tscrunch", &ScrunchParams::tscrunch)
      .def_readwrite("sigma_out", &ScrunchParams::sigma_out);

  // ---- the host steps (no GPU)
  m.def(
      "scrunch_offsets",
      [](float dm, const std::vector<float>& delays, int nsub) {
        const ScrunchOffsets o = scrunch_offsets(dm, delays, nsub);
        return py::make_tuple(as_array(o.rel, {static_cast<py::ssize_t>(o.rel.size())}), o.R);
      },
      py::arg("dm"), py::arg("delays"), py::arg("nsub"));
  m.def(
      "scrunch_scale",
      [](U64 S1, U64 S2, uint64_t nout, I32 nactive, double sigma_out) {
        PSOUP_CHECK(S1.ndim() == 2 && S2.ndim() == 2 && S1.shape(0) == S2.shape(0) && S1.shape(1) == S2.shape(1),
                    "scrunch_scale: S1 and S2 must be [nsub, nblk]");
        return scale_dict(
            scrunch_scale(to_vector(S1), to_vector(S2), static_cast<int>(S1.shape(0)), nout, to_vector(nactive), sigma_out));
      },
      py::arg("S1"), py::arg("S2"), py::arg("nout"), py::arg("nactive"), py::arg("sigma_out") = 16.0);
  m.def(
      "scrunch_plan",
      [](double tsamp, double fch1, double foff, int nchans, double dm_end) {
        py::list out;
        for (const ScrunchTier& t : scrunch_plan(tsamp, fch1, foff, nchans, dm_end))
          out.append(py::make_tuple(t.dm_lo, t.dm_hi, t.tscrunch));
        return out;
      },
      py::arg("tsamp"), py::arg("fch1"), py::arg("foff"), py::arg("nchans"), py::arg("dm_end"));

  // ---- rows / y / A / S1 / S2: device addresses
  py::class_<Scruncher>(m, "Scruncher")
      .def(py::init([](uintptr_t rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias, double foff,
                       const std::vector<float>& delays, const std::vector<int>& killmask, const ScrunchParams& p,
                       uintptr_t stream, size_t budget_bytes) {
             return new Scruncher(reinterpret_cast<const int8_t*>(rows), stride, nsamps, nchans, nbits, bias, foff,
                                  delays, killmask, p, reinterpret_cast<hipStream_t>(stream), budget_bytes);
           }),
           py::arg("rows"), py::arg("stride"), py::arg("nsamps"), py::arg("nchans"), py::arg("nbits"), py::arg("bias"),
           py::arg("foff"), py::arg("delays"), py::arg("killmask"), py::arg("params"), py::arg("stream") = 0,
           py::arg("budget_bytes") = Scruncher::kDefaultBudgetBytes)
      .def(
          "run",
          [](Scruncher& s, uintptr_t y, uint64_t y_stride) {
            ScrunchResult r;
            {
              py::gil_scoped_release nogil;
              r = s.run(reinterpret_cast<int8_t*>(y), y_stride);
            }
            return result_dict(r);
          },
          py::arg("y"), py::arg("y_stride"))
      .def_property_readonly("nout", &Scruncher::nout)
      .def_property_readonly("nsub", &Scruncher::nsub)
      .def_property_readonly("chunk_outputs", &Scruncher::chunk_outputs)
      .def_property_readonly("launches", &Scruncher::launches)
      .def_property_readonly("nactive", [](const Scruncher& s) {
        return as_array(s.nactive(), {static_cast<py::ssize_t>(s.nactive().size())});
      });
  m.def(
      "scrunch_sums_raw",
      [](uintptr_t rows, uint64_t stride, uint64_t nsamps, int nchans, int bias, int f, int nsub, I32 rel,
         const std::vector<int>& killmask, uint64_t nout, uintptr_t A, uint64_t a_stride, uintptr_t S1, uintptr_t S2,
         uintptr_t s) {
        const std::vector<int32_t> r = to_vector(rel);
        py::gil_scoped_release nogil;
        Scruncher::sums(reinterpret_cast<const int8_t*>(rows), stride, nsamps, nchans, bias, f, nsub, r, killmask, nout,
                        reinterpret_cast<int32_t*>(A), a_stride, reinterpret_cast<uint64_t*>(S1),
                        reinterpret_cast<uint64_t*>(S2), reinterpret_cast<hipStream_t>(s));
      });
  m.def("scrunch_quant_raw", [](uintptr_t A, uint64_t a_stride, int nsub, uint64_t nout, I32 M, U8 live, int32_t mul,
                                uintptr_t y, uint64_t y_stride, uintptr_t s) {
    const std::vector<int32_t> mv = to_vector(M);
    const std::vector<uint8_t> lv = to_vector(live);
    py::gil_scoped_release nogil;
    Scruncher::quant(reinterpret_cast<const int32_t*>(A), a_stride, nsub, nout, mv, lv, mul,
                     reinterpret_cast<int8_t*>(y), y_stride, reinterpret_cast<hipStream_t>(s));
  });

  m.def("run_scrunch_pipeline", [](const ScrunchCmdLineOptions& a) {
    ScrunchRun run;
    {
      py::gil_scoped_release nogil;
      run = run_scrunch_pipeline(a);
    }
    py::dict d = result_dict(run.result);
    d["timers"] = run.timers;
    return d;
  });
}
