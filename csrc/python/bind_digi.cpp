// pybind11 bindings of fildigi (digi.hpp): options, params, the host steps (no
// GPU needed), the raw reader's checks, Digitiser over a host array, the two
// kernels over raw device addresses with explicit tables, the pipeline.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/digi.hpp"

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
using U32 = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;
using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using I64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using U64 = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;
using F64 = py::array_t<double, py::array::c_style | py::array::forcecast>;

kern::DigiType type_of(int nbits, bool is_signed) {
  PSOUP_CHECK(nbits == 8 || nbits == 16 || nbits == 32, "digi: nbits must be 8, 16 or 32, got " << nbits);
  if (nbits == 32) return kern::DigiType::F32;
  if (nbits == 16) return kern::DigiType::U16;
  return is_signed ? kern::DigiType::I8 : kern::DigiType::U8;
}

py::dict scale_dict(const DigiScale& sc, int nchans) {
  py::dict d;
  const py::ssize_t ni = sc.nint, nc = nchans;
  d["nint"] = sc.nint;
  d["mean"] = as_array(sc.mean, {ni, nc});
  d["gain"] = as_array(sc.gain, {ni, nc});
  d["live"] = as_array(sc.live, {ni, nc});
  d["alive"] = sc.alive;
  d["nlive"] = sc.nlive;
  d["gain_min"] = sc.gain_min;
  d["gain_max"] = sc.gain_max;
  return d;
}

py::dict result_dict(const DigiResult& r) {
  py::dict d = scale_dict(r.scale, r.nchans);
  const py::ssize_t nc = r.nchans, nblk = static_cast<py::ssize_t>(r.nblk);
  d["nsamps"] = r.nsamps;
  d["nchans"] = r.nchans;
  d["nblk"] = r.nblk;
  d["nclip"] = r.nclip;
  d["chunks"] = r.chunks;
  d["flip"] = r.flip;
  d["N"] = as_array(r.N, {nc, nblk});
  d["S1"] = as_array(r.S1, {nc, nblk});
  d["S2"] = as_array(r.S2, {nc, nblk});
  d["E"] = as_array(r.E, {nc, nblk});
  d["nbad"] = as_array(r.nbad, {nc});
  d["killmask"] = r.killmask;
  return d;
}

struct PyDigitiser {
  U8 data;  // keeps the host samples alive
  std::unique_ptr<Digitiser> dig;
  uint64_t nsamps = 0;
  int nchans = 0;
};

}  // namespace

void bind_digi(py::module_& m) {
  py::class_<DigiCmdLineOptions>(m, "DigiCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &DigiCmdLineOptions::infilename)
      .def_readwrite("outfilename", &DigiCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &DigiCmdLineOptions::killfilename)
      .def_readwrite("killoutfilename", &DigiCmdLineOptions::killoutfilename)
      .def_readwrite("sigma_out", &DigiCmdLineOptions::sigma_out)
      .def_readwrite("scale", &DigiCmdLineOptions::scale)
      .def_readwrite("rescale_blocks", &DigiCmdLineOptions::rescale_blocks)
      .def_readwrite("verbose", &DigiCmdLineOptions::verbose);
  m.def("parse_digi_cmdline", [](const std::vector<std::string>& argv) {
    DigiCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_digi_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("digi_stat_block", []() { return kern::kDigiStatBlock; });
  m.def("digi_tile", []() { return kern::kDigiTile; });

  py::class_<DigiParams>(m, "DigiParams")
      .def(py::init<>())
      .def(py::init([](double sigma_out, const std::string& scale, int rescale_blocks) {
             DigiParams p;
             p.sigma_out = sigma_out;
             PSOUP_CHECK(scale == "channel" || scale == "file", "digi: scale must be channel or file, got " << scale);
             p.scale = scale == "file" ? DigiScaleMode::File : DigiScaleMode::Channel;
             p.rescale_blocks = rescale_blocks;
             return p;
           }),
           py::arg("sigma_out") = 16.0, py::arg("scale") = "channel", py::arg("rescale_blocks") = 0)
      .def_readwrite("sigma_out", &DigiParams::sigma_out)
      .def_readwrite("rescale_blocks", &DigiParams::rescale_blocks)
      .def_property_readonly("scale",
                             [](const DigiParams& p) { return p.scale == DigiScaleMode::File ? "file" : "channel"; });
  m.def("digi_params_from", &digi_params_from);
  m.def("digi_check_params", &digi_check_params);
  m.def(
      "digi_check_header",
      [](int nbits, int is_signed, int nifs, double foff, int nchans) {
        return static_cast<int>(digi_check_header(nbits, is_signed, nifs, foff, nchans));
      },
      py::arg("nbits"), py::arg("signed"), py::arg("nifs"), py::arg("foff"), py::arg("nchans"));

  // ---- the host steps (no GPU)
  m.def(
      "digi_scale",
      [](U32 N, I64 S1, U64 S2, I32 E, const std::vector<int>& killmask, const DigiParams& p) {
        PSOUP_CHECK(N.ndim() == 2 && S1.ndim() == 2 && S2.ndim() == 2 && E.ndim() == 2,
                    "digi_scale: N, S1, S2 and E must be [nchans, nblk]");
        const int nchans = static_cast<int>(N.shape(0));
        return scale_dict(digi_scale(to_vector(N), to_vector(S1), to_vector(S2), to_vector(E), nchans,
                                     static_cast<uint64_t>(N.shape(1)), killmask, p),
                          nchans);
      },
      py::arg("N"), py::arg("S1"), py::arg("S2"), py::arg("E"), py::arg("killmask"), py::arg("params"));
  m.def(
      "digi_band",
      [](double fch1, double foff, int nchans) {
        const DigiBand b = digi_band(fch1, foff, nchans);
        return py::make_tuple(b.flip, b.fch1, b.foff);
      },
      py::arg("fch1"), py::arg("foff"), py::arg("nchans"));
  m.def("read_raw_filterbank_info", [](const std::string& f) {
    const RawFilterbank fb = RawFilterbank::from_file(f);
    py::dict d;
    d["nsamps"] = fb.nsamps();
    d["nchans"] = fb.nchans();
    d["type"] = static_cast<int>(fb.type());
    d["bytes_per_sample"] = fb.bytes_per_sample();
    return d;
  });

  // ---- Digitiser: the samples are a host array (the file), y comes back as one
  py::class_<PyDigitiser>(m, "Digitiser")
      .def(py::init([](U8 data, int nbits, bool is_signed, uint64_t nsamps, int nchans, double foff,
                       const std::vector<int>& killmask, const DigiParams& p, uintptr_t stream, size_t budget_bytes) {
             const kern::DigiType t = type_of(nbits, is_signed);
             PSOUP_CHECK(nchans >= 1, "digi: no channels");
             PSOUP_CHECK(static_cast<uint64_t>(data.size()) >=
                             nsamps * static_cast<uint64_t>(nchans) * static_cast<uint64_t>(kern::digi_type_bytes(t)),
                         "digi: the array is smaller than nsamps x nchans samples");
             auto d = std::make_unique<PyDigitiser>();
             d->data = data;
             d->nsamps = nsamps;
             d->nchans = nchans;
             d->dig = std::make_unique<Digitiser>(nsamps ? data.data() : nullptr, t, nsamps, nchans, foff, killmask, p,
                                                  reinterpret_cast<hipStream_t>(stream), budget_bytes);
             return d;
           }),
           py::arg("data"), py::arg("nbits"), py::arg("signed"), py::arg("nsamps"), py::arg("nchans"), py::arg("foff"),
           py::arg("killmask"), py::arg("params"), py::arg("stream") = 0,
           py::arg("budget_bytes") = Digitiser::kDefaultBudgetBytes)
      .def("run",
           [](PyDigitiser& d) {
             py::array_t<uint8_t> y({static_cast<py::ssize_t>(d.nsamps), static_cast<py::ssize_t>(d.nchans)});
             DigiResult r;
             {
               uint8_t* out = y.mutable_data();
               py::gil_scoped_release nogil;
               r = d.dig->run(out);
             }
             return py::make_tuple(y, result_dict(r));
           })
      .def_property_readonly("chunk_samples", [](const PyDigitiser& d) { return d.dig->chunk_samples(); })
      .def_property_readonly("launches", [](const PyDigitiser& d) { return d.dig->launches(); });

  // ---- x / y / N / S1 / S2 / E: device addresses
  m.def("digi_block_sums_raw", [](uintptr_t x, int nbits, bool is_signed, uint64_t nsamps, int nchans, uintptr_t N,
                                  uintptr_t S1, uintptr_t S2, uintptr_t E, uintptr_t s) {
    const kern::DigiType t = type_of(nbits, is_signed);
    py::gil_scoped_release nogil;
    Digitiser::sums(reinterpret_cast<const void*>(x), t, nsamps, nchans, reinterpret_cast<uint32_t*>(N),
                    reinterpret_cast<int64_t*>(S1), reinterpret_cast<uint64_t*>(S2), reinterpret_cast<int32_t*>(E),
                    reinterpret_cast<hipStream_t>(s));
  });
  m.def("digi_quant_raw", [](uintptr_t x, int nbits, bool is_signed, uint64_t nsamps, int nchans, int J, F64 mean,
                             F64 gain, bool flip, uintptr_t y, uintptr_t s) {
    const kern::DigiType t = type_of(nbits, is_signed);
    const std::vector<double> mv = to_vector(mean), gv = to_vector(gain);
    py::gil_scoped_release nogil;
    return Digitiser::quant(reinterpret_cast<const void*>(x), t, nsamps, nchans, J, mv, gv, flip,
                            reinterpret_cast<uint8_t*>(y), reinterpret_cast<hipStream_t>(s));
  });

  m.def("run_digi_pipeline", [](const DigiCmdLineOptions& a) {
    DigiRun run;
    {
      py::gil_scoped_release nogil;
      run = run_digi_pipeline(a);
    }
    py::dict d = result_dict(run.result);
    d["timers"] = run.timers;
    return d;
  });
}
