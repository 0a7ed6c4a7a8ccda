// pybind11 bindings of filinject (inject.hpp): options, signals, the host steps
// (no GPU needed), Injector over a host array, the kernel alone over a raw
// device address with explicit tables, the pipeline.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/inject.hpp"

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
using U16 = py::array_t<uint16_t, py::array::c_style | py::array::forcecast>;
using U32 = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;
using U64 = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;
using F64 = py::array_t<double, py::array::c_style | py::array::forcecast>;

InjectGeometry geometry(int nchans, int nbits, uint64_t nsamps, double tsamp, double fch1, double foff) {
  InjectGeometry g;
  g.nchans = nchans;
  g.nbits = nbits;
  g.nsamps = nsamps;
  g.tsamp = tsamp;
  g.fch1 = fch1;
  g.foff = foff;
  return g;
}

py::dict tables_dict(const InjectTables& t) {
  py::dict d;
  const py::ssize_t ns = t.nsig, nc = t.nchans;
  d["nsig"] = t.nsig;
  d["nchans"] = t.nchans;
  d["tsamp"] = t.tsamp;
  d["nlive"] = t.nlive;
  d["sigc"] = as_array(t.sigc, {ns, static_cast<py::ssize_t>(kern::kInjectSigDoubles)});
  d["delay"] = as_array(t.delay, {ns, nc});
  d["inv_w"] = as_array(t.inv_w, {ns, nc});
  d["w"] = as_array(t.w, {ns, nc});
  d["A_q"] = as_array(t.A_q, {ns, nc});
  d["T"] = as_array(t.T, {static_cast<py::ssize_t>(t.T.size())});
  return d;
}

InjectTables tables_from(F64 sigc, double tsamp, F64 delay, F64 inv_w, U32 A_q, U16 T) {
  PSOUP_CHECK(sigc.ndim() == 2 && delay.ndim() == 2 && inv_w.ndim() == 2 && A_q.ndim() == 2 && T.ndim() == 1,
              "inject: sigc [nsig, 4], delay, inv_w and A_q [nsig, nchans], T [1537]");
  InjectTables t;
  t.nsig = static_cast<int>(delay.shape(0));
  t.nchans = static_cast<int>(delay.shape(1));
  t.tsamp = tsamp;
  t.sigc = to_vector(sigc);
  t.delay = to_vector(delay);
  t.inv_w = to_vector(inv_w);
  t.A_q = to_vector(A_q);
  t.T = to_vector(T);
  return t;
}

py::list truth_list(const std::vector<InjectTruth>& tr) {
  py::list l;
  for (const InjectTruth& t : tr) l.append(py::make_tuple(t.npulses, t.peak, t.snr));
  return l;
}

py::dict result_dict(const InjectResult& r) {
  py::dict d = tables_dict(r.tables);
  d["nsamps"] = r.nsamps;
  d["nclip"] = r.nclip;
  d["chunks"] = r.chunks;
  d["sigma"] = as_array(r.sigma, {static_cast<py::ssize_t>(r.sigma.size())});
  d["touched"] = as_array(r.touched, {static_cast<py::ssize_t>(r.touched.size())});
  d["truth"] = truth_list(r.truth);
  return d;
}

struct PyInjector {
  U8 data;  // keeps the host bytes alive
  std::unique_ptr<Injector> inj;
  size_t bytes = 0;
};

}  // namespace

void bind_inject(py::module_& m) {
  py::class_<InjectCmdLineOptions>(m, "InjectCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &InjectCmdLineOptions::infilename)
      .def_readwrite("outfilename", &InjectCmdLineOptions::outfilename)
      .def_readwrite("injfilename", &InjectCmdLineOptions::injfilename)
      .def_readwrite("killfilename", &InjectCmdLineOptions::killfilename)
      .def_readwrite("truthfilename", &InjectCmdLineOptions::truthfilename)
      .def_readwrite("seed", &InjectCmdLineOptions::seed)
      .def_readwrite("units", &InjectCmdLineOptions::units)
      .def_readwrite("no_smear", &InjectCmdLineOptions::no_smear)
      .def_readwrite("verbose", &InjectCmdLineOptions::verbose);
  m.def("parse_inject_cmdline", [](const std::vector<std::string>& argv) {
    InjectCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_inject_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("inject_stat_block", []() { return kern::kInjectStatBlock; });
  m.def("inject_tile", []() { return kern::kInjectTile; });
  m.def("inject_max_signals", []() { return kern::kInjectMaxSignals; });

  py::class_<InjectSignal>(m, "InjectSignal")
      .def(py::init([](const std::string& kind, double t, double dm, double amp, double width, double acc,
                       double phase, double alpha) {
             PSOUP_CHECK(kind == "pulsar" || kind == "burst", "inject: unknown kind '" << kind << "' (pulsar or burst)");
             InjectSignal s;
             s.kind = kind == "burst" ? InjectKind::Burst : InjectKind::Pulsar;
             s.t = t;
             s.dm = dm;
             s.amp = amp;
             s.width = width;
             s.acc = acc;
             s.phase = phase;
             s.alpha = alpha;
             return s;
           }),
           py::arg("kind"), py::arg("t"), py::arg("dm"), py::arg("amp"), py::arg("width"), py::arg("acc") = 0.0,
           py::arg("phase") = 0.0, py::arg("alpha") = 0.0)
      .def_property_readonly("kind",
                             [](const InjectSignal& s) { return s.kind == InjectKind::Burst ? "burst" : "pulsar"; })
      .def_readwrite("t", &InjectSignal::t)
      .def_readwrite("dm", &InjectSignal::dm)
      .def_readwrite("amp", &InjectSignal::amp)
      .def_readwrite("width", &InjectSignal::width)
      .def_readwrite("acc", &InjectSignal::acc)
      .def_readwrite("phase", &InjectSignal::phase)
      .def_readwrite("alpha", &InjectSignal::alpha);

  // ---- the host steps (no GPU)
  m.def("inject_check_signals", &inject_check_signals);
  m.def("inject_parse", &inject_parse);
  m.def("inject_read_file", &inject_read_file);
  m.def("inject_check_geometry", [](int nchans, int nbits, uint64_t nsamps, double tsamp, double fch1, double foff) {
    inject_check_geometry(geometry(nchans, nbits, nsamps, tsamp, fch1, foff));
  });
  m.def("inject_hash", &inject_hash, py::arg("seed"), py::arg("c"), py::arg("t"));
  m.def("inject_profile_table", []() {
    const std::vector<uint16_t> T = inject_profile_table();
    return as_array(T, {static_cast<py::ssize_t>(T.size())});
  });
  m.def(
      "inject_sigma",
      [](U64 S1, U64 S2, uint64_t nsamps) {
        PSOUP_CHECK(S1.ndim() == 2 && S2.ndim() == 2, "inject_sigma: S1 and S2 must be [nchans, nblk]");
        const int nchans = static_cast<int>(S1.shape(0));
        const std::vector<double> s = inject_sigma(to_vector(S1), to_vector(S2), nchans, nsamps);
        return as_array(s, {static_cast<py::ssize_t>(s.size())});
      },
      py::arg("S1"), py::arg("S2"), py::arg("nsamps"));
  m.def(
      "inject_tables",
      [](const std::vector<InjectSignal>& signals, int nchans, int nbits, uint64_t nsamps, double tsamp, double fch1,
         double foff, F64 unit, bool smear) {
        return tables_dict(
            inject_tables(signals, geometry(nchans, nbits, nsamps, tsamp, fch1, foff), to_vector(unit), smear));
      },
      py::arg("signals"), py::arg("nchans"), py::arg("nbits"), py::arg("nsamps"), py::arg("tsamp"), py::arg("fch1"),
      py::arg("foff"), py::arg("unit"), py::arg("smear") = true);
  m.def(
      "inject_truth",
      [](const std::vector<InjectSignal>& signals, int nchans, int nbits, uint64_t nsamps, double tsamp, double fch1,
         double foff, F64 unit, F64 sigma, bool smear) {
        const InjectGeometry g = geometry(nchans, nbits, nsamps, tsamp, fch1, foff);
        const std::vector<double> u = to_vector(unit);
        const InjectTables t = inject_tables(signals, g, u, smear);
        return truth_list(inject_truth(signals, t, g, u, to_vector(sigma)));
      },
      py::arg("signals"), py::arg("nchans"), py::arg("nbits"), py::arg("nsamps"), py::arg("tsamp"), py::arg("fch1"),
      py::arg("foff"), py::arg("unit"), py::arg("sigma"), py::arg("smear") = true);

  // ---- Injector: the packed bytes are a host array (the file's data block)
  py::class_<PyInjector>(m, "Injector")
      .def(py::init([](U8 data, int nchans, int nbits, uint64_t nsamps, double tsamp, double fch1, double foff,
                       const std::vector<InjectSignal>& signals, const std::vector<int>& killmask, bool sigma_units,
                       bool smear, uint64_t seed, uintptr_t stream, size_t budget_bytes) {
             const InjectGeometry g = geometry(nchans, nbits, nsamps, tsamp, fch1, foff);
             inject_check_geometry(g);
             const size_t bytes = static_cast<size_t>(nsamps) * static_cast<size_t>(nchans) *
                                  static_cast<size_t>(nbits) / 8;
             PSOUP_CHECK(static_cast<size_t>(data.size()) >= bytes, "inject: the array is smaller than the data block");
             auto d = std::make_unique<PyInjector>();
             d->data = data;
             d->bytes = bytes;
             d->inj = std::make_unique<Injector>(data.data(), g, signals, killmask, sigma_units, smear, seed,
                                                 reinterpret_cast<hipStream_t>(stream), budget_bytes);
             return d;
           }),
           py::arg("data"), py::arg("nchans"), py::arg("nbits"), py::arg("nsamps"), py::arg("tsamp"), py::arg("fch1"),
           py::arg("foff"), py::arg("signals"), py::arg("killmask"), py::arg("sigma_units") = true,
           py::arg("smear") = true, py::arg("seed") = 0, py::arg("stream") = 0,
           py::arg("budget_bytes") = Injector::kDefaultBudgetBytes)
      .def("run",
           [](PyInjector& d) {
             py::array_t<uint8_t> y({static_cast<py::ssize_t>(d.bytes)});
             InjectResult r;
             {
               uint8_t* out = y.mutable_data();
               py::gil_scoped_release nogil;
               r = d.inj->run(out);
             }
             return py::make_tuple(y, result_dict(r));
           })
      .def_property_readonly("chunk_samples", [](const PyInjector& d) { return d.inj->chunk_samples(); });

  // ---- rows: a device address; returns (nclip, touched)
  m.def("inject_raw", [](uintptr_t rows, uint64_t stride, uint64_t count, int nbits, int bias, uint64_t t0, F64 sigc,
                         double tsamp, F64 delay, F64 inv_w, U32 A_q, U16 T, uint64_t seed, uintptr_t s) {
    const InjectTables t = tables_from(sigc, tsamp, delay, inv_w, A_q, T);
    std::vector<uint64_t> touched;
    uint64_t nclip;
    {
      py::gil_scoped_release nogil;
      nclip = Injector::apply(reinterpret_cast<int8_t*>(rows), stride, count, nbits, bias, t0, t, seed, &touched,
                              reinterpret_cast<hipStream_t>(s));
    }
    return py::make_tuple(nclip, as_array(touched, {static_cast<py::ssize_t>(touched.size())}));
  });

  m.def("inject_truth_text", [](const std::vector<InjectSignal>& signals,
                                const std::vector<std::tuple<uint64_t, double, double>>& truth,
                                const std::string& units, uint64_t seed) {
    std::vector<InjectTruth> tr;
    for (const auto& t : truth) {
      InjectTruth x;
      x.npulses = std::get<0>(t);
      x.peak = std::get<1>(t);
      x.snr = std::get<2>(t);
      tr.push_back(x);
    }
    return inject_truth_text(signals, tr, units, seed);
  });

  m.def("run_inject_pipeline", [](const InjectCmdLineOptions& a) {
    InjectRun run;
    {
      py::gil_scoped_release nogil;
      run = run_inject_pipeline(a);
    }
    py::dict d = result_dict(run.result);
    d["signals"] = run.signals;
    d["timers"] = run.timers;
    return d;
  });
}
