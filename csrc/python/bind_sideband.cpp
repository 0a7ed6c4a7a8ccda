// pybind11 bindings of sbsearch (sideband.hpp): options, the host steps (no GPU
// needed), the kernels alone over raw device addresses, SidebandSearcher over a
// resident filterbank and the output text.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>

#include "psoup/common.hpp"
#include "psoup/sideband.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

using EvTuple = std::tuple<int, int, int, int, float>;  // (dm_idx, m, seg, j, S)
using F32 = py::array_t<float, py::array::c_style | py::array::forcecast>;
using C64 = py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast>;

std::vector<SbEvent> events_of(const std::vector<EvTuple>& ev) {
  std::vector<SbEvent> out;
  for (const EvTuple& e : ev)
    out.push_back(SbEvent{std::get<0>(e), std::get<1>(e), std::get<2>(e), std::get<3>(e), std::get<4>(e)});
  return out;
}
EvTuple tuple_of(const SbEvent& e) { return EvTuple(e.dm_idx, e.m, e.seg, e.j, e.S); }
std::vector<EvTuple> tuples_of(const std::vector<SbEvent>& ev) {
  std::vector<EvTuple> out;
  for (const SbEvent& e : ev) out.push_back(tuple_of(e));
  return out;
}

SbParams params_of(int m_lo, int m_hi, int j_min, float clip, float min_power) {
  SbParams p;
  p.m_lo = m_lo;
  p.m_hi = m_hi;
  p.j_min = j_min;
  p.clip = clip;
  p.min_power = min_power;
  return p;
}

// The geometry of a band given in bins (the raw entries: no frequencies).
SbGeometry band_geometry(int64_t k_lo, int64_t k_hi, int m_lo, int m_hi) {
  PSOUP_CHECK(m_lo >= kSbMinM && m_hi <= kSbMaxM && m_lo <= m_hi, "sideband: the sizes are outside 5..13");
  PSOUP_CHECK(k_lo >= 0 && k_lo <= k_hi, "sideband: a band with k_lo above k_hi");
  SbGeometry g;
  g.k_lo = k_lo;
  g.k_hi = k_hi;
  g.m_lo = m_lo;
  g.m_hi = m_hi;
  const int64_t band = k_hi - k_lo;
  g.nranges = static_cast<int>((band + kSbRange - 1) / kSbRange);
  for (int m = m_lo; m <= m_hi; ++m) {
    const int64_t n = sb_nseg(band, m);
    g.nseg.push_back(n);
    g.seg_stride = std::max(g.seg_stride, n);
    if (n > 0) g.nwin = std::max<int64_t>(g.nwin, (n - 1) / sbk::owned(m) + 1);
  }
  return g;
}

}  // namespace

void bind_sideband(py::module_& m) {
  py::class_<SbCmdLineOptions>(m, "SbCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("search", &SbCmdLineOptions::search)
      .def_readwrite("outfilename", &SbCmdLineOptions::outfilename)
      .def_readwrite("min_power", &SbCmdLineOptions::min_power)
      .def_readwrite("m_min", &SbCmdLineOptions::m_min)
      .def_readwrite("m_max", &SbCmdLineOptions::m_max)
      .def_readwrite("j_min", &SbCmdLineOptions::j_min)
      .def_readwrite("clip", &SbCmdLineOptions::clip);
  m.def("parse_sb_cmdline", [](const std::vector<std::string>& argv) {
    SbCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_sb_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.attr("SB_WINDOW") = kSbWindow;
  m.attr("SB_HOP") = kSbHop;
  m.attr("SB_RANGE") = kSbRange;
  m.attr("SB_RANGE_LANES") = kSbRangeLanes;
  m.attr("SB_MAX_SPAN") = kSbMaxSpan;
  m.attr("SB_EVENT_BYTES") = sizeof(SbEvent);

  py::class_<SbGeometry>(m, "SbGeometry")
      .def_readonly("fft_size", &SbGeometry::fft_size)
      .def_readonly("tobs", &SbGeometry::tobs)
      .def_readonly("k_lo", &SbGeometry::k_lo)
      .def_readonly("k_hi", &SbGeometry::k_hi)
      .def_readonly("m_lo", &SbGeometry::m_lo)
      .def_readonly("m_hi", &SbGeometry::m_hi)
      .def_readonly("nseg", &SbGeometry::nseg)
      .def_readonly("seg_stride", &SbGeometry::seg_stride)
      .def_readonly("nwin", &SbGeometry::nwin)
      .def_readonly("nranges", &SbGeometry::nranges);

  // ---- the host steps (no GPU)
  m.def("sb_nseg", &sb_nseg, py::arg("band"), py::arg("m"));
  m.def("sb_geometry", &sb_geometry, py::arg("min_freq"), py::arg("max_freq"), py::arg("fft_size"), py::arg("tsamp"),
        py::arg("m_lo") = 5, py::arg("m_hi") = 13);
  m.def("sb_band_geometry", &band_geometry, py::arg("k_lo"), py::arg("k_hi"), py::arg("m_lo") = 5,
        py::arg("m_hi") = 13);
  m.def(
      "sb_check",
      [](float min_freq, float max_freq, uint64_t fft_size, float tsamp, int m_lo, int m_hi, int j_min, float clip,
         float min_power) { sb_check(params_of(m_lo, m_hi, j_min, clip, min_power), min_freq, max_freq, fft_size, tsamp); },
      py::arg("min_freq"), py::arg("max_freq"), py::arg("fft_size"), py::arg("tsamp"), py::arg("m_lo") = 5,
      py::arg("m_hi") = 13, py::arg("j_min") = 2, py::arg("clip") = 32.f, py::arg("min_power") = 30.f);
  m.def("sb_twiddles", [] {
    const std::vector<float2> t = sb_twiddles();
    py::array_t<std::complex<float>> a(static_cast<py::ssize_t>(t.size()));
    std::memcpy(a.mutable_data(), t.data(), t.size() * sizeof(float2));
    return a;
  });
  m.def("sb_event_values", [](const SbGeometry& g, EvTuple e) {
    const SbEvent ev{std::get<0>(e), std::get<1>(e), std::get<2>(e), std::get<3>(e), std::get<4>(e)};
    return py::make_tuple(sb_event_freq(g, ev), sb_event_freq_half_width(g, ev), sb_event_pb(g, ev),
                          sb_event_pb_res(g, ev));
  });
  // -> [(event, members, dm_lo, dm_hi)]
  m.def("sb_cluster", [](const std::vector<EvTuple>& ev) {
    std::vector<std::tuple<EvTuple, int, int, int>> out;
    for (const SbCandidate& c : sb_cluster(events_of(ev))) out.emplace_back(tuple_of(c.ev), c.members, c.dm_lo, c.dm_hi);
    return out;
  });
  m.def(
      "sb_power_host",
      [](C64 spec, const std::vector<uint32_t>& zapmask, int64_t k_lo, int64_t k_hi) {
        PSOUP_CHECK(spec.ndim() == 2, "sb_power_host: spec must be [nrows, nbins]");
        const int nrows = static_cast<int>(spec.shape(0));
        const uint64_t nb = static_cast<uint64_t>(spec.shape(1));
        py::array_t<double> mu(static_cast<py::ssize_t>(nrows));
        py::array_t<float> P({static_cast<py::ssize_t>(nrows), static_cast<py::ssize_t>(nb)});
        std::fill(P.mutable_data(), P.mutable_data() + P.size(), 0.f);
        sb_power_host(reinterpret_cast<const float2*>(spec.data()), nb, nrows, zapmask, k_lo, k_hi, mu.mutable_data(),
                      P.mutable_data(), nb);
        return py::make_tuple(mu, P);
      },
      py::arg("spec"), py::arg("zapmask"), py::arg("k_lo"), py::arg("k_hi"));
  // -> (best_S [nrows, nm, seg_stride], best_j likewise (-1 / NaN where there is no segment), events)
  m.def(
      "sb_search_host",
      [](F32 P, int64_t k_lo, int64_t k_hi, int m_lo, int m_hi, int j_min, float clip, float min_power, int dm0) {
        PSOUP_CHECK(P.ndim() == 2, "sb_search_host: P must be [nrows, stride]");
        const int nrows = static_cast<int>(P.shape(0));
        const SbGeometry g = band_geometry(k_lo, k_hi, m_lo, m_hi);
        const py::ssize_t nm = m_hi - m_lo + 1, ss = std::max<int64_t>(g.seg_stride, 1);
        py::array_t<float> bs({static_cast<py::ssize_t>(nrows), nm, ss});
        py::array_t<int32_t> bj({static_cast<py::ssize_t>(nrows), nm, ss});
        std::fill(bs.mutable_data(), bs.mutable_data() + bs.size(), std::nanf(""));
        std::fill(bj.mutable_data(), bj.mutable_data() + bj.size(), -1);
        SbGeometry gg = g;
        gg.seg_stride = ss;
        std::vector<SbEvent> ev;
        sb_search_host(P.data(), static_cast<uint64_t>(P.shape(1)), nrows, gg,
                       params_of(m_lo, m_hi, j_min, clip, min_power), dm0, bs.mutable_data(), bj.mutable_data(), &ev);
        return py::make_tuple(bs, bj, tuples_of(ev));
      },
      py::arg("P"), py::arg("k_lo"), py::arg("k_hi"), py::arg("m_lo") = 5, py::arg("m_hi") = 13, py::arg("j_min") = 2,
      py::arg("clip") = 32.f, py::arg("min_power") = 30.f, py::arg("dm0") = 0);

  // ---- the kernels alone: device addresses, which the caller keeps alive until the stream has run them
  m.def(
      "sb_power_raw",
      [](uintptr_t spec, uint64_t spec_stride, int nrows, uintptr_t zapmask, int64_t k_lo, int64_t k_hi, uint64_t count,
         uintptr_t partials, uintptr_t mu, uintptr_t P, uint64_t stride, uintptr_t s) {
        PSOUP_CHECK(spec % 8 == 0 && partials % 8 == 0 && mu % 8 == 0 && P % 4 == 0 && zapmask % 4 == 0,
                    "sb_power: a misaligned device address");
        kern::sb_power(reinterpret_cast<const float2*>(spec), spec_stride, nrows,
                       reinterpret_cast<const uint32_t*>(zapmask), k_lo, k_hi, count,
                       reinterpret_cast<double*>(partials), reinterpret_cast<double*>(mu), reinterpret_cast<float*>(P),
                       stride, reinterpret_cast<hipStream_t>(s));
      },
      py::arg("spec"), py::arg("spec_stride"), py::arg("nrows"), py::arg("zapmask"), py::arg("k_lo"), py::arg("k_hi"),
      py::arg("count"), py::arg("partials"), py::arg("mu"), py::arg("P"), py::arg("stride"), py::arg("stream") = 0);
  m.def(
      "sb_search_raw",
      [](uintptr_t P, uint64_t stride, int nrows, int64_t k_lo, int64_t k_hi, int m_lo, int m_hi, int j_min, float clip,
         float min_power, int dm0, uintptr_t tw, uintptr_t best_S, uintptr_t best_j, int64_t seg_stride,
         uintptr_t events, uint32_t capacity, uintptr_t count, uintptr_t s) {
        SbGeometry g = band_geometry(k_lo, k_hi, m_lo, m_hi);
        if (best_S != 0) {
          PSOUP_CHECK(seg_stride >= g.seg_stride, "sb_search: seg_stride below the segment count");
          g.seg_stride = seg_stride;
        }
        PSOUP_CHECK(tw % 8 == 0 && best_S % 4 == 0 && best_j % 4 == 0 && events % 4 == 0 && count % 4 == 0,
                    "sb_search: a misaligned device address");
        kern::sb_search(reinterpret_cast<const float*>(P), stride, nrows, g, params_of(m_lo, m_hi, j_min, clip, min_power),
                        dm0, reinterpret_cast<const float2*>(tw), reinterpret_cast<float*>(best_S),
                        reinterpret_cast<int32_t*>(best_j), reinterpret_cast<SbEvent*>(events), capacity,
                        reinterpret_cast<uint32_t*>(count), reinterpret_cast<hipStream_t>(s));
      },
      py::arg("P"), py::arg("stride"), py::arg("nrows"), py::arg("k_lo"), py::arg("k_hi"), py::arg("m_lo"),
      py::arg("m_hi"), py::arg("j_min"), py::arg("clip"), py::arg("min_power"), py::arg("dm0"), py::arg("tw"),
      py::arg("best_S"), py::arg("best_j"), py::arg("seg_stride"), py::arg("events"), py::arg("capacity"),
      py::arg("count"), py::arg("stream") = 0);

  // ---- setup, searcher, output
  py::class_<SbSetup>(m, "SbSetup")
      .def_readonly("nrow", &SbSetup::nrow)
      .def_readonly("geom", &SbSetup::geom)
      .def_readonly("zapmask", &SbSetup::zapmask)
      .def_readonly("unzapped", &SbSetup::unzapped)
      .def_property_readonly("m_lo", [](const SbSetup& s) { return s.params.m_lo; })
      .def_property_readonly("m_hi", [](const SbSetup& s) { return s.params.m_hi; })
      .def_property_readonly("j_min", [](const SbSetup& s) { return s.params.j_min; })
      .def_property_readonly("clip", [](const SbSetup& s) { return s.params.clip; })
      .def_property_readonly("min_power", [](const SbSetup& s) { return s.params.min_power; })
      .def_property_readonly("dm_list", [](const SbSetup& s) { return s.search.dm_list; })
      .def_property_readonly("killmask", [](const SbSetup& s) { return s.search.killmask; })
      .def_property_readonly("fft_size", [](const SbSetup& s) { return s.search.fft_size; })
      .def_property_readonly("tsamp", [](const SbSetup& s) { return s.search.search.tsamp; })
      .def_property_readonly("nsamps", [](const SbSetup& s) { return s.search.nsamps; })
      .def_property_readonly("geometry", [](const SbSetup& s) {
        return DedispGeometry::make(s.search.header, s.search.nsamps, s.search.dm_list, s.search.killmask);
      });
  // reads the header of args.search.infilename; every refusal is raised here
  m.def("sb_setup", [](const SbCmdLineOptions& a) { return make_sb_setup(a, read_header_file(a.search.infilename)); });

  py::class_<SidebandSearcher>(m, "SidebandSearcher")
      .def(py::init([](const SbSetup& setup, const DeviceFilterbank& fb, uintptr_t s, uint32_t capacity) {
             return new SidebandSearcher(setup, fb, reinterpret_cast<hipStream_t>(s), capacity);
           }),
           py::arg("setup"), py::arg("filterbank"), py::arg("stream") = 0, py::arg("capacity") = 1u << 16,
           py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
      .def("search",
           [](SidebandSearcher& ss, int d0, int d1) {
             std::vector<SbEvent> ev;
             {
               py::gil_scoped_release nogil;
               ev = ss.search(d0, d1);
             }
             return tuples_of(ev);
           },
           py::arg("d0") = 0, py::arg("d1") = -1)
      // -> (P float32 [d1 - d0, power_stride], mu float64 [d1 - d0])
      .def("power_rows",
           [](SidebandSearcher& ss, int d0, int d1) {
             std::vector<double> mu;
             const std::vector<float> P = ss.power_rows(d0, d1, &mu);
             py::array_t<float> a({static_cast<py::ssize_t>(d1 - d0), static_cast<py::ssize_t>(ss.power_stride())});
             std::memcpy(a.mutable_data(), P.data(), P.size() * sizeof(float));
             py::array_t<double> b(static_cast<py::ssize_t>(mu.size()));
             std::memcpy(b.mutable_data(), mu.data(), mu.size() * sizeof(double));
             return py::make_tuple(a, b);
           },
           py::arg("d0"), py::arg("d1"))
      .def_property_readonly("power_stride", &SidebandSearcher::power_stride)
      .def_property_readonly("reruns", &SidebandSearcher::reruns);

  py::class_<SbCandidate>(m, "SbCandidate")
      .def_property_readonly("event", [](const SbCandidate& c) { return tuple_of(c.ev); })
      .def_readonly("members", &SbCandidate::members)
      .def_readonly("dm_lo", &SbCandidate::dm_lo)
      .def_readonly("dm_hi", &SbCandidate::dm_hi);
  m.def("sb_cluster_candidates",
        [](const std::vector<EvTuple>& ev) { return sb_cluster(events_of(ev)); });
  m.def("sb_output_text", &sb_output_text);
  m.def("write_sb_output", &write_sb_output);
}
