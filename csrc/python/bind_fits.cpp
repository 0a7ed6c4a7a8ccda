// pybind11 bindings of fits2fil (psrfits.hpp): options, the host steps (no GPU
// needed: the parser, rows and slots, the band, the polarisations, the header),
// FitsDigitiser over a host buffer, the decode kernel over raw device
// addresses, the pipeline.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <sstream>

#include "psoup/common.hpp"
#include "psoup/psrfits.hpp"

namespace py = pybind11;
using namespace psoup;

namespace {

template <class T>
py::array_t<T> as_array(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

using U8 = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;

py::dict layout_dict(const FitsLayout& l) {
  py::dict d;
  d["table_off"] = l.table_off;
  d["row_bytes"] = l.row_bytes;
  d["nrows"] = l.nrows;
  d["npol"] = l.npol;
  d["nbits"] = l.nbits;
  d["nchan"] = l.nchan;
  d["nsblk"] = l.nsblk;
  d["signint"] = l.signint;
  d["tbin"] = l.tbin;
  d["chan_bw"] = l.chan_bw;
  d["z"] = l.z;
  d["pol_type"] = l.pol_type;
  py::list cols;
  for (const FitsColumn& c : l.columns)
    cols.append(py::make_tuple(c.name, std::string(1, c.form.type), c.form.repeat, c.offset, c.form.bytes));
  d["columns"] = cols;
  py::dict prim, sub;
  for (const auto& e : l.primary.kv) prim[py::str(e.first)] = e.second;
  for (const auto& e : l.subint.kv) sub[py::str(e.first)] = e.second;
  d["primary"] = prim;
  d["subint"] = sub;
  return d;
}

py::dict slots_dict(const FitsSlots& s) {
  py::dict d;
  d["slot"] = s.slot;
  d["slot_row"] = s.slot_row;
  d["nslots"] = s.nslots;
  d["nsamps"] = s.nsamps;
  d["ndropped"] = s.ndropped;
  d["offs_sub0"] = s.offs_sub0;
  return d;
}

py::dict header_dict(const SigprocHeader& h) {
  py::dict d;
  d["source_name"] = h.source_name;
  d["rawdatafile"] = h.rawdatafile;
  d["telescope_id"] = h.telescope_id;
  d["machine_id"] = h.machine_id;
  d["data_type"] = h.data_type;
  d["src_raj"] = h.src_raj;
  d["src_dej"] = h.src_dej;
  d["tstart"] = h.tstart;
  d["tsamp"] = h.tsamp;
  d["fch1"] = h.fch1;
  d["foff"] = h.foff;
  d["nchans"] = h.nchans;
  d["nbits"] = h.nbits;
  d["nifs"] = h.nifs;
  d["nsamples"] = h.nsamples;
  d["barycentric"] = h.barycentric;
  d["ibeam"] = h.ibeam;
  d["_present"] = h.keys_present;
  std::ostringstream os;
  write_header(os, h);
  d["bytes"] = py::bytes(os.str());
  return d;
}

py::dict result_dict(const FitsResult& f) {
  const DigiResult& r = f.digi;
  const DigiScale& sc = r.scale;
  py::dict d;
  const py::ssize_t nc = r.nchans, nblk = static_cast<py::ssize_t>(r.nblk), ni = sc.nint;
  d["rows"] = f.rows;
  d["nslots"] = f.nslots;
  d["ndropped"] = f.ndropped;
  d["pols"] = py::make_tuple(f.pol_a, f.pol_b);
  d["z"] = f.z;
  d["header"] = header_dict(f.header);
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

FitsOptions make_options(int pol, bool no_scales, bool no_offsets, bool no_weights, int telescope_id, int machine_id) {
  FitsOptions o;
  o.pol = pol;
  o.no_scales = no_scales;
  o.no_offsets = no_offsets;
  o.no_weights = no_weights;
  o.telescope_id = telescope_id;
  o.machine_id = machine_id;
  return o;
}

struct PyFitsDigitiser {
  U8 file;  // keeps the file's bytes alive
  std::unique_ptr<FitsDigitiser> dig;
};

}  // namespace

void bind_fits(py::module_& m) {
  py::class_<FitsCmdLineOptions>(m, "FitsCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &FitsCmdLineOptions::infilename)
      .def_readwrite("outfilename", &FitsCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &FitsCmdLineOptions::killfilename)
      .def_readwrite("killoutfilename", &FitsCmdLineOptions::killoutfilename)
      .def_readwrite("sigma_out", &FitsCmdLineOptions::sigma_out)
      .def_readwrite("scale", &FitsCmdLineOptions::scale)
      .def_readwrite("rescale_blocks", &FitsCmdLineOptions::rescale_blocks)
      .def_readwrite("pol", &FitsCmdLineOptions::pol)
      .def_readwrite("no_scales", &FitsCmdLineOptions::no_scales)
      .def_readwrite("no_offsets", &FitsCmdLineOptions::no_offsets)
      .def_readwrite("no_weights", &FitsCmdLineOptions::no_weights)
      .def_readwrite("telescope_id", &FitsCmdLineOptions::telescope_id)
      .def_readwrite("machine_id", &FitsCmdLineOptions::machine_id)
      .def_readwrite("verbose", &FitsCmdLineOptions::verbose);
  m.def("parse_fits_cmdline", [](const std::vector<std::string>& argv) {
    FitsCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_fits_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  py::class_<FitsOptions>(m, "FitsOptions")
      .def(py::init(&make_options), py::arg("pol") = -1, py::arg("no_scales") = false, py::arg("no_offsets") = false,
           py::arg("no_weights") = false, py::arg("telescope_id") = -1, py::arg("machine_id") = 0)
      .def_readwrite("pol", &FitsOptions::pol)
      .def_readwrite("no_scales", &FitsOptions::no_scales)
      .def_readwrite("no_offsets", &FitsOptions::no_offsets)
      .def_readwrite("no_weights", &FitsOptions::no_weights)
      .def_readwrite("telescope_id", &FitsOptions::telescope_id)
      .def_readwrite("machine_id", &FitsOptions::machine_id);
  m.def("fits_options_from", &fits_options_from);
  m.def("fits_digi_params_from", &fits_digi_params_from);

  // ---- the host steps (no GPU)
  m.def("fits_tform", [](const std::string& s) {
    const FitsTform f = fits_tform(s);
    return py::make_tuple(f.repeat, std::string(1, f.type), f.bytes);
  });
  m.def("fits_parse", [](U8 file) { return layout_dict(fits_parse(file.data(), static_cast<uint64_t>(file.size()))); });
  m.def(
      "fits_row_slots",
      [](const std::vector<double>& offs_sub, uint64_t nrows, int nsblk, double tbin) {
        return slots_dict(fits_row_slots(offs_sub, nrows, nsblk, tbin));
      },
      py::arg("offs_sub"), py::arg("nrows"), py::arg("nsblk"), py::arg("tbin"));
  m.def(
      "fits_band",
      [](const std::vector<double>& freq, double chan_bw) {
        const FitsBand b = fits_band(freq, chan_bw);
        return py::make_tuple(b.fch1, b.foff);
      },
      py::arg("freq"), py::arg("chan_bw") = 0.0);
  m.def("fits_pols", &fits_pols, py::arg("npol"), py::arg("pol_type"), py::arg("pol") = -1);
  m.def("fits_telescope_id", &fits_telescope_id);
  m.def("fits_sexagesimal", &fits_sexagesimal);
  // The whole validation of a file in memory: layout, slots, band and the header written.
  m.def(
      "fits_inspect",
      [](U8 file, const FitsOptions& opt, const std::string& rawdatafile) {
        const PsrfitsFile f = PsrfitsFile::from_memory(file.data(), static_cast<uint64_t>(file.size()));
        py::dict d = layout_dict(f.layout());
        d["slots"] = slots_dict(f.slots());
        d["band"] = py::make_tuple(f.band().fch1, f.band().foff);
        d["pols"] = fits_pols(f.layout().npol, f.layout().pol_type, opt.pol);
        d["header"] = header_dict(fits_header(f.layout(), f.slots(), f.band(), opt, rawdatafile));
        return d;
      },
      py::arg("file"), py::arg("options") = FitsOptions(), py::arg("rawdatafile") = "");

  // ---- FitsDigitiser: the file is a host array, y comes back as one
  py::class_<PyFitsDigitiser>(m, "FitsDigitiser")
      .def(py::init([](U8 file, const FitsOptions& opt, const std::vector<int>& killmask, const DigiParams& p,
                       const std::string& rawdatafile, uintptr_t stream, size_t budget_bytes) {
             auto d = std::make_unique<PyFitsDigitiser>();
             d->file = file;
             d->dig = std::make_unique<FitsDigitiser>(file.data(), static_cast<uint64_t>(file.size()), opt, killmask, p,
                                                      rawdatafile, reinterpret_cast<hipStream_t>(stream), budget_bytes);
             return d;
           }),
           py::arg("file"), py::arg("options"), py::arg("killmask"), py::arg("params"), py::arg("rawdatafile") = "",
           py::arg("stream") = 0, py::arg("budget_bytes") = FitsDigitiser::kDefaultBudgetBytes)
      .def("run",
           [](PyFitsDigitiser& d) {
             py::array_t<uint8_t> y({static_cast<py::ssize_t>(d.dig->nsamps()), static_cast<py::ssize_t>(d.dig->nchan())});
             FitsResult r;
             {
               uint8_t* out = y.mutable_data();
               py::gil_scoped_release nogil;
               r = d.dig->run(out);
             }
             return py::make_tuple(y, result_dict(r));
           })
      .def_property_readonly("nsamps", [](const PyFitsDigitiser& d) { return d.dig->nsamps(); })
      .def_property_readonly("nchan", [](const PyFitsDigitiser& d) { return d.dig->nchan(); })
      .def_property_readonly("chunk_samples", [](const PyFitsDigitiser& d) { return d.dig->chunk_samples(); })
      .def_property_readonly("launches", [](const PyFitsDigitiser& d) { return d.dig->launches(); })
      .def_property_readonly("header", [](const PyFitsDigitiser& d) { return header_dict(d.dig->header()); });

  // ---- data / scl / offs / wts / out: device addresses; the slot table is a host list
  m.def(
      "fits_decode_raw",
      [](uintptr_t data, uintptr_t scl, uintptr_t offs, uintptr_t wts, int nrows, const std::vector<int32_t>& slot_row,
         int nsblk, int npol, int nchan, int nbits, bool is_signed, int pol_a, int pol_b, double z, uint64_t t0,
         uint64_t count, uintptr_t out, uintptr_t s) {
        kern::FitsDecodeArgs a;
        a.data = reinterpret_cast<const uint8_t*>(data);
        a.scl = reinterpret_cast<const float*>(scl);
        a.offs = reinterpret_cast<const float*>(offs);
        a.wts = reinterpret_cast<const float*>(wts);
        a.nrows = nrows;
        a.nsblk = nsblk;
        a.npol = npol;
        a.nchan = nchan;
        a.nbits = nbits;
        a.is_signed = is_signed ? 1 : 0;
        a.pol_a = pol_a;
        a.pol_b = pol_b;
        a.z = z;
        py::gil_scoped_release nogil;
        FitsDigitiser::decode(a, slot_row, t0, count, reinterpret_cast<float*>(out), reinterpret_cast<hipStream_t>(s));
      },
      py::arg("data"), py::arg("scl"), py::arg("offs"), py::arg("wts"), py::arg("nrows"), py::arg("slot_row"),
      py::arg("nsblk"), py::arg("npol"), py::arg("nchan"), py::arg("nbits"), py::arg("signed"), py::arg("pol_a"),
      py::arg("pol_b"), py::arg("z"), py::arg("t0"), py::arg("count"), py::arg("out"), py::arg("stream") = 0);

  m.def("run_fits_pipeline", [](const FitsCmdLineOptions& a) {
    FitsRun run;
    {
      py::gil_scoped_release nogil;
      run = run_fits_pipeline(a);
    }
    py::dict d = result_dict(run.result);
    d["timers"] = run.timers;
    return d;
  });
}
