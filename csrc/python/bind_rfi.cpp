// pybind11 bindings of the RFI excision (rfi.hpp): options, params, mask,
// the host flagging step, RfiCleaner over raw device addresses, the mask
// file, the pipeline and the raw kernel launchers.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "psoup/common.hpp"
#include "psoup/rfi.hpp"

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

}  // namespace

void bind_rfi(py::module_& m) {
  py::class_<RfiCmdLineOptions>(m, "RfiCmdLineOptions")
      .def(py::init<>())
      .def_readwrite("infilename", &RfiCmdLineOptions::infilename)
      .def_readwrite("outfilename", &RfiCmdLineOptions::outfilename)
      .def_readwrite("killfilename", &RfiCmdLineOptions::killfilename)
      .def_readwrite("maskfilename", &RfiCmdLineOptions::maskfilename)
      .def_readwrite("killoutfilename", &RfiCmdLineOptions::killoutfilename)
      .def_readwrite("rfi_block", &RfiCmdLineOptions::rfi_block)
      .def_readwrite("rfi_thresh", &RfiCmdLineOptions::rfi_thresh)
      .def_readwrite("rfi_chan_frac", &RfiCmdLineOptions::rfi_chan_frac)
      .def_readwrite("rfi_block_frac", &RfiCmdLineOptions::rfi_block_frac)
      .def_readwrite("zero_dm", &RfiCmdLineOptions::zero_dm)
      .def_readwrite("verbose", &RfiCmdLineOptions::verbose);
  m.def("parse_rfi_cmdline", [](const std::vector<std::string>& argv) {
    RfiCmdLineOptions a;
    bool exit_now = false;
    bool ok = parse_rfi_cmdline(a, argv, &exit_now);
    return py::make_tuple(ok, exit_now, a);
  });
  m.def("rfi_params_from", &rfi_params_from);
  m.def("rfi_tile", []() { return kern::kRfiTile; });
  m.def("rfi_rdiv", &rfi_rdiv);

  py::class_<RfiParams>(m, "RfiParams")
      .def(py::init<>())
      .def(py::init([](uint64_t block, double thresh, double chan_frac, double block_frac, bool zero_dm) {
             RfiParams p;
             p.block = block;
             p.thresh = thresh;
             p.chan_frac = chan_frac;
             p.block_frac = block_frac;
             p.zero_dm = zero_dm;
             return p;
           }),
           py::arg("block") = 4096, py::arg("thresh") = 5.0, py::arg("chan_frac") = 0.3, py::arg("block_frac") = 0.3,
           py::arg("zero_dm") = false)
      .def_readwrite("block", &RfiParams::block)
      .def_readwrite("thresh", &RfiParams::thresh)
      .def_readwrite("chan_frac", &RfiParams::chan_frac)
      .def_readwrite("block_frac", &RfiParams::block_frac)
      .def_readwrite("zero_dm", &RfiParams::zero_dm);

  py::class_<RfiMask>(m, "RfiMask")
      .def(py::init([](uint64_t nsamps, uint64_t block, U8 chan_flag, U8 block_flag, U8 cell, I32 fill, I32 G, I32 nb,
                       const std::vector<int>& killmask) {
             RfiMask k;
             k.nchans = static_cast<int>(chan_flag.size());
             k.nblk = static_cast<uint64_t>(block_flag.size());
             k.nsamps = nsamps;
             k.block = block;
             k.chan_flag = to_vector(chan_flag);
             k.block_flag = to_vector(block_flag);
             k.cell = to_vector(cell);
             k.fill = to_vector(fill);
             k.G = to_vector(G);
             k.nb = to_vector(nb);
             k.killmask = killmask;
             return k;
           }),
           py::arg("nsamps"), py::arg("block"), py::arg("chan_flag"), py::arg("block_flag"), py::arg("cell"),
           py::arg("fill"), py::arg("G"), py::arg("nb"), py::arg("killmask"))
      .def_readonly("nchans", &RfiMask::nchans)
      .def_readonly("nblk", &RfiMask::nblk)
      .def_readonly("nsamps", &RfiMask::nsamps)
      .def_readonly("block", &RfiMask::block)
      .def_property_readonly("chan_flag", [](const RfiMask& k) { return as_array(k.chan_flag, {k.nchans}); })
      .def_property_readonly("block_flag",
                             [](const RfiMask& k) { return as_array(k.block_flag, {static_cast<py::ssize_t>(k.nblk)}); })
      .def_property_readonly(
          "cell", [](const RfiMask& k) { return as_array(k.cell, {k.nchans, static_cast<py::ssize_t>(k.nblk)}); })
      .def_property_readonly("fill", [](const RfiMask& k) { return as_array(k.fill, {k.nchans}); })
      .def_property_readonly("G", [](const RfiMask& k) { return as_array(k.G, {static_cast<py::ssize_t>(k.nblk)}); })
      .def_property_readonly("nb", [](const RfiMask& k) { return as_array(k.nb, {static_cast<py::ssize_t>(k.nblk)}); })
      .def_readonly("killmask", &RfiMask::killmask)
      .def_property_readonly("flagged_cells", &RfiMask::flagged_cells)
      .def_property_readonly("flagged_chans", &RfiMask::flagged_chans)
      .def_property_readonly("flagged_blocks", &RfiMask::flagged_blocks);

  m.def(
      "rfi_flag",
      [](U64 S1, U64 S2, uint64_t nsamps, const std::vector<int>& killmask, const RfiParams& p) {
        PSOUP_CHECK(S1.ndim() == 2 && S2.ndim() == 2 && S1.shape(0) == S2.shape(0) && S1.shape(1) == S2.shape(1),
                    "rfi_flag: S1 and S2 must be [nchans, nblk]");
        return rfi_flag(to_vector(S1), to_vector(S2), static_cast<int>(S1.shape(0)), nsamps, killmask, p);
      },
      py::arg("S1"), py::arg("S2"), py::arg("nsamps"), py::arg("killmask"), py::arg("params"));

  py::class_<RfiMaskHeader>(m, "RfiMaskHeader")
      .def(py::init<>())
      .def(py::init([](uint32_t nbits, double tsamp) {
             RfiMaskHeader h;
             h.nbits = nbits;
             h.tsamp = tsamp;
             return h;
           }),
           py::arg("nbits"), py::arg("tsamp"))
      .def_readwrite("nbits", &RfiMaskHeader::nbits)
      .def_readwrite("tsamp", &RfiMaskHeader::tsamp);
  m.def("write_rfi_mask", &write_rfi_mask, py::arg("path"), py::arg("mask"), py::arg("params"), py::arg("header"));
  m.def("read_rfi_mask", [](const std::string& path) {
    RfiParams p;
    RfiMaskHeader h;
    RfiMask k = read_rfi_mask(path, &p, &h);
    return py::make_tuple(k, p, h);
  });
  m.def("write_killfile", &write_killfile);
  m.def("rfi_summary_comment", &rfi_summary_comment);

  // rows / dst: device addresses of int8 [nchans][stride] (x - bias).
  py::class_<RfiCleaner>(m, "RfiCleaner")
      .def(py::init([](const RfiParams& p, uintptr_t stream) {
             return new RfiCleaner(p, reinterpret_cast<hipStream_t>(stream));
           }),
           py::arg("params"), py::arg("stream") = 0)
      .def(
          "clean",
          [](RfiCleaner& c, uintptr_t rows, uint64_t stride, int nchans, uint64_t nsamps, int nbits, int bias,
             const std::vector<int>& killmask, uintptr_t dst, uint64_t dst_stride) {
            py::gil_scoped_release nogil;
            return c.clean(reinterpret_cast<int8_t*>(rows), stride, nchans, nsamps, nbits, bias, killmask,
                           reinterpret_cast<int8_t*>(dst), dst_stride);
          },
          py::arg("rows"), py::arg("stride"), py::arg("nchans"), py::arg("nsamps"), py::arg("nbits"), py::arg("bias"),
          py::arg("killmask"), py::arg("dst") = 0, py::arg("dst_stride") = 0)
      .def(
          "clean_packed",
          [](RfiCleaner& c, uintptr_t packed, int nchans, uint64_t nsamps, int nbits,
             const std::vector<int>& killmask) {
            py::gil_scoped_release nogil;
            return c.clean_packed(reinterpret_cast<uint8_t*>(packed), nchans, nsamps, nbits, killmask);
          },
          py::arg("packed"), py::arg("nchans"), py::arg("nsamps"), py::arg("nbits"), py::arg("killmask"))
      .def(
          "apply",
          [](RfiCleaner& c, uintptr_t rows, uint64_t stride, uintptr_t dst, uint64_t dst_stride, int nchans,
             uint64_t nsamps, int nbits, int bias, const RfiMask& k) {
            py::gil_scoped_release nogil;
            c.apply(reinterpret_cast<const int8_t*>(rows), stride, reinterpret_cast<int8_t*>(dst), dst_stride, nchans,
                    nsamps, nbits, bias, k);
          },
          py::arg("rows"), py::arg("stride"), py::arg("dst"), py::arg("dst_stride"), py::arg("nchans"),
          py::arg("nsamps"), py::arg("nbits"), py::arg("bias"), py::arg("mask"))
      .def("set_mask", &RfiCleaner::set_mask, py::arg("mask"), py::call_guard<py::gil_scoped_release>())
      .def(
          "apply_uploaded",
          [](RfiCleaner& c, uintptr_t rows, uint64_t stride, uintptr_t dst, uint64_t dst_stride, int nchans,
             uint64_t nsamps, int nbits, int bias) {
            c.apply_uploaded(reinterpret_cast<const int8_t*>(rows), stride, reinterpret_cast<int8_t*>(dst), dst_stride,
                             nchans, nsamps, nbits, bias);
          },
          py::arg("rows"), py::arg("stride"), py::arg("dst"), py::arg("dst_stride"), py::arg("nchans"),
          py::arg("nsamps"), py::arg("nbits"), py::arg("bias"));

  py::class_<RfiRun>(m, "RfiRun").def_readonly("mask", &RfiRun::mask).def_readonly("timers", &RfiRun::timers);
  m.def("run_rfi_pipeline", [](const RfiCmdLineOptions& a) {
    py::gil_scoped_release nogil;
    return run_rfi_pipeline(a);
  });

  // raw launchers (addresses + stream handle)
  m.def("rfi_block_sums_raw", [](uintptr_t rows, uint64_t stride, int nchans, uint64_t nsamps, uint64_t block, int bias,
                                 uintptr_t S1, uintptr_t S2, uintptr_t s) {
    kern::rfi_block_sums(reinterpret_cast<const int8_t*>(rows), stride, nchans, nsamps, block, bias,
                         reinterpret_cast<uint64_t*>(S1), reinterpret_cast<uint64_t*>(S2),
                         reinterpret_cast<hipStream_t>(s));
  });
  m.def("pack_transpose_raw", [](uintptr_t rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias,
                                 uintptr_t packed, uintptr_t s) {
    kern::pack_transpose(reinterpret_cast<const int8_t*>(rows), stride, nsamps, nchans, nbits, bias,
                         reinterpret_cast<uint8_t*>(packed), reinterpret_cast<hipStream_t>(s));
  });
}
