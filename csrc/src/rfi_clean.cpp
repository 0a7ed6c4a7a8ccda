// RFI excision, device side: the cleaner (block sums -> host flags -> apply)
// and the rficlean file pipeline.  See psoup/rfi.hpp.
#include <algorithm>
#include <cstdio>
#include <fstream>

#include "psoup/engine.hpp"
#include "psoup/kernels.hpp"
#include "psoup/rfi.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

RfiCleaner::RfiCleaner(const RfiParams& p, hipStream_t stream) : p_(p), stream_(stream) { rfi_check_params(p_); }

void RfiCleaner::set_mask(const RfiMask& m) {
  const size_t nc = static_cast<size_t>(m.nchans), nblk = static_cast<size_t>(m.nblk);
  PSOUP_CHECK(m.nchans > 0 && nblk > 0 && m.block == p_.block && m.cell.size() == nc * nblk && m.fill.size() == nc &&
                  m.G.size() == nblk && m.nb.size() == nblk,
              "rfi apply: inconsistent mask");
  // block-major flags (a tile reads its block's nchans bytes contiguously),
  // turned in 64 x 64 pieces; fill | G | n_b | flagged cells per block in one
  // int32 table; both through pinned staging
  h_cell_t_.resize(nblk * nc);
  h_tab_.resize(nc + 3 * nblk);
  uint8_t* ct = h_cell_t_.data();
  int32_t* tab = h_tab_.data();
  std::fill(tab, tab + nc + 3 * nblk, 0);
  for (size_t c0 = 0; c0 < nc; c0 += 64)
    for (size_t b0 = 0; b0 < nblk; b0 += 64) {
      const size_t c1 = std::min(nc, c0 + 64), b1 = std::min(nblk, b0 + 64);
      for (size_t c = c0; c < c1; ++c)
        for (size_t b = b0; b < b1; ++b) ct[b * nc + c] = m.cell[c * nblk + b];
    }
  for (size_t b = 0; b < nblk; ++b) {
    int32_t n = 0;
    for (size_t c = 0; c < nc; ++c) n += ct[b * nc + c];
    tab[nc + b] = m.G[b];
    tab[nc + nblk + b] = m.nb[b];
    tab[nc + 2 * nblk + b] = n;
  }
  std::copy(m.fill.begin(), m.fill.end(), tab);
  cell_t_.resize(nblk * nc);
  tab_.resize(nc + 3 * nblk);
  PSOUP_HIP_CHECK(hipMemcpyAsync(cell_t_.data(), ct, nblk * nc, hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(
      hipMemcpyAsync(tab_.data(), tab, (nc + 3 * nblk) * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // the stages may be refilled
  mask_nc_ = nc;
  mask_nblk_ = nblk;
  mask_nsamps_ = m.nsamps;
}

void RfiCleaner::apply_uploaded(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans,
                                uint64_t nsamps, int nbits, int bias) {
  PSOUP_CHECK(mask_nc_ == static_cast<size_t>(nchans) && mask_nsamps_ == nsamps && mask_nblk_ > 0,
              "rfi apply: the uploaded mask does not fit the data");
  const size_t nc = mask_nc_, nblk = mask_nblk_;
  const int32_t* t = tab_.data();
  kern::rfi_apply(rows, stride, dst, dst_stride, nchans, nsamps, p_.block, nbits, bias, p_.zero_dm, cell_t_.data(), t,
                  t + nc, t + nc + nblk, t + nc + 2 * nblk, stream_);
}

void RfiCleaner::apply(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans,
                       uint64_t nsamps, int nbits, int bias, const RfiMask& m) {
  PSOUP_CHECK(m.nchans == nchans && m.nsamps == nsamps, "rfi apply: the mask does not fit the data");
  set_mask(m);
  apply_uploaded(rows, stride, dst, dst_stride, nchans, nsamps, nbits, bias);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
}

RfiMask RfiCleaner::clean(int8_t* rows, uint64_t stride, int nchans, uint64_t nsamps, int nbits, int bias,
                          const std::vector<int>& killmask, int8_t* dst, uint64_t dst_stride) {
  PSOUP_CHECK(nchans > 0 && nsamps > 0, "rfi clean: empty filterbank");
  const size_t nblk = static_cast<size_t>((nsamps + p_.block - 1) / p_.block);
  const size_t ncell = static_cast<size_t>(nchans) * nblk;
  sums_.resize(2 * ncell);
  kern::rfi_block_sums(rows, stride, nchans, nsamps, p_.block, bias, sums_.data(), sums_.data() + ncell, stream_);
  std::vector<uint64_t> S1(ncell), S2(ncell);
  PSOUP_HIP_CHECK(hipMemcpyAsync(S1.data(), sums_.data(), ncell * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(
      hipMemcpyAsync(S2.data(), sums_.data() + ncell, ncell * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  RfiMask m = rfi_flag(S1, S2, nchans, nsamps, killmask, p_);
  if (!dst) {
    dst = rows;
    dst_stride = stride;
  }
  apply(rows, stride, dst, dst_stride, nchans, nsamps, nbits, bias, m);
  return m;
}

RfiMask RfiCleaner::clean_packed(uint8_t* d_packed, int nchans, uint64_t nsamps, int nbits,
                                 const std::vector<int>& killmask) {
  const uint64_t stride = (nsamps + 255) / 256 * 256;
  const int bias = (nbits == 8) ? 128 : 0;  // DedispGeometry's
  scratch_.resize(stride * static_cast<uint64_t>(nchans));
  kern::unpack_transpose(d_packed, nsamps, nchans, nbits, scratch_.data(), stride, bias, stream_);
  RfiMask m = clean(scratch_.data(), stride, nchans, nsamps, nbits, bias, killmask);
  kern::pack_transpose(scratch_.data(), stride, nsamps, nchans, nbits, bias, d_packed, stream_);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  return m;
}

// ------------------------------------------------------------ pipeline ----
RfiRun run_rfi_pipeline(const RfiCmdLineOptions& args) {
  RfiRun run;
  Stopwatch t_total, t_read, t_clean, t_write;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  const RfiParams p = rfi_params_from(args);
  t_read.start();
  Filterbank fb = Filterbank::from_file(args.infilename);
  const SigprocHeader& hdr = fb.header();
  const uint64_t nsamps = fb.nsamps();
  const uint64_t bytes = nsamps * fb.bytes_per_sample();
  PSOUP_CHECK(nsamps > 0 && bytes <= fb.data_bytes(), "rficlean: empty or truncated filterbank");
  std::vector<int> kill(static_cast<size_t>(hdr.nchans), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, hdr.nchans);
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  Stream stream;
  DeviceBuffer<uint8_t> d_packed(bytes);
  staged_upload(
      bytes, 64ull << 20, [&](uint64_t off, uint64_t n, uint8_t* dst) { fb.read_data(off, n, dst); }, d_packed.data(),
      stream.get());
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream.get()));
  t_read.stop();
  t_clean.start();
  RfiCleaner cleaner(p, stream.get());
  run.mask = cleaner.clean_packed(d_packed.data(), hdr.nchans, nsamps, hdr.nbits, kill);
  t_clean.stop();
  log_verbose("rfi: " + std::to_string(run.mask.flagged_chans()) + " channels, " +
              std::to_string(run.mask.flagged_blocks()) + " blocks, " + std::to_string(run.mask.flagged_cells()) +
              " of " + std::to_string(run.mask.cell.size()) + " cells flagged");
  t_write.start();
  if (!args.outfilename.empty()) {
    // the header bytes verbatim, then the cleaned data block
    std::vector<char> head(static_cast<size_t>(hdr.size));
    {
      std::ifstream in(args.infilename, std::ios::binary);
      PSOUP_CHECK(static_cast<bool>(in.read(head.data(), static_cast<std::streamsize>(head.size()))),
                  "cannot read the header of " << args.infilename);
    }
    std::vector<uint8_t> data(bytes);
    PSOUP_HIP_CHECK(hipMemcpy(data.data(), d_packed.data(), bytes, hipMemcpyDeviceToHost));
    const std::string tmp = args.outfilename + ".tmp";
    FILE* fo = std::fopen(tmp.c_str(), "wb");
    PSOUP_CHECK(fo != nullptr, "cannot open output " << tmp);
    const bool ok = std::fwrite(head.data(), 1, head.size(), fo) == head.size() &&
                    std::fwrite(data.data(), 1, data.size(), fo) == data.size();
    if (std::fclose(fo) != 0 || !ok) {
      std::remove(tmp.c_str());
      PSOUP_THROW("cannot write output " << tmp);
    }
    PSOUP_CHECK(std::rename(tmp.c_str(), args.outfilename.c_str()) == 0,
                "cannot rename " << tmp << " to " << args.outfilename);
  }
  if (!args.maskfilename.empty()) {
    RfiMaskHeader h;
    h.nbits = static_cast<uint32_t>(hdr.nbits);
    h.tsamp = hdr.tsamp;
    write_rfi_mask(args.maskfilename, run.mask, p, h);
  }
  if (!args.killoutfilename.empty()) write_killfile(args.killoutfilename, run.mask.killmask);
  t_write.stop();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["cleaning"] = t_clean.get_time();
  run.timers["writing"] = t_write.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
