// fits2fil, device side: the FitsDigitiser (decode -> block sums -> host scale
// -> decode -> requantise, in time chunks) and the file pipeline.  See
// psoup/psrfits.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "psoup/psrfits.hpp"
#include "psoup/rfi.hpp"

namespace psoup {

namespace {

constexpr uint64_t kL = kern::kDigiStatBlock;

void write_atomically(const std::string& path, const std::string& head, const std::vector<uint8_t>& data) {
  const std::string tmp = path + ".tmp";
  FILE* fo = std::fopen(tmp.c_str(), "wb");
  PSOUP_CHECK(fo != nullptr, "cannot open output " << tmp);
  const bool ok = std::fwrite(head.data(), 1, head.size(), fo) == head.size() &&
                  std::fwrite(data.data(), 1, data.size(), fo) == data.size();
  if (std::fclose(fo) != 0 || !ok) {
    std::remove(tmp.c_str());
    PSOUP_THROW("cannot write output " << tmp);
  }
  PSOUP_CHECK(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot rename " << tmp << " to " << path);
}

std::string base_name(const std::string& path) {
  const size_t slash = path.find_last_of('/');
  return slash == std::string::npos ? path : path.substr(slash + 1);
}

// The file rows [ra, rb) whose slots lie in [k0, k1] (slots increase with the row).
std::pair<uint64_t, uint64_t> rows_of(const std::vector<int64_t>& slot, uint64_t k0, uint64_t k1) {
  const auto a = std::lower_bound(slot.begin(), slot.end(), static_cast<int64_t>(k0));
  const auto b = std::upper_bound(slot.begin(), slot.end(), static_cast<int64_t>(k1));
  return {static_cast<uint64_t>(a - slot.begin()), static_cast<uint64_t>(b - slot.begin())};
}

}  // namespace

// ------------------------------------------------------------- digitiser ----
FitsDigitiser::FitsDigitiser(const uint8_t* file, uint64_t nbytes, const FitsOptions& opt,
                             const std::vector<int>& killmask, const DigiParams& p, const std::string& rawdatafile,
                             hipStream_t stream, size_t budget_bytes)
    : file_(PsrfitsFile::from_memory(file, nbytes)), opt_(opt), kill_(killmask), p_(p), stream_(stream) {
  digi_check_params(p);
  const FitsLayout& lay = file_.layout();
  const FitsSlots& sl = file_.slots();
  const size_t nc = static_cast<size_t>(lay.nchan);
  pols_ = fits_pols(lay.npol, lay.pol_type, opt.pol);
  PSOUP_CHECK(opt.machine_id >= 0, "fits: --machine_id must be non-negative");
  PSOUP_CHECK(killmask.empty() || killmask.size() == nc, "fits: killmask size != NCHAN");
  if (kill_.empty()) kill_.assign(nc, 1);
  // a channel whose weight is 0 in every present row is killed
  if (!opt.no_weights) {
    std::vector<uint8_t> seen(nc, 0);
    std::vector<float> w(nc);
    for (uint64_t r = 0; r < lay.nrows; ++r) {
      file_.read_floats(r, lay.c_dat_wts, nc, w.data());
      for (size_t c = 0; c < nc; ++c)
        if (w[c] != 0.0f) seen[c] = 1;
    }
    for (size_t c = 0; c < nc; ++c)
      if (!seen[c]) kill_[c] = 0;
  }
  PSOUP_CHECK(std::any_of(kill_.begin(), kill_.end(), [](int k) { return k != 0; }),
              "fits: no live channel (every channel is killed or has zero weight)");
  header_ = fits_header(lay, sl, file_.band(), opt, rawdatafile);
  flip_ = file_.band().foff > 0;
  // chunks: whole statistics blocks, at least one
  const uint64_t per_sample = static_cast<uint64_t>(lay.nchan) * 5 +
                              static_cast<uint64_t>(lay.npol) * static_cast<uint64_t>(lay.nchan) *
                                  static_cast<uint64_t>(lay.nbits) / 8 +
                              1;
  chunk_ = std::max<uint64_t>(kL, static_cast<uint64_t>(budget_bytes) / per_sample / kL * kL);
  chunk_ = std::min<uint64_t>(chunk_, 65535 * kL);  // the sums' grid
}

FitsResult FitsDigitiser::run(uint8_t* h_y) {
  PSOUP_CHECK(h_y != nullptr, "fits: no output buffer");
  const FitsLayout& lay = file_.layout();
  const FitsSlots& sl = file_.slots();
  const size_t nc = static_cast<size_t>(lay.nchan), np = static_cast<size_t>(lay.npol);
  const uint64_t nsamps = sl.nsamps, nsblk = static_cast<uint64_t>(lay.nsblk);
  const uint64_t dbytes = lay.data_bytes();
  FitsResult out;
  out.rows = lay.nrows;
  out.nslots = sl.nslots;
  out.ndropped = sl.ndropped;
  out.pol_a = pols_.first;
  out.pol_b = pols_.second;
  out.z = lay.z;
  out.header = header_;
  DigiResult& res = out.digi;
  res.nsamps = nsamps;
  res.nchans = lay.nchan;
  res.nblk = digi_nblk(nsamps);
  res.flip = flip_;
  const size_t ncell = nc * static_cast<size_t>(res.nblk);
  const uint64_t nchunks = (nsamps + chunk_ - 1) / chunk_;
  res.chunks = static_cast<int>(nchunks);

  // the most rows and slots a chunk touches
  uint64_t max_rows = 1, max_slots = 1;
  for (uint64_t t0 = 0; t0 < nsamps; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps - t0);
    const uint64_t k0 = t0 / nsblk, k1 = (t0 + count - 1) / nsblk;
    const auto rr = rows_of(sl.slot, k0, k1);
    max_rows = std::max(max_rows, rr.second - rr.first);
    max_slots = std::max(max_slots, k1 - k0 + 1);
  }
  const uint64_t xrows = std::min(chunk_, nsamps);
  DeviceBuffer<uint8_t> ddata(max_rows * dbytes);
  DeviceBuffer<float> dscl(max_rows * np * nc), doffs(max_rows * np * nc), dwts(max_rows * nc);
  DeviceBuffer<int32_t> dslot(max_slots);
  DeviceBuffer<float> dx(xrows * nc);
  DeviceBuffer<uint8_t> dy((xrows * nc + 15) / 16 * 16);
  DeviceBuffer<uint32_t> dN(ncell);
  DeviceBuffer<int64_t> dS1(ncell);
  DeviceBuffer<uint64_t> dS2(ncell);
  DeviceBuffer<int32_t> dE(ncell);
  std::vector<uint8_t> hdata;
  std::vector<float> hscl, hoffs, hwts;
  std::vector<int32_t> hslot;

  // uploads the rows of [t0, t0 + count) and decodes them into dx
  auto decode = [&](uint64_t t0, uint64_t count) {
    const uint64_t k0 = t0 / nsblk, k1 = (t0 + count - 1) / nsblk;
    const auto rr = rows_of(sl.slot, k0, k1);
    const uint64_t ra = rr.first, nr = rr.second - rr.first;
    hslot.assign(k1 - k0 + 1, -1);
    for (uint64_t k = k0; k <= k1; ++k)
      if (sl.slot_row[k] >= 0) hslot[k - k0] = sl.slot_row[k] - static_cast<int32_t>(ra);
    hdata.resize(nr * dbytes);
    hscl.assign(nr * np * nc, 1.0f);
    hoffs.assign(nr * np * nc, 0.0f);
    hwts.assign(nr * nc, 1.0f);
    for (uint64_t i = 0; i < nr; ++i) {
      std::memcpy(hdata.data() + i * dbytes, file_.row_data(ra + i), dbytes);
      if (!opt_.no_scales) file_.read_floats(ra + i, lay.c_dat_scl, np * nc, hscl.data() + i * np * nc);
      if (!opt_.no_offsets) file_.read_floats(ra + i, lay.c_dat_offs, np * nc, hoffs.data() + i * np * nc);
      if (!opt_.no_weights) file_.read_floats(ra + i, lay.c_dat_wts, nc, hwts.data() + i * nc);
    }
    if (nr > 0) {
      PSOUP_HIP_CHECK(hipMemcpyAsync(ddata.data(), hdata.data(), hdata.size(), hipMemcpyHostToDevice, stream_));
      PSOUP_HIP_CHECK(hipMemcpyAsync(dscl.data(), hscl.data(), hscl.size() * 4, hipMemcpyHostToDevice, stream_));
      PSOUP_HIP_CHECK(hipMemcpyAsync(doffs.data(), hoffs.data(), hoffs.size() * 4, hipMemcpyHostToDevice, stream_));
      PSOUP_HIP_CHECK(hipMemcpyAsync(dwts.data(), hwts.data(), hwts.size() * 4, hipMemcpyHostToDevice, stream_));
    }
    PSOUP_HIP_CHECK(hipMemcpyAsync(dslot.data(), hslot.data(), hslot.size() * 4, hipMemcpyHostToDevice, stream_));
    kern::FitsDecodeArgs a;
    a.data = ddata.data();
    a.scl = dscl.data();
    a.offs = doffs.data();
    a.wts = dwts.data();
    a.slot_row = dslot.data();
    a.nrows = static_cast<int>(nr);
    a.nsblk = lay.nsblk;
    a.npol = lay.npol;
    a.nchan = lay.nchan;
    a.nbits = lay.nbits;
    a.is_signed = lay.signint;
    a.pol_a = pols_.first;
    a.pol_b = pols_.second;
    a.z = lay.z;
    nlaunch_ += static_cast<uint64_t>(kern::fits_decode(a, t0, count, dx.data(), stream_));
  };

  // pass 1: the block sums
  for (uint64_t t0 = 0; t0 < nsamps; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps - t0);
    decode(t0, count);
    kern::digi_block_sums(dx.data(), kern::DigiType::F32, count, lay.nchan, t0, dN.data(), dS1.data(), dS2.data(),
                          dE.data(), res.nblk, stream_);
    ++nlaunch_;
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));  // the host stages are filled again next
  }
  res.N.resize(ncell);
  res.S1.resize(ncell);
  res.S2.resize(ncell);
  res.E.resize(ncell);
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.N.data(), dN.data(), ncell * 4, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.S1.data(), dS1.data(), ncell * 8, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.S2.data(), dS2.data(), ncell * 8, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipMemcpyAsync(res.E.data(), dE.data(), ncell * 4, hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  res.nbad.assign(nc, nsamps);
  for (size_t c = 0; c < nc; ++c)
    for (size_t b = 0; b < res.nblk; ++b) res.nbad[c] -= res.N[c * res.nblk + b];
  res.scale = digi_scale(res.N, res.S1, res.S2, res.E, lay.nchan, res.nblk, kill_, p_);
  res.killmask.assign(nc, 0);
  for (size_t c = 0; c < nc; ++c) res.killmask[flip_ ? nc - 1 - c : c] = res.scale.alive[c];
  // pass 2: requantise, from the resident samples (one chunk) or decoded again
  std::vector<double2> tab(res.scale.mean.size());
  for (size_t i = 0; i < tab.size(); ++i) tab[i] = make_double2(res.scale.mean[i], res.scale.gain[i]);
  DeviceBuffer<double2> dtab(tab.size());
  DeviceBuffer<unsigned long long> dclip(1);
  PSOUP_HIP_CHECK(hipMemcpyAsync(dtab.data(), tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice, stream_));
  dclip.zero_async(stream_);
  for (uint64_t t0 = 0; t0 < nsamps; t0 += chunk_) {
    const uint64_t count = std::min(chunk_, nsamps - t0);
    if (nchunks > 1) decode(t0, count);
    kern::digi_quant(dx.data(), kern::DigiType::F32, count, lay.nchan, t0, p_.rescale_blocks, res.scale.nint,
                     dtab.data(), flip_, dy.data(), dclip.data(), stream_);
    ++nlaunch_;
    PSOUP_HIP_CHECK(hipMemcpyAsync(h_y + t0 * nc, dy.data(), count * nc, hipMemcpyDeviceToHost, stream_));
    PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  unsigned long long nclip = 0;
  PSOUP_HIP_CHECK(hipMemcpyAsync(&nclip, dclip.data(), sizeof(nclip), hipMemcpyDeviceToHost, stream_));
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream_));
  res.nclip = nclip;
  return out;
}

void FitsDigitiser::decode(kern::FitsDecodeArgs a, const std::vector<int32_t>& slot_row, uint64_t t0, uint64_t count,
                           float* d_out, hipStream_t stream) {
  PSOUP_CHECK(count >= 1 && a.nsblk >= 1, "fits decode: empty range");
  const uint64_t nsblk = static_cast<uint64_t>(a.nsblk);
  const uint64_t want = (t0 + count - 1) / nsblk - t0 / nsblk + 1;
  PSOUP_CHECK(slot_row.size() == want, "fits decode: the slot table must cover the " << want << " slots of the range");
  for (int32_t r : slot_row) PSOUP_CHECK(r >= -1 && r < a.nrows, "fits decode: slot table entry " << r << " out of range");
  DeviceBuffer<int32_t> dslot(slot_row.size());
  PSOUP_HIP_CHECK(hipMemcpyAsync(dslot.data(), slot_row.data(), slot_row.size() * 4, hipMemcpyHostToDevice, stream));
  a.slot_row = dslot.data();
  kern::fits_decode(a, t0, count, d_out, stream);
  PSOUP_HIP_CHECK(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------ pipeline ----
FitsRun run_fits_pipeline(const FitsCmdLineOptions& args) {
  FitsRun run;
  Stopwatch t_total, t_read, t_work, t_write;
  t_total.start();
  if (args.verbose) set_log_level(LogLevel::Verbose);
  t_read.start();
  const DigiParams p = fits_digi_params_from(args);
  digi_check_params(p);
  const FitsOptions opt = fits_options_from(args);
  const PsrfitsFile file = PsrfitsFile::from_file(args.infilename);
  const int nchan = file.layout().nchan;
  std::vector<int> kill(static_cast<size_t>(nchan), 1);
  if (!args.killfilename.empty()) kill = read_killfile(args.killfilename, nchan);
  fits_pols(file.layout().npol, file.layout().pol_type, opt.pol);
  t_read.stop();
  t_work.start();
  PSOUP_CHECK(device_count() > 0, "no HIP devices visible");
  Stream stream;
  FitsDigitiser dig(file.bytes(), file.size(), opt, kill, p, base_name(args.infilename), stream.get());
  std::vector<uint8_t> data(dig.nsamps() * static_cast<uint64_t>(nchan));
  run.result = dig.run(data.data());
  t_work.stop();
  t_write.start();
  std::ostringstream head;
  write_header(head, run.result.header);
  write_atomically(args.outfilename, head.str(), data);
  if (!args.killoutfilename.empty()) write_killfile(args.killoutfilename, run.result.digi.killmask);
  t_write.stop();
  t_total.stop();
  run.timers["reading"] = t_read.get_time();
  run.timers["converting"] = t_work.get_time();
  run.timers["writing"] = t_write.get_time();
  run.timers["total"] = t_total.get_time();
  return run;
}

}  // namespace psoup
