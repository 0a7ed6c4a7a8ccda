// Burst cutouts: the dedispersed dynamic spectrum (waterfall) and the DM-time
// plane around each single-pulse candidate, foldcube's counterpart for
// transients and an extension beyond the reference.  Kernel in
// csrc/kernels/burstcube.hip, BurstCutter / readers / pipeline / file writer in
// csrc/src/burstcube.cpp, CLI bin/burstcube (csrc/apps/burstcube_main.cpp).
//
// Definition.  The raw sample is x[c][u] = stored int8 + bias (>= 0); N is the
// number of valid samples per row.  A candidate is (sample, width, dm): sample
// is the first sample of the boxcar in the dedispersed series (spsearch's own
// column: the dedispersed sample t at offsets o reads x[c][t + o[c]]), width
// is in samples.  Offsets are off_d[c] = int32(float(d) * delays[c] + 0.5f).
// With the parameters ntime (time bins), nsub (subbands), ndm (DM rows) and
// tscrunch:
//   f    = tscrunch if tscrunch > 0 else max(1, width / 2)   (samples per time bin)
//   tc   = sample + width / 2
//   t0   = tc - (ntime / 2) * f                              (int64, may be negative)
//   row(Cset, o), k in [0, ntime):
//     sums[k] = sum over c in Cset, i in [0, f) of x[c][u], u = t0 + k f + i + o[c],
//               only where 0 <= u < N
//     hits[k] = number of such (c, i) pairs
//   waterfall ds[s],  s in [0, nsub): Cset = unkilled c with floor(c nsub / nchans) == s, o = off_dm
//   DM-time  dmt[j],  j in [0, ndm):  Cset = every unkilled c,                            o = off_{dm_j}
//     half = dm (or min(dm, dm_half_range) when that option is > 0); step = 2 half / ndm (double)
//     dm_j = float32(max(0, double(dm) + (j - ndm / 2) * step))   (row ndm / 2 is exactly dm)
//   nactive[s] = unkilled channels of subband s
// Every output is int32 and independent of the summation order: two runs, and
// the kernel and the NumPy oracle, agree to the byte; dmt_sums[ndm / 2] ==
// ds_sums.sum(axis 0), likewise the hits.  Samples outside [0, N) contribute
// nothing and are not counted: a burst at the edge of the file, or a DM row
// whose sweep runs off the end, gives short or empty bins and is not refused.
// 32-bit bound, checked for every candidate before anything is launched:
//   255 f (unkilled channels) < 2^31     (8-bit data, 4096 channels: f <= 2048).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/common.hpp"
#include "psoup/engine.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kBurstWindow = 16384;  // bytes of a channel staged in LDS per row tile (x 2 buffers)
constexpr int kBurstMaxRows = 256;   // rows of one tile
constexpr int kBurstMaxOut = 16;     // (row, bin) outputs per lane group
constexpr int kBurstMaxF = 4096;     // samples per time bin
constexpr int kBurstThreads = 256;

// lanes that share one (row, bin) output: a power of two in 1..64
inline int burst_lanes_log2(int f) {
  int lg = 0;
  while (lg < 6 && (16 << lg) <= f) ++lg;
  return lg;
}

struct BurstJob {
  int64_t t0 = 0;         // first sample of time bin 0 at offset 0
  int32_t f = 1;          // samples per time bin
  int32_t bins_per_tile = 1;
  int32_t lanes_log2 = 0;
  int32_t pad = 0;
};

// One tile of rows that share their channels' staged windows.  The rows are
// row0 .. row0 + nrows of the candidate's nsub + ndm output rows; the channels
// are active[ia .. ie).  For its q-th channel the tile's window starts at
// win[2 (win0 + q)] (the smallest offset of its rows) and is win[2 (win0 + q)
// + 1] samples longer than one row's; row r reads rel[rel0 + q nrows + r]
// samples into it.
struct BurstTile {
  int32_t cand = 0;
  int32_t row0 = 0, nrows = 0;
  int32_t ia = 0, ie = 0;
  uint32_t rel0 = 0, win0 = 0;
  int32_t pad = 0;
};

struct BurstGeom {
  int nchans = 0;
  uint64_t stride = 0;  // bytes per row (a multiple of 16); reads stay inside a row
  uint64_t nsamps = 0;  // valid samples per row (<= stride)
  int bias = 0;
  int ntime = 0;
  int nrows = 0;        // output rows per candidate: nsub + ndm
};

// chan_major: int8 [nchans][stride], 16-byte aligned.  tiles / jobs / rel /
// win: see BurstTile (built and bounds-checked by BurstCutter).  sums and hits:
// int32 [ncand][nrows][ntime]; every element is written exactly once, by
// plain stores.  bin_tiles: the most time tiles of any job.
void burst_cube(const int8_t* chan_major, const BurstGeom& g, const int32_t* d_active, const BurstTile* d_tiles,
                uint32_t ntiles, const BurstJob* d_jobs, const int32_t* d_rel, const int32_t* d_win, int bin_tiles,
                int32_t* d_sums, int32_t* d_hits, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// burstcube options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct BurstCubeCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string spfilename;    // an spsearch output
  std::string candfilename;  // 'sample width dm [snr]' lines
  std::string killfilename;
  int ntime = 256;
  int nsub = 256;  // capped at nchans
  int ndm = 256;
  int tscrunch = 0;          // 0 = from the width
  float dm_half_range = 0;   // 0 = the candidate's DM
  int limit = 100;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_burstcube.bursts" in UTC.
std::string default_burst_output_filename();
bool parse_burst_cmdline(BurstCubeCmdLineOptions& args, const std::vector<std::string>& argv,
                         bool* exit_now = nullptr);

// --------------------------------------------------------------- cutter ----
struct BurstParams {
  int ntime = 256;
  int nsub = 256;
  int ndm = 256;
  int tscrunch = 0;
  float dm_half_range = 0;
};

struct BurstCandidate {
  uint64_t sample = 0;
  uint32_t width = 1;
  float dm = 0;
  float snr = 0;  // 0 if unknown
};

struct BurstResult {
  uint32_t tscrunch = 1;  // the f used
  int64_t t0 = 0;
  std::vector<float> dms;        // [ndm]
  std::vector<int32_t> nactive;  // [nsub]
  std::vector<int32_t> ds_sums, ds_hits;    // [nsub][ntime]
  std::vector<int32_t> dmt_sums, dmt_hits;  // [ndm][ntime]
};

// f, t0 and the DM rows of the definition above.
int burst_tscrunch(uint32_t width, int tscrunch);
int64_t burst_t0(uint64_t sample, uint32_t width, int f, int ntime);
std::vector<float> burst_dms(float dm, int ndm, float dm_half_range = 0);

// Candidate file: '#' lines skipped, else "sample width dm [snr]" (extra
// columns ignored); a malformed line is an error naming its line number.  At
// most `limit` candidates from the top (limit < 0: all).
std::vector<BurstCandidate> read_burst_candfile(const std::string& path, int limit = -1);
// An spsearch output: '#' lines skipped; the columns used are S/N (1), sample
// (2), width (4) and DM (6), the DM as printed.
std::vector<BurstCandidate> read_sp_output(const std::string& path, int limit = -1);

class BurstCutter {
 public:
  static constexpr size_t kDefaultBatchBytes = size_t(1) << 30;
  // The filterbank (and its geometry's delays, killmask, bias) must outlive
  // the cutter.  batch_bytes: device bytes a batch of candidates may hold.
  BurstCutter(const DeviceFilterbank& fb, const BurstParams& p, hipStream_t stream,
              size_t batch_bytes = kDefaultBatchBytes);
  // Raw rows: int8 [nchans][stride] at d_chan_major with explicit delays
  // (float [nchans]) and killmask (int [nchans], empty = none killed);
  // row_valid = N, the samples of a row that may be read.
  BurstCutter(const int8_t* d_chan_major, uint64_t stride, uint64_t row_valid, int nchans, int bias,
              const std::vector<float>& delays, const std::vector<int>& killmask, const BurstParams& p,
              hipStream_t stream, size_t batch_bytes = kDefaultBatchBytes);
  ~BurstCutter();
  // Validates every candidate first (nothing is launched on an error), then
  // cuts in batches; results in input order.
  std::vector<BurstResult> cut(const std::vector<BurstCandidate>& cands);
  // As cut() with explicit offsets (h_ds_offsets int32 [ncand][nchans],
  // h_dmt_offsets int32 [ncand][ndm][nchans]), t0 and f per candidate, and the
  // results left on the device: d_sums and d_hits int32 [ncand][nsub +
  // ndm][ntime], the nsub waterfall rows first.  The torch op's path.
  void cut_offsets(const int32_t* h_ds_offsets, const int32_t* h_dmt_offsets, const std::vector<int64_t>& t0,
                   const std::vector<int>& f, int32_t* d_sums, int32_t* d_hits);
  const BurstParams& params() const { return p_; }
  const std::vector<int32_t>& nactive() const { return nactive_; }
  size_t bytes_per_candidate() const;  // device bytes one candidate of a batch holds
  int batch_size() const;              // candidates per launch
  uint64_t batches() const { return nbatches_; }  // launches so far
  uint64_t tiles() const { return ntiles_; }      // row tiles launched so far
  uint64_t single_row_tiles() const { return nsingle_; }  // DM-row tiles of one row among them

 private:
  void init(const std::vector<int>& killmask);
  void check_job(size_t i, int64_t t0, int f) const;
  void launch(const int32_t* h_ds, const int32_t* h_dmt, const int64_t* t0, const int* f, int ncand, size_t first,
              int32_t* d_sums, int32_t* d_hits);
  const int8_t* x_;
  uint64_t stride_, row_valid_;
  int nchans_, bias_;
  std::vector<float> delays_;
  BurstParams p_;
  hipStream_t stream_;
  size_t batch_bytes_;
  int nactive_total_ = 0;
  std::vector<int32_t> nactive_, active_, sub_first_;
  DeviceBuffer<int32_t> d_active_, d_rel_, d_win_, d_sums_, d_hits_;
  DeviceBuffer<kern::BurstTile> d_tiles_;
  DeviceBuffer<kern::BurstJob> d_jobs_;
  uint64_t nbatches_ = 0, ntiles_ = 0, nsingle_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct BurstFileHeader {
  uint32_t ncand = 0, ntime = 0, nsub = 0, ndm = 0, nchans = 0, nbits = 0;
  uint64_t nsamps = 0;
  double tsamp = 0, fch1 = 0, foff = 0;
};

struct BurstRun {
  BurstFileHeader header;
  std::vector<BurstCandidate> candidates;
  std::vector<BurstResult> cutouts;
  std::map<std::string, double> timers;  // reading, cutting, total (s)
};
// Reads the filterbank and the candidates (--spfile or --candfile), applies
// the killfile, cuts on device 0 and writes args.outfilename.
BurstRun run_burst_pipeline(const BurstCubeCmdLineOptions& args);
// Little-endian: "PSBRST01", uint32 ncand ntime nsub ndm nchans nbits, uint64
// nsamps, double tsamp fch1 foff (64 bytes); per candidate uint64 sample,
// uint32 width, uint32 tscrunch (the f used), int64 t0, float dm, float snr,
// float dms[ndm], int32 nactive[nsub], then int32 ds_sums[nsub][ntime],
// ds_hits[nsub][ntime], dmt_sums[ndm][ntime], dmt_hits[ndm][ntime].  Written
// to a temporary file, then renamed.
void write_burst_file(const std::string& path, const BurstFileHeader& h, const std::vector<BurstCandidate>& cands,
                      const std::vector<BurstResult>& cutouts);

}  // namespace psoup
