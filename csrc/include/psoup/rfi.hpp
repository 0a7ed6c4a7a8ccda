// RFI excision on the device filterbank: a block-statistics mask and a
// zero-DM filter, deterministic and integer-exact.  Kernels in
// csrc/kernels/rfi.hip, the host flagging step and the mask file in
// csrc/src/rfi.cpp, the cleaner and the file pipeline in
// csrc/src/rfi_clean.cpp, CLI bin/rficlean (csrc/apps/rfi_main.cpp).
//
// Definition.  Raw samples x[c][t] in 0..V, V = 2^nbits - 1, c < nchans,
// t < nsamps; the device rows hold x - bias.  Input killmask k[c] (0 = killed).
// Block length L samples, a multiple of 256 in [256, 65536];
// nblk = ceil(nsamps / L), len_b the length of block b (the last may be short).
//
// 1. Block sums (device): S1[c][b] = sum x, S2[c][b] = sum x^2 over block b,
//    exact, as uint64.
// 2. Flags (host, double, only correctly rounded operations on exact integers):
//      m = S1 / len_b,  v = (len_b S2 - S1^2) / (len_b len_b)  (integer numerator)
//    For each channel with k[c] = 1: median and MAD of m over its blocks, the
//    same for v (the median of an even count is the mean of the two middle
//    values, as numpy.median).  With s = (thresh * 1.4826) * MAD, cell (c, b)
//    is flagged if |m - med_m| > s_m or |v - med_v| > s_v; where a MAD is 0
//    the cell is flagged iff the value differs from the median.  A channel
//    whose med_v is 0 (dead) has every cell flagged.  Promotion, from the cell
//    flags as they stand before any promotion: channel c is flagged whole if
//    (flagged blocks) / nblk > chan_frac; block b is flagged whole if
//    (flagged live channels) / (live channels) > block_frac.  Killed channels
//    have all cells flagged and count in no share.
// 3. Fill value: f_c = rdiv(sum S1, sum len_b) over the unflagged cells of c,
//    rdiv(a, n) = floor((2a + n) / (2n)); f_c = 0 for a channel without an
//    unflagged cell, and such channels are cleared in the output killmask.
// 4. Apply (device).  Without zero-DM: y = x in an unflagged cell, else f_c.
//    With zero-DM, for sample t of block b: A_b the channels whose cell (c, b)
//    is unflagged, n_b = |A_b|, Z_t = sum_{c in A_b} x[c][t],
//    zbar_t = rdiv(Z_t, n_b) (0 if n_b = 0), G_b = rdiv(sum_{c in A_b} f_c, n_b)
//    (host), y = clamp(x - zbar_t + G_b, 0, V) for c in A_b; flagged cells
//    get f_c.  The bit width never changes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/common.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

// Samples per workgroup of rfi_apply.  It divides every legal block length,
// so a tile lies in exactly one block.
constexpr int kRfiTile = 256;
static_assert(256 % kRfiTile == 0, "rfi_apply reads one row of flags per tile: the tile must divide every block length");
constexpr int kRfiMaxChans = 32768;  // the tile's cell flags are staged in LDS (one byte per channel)

// rows: int8 [nchans][stride] (x - bias), 16-byte aligned, stride a multiple
// of 16 and >= nsamps.  S1, S2: uint64 [nchans][nblk], raw sums.
void rfi_block_sums(const int8_t* rows, uint64_t stride, int nchans, uint64_t nsamps, uint64_t block, int bias,
                    uint64_t* S1, uint64_t* S2, hipStream_t s);
// cell_t: uint8 [nblk][nchans] final cell flags (block-major), fill: int32
// [nchans] raw f_c, G and nb: int32 [nblk] (read with zero_dm only), nflag:
// int32 [nblk] flagged cells of each block.  dst may equal rows (in place);
// both obey the layout above with their own strides.
void rfi_apply(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans, uint64_t nsamps,
               uint64_t block, int nbits, int bias, bool zero_dm, const uint8_t* cell_t, const int32_t* fill,
               const int32_t* G, const int32_t* nb, const int32_t* nflag, hipStream_t s);
// The inverse of unpack_transpose: channel-major int8 rows (x - bias) ->
// time-major SIGPROC bytes, LSB-first, nbits 1 / 2 / 4 / 8.
void pack_transpose(const int8_t* rows, uint64_t stride, uint64_t nsamps, int nchans, int nbits, int bias,
                    uint8_t* packed, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
struct RfiParams {
  uint64_t block = 4096;  // L, samples
  double thresh = 5.0;
  double chan_frac = 0.3;
  double block_frac = 0.3;
  bool zero_dm = false;
};
// Throws unless block is a multiple of 256 in [256, 65536] and the other
// parameters are finite and non-negative.
void rfi_check_params(const RfiParams& p);

// rficlean options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct RfiCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string killfilename;
  std::string maskfilename;     // --mask_out
  std::string killoutfilename;  // --kill_out
  int rfi_block = 4096;
  double rfi_thresh = 5.0;
  double rfi_chan_frac = 0.3;
  double rfi_block_frac = 0.3;
  bool zero_dm = false;
  bool verbose = false;
};
bool parse_rfi_cmdline(RfiCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);
RfiParams rfi_params_from(const RfiCmdLineOptions& args);

// ----------------------------------------------------------------- mask ----
struct RfiMask {
  int nchans = 0;
  uint64_t nblk = 0, nsamps = 0, block = 0;
  std::vector<uint8_t> chan_flag;   // [nchans] 1 = flagged whole (killed, dead or promoted)
  std::vector<uint8_t> block_flag;  // [nblk] 1 = promoted
  std::vector<uint8_t> cell;        // [nchans][nblk] final flags
  std::vector<int32_t> fill;        // [nchans] f_c (raw)
  std::vector<int32_t> G;           // [nblk] G_b (raw)
  std::vector<int32_t> nb;          // [nblk] n_b
  std::vector<int> killmask;        // [nchans] output killmask (0 = killed)
  uint64_t flagged_cells() const;
  uint64_t flagged_chans() const;
  uint64_t flagged_blocks() const;
};

inline int64_t rfi_rdiv(int64_t a, int64_t n) { return (2 * a + n) / (2 * n); }  // a >= 0, n > 0

// The host step (2 and 3 of the definition) on the table of raw block sums
// S1, S2 [nchans][nblk]; killmask empty = all ones.
RfiMask rfi_flag(const std::vector<uint64_t>& S1, const std::vector<uint64_t>& S2, int nchans, uint64_t nsamps,
                 const std::vector<int>& killmask, const RfiParams& p);

struct RfiMaskHeader {
  uint32_t nbits = 0;
  double tsamp = 0;
};
// Little-endian: magic PSMASK01, uint32 nchans nblk nbits zero_dm, uint64
// nsamps block, double tsamp thresh chan_frac block_frac; then uint8
// chan_flag[nchans], block_flag[nblk], cell[nchans][nblk], int32
// fill[nchans], G[nblk].  Written to a temporary file and renamed.
void write_rfi_mask(const std::string& path, const RfiMask& m, const RfiParams& p, const RfiMaskHeader& h);
RfiMask read_rfi_mask(const std::string& path, RfiParams* p = nullptr, RfiMaskHeader* h = nullptr);
// One 0 / 1 per line, 0 = killed (the killfile format of -k).
void write_killfile(const std::string& path, const std::vector<int>& killmask);

// -------------------------------------------------------------- cleaner ----
class RfiCleaner {
 public:
  RfiCleaner(const RfiParams& p, hipStream_t stream);
  // Cleans int8 rows [nchans][stride] (x - bias) on the current device, in
  // place or into dst (own stride); synchronises the stream.  The rows must
  // be 16-byte aligned with strides that are multiples of 16.
  RfiMask clean(int8_t* rows, uint64_t stride, int nchans, uint64_t nsamps, int nbits, int bias,
                const std::vector<int>& killmask, int8_t* dst = nullptr, uint64_t dst_stride = 0);
  // Packed SIGPROC bytes on the device, cleaned in place: unpack_transpose
  // into a scratch buffer, clean, pack_transpose back.
  RfiMask clean_packed(uint8_t* d_packed, int nchans, uint64_t nsamps, int nbits, const std::vector<int>& killmask);
  // Step 4 alone with a given mask: set_mask, apply_uploaded, synchronise.
  void apply(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans, uint64_t nsamps,
             int nbits, int bias, const RfiMask& m);
  // The two halves: the mask's tables to the device (block-major flags through
  // pinned staging; synchronises), and the kernel launch alone (asynchronous)
  // with the tables uploaded last.
  void set_mask(const RfiMask& m);
  void apply_uploaded(const int8_t* rows, uint64_t stride, int8_t* dst, uint64_t dst_stride, int nchans,
                      uint64_t nsamps, int nbits, int bias);
  const RfiParams& params() const { return p_; }

 private:
  RfiParams p_;
  hipStream_t stream_;
  DeviceBuffer<uint64_t> sums_;
  DeviceBuffer<uint8_t> cell_t_;
  DeviceBuffer<int32_t> tab_;
  PinnedBuffer<uint8_t> h_cell_t_;
  PinnedBuffer<int32_t> h_tab_;
  size_t mask_nc_ = 0, mask_nblk_ = 0;
  uint64_t mask_nsamps_ = 0;
  DeviceBuffer<int8_t> scratch_;
};

// Comment lines ("# rfi: ...") for a text output's header.
std::string rfi_summary_comment(const RfiMask& m, const RfiParams& p);

// ------------------------------------------------------------ pipeline ----
struct RfiRun {
  RfiMask mask;
  std::map<std::string, double> timers;  // reading, cleaning, writing, total (s)
};
// Reads the filterbank, cleans it on the current device and writes the
// cleaned .fil (header bytes copied verbatim), the mask file and the killfile
// (each when its name is given; temporary file + rename).
RfiRun run_rfi_pipeline(const RfiCmdLineOptions& args);

}  // namespace psoup
