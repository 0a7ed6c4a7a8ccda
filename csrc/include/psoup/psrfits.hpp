// fits2fil: read one search-mode PSRFITS file into the 8-bit, descending-
// frequency SIGPROC filterbank every other tool reads, an extension beyond the
// reference.  Decode kernel in csrc/kernels/psrfits.hip, the host steps (FITS
// parser, rows, band, header, polarisations, the mmap reader) in
// csrc/src/psrfits_host.cpp, FitsDigitiser and the file pipeline in
// csrc/src/psrfits.cpp, CLI bin/fits2fil (csrc/apps/fits_main.cpp).
//
// Definition.
//
// File layout.  FITS blocks are 2880 bytes and cards are 80 characters: key in
// columns 1-8, "= " in 9-10, the value from column 11 (a string between single
// quotes, '' standing for one quote and trailing blanks dropped; otherwise the
// text up to a '/', trimmed; D as an exponent letter counts as E).  A header
// ends at END and is padded to a block; the data area of each HDU is padded to
// a block.  Everything is big-endian.
//  - The primary HDU must have OBS_MODE = 'SEARCH'.  Keys used: TELESCOP,
//    SRC_NAME, RA, DEC, STT_IMJD, STT_SMJD, STT_OFFS, and BEAM_ID when present.
//  - HDUs are skipped by NAXIS1 x NAXIS2 + PCOUNT (0 when NAXIS = 0), padded to
//    a block, until the BINTABLE with EXTNAME = 'SUBINT'.
//  - Keys used from the SUBINT HDU: NAXIS1 (row bytes), NAXIS2 (rows), TFIELDS,
//    TTYPEn, TFORMn, NPOL, POL_TYPE, TBIN, NBITS, NCHAN, NSBLK, ZERO_OFF,
//    SIGNINT, CHAN_BW.
//  - Column byte offsets are the running sum of the TFORM sizes (rB 1 byte, rI
//    2, rJ 4, rE 4, rD 8, rA 1, rX ceil(r / 8), each times the repeat r, which
//    is 1 when not written).  Their total must equal NAXIS1.
//  - Columns used: OFFS_SUB (D, optional); DAT_FREQ (E or D, NCHAN entries);
//    DAT_WTS (E, NCHAN entries); DAT_OFFS and DAT_SCL (E, NPOL x NCHAN
//    entries, order [pol][chan]); DATA (B or I) whose size in bytes must be
//    NSBLK x NPOL x NCHAN x NBITS / 8.
//
// Samples.  DATA of a row is raw[s][p][c], s < NSBLK, p < NPOL, c < NCHAN,
// flattened in that order.  NBITS < 8 is unsigned and packed most-significant
// bits first (the first sample of a byte sits in its top bits); NCHAN x NBITS
// must be a multiple of 8.  NBITS = 8 is one byte, two's complement when
// SIGNINT = 1, else unsigned.  NBITS = 16 is two bytes big-endian, signed when
// SIGNINT = 1, else unsigned.  z = |float(ZERO_OFF)|, the magnitude as PRESTO
// takes it; z = 0 when the key is absent, does not parse or is not finite.
//
// Polarisations.  With --pol auto: NPOL = 1 uses polarisation 0; POL_TYPE
// starting AABB (case-insensitive) sums polarisations 0 and 1; IQUV uses
// polarisation 0; any other type with NPOL > 1 is refused unless --pol P
// names one.  --pol P (0 <= P < NPOL) takes that polarisation alone.
//
// Rows and time.  Rows occupy output slots of NSBLK samples:
//   slot_i = rint((OFFS_SUB[i] - OFFS_SUB[0]) / (NSBLK x TBIN))
// and rows are contiguous (slot_i = i) when the column is absent or all zero.
// Slots must increase strictly and sit within 1e-3 of a whole row; nslots =
// slot_last + 1 must not exceed 2 x NAXIS2; nsamps = nslots x NSBLK must be
// below 2^31 (nsamples is an int in SigprocHeader).  An output slot without a
// row is a dropped row.
//
// Decode (device, double, no FMA contraction).  For sample t in row slot k with
// file row r, offset s and channel c:
//   u_p = (double(raw[s][p][c]) - double(z)) * double(SCL[r][p][c]) + double(OFFS[r][p][c])
//   v   = (u_a [+ u_b]) * double(WTS[r][c])
//   x[t][c] = float32(v)     // round to nearest even, subnormals kept, overflow to +-inf
// Every operation is correctly rounded.  x[t][c] is the quiet NaN 0x7fc00000
// when the slot has no row, when WTS[r][c] == 0, and (refinement: the sign and
// payload of a NaN an operation produces differ between processors) whenever v
// is a NaN.  --no_scales, --no_offsets and --no_weights substitute 1, 0 and 1
// for the respective columns.  A non-finite scale, offset or weight gives a
// non-finite x; fildigi excludes those from the statistics, counts them in
// nbad and writes 128 for them.  The conversions float -> double of the tables
// and double -> float of v are done so that the kernel's denormal mode does
// not matter (a subnormal goes through integer arithmetic).
//
// Then fildigi's steps 1 to 6 (psoup/digi.hpp), unchanged, on x as float32
// input: --sigma_out, --scale channel|file, --rescale_blocks and -k (input
// channel order) work as they do for fildigi.  The band flips when foff > 0.  A
// channel whose weight is 0 in every present row is killed before anything is
// launched (not with --no_weights).  --kill_out is written in output channel
// order.
//
// Band.  f[c] is DAT_FREQ of the first row, as double.  fch1 = f[0]; foff =
// (f[NCHAN-1] - f[0]) / (NCHAN - 1), or CHAN_BW when NCHAN = 1.  The file is
// refused when any |f[c] - (fch1 + c foff)| > 0.01 |foff|, or when foff = 0.
//
// Header written.  source_name (SRC_NAME, trimmed), rawdatafile (the input's
// base name), telescope_id from TELESCOP, case-insensitive (Arecibo 1, Ooty 2,
// Nancay 3, Parkes 4, Jodrell 5, GBT 6, GMRT 7, Effelsberg 8, LOFAR 11, VLA 12,
// MeerKAT 64, anything else 0; --telescope_id N overrides), machine_id
// (--machine_id, default 0), data_type = 1, src_raj / src_dej (hh:mm:ss.s and
// +-dd:mm:ss.s as the doubles hhmmss.s = (hh 10000 + mm 100) + ss.s and
// +-ddmmss.s; 0 when the text does not parse),
//   tstart = STT_IMJD + (((STT_SMJD + STT_OFFS) + OFFS_SUB[0]) - (0.5 NSBLK) TBIN) / 86400
// in double in that order, OFFS_SUB[0] taken as (0.5 NSBLK) TBIN when the
// column is absent or zero; tsamp = TBIN, fch1 and foff after digi_band,
// nchans, nbits = 8, nifs = 1, nsamples, barycentric = 0, and ibeam when
// BEAM_ID parses as an integer.  The file is written to a temporary name and
// renamed.
//
// Refused by name, before anything is launched: not FITS (no SIMPLE = T),
// OBS_MODE not SEARCH, no SUBINT table, a missing required key or column,
// NBITS not in 1/2/4/8/16, NCHAN x NBITS not a multiple of 8, a DATA column of
// the wrong size, a DAT_* column of the wrong length, column sizes that do not
// add up to NAXIS1, a table that runs past the end of the file, NAXIS2 = 0,
// the row and slot violations, the band violations, the polarisation cases,
// fildigi's parameter refusals, no live channel.
//
// Out of scope: 32-bit float DATA, several files of one observation, gaps that
// are not whole rows, NSUBOFFS, fold-mode files, reading PSRFITS directly in
// the search tools, output widths below 8 bits.
//
// FitsDigitiser::run works in time chunks of whole 4096-sample statistics
// blocks sized to a device-memory budget.  Per chunk it uploads the DATA fields
// and tables of the rows the chunk touches, decodes them and forms the block
// sums; after the host scale a second pass decodes again and requantises.  A
// file that is one chunk is decoded once and stays resident.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "psoup/common.hpp"
#include "psoup/digi.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// ------------------------------------------------------------- kernel ----
namespace kern {

constexpr int kFitsGroup = 8;            // adjacent channels a thread owns
constexpr int kFitsThreads = 256;        // 64 groups along the channels x 4 sample lanes
constexpr int kFitsBlockSamples = 128;   // samples of one row slot a workgroup walks
constexpr int kFitsMaxSlots = 65535;     // row slots per launch (grid.y)

// The rows a time range touches, on the device.  Local row i is file row
// row0 + i of the upload; every pointer is to device memory.
struct FitsDecodeArgs {
  const uint8_t* data = nullptr;      // [nrows][NSBLK x NPOL x NCHAN x NBITS / 8], the DATA fields as in the file
  const float* scl = nullptr;         // [nrows][npol][nchan], host byte order
  const float* offs = nullptr;        // [nrows][npol][nchan]
  const float* wts = nullptr;         // [nrows][nchan]
  const int32_t* slot_row = nullptr;  // [nslots]: the local row of slot k0 + i, or -1 for a dropped slot
  int nrows = 0;
  int nsblk = 0, npol = 0, nchan = 0, nbits = 0, is_signed = 0;
  int pol_a = 0, pol_b = -1;  // pol_b < 0: one polarisation
  double z = 0.0;
};
// Samples [t0, t0 + count) -> out: float [count][nchan] time-major.  slot_row
// covers slots t0 / nsblk ... (t0 + count - 1) / nsblk in that order; the
// caller has checked that its entries are -1 or below nrows.  One launch per
// kFitsMaxSlots slots; returns the number of launches.
int fits_decode(const FitsDecodeArgs& a, uint64_t t0, uint64_t count, float* out, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
// fits2fil options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct FitsCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string killfilename;
  std::string killoutfilename;  // --kill_out
  double sigma_out = 16.0;
  std::string scale = "channel";  // channel | file
  int rescale_blocks = 0;
  std::string pol = "auto";  // auto | P
  bool no_scales = false, no_offsets = false, no_weights = false;
  int telescope_id = -1;  // -1: from TELESCOP
  int machine_id = 0;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_fits2fil.fil" in UTC.
std::string default_fits_output_filename();
bool parse_fits_cmdline(FitsCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);

// What of the options reaches the conversion itself.
struct FitsOptions {
  int pol = -1;  // -1: auto
  bool no_scales = false, no_offsets = false, no_weights = false;
  int telescope_id = -1;
  int machine_id = 0;
};
// Throws by name when --pol is neither auto nor a non-negative integer.
FitsOptions fits_options_from(const FitsCmdLineOptions& args);
DigiParams fits_digi_params_from(const FitsCmdLineOptions& args);

// ----------------------------------------------------------- host steps ----
// TFORM "rT": the repeat (1 when absent) and the type letter; bytes = the
// field's size.  Throws "unsupported TFORM" for anything else.
struct FitsTform {
  uint64_t repeat = 1;
  char type = 0;
  uint64_t bytes = 0;
};
FitsTform fits_tform(const std::string& s);

struct FitsColumn {
  std::string name;
  FitsTform form;
  uint64_t offset = 0;  // bytes from the start of a row
};

// One header: the cards' keys and values in order (strings unquoted).
struct FitsCards {
  std::vector<std::pair<std::string, std::string>> kv;
  const std::string* find(const std::string& key) const;
  // Required keys: throw "missing key" by name.
  std::string str(const std::string& key, const char* hdu) const;
  double num(const std::string& key, const char* hdu) const;
  int64_t integer(const std::string& key, const char* hdu) const;
};

// Everything fits_parse learns from the headers.
struct FitsLayout {
  FitsCards primary, subint;
  uint64_t table_off = 0;  // first byte of the SUBINT table
  uint64_t row_bytes = 0;  // NAXIS1
  uint64_t nrows = 0;      // NAXIS2
  int npol = 0, nbits = 0, nchan = 0, nsblk = 0, signint = 0;
  double tbin = 0, chan_bw = 0;
  double z = 0;  // |float(ZERO_OFF)| or 0
  std::string pol_type;
  std::vector<FitsColumn> columns;
  int c_offs_sub = -1, c_dat_freq = -1, c_dat_wts = -1, c_dat_offs = -1, c_dat_scl = -1, c_data = -1;
  uint64_t data_bytes() const {
    return static_cast<uint64_t>(nsblk) * static_cast<uint64_t>(npol) * static_cast<uint64_t>(nchan) *
           static_cast<uint64_t>(nbits) / 8;
  }
};
// Cards, TFORM, column offsets and every structural refusal, on bytes [p, p +
// n); reads nothing outside them.
FitsLayout fits_parse(const uint8_t* p, uint64_t n);

// Rows and time.  offs_sub empty = the column is absent.
struct FitsSlots {
  std::vector<int64_t> slot;      // [nrows]
  std::vector<int32_t> slot_row;  // [nslots]: file row or -1
  uint64_t nslots = 0, nsamps = 0, ndropped = 0;
  double offs_sub0 = 0;  // as tstart takes it
};
FitsSlots fits_row_slots(const std::vector<double>& offs_sub, uint64_t nrows, int nsblk, double tbin);

// Band from the first row's DAT_FREQ.
struct FitsBand {
  double fch1 = 0, foff = 0;
};
FitsBand fits_band(const std::vector<double>& freq, double chan_bw);

// Polarisations: {a, b}, b = -1 when one is taken.  pol = -1 is auto.
std::pair<int, int> fits_pols(int npol, const std::string& pol_type, int pol);

int fits_telescope_id(const std::string& telescop);
// "hh:mm:ss.s" or "+-dd:mm:ss.s" -> hhmmss.s / +-ddmmss.s; 0 when it does not parse.
double fits_sexagesimal(const std::string& s);
// The output's header (fch1 / foff already through digi_band).
SigprocHeader fits_header(const FitsLayout& lay, const FitsSlots& slots, const FitsBand& band, const FitsOptions& opt,
                          const std::string& rawdatafile);

// ---------------------------------------------------------------- reader ----
// A search-mode PSRFITS file in memory (mapped read-only, or a caller's
// buffer), parsed and validated; the small columns come back in host byte order.
class PsrfitsFile {
 public:
  // Throw by name: fits_parse's, fits_row_slots' and fits_band's refusals.
  static PsrfitsFile from_file(const std::string& filename);
  static PsrfitsFile from_memory(const uint8_t* p, uint64_t n);
  const FitsLayout& layout() const { return lay_; }
  const FitsSlots& slots() const { return slots_; }
  const FitsBand& band() const { return band_; }
  const uint8_t* bytes() const { return base_; }
  uint64_t size() const { return size_; }
  const uint8_t* row(uint64_t r) const { return base_ + lay_.table_off + r * lay_.row_bytes; }
  const uint8_t* row_data(uint64_t r) const { return row(r) + lay_.columns[lay_.c_data].offset; }
  // Column `col` of row r as floats (E) or doubles (E or D), n entries.
  void read_floats(uint64_t r, int col, size_t n, float* dst) const;
  void read_doubles(uint64_t r, int col, size_t n, double* dst) const;

 private:
  void init(const uint8_t* p, uint64_t n);
  std::shared_ptr<void> owner_;
  const uint8_t* base_ = nullptr;
  uint64_t size_ = 0;
  FitsLayout lay_;
  FitsSlots slots_;
  FitsBand band_;
};

// ------------------------------------------------------------- digitiser ----
struct FitsResult {
  DigiResult digi;  // chunks, tables, scale, nbad, nclip, killmask (output order)
  uint64_t rows = 0, nslots = 0, ndropped = 0;
  int pol_a = 0, pol_b = -1;
  double z = 0;
  SigprocHeader header;
};

class FitsDigitiser {
 public:
  static constexpr size_t kDefaultBudgetBytes = size_t(2) << 30;
  // file: the whole PSRFITS file in host memory.  budget_bytes: device bytes
  // the DATA fields, the decoded samples and the output of one time chunk may
  // hold (a chunk is at least L samples).  Validates everything (the file,
  // the options, the parameters, the killmask's size, a live channel) and
  // throws by name; launches and uploads nothing.
  FitsDigitiser(const uint8_t* file, uint64_t nbytes, const FitsOptions& opt, const std::vector<int>& killmask,
                const DigiParams& p, const std::string& rawdatafile, hipStream_t stream,
                size_t budget_bytes = kDefaultBudgetBytes);
  // Decode and fildigi's steps 1 to 6 into h_y: nsamps * nchan bytes in host
  // memory.  Synchronises the stream.
  FitsResult run(uint8_t* h_y);
  uint64_t nsamps() const { return file_.slots().nsamps; }
  int nchan() const { return file_.layout().nchan; }
  uint64_t chunk_samples() const { return chunk_; }
  uint64_t launches() const { return nlaunch_; }  // kernel launches so far
  const SigprocHeader& header() const { return header_; }

  // The kernel alone on device memory with a host slot table (the torch op's
  // path): checks the table against nrows, uploads it, launches and
  // synchronises the stream.  slot_row covers the slots of [t0, t0 + count).
  static void decode(kern::FitsDecodeArgs a, const std::vector<int32_t>& slot_row, uint64_t t0, uint64_t count,
                     float* d_out, hipStream_t stream);

 private:
  PsrfitsFile file_;
  FitsOptions opt_;
  std::vector<int> kill_;  // [nchan] input order, zero-weight channels included
  DigiParams p_;
  hipStream_t stream_;
  std::pair<int, int> pols_;
  SigprocHeader header_;
  bool flip_ = false;
  uint64_t chunk_ = 0, nlaunch_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct FitsRun {
  FitsResult result;
  std::map<std::string, double> timers;  // reading, converting, writing, total (s)
};
// Maps the file, applies the killfile, converts on the current device and
// writes the .fil (temporary file + rename) and, with --kill_out, the killfile
// in output channel order.
FitsRun run_fits_pipeline(const FitsCmdLineOptions& args);

}  // namespace psoup
