// fildigi: digitise an 8 / 16 / 32-bit SIGPROC filterbank of either band order
// into the 8-bit, descending-frequency file every other tool reads, an
// extension beyond the reference.  Kernels in csrc/kernels/digi.hip, the host
// steps (parameters, scale, band flip) in csrc/src/digi_host.cpp, the raw
// reader, Digitiser and the file pipeline in csrc/src/digi.cpp, CLI bin/fildigi
// (csrc/apps/digi_main.cpp).
//
// Definition.  Samples x[t][c], t < nsamps, c < nchans, time-major as in the
// file: nbits 8 (unsigned, or signed when the header's `signed` is 1), 16
// (unsigned little-endian) or 32 (IEEE float little-endian); nifs = 1; foff of
// either sign.  Input killmask k[c] (0 = killed).  L = 4096 samples per
// statistics block, nblk = ceil(nsamps / L); the last block may be short.
//
// 1. Block quantum.  For float input, per (channel, block), amax is the largest
//    |x| over the block's finite samples and e its biased exponent field, a
//    subnormal amax counting as e = 1:
//      E = e - 127 - 22        (floor(log2(amax)) - 22 for a normal amax)
//    so |x| / 2^E < 2^23.  E = 0 when amax is 0, when the block has no finite
//    sample, and for integer input.
//      q[t][c] = int32(rint(double(x) * 2^-E))      (round half to even)
//    The scaling is exact; integer input gives q = x.  A maximum does not
//    depend on the order and the scaling by a power of two is exact, so
//    everything after this step is integer.
// 2. Block sums (device).  Per (c, b), over finite samples only: N (uint32),
//    S1 = sum q (int64), S2 = sum q^2 (uint64; below 2^58).  nbad[c], the
//    count of non-finite samples, is nsamps - sum_b N[c][b].
// 3. Scale (host; double, only correctly rounded operations on exact integers,
//    no FMA contraction).  For every block with N > 0:
//      m = ldexp(S1 / N, E)      v = ldexp((N S2 - S1^2) / N^2, 2 E)
//    with the numerator formed exactly in 128-bit integers and converted to
//    double once.  Per channel and interval (4.), med_m and med_v are the
//    medians over those blocks (an even count takes the mean of the two middle
//    values, as numpy.median).  A channel is live in an interval if it is not
//    killed, has such a block there, and med_v > 0.
//      --scale channel (default; flattens the bandpass):
//          gain[c] = sigma_out / sqrt(med_v[c])
//      --scale file (keeps the channel weights, as filscrunch does):
//          gain = sigma_out / median over the interval's live c of sqrt(med_v[c])
//      mean[c] = med_m[c]
// 4. Intervals.  rescale_blocks J = 0 (default): one interval for the file.
//    Otherwise block b belongs to interval j = b / J, nint = ceil(nblk / J),
//    the last may be short.  mean and gain are piecewise constant per interval
//    (steps at the interval edges).  A channel live in no interval is dead; a
//    file with no live channel is refused.
// 5. Requantise (device, double, no FMA contraction):
//      y = clamp(rint((double(x) - mean) * gain) + 128, 0, 255)
//    two correctly rounded operations and a round half to even.  A non-finite
//    sample gives 128; a killed channel, a dead channel or a channel not live
//    in the sample's interval gives 128.  nclip is the count of outputs whose
//    value before the clamp was below 0 or above 255, one total.
// 6. Band order.  With foff > 0 output channel c' = nchans - 1 - c,
//    fch1' = fch1 + (nchans - 1) foff and foff' = -foff; otherwise the band is
//    unchanged.  -k refers to input channels; --kill_out is written in output
//    order, in the -k format, with 0 for killed or dead channels.
// 7. Output: every header key of the input is written again with nbits = 8,
//    `signed` dropped, fch1 / foff as in 6. and nsamples unchanged (where the
//    key was present).  The body is y time-major, written to a temporary file
//    and renamed.
//
// Refused by name before anything is launched: nbits not in 8/16/32, nifs != 1,
// foff == 0, sigma_out <= 0, J < 0, a file shorter than one sample, no live
// channel (every channel killed; data without variance is refused after the
// sums pass, before anything is requantised).
//
// Digitiser::run works in time chunks of whole blocks sized to a device-memory
// budget: one pass of uploads for the block sums, the host step, a second pass
// of uploads for the requantisation.  A file that is one chunk is uploaded
// once and stays resident.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "psoup/common.hpp"
#include "psoup/sigproc.hpp"

namespace psoup {

// ------------------------------------------------------------- kernels ----
namespace kern {

constexpr int kDigiStatBlock = 4096;  // L: samples per statistics block
constexpr int kDigiTile = 64;         // adjacent channels per workgroup of digi_block_sums
constexpr int kDigiThreads = 256;

// Sample type of the input.
enum class DigiType : int { U8 = 0, I8 = 1, U16 = 2, F32 = 3 };
inline int digi_type_bytes(DigiType t) { return t == DigiType::F32 ? 4 : (t == DigiType::U16 ? 2 : 1); }

// x: rows [count][nchans] of `type`, time-major, holding samples [t0, t0 +
// count) of a file of nsamps samples; t0 a multiple of L.  Writes the cells
// (c, b) of blocks b in [t0 / L, ceil((t0 + count) / L)) of N (uint32), S1
// (int64), S2 (uint64) and E (int32), all [nchans][nblk], by plain stores.
// Uses 16-byte loads when the rows are 16-byte aligned (x aligned and
// nchans * bytes a multiple of 16), scalar loads otherwise.
void digi_block_sums(const void* x, DigiType type, uint64_t count, int nchans, uint64_t t0, uint32_t* N, int64_t* S1,
                     uint64_t* S2, int32_t* E, uint64_t nblk, hipStream_t s);
// x as above -> y: uint8, count * nchans bytes time-major in output order (the
// band reversed when flip), 16-byte aligned with room for the byte count
// rounded up to 16.  tab: double2 {mean, gain} [nint][nchans] in input channel
// order, gain 0 where the channel is not live; the interval of sample t is
// J ? (t / L) / J : 0 and must be below nint.  nclip (one uint64, zeroed by
// the caller) takes one atomic add per workgroup.
void digi_quant(const void* x, DigiType type, uint64_t count, int nchans, uint64_t t0, int J, int nint,
                const double2* tab, bool flip, uint8_t* y, unsigned long long* nclip, hipStream_t s);

}  // namespace kern

// -------------------------------------------------------------- options ----
enum class DigiScaleMode : int { Channel = 0, File = 1 };

struct DigiParams {
  double sigma_out = 16.0;
  DigiScaleMode scale = DigiScaleMode::Channel;
  int rescale_blocks = 0;  // J: blocks per interval, 0 = one interval
};
// Throws by name unless sigma_out > 0 (finite) and rescale_blocks >= 0.
void digi_check_params(const DigiParams& p);
// Throws by name unless the header can be digitised: nbits in 8/16/32,
// nifs == 1 (0 counts as 1), foff != 0, nchans >= 1; returns the sample type.
kern::DigiType digi_check_header(int nbits, int is_signed, int nifs, double foff, int nchans);

// fildigi options.  Declared here and not in cli.hpp, which is part of the
// checkpoint's numerics build id; parsed in cli.cpp with the other CLIs.
struct DigiCmdLineOptions {
  std::string infilename;
  std::string outfilename;
  std::string killfilename;
  std::string killoutfilename;  // --kill_out
  double sigma_out = 16.0;
  std::string scale = "channel";  // channel | file
  int rescale_blocks = 0;
  bool verbose = false;
};
// "%Y-%m-%d-%H:%M_fildigi.fil" in UTC.
std::string default_digi_output_filename();
bool parse_digi_cmdline(DigiCmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now = nullptr);
DigiParams digi_params_from(const DigiCmdLineOptions& args);

// ----------------------------------------------------------- host steps ----
inline uint64_t digi_nblk(uint64_t nsamps) { return (nsamps + kern::kDigiStatBlock - 1) / kern::kDigiStatBlock; }
inline int digi_nint(uint64_t nblk, int J) {
  return J > 0 ? static_cast<int>((nblk + static_cast<uint64_t>(J) - 1) / static_cast<uint64_t>(J)) : 1;
}

struct DigiScale {
  int nint = 0;
  std::vector<double> mean, gain;  // [nint][nchans], input channel order; gain 0 where not live
  std::vector<uint8_t> live;       // [nint][nchans]
  std::vector<int> alive;          // [nchans] input order: 1 = live in some interval (0 = killed or dead)
  int nlive = 0;                   // channels live in some interval
  double gain_min = 0, gain_max = 0;  // over the live cells
};
// Steps 3 and 4 on the block tables N, S1, S2, E [nchans][nblk] (killmask
// empty = none killed).  Throws "no live channel" when nothing is live.
DigiScale digi_scale(const std::vector<uint32_t>& N, const std::vector<int64_t>& S1, const std::vector<uint64_t>& S2,
                     const std::vector<int32_t>& E, int nchans, uint64_t nblk, const std::vector<int>& killmask,
                     const DigiParams& p);

// Step 6: the output's fch1 and foff.
struct DigiBand {
  bool flip = false;
  double fch1 = 0, foff = 0;
};
DigiBand digi_band(double fch1, double foff, int nchans);
// Step 7: the output's header from the input's.
SigprocHeader digi_header(const SigprocHeader& in);

// ---------------------------------------------------------------- reader ----
// A SIGPROC filterbank of 8, 16 or 32 bits, memory-mapped read-only.
// (Filterbank, the reader of the search tools, admits 1/2/4/8 bits only.)
class RawFilterbank {
 public:
  // Throws by name: digi_check_header's refusals and "shorter than one sample".
  static RawFilterbank from_file(const std::string& filename);
  const SigprocHeader& header() const { return hdr_; }
  const uint8_t* data() const { return data_; }
  uint64_t nsamps() const { return nsamps_; }
  int nchans() const { return hdr_.nchans; }
  kern::DigiType type() const { return type_; }
  uint64_t bytes_per_sample() const {
    return static_cast<uint64_t>(hdr_.nchans) * static_cast<uint64_t>(kern::digi_type_bytes(type_));
  }

 private:
  SigprocHeader hdr_;
  std::shared_ptr<void> owner_;
  const uint8_t* data_ = nullptr;
  uint64_t nsamps_ = 0;
  kern::DigiType type_ = kern::DigiType::U8;
};

// ------------------------------------------------------------- digitiser ----
struct DigiResult {
  uint64_t nsamps = 0, nblk = 0, nclip = 0;
  int nchans = 0, chunks = 0;
  bool flip = false;
  std::vector<uint32_t> N;  // [nchans][nblk]
  std::vector<int64_t> S1;
  std::vector<uint64_t> S2;
  std::vector<int32_t> E;
  std::vector<uint64_t> nbad;  // [nchans]
  DigiScale scale;
  std::vector<int> killmask;  // [nchans] in output order (0 = killed or dead)
};

class Digitiser {
 public:
  static constexpr size_t kDefaultBudgetBytes = size_t(2) << 30;
  // h_x: the file's samples in host memory, [nsamps][nchans] of `type`.
  // budget_bytes: device bytes the input and output of one time chunk may
  // hold (a chunk is at least L samples).  Validates everything (parameters,
  // foff != 0, nsamps >= 1, the killmask's size, an unkilled channel) and
  // throws by name; launches and uploads nothing.
  Digitiser(const void* h_x, kern::DigiType type, uint64_t nsamps, int nchans, double foff,
            const std::vector<int>& killmask, const DigiParams& p, hipStream_t stream,
            size_t budget_bytes = kDefaultBudgetBytes);
  // Steps 1 to 6 into h_y: nsamps * nchans bytes in host memory.
  // Synchronises the stream.
  DigiResult run(uint8_t* h_y);
  uint64_t chunk_samples() const { return chunk_; }
  uint64_t launches() const { return nlaunch_; }  // kernel launches so far

  // The two kernels alone on device memory with explicit host tables (the
  // torch ops' path); both synchronise the stream.  sums: d_x [nsamps][nchans]
  // -> d_N, d_S1, d_S2, d_E [nchans][ceil(nsamps / L)].
  static void sums(const void* d_x, kern::DigiType type, uint64_t nsamps, int nchans, uint32_t* d_N, int64_t* d_S1,
                   uint64_t* d_S2, int32_t* d_E, hipStream_t stream);
  // quant: mean, gain [nint][nchans] (gain 0 = not live) -> d_y (nsamps *
  // nchans bytes rounded up to 16, 16-byte aligned); returns nclip.
  static uint64_t quant(const void* d_x, kern::DigiType type, uint64_t nsamps, int nchans, int J,
                        const std::vector<double>& mean, const std::vector<double>& gain, bool flip, uint8_t* d_y,
                        hipStream_t stream);

 private:
  const uint8_t* x_;
  kern::DigiType type_;
  uint64_t nsamps_;
  int nchans_;
  bool flip_;
  std::vector<int> kill_;
  DigiParams p_;
  hipStream_t stream_;
  uint64_t chunk_ = 0, nlaunch_ = 0;
};

// ------------------------------------------------------------ pipeline ----
struct DigiRun {
  DigiResult result;
  std::map<std::string, double> timers;  // reading, digitising, writing, total (s)
};
// Maps the filterbank, applies the killfile, digitises on the current device
// and writes the .fil (temporary file + rename) and, with --kill_out, the
// killfile in output channel order.
DigiRun run_digi_pipeline(const DigiCmdLineOptions& args);

}  // namespace psoup
