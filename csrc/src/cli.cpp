#include "psoup/cli.hpp"
#include "psoup/burstcube.hpp"
#include "psoup/burstopt.hpp"
#include "psoup/cubeopt.hpp"
#include "psoup/digi.hpp"
#include "psoup/inject.hpp"
#include "psoup/jerk.hpp"
#include "psoup/orbit.hpp"
#include "psoup/orbopt.hpp"
#include "psoup/sideband.hpp"
#include "psoup/psrfits.hpp"
#include "psoup/foldcube.hpp"
#include "psoup/rfi.hpp"
#include "psoup/scrunch.hpp"
#include "psoup/singlepulse.hpp"

#include <cstdlib>
#include <ctime>
#include <functional>
#include <iostream>
#include <sstream>

namespace psoup {

namespace {

struct Spec {
  std::string shortf;  // without '-'
  std::string longf;   // without '--'
  std::string help;
  bool is_switch;
  bool required;
  std::function<bool(const std::string&)> set;  // returns false on bad value
  std::function<void()> flip;                    // for switches
};

template <class T>
bool parse_num(const std::string& s, T& out) {
  std::istringstream ss(s);
  T v;
  ss >> v;
  if (ss.fail()) return false;
  std::string rest;
  ss >> rest;
  if (!rest.empty()) return false;
  out = v;
  return true;
}

bool parse_uint(const std::string& s, unsigned int& out) {
  if (!s.empty() && s[0] == '-') return false;
  unsigned long long v;
  if (!parse_num(s, v)) return false;
  out = static_cast<unsigned int>(v);
  return true;
}

Spec val_s(const char* s, const char* l, const char* help, std::string& dst, bool required = false) {
  return Spec{s, l, help, false, required, [&dst](const std::string& v) { dst = v; return true; }, nullptr};
}
template <class T>
Spec val_n(const char* s, const char* l, const char* help, T& dst) {
  return Spec{s, l, help, false, false, [&dst](const std::string& v) { return parse_num(v, dst); }, nullptr};
}
Spec val_u(const char* s, const char* l, const char* help, unsigned int& dst) {
  return Spec{s, l, help, false, false, [&dst](const std::string& v) { return parse_uint(v, dst); }, nullptr};
}
Spec sw(const char* s, const char* l, const char* help, bool& dst) {
  return Spec{s, l, help, true, false, nullptr, [&dst]() { dst = true; }};
}

std::string usage_of(const std::string& prog, const std::vector<Spec>& specs, const std::string& positional) {
  std::ostringstream os;
  os << "USAGE: \n\n   " << prog;
  for (const auto& s : specs) {
    os << " ";
    if (!s.required) os << "[";
    os << (s.shortf.empty() ? "--" + s.longf : "-" + s.shortf);
    if (!s.is_switch) os << " <value>";
    if (!s.required) os << "]";
  }
  if (!positional.empty()) os << " <" << positional << "> ...";
  os << "\n\nWhere: \n\n";
  for (const auto& s : specs) {
    os << "   ";
    if (!s.shortf.empty()) os << "-" << s.shortf << ",  ";
    os << "--" << s.longf << "\n     " << s.help << "\n\n";
  }
  os << "   -h,  --help\n     Displays usage information and exits.\n\n";
  os << "   --version\n     Displays version information and exits.\n";
  return os.str();
}

// Generic parser.  positional != nullptr collects unlabeled arguments.
bool run_parser(const std::vector<Spec>& specs, const std::vector<std::string>& argv, const std::string& title,
                std::vector<std::string>* positional, bool* exit_now) {
  if (exit_now) *exit_now = false;
  std::vector<bool> seen(specs.size(), false);
  auto find_short = [&](const std::string& f) -> int {
    for (size_t i = 0; i < specs.size(); ++i)
      if (!specs[i].shortf.empty() && specs[i].shortf == f) return static_cast<int>(i);
    return -1;
  };
  auto find_long = [&](const std::string& f) -> int {
    for (size_t i = 0; i < specs.size(); ++i)
      if (specs[i].longf == f) return static_cast<int>(i);
    return -1;
  };
  const std::string prog = argv.empty() ? "peasoup" : argv[0];
  for (size_t i = 1; i < argv.size(); ++i) {
    const std::string& a = argv[i];
    if (a == "-h" || a == "--help") {
      std::cout << title << "\n\n" << usage_of(prog, specs, positional ? "filterbanks" : "") << std::endl;
      if (exit_now) *exit_now = true;
      return true;
    }
    if (a == "--version") {
      std::cout << "\n" << prog << "  version: 1.0\n" << std::endl;
      if (exit_now) *exit_now = true;
      return true;
    }
    int idx = -1;
    std::string value;
    bool has_value = false;
    if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
      std::string name = a.substr(2);
      auto eq = name.find('=');
      if (eq != std::string::npos) {
        value = name.substr(eq + 1);
        name = name.substr(0, eq);
        has_value = true;
      }
      idx = find_long(name);
      if (idx < 0) {
        std::cerr << "Error: Couldn't find match for argument " << a << std::endl;
        return false;
      }
    } else if (a.size() > 1 && a[0] == '-' && !(std::isdigit(static_cast<unsigned char>(a[1])) || a[1] == '.')) {
      std::string name = a.substr(1);
      idx = find_short(name);
      if (idx < 0) {
        // combined switches, e.g. -vp
        bool all = true;
        for (char ch : name) {
          int k = find_short(std::string(1, ch));
          if (k < 0 || !specs[k].is_switch) {
            all = false;
            break;
          }
        }
        if (!all) {
          std::cerr << "Error: Couldn't find match for argument " << a << std::endl;
          return false;
        }
        for (char ch : name) {
          int k = find_short(std::string(1, ch));
          specs[k].flip();
          seen[k] = true;
        }
        continue;
      }
    } else {
      if (positional) {
        positional->push_back(a);
        continue;
      }
      std::cerr << "Error: Couldn't find match for argument " << a << std::endl;
      return false;
    }
    const Spec& s = specs[idx];
    if (s.is_switch) {
      if (has_value) {
        std::cerr << "Error: switch " << a << " takes no value" << std::endl;
        return false;
      }
      s.flip();
      seen[idx] = true;
      continue;
    }
    if (!has_value) {
      if (i + 1 >= argv.size()) {
        std::cerr << "Error: Missing a value for this argument! for arg " << a << std::endl;
        return false;
      }
      value = argv[++i];
    }
    if (!s.set(value)) {
      std::cerr << "Error: Couldn't read argument value from string '" << value << "' for arg " << a << std::endl;
      return false;
    }
    seen[idx] = true;
  }
  for (size_t i = 0; i < specs.size(); ++i) {
    if (specs[i].required && !seen[i]) {
      std::cerr << "Error: Required argument missing: " << (specs[i].shortf.empty() ? "" : "-" + specs[i].shortf + ", ")
                << "--" << specs[i].longf << std::endl;
      return false;
    }
  }
  return true;
}

}  // namespace

std::string default_outdir() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "./%Y-%m-%d-%H:%M_peasoup/", std::gmtime(&t));
  return std::string(buf);
}

static std::vector<Spec> peasoup_specs(CmdLineOptions& a) {
  return {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outdir", "The output directory", a.outdir),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_s("z", "zapfile", "Birdie list file", a.zapfilename),
      val_n("t", "num_threads", "The number of GPUs to use", a.max_num_threads),
      val_n("", "limit", "upper limit on number of candidates to write out", a.limit),
      val_u("", "fft_size", "Transform size to use (defaults to lower power of two)", a.size),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      val_n("", "acc_start", "First acceleration to resample to", a.acc_start),
      val_n("", "acc_end", "Last acceleration to resample to", a.acc_end),
      val_n("", "acc_tol", "Acceleration smearing tolerance (1.11=10%)", a.acc_tol),
      val_n("", "acc_pulse_width", "Minimum pulse width for which acc_tol is valid", a.acc_pulse_width),
      val_n("", "boundary_5_freq", "Frequency at which to switch from median5 to median25", a.boundary_5_freq),
      val_n("", "boundary_25_freq", "Frequency at which to switch from median25 to median125", a.boundary_25_freq),
      val_n("n", "nharmonics", "Number of harmonic sums to perform", a.nharmonics),
      val_n("", "npdmp", "Number of candidates to fold and pdmp", a.npdmp),
      val_n("m", "min_snr", "The minimum S/N for a candidate", a.min_snr),
      val_n("", "min_freq", "Lowest Fourier freqency to consider", a.min_freq),
      val_n("", "max_freq", "Highest Fourier freqency to consider", a.max_freq),
      val_n("", "max_harm_match", "Maximum harmonic for related candidates", a.max_harm),
      val_n("", "freq_tol", "Tolerance for distilling frequencies (0.0001 = 0.01%)", a.freq_tol),
      sw("v", "verbose", "verbose mode", a.verbose),
      sw("p", "progress_bar", "Enable progress bar for DM search", a.progress_bar),
      // MI355X-native extensions
      val_s("", "accel_convention", "Acceleration-plan unit convention: legacy (default, golden) | reference",
            a.accel_convention),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
      val_n("", "accel_batch", "Acceleration trials per batched FFT (0 = auto)", a.accel_batch),
      val_n("", "engines_per_gpu",
            "Search engines per GPU, each on its own stream and host thread, dealt every N-th DM of a chunk "
            "(0 = auto: Python driver 3 when DMs have < 128 acceleration trials, else 1; native pipeline 1)",
            a.engines_per_gpu),
      val_s("", "dm_schedule",
            "Multi-rank DM distribution (python -m peasoup_amd under torchrun): dynamic = ranks claim DM chunks "
            "from a shared first-come queue, like the reference's DMDispenser; static = contiguous shards balanced "
            "by acceleration-trial count; auto = dynamic when the list has >= 4 chunks per rank",
            a.dm_schedule),
      val_n("", "accel_slices",
            "Multi-rank Python driver: acceleration-trial slices per DM work unit, so DMs with many trials "
            "spread over the ranks (0 = auto: split when the job has fewer than 4 DM chunks per rank; 1 = never)",
            a.accel_slices),
      val_n("", "sub_batch", "Fused-FFT trials per sub-batch on two alternating streams (0 = off, -1 = auto)",
            a.sub_batch),
      val_n("", "fft_mode", "Accel-trial FFT: 2 = fused resample + four-step FFT (default), 1 = rocFFT C2C(N/2), 0 = rocFFT R2C",
            a.fft_mode),
      sw("", "use_boundaries", "Honour --boundary_* in the running median (reference ignores them)",
         a.use_boundaries),
      val_s("", "checkpoint_dir", "Spill per-DM candidates here and resume from it", a.checkpoint_dir),
      val_s("", "trace_json", "Write per-stage timings as JSON to this file", a.trace_json),
      val_n("", "fault_after_dms", "Testing: abort after this many DM trials", a.fault_after_dms),
      sw("", "time_shards",
         "Python driver under torchrun: each rank holds only its time slice of the filterbank; ring halo exchange "
         "+ all-to-all corner turn to DM shards (series too long to replicate on every GPU)",
         a.time_shards),
  };
}

bool parse_cmdline(CmdLineOptions& args, const std::vector<std::string>& argv, bool* exit_now) {
  args.outdir = default_outdir();
  auto specs = peasoup_specs(args);
  return run_parser(specs, argv, "Peasoup - a GPU pulsar search pipeline", nullptr, exit_now);
}

bool parse_cmdline(CmdLineOptions& args, int argc, const char* const* argv, bool* exit_now) {
  std::vector<std::string> v(argv, argv + argc);
  return parse_cmdline(args, v, exit_now);
}

std::string cmdline_usage() {
  CmdLineOptions a;
  return usage_of("peasoup", peasoup_specs(a), "");
}

bool parse_coincidencer_cmdline(CoincidencerOptions& a, int argc, const char* const* argv, bool* exit_now) {
  std::vector<Spec> specs = {
      val_s("", "o", "Sample mask output filename", a.samp_outfilename),
      val_s("", "o2", "Birdie list output filename", a.spec_outfilename),
      val_n("l", "boundary_5_freq", "Frequency at which to switch from median5 to median25", a.boundary_5_freq),
      val_n("a", "boundary_25_freq", "Frequency at which to switch from median25 to median125", a.boundary_25_freq),
      val_n("n", "nharmonics", "Number of harmonic sums to perform", a.nharmonics),
      val_n("", "thresh", "The S/N threshold for a candidate to be considered for coincidencing matching",
            a.threshold),
      val_n("", "beam_thresh", "The number of beams a candidate must appear in to be considered multibeam",
            a.beam_threshold),
      val_n("L", "min_freq", "Lowest Fourier freqency to consider", a.min_freq),
      val_n("H", "max_freq", "Highest Fourier freqency to consider", a.max_freq),
      val_n("b", "max_harm", "Maximum harmonic for related candidates", a.max_harm),
      val_n("f", "freq_tol", "Tolerance for distilling frequencies (0.0001 = 0.01%)", a.freq_tol),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  std::vector<std::string> v(argv, argv + argc);
  if (!run_parser(specs, v, "Peasoup - a GPU pulsar search pipeline", &a.filterbanks, exit_now)) return false;
  if ((!exit_now || !*exit_now) && a.filterbanks.empty()) {
    std::cerr << "Error: Required argument missing: filterbanks" << std::endl;
    return false;
  }
  return true;
}

std::string default_ffa_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_ffaster.output", std::gmtime(&t));
  return std::string(buf);
}

bool parse_ffa_cmdline(FfaCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_ffa_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("t", "num_threads", "The number of GPUs to use", a.max_num_threads),
      val_u("", "nstreams", "The number of CUDA streams to use", a.nstreams),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      val_n("", "p_start", "Start period for FFA search", a.p_start),
      val_n("", "p_end", "End period for FFA search", a.p_end),
      val_n("", "min_dc", "Minimum duty cycle", a.min_dc),
      sw("v", "verbose", "verbose mode", a.verbose),
      sw("p", "progress_bar", "Enable progress bar for DM search", a.progress_bar),
      // MI355X-native extensions
      val_n("m", "min_snr", "Minimum boxcar S/N of a folded profile", a.min_snr),
      val_n("", "bins", "Base bins per period (periods span [bins, 2 bins)); 0 = from --min_dc", a.nbins),
      val_n("", "limit", "Upper limit on the number of candidates written", a.limit),
      val_n("", "cluster_tol", "Peak clustering tolerance in units of 1/T_obs", a.cluster_tol),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
  };
  return run_parser(specs, argv, "Peasoup/FFAster extension - a GPU FFA pulsar search pipeline", nullptr, exit_now);
}

std::string default_sp_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_spsearch.output", std::gmtime(&t));
  return std::string(buf);
}

bool parse_sp_cmdline(SpCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_sp_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("t", "num_threads", "The number of GPUs to use", a.max_num_threads),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      sw("v", "verbose", "verbose mode", a.verbose),
      sw("p", "progress_bar", "Enable progress bar for DM search", a.progress_bar),
      val_n("m", "min_snr", "Minimum boxcar S/N of a single pulse", a.min_snr),
      val_n("", "boxcar_max", "Widest boxcar in samples (widths are the powers of two up to it)", a.boxcar_max),
      val_n("", "baseline", "Length of the trend blocks in seconds", a.baseline),
      val_n("", "limit", "Upper limit on the number of candidates written", a.limit),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
      sw("", "rfi", "Clean the filterbank first: block-statistics RFI mask", a.rfi),
      sw("", "zero_dm", "Also subtract the band mean of the unflagged channels (implies --rfi)", a.zero_dm),
      val_n("", "rfi_block", "RFI block length in samples (a multiple of 256 in [256, 65536])", a.rfi_block),
      val_n("", "rfi_thresh", "RFI flagging threshold in robust sigmas (1.4826 MAD)", a.rfi_thresh),
      val_n("", "rfi_chan_frac", "Flag a channel whole above this flagged share of its blocks", a.rfi_chan_frac),
      val_n("", "rfi_block_frac", "Flag a block whole above this flagged share of its live channels",
            a.rfi_block_frac),
      val_s("", "rfi_mask_out", "RFI mask output filename", a.rfi_maskfilename),
  };
  if (!run_parser(specs, argv, "Peasoup single-pulse extension - a GPU transient search pipeline", nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.zero_dm) a.rfi = true;
  if (a.rfi_block < 256 || a.rfi_block > 65536 || a.rfi_block % 256 != 0) {
    std::cerr << "Error: --rfi_block must be a multiple of 256 in [256, 65536]" << std::endl;
    return false;
  }
  if (!(a.rfi_thresh >= 0) || !(a.rfi_chan_frac >= 0) || !(a.rfi_block_frac >= 0)) {
    std::cerr << "Error: --rfi_thresh, --rfi_chan_frac and --rfi_block_frac must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_cube_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_foldcube.cubes", std::gmtime(&t));
  return std::string(buf);
}

bool parse_cube_cmdline(FoldCubeCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_cube_output_filename();
  long long fold_nsamps = static_cast<long long>(a.fold_nsamps);
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_s("", "candfile", "Candidate list: one 'period_s dm acc' per line, '#' comments", a.candfilename),
      val_s("", "overview", "overview.xml of a finished search (python -m peasoup_amd cube only)",
            a.overviewfilename),
      val_n("", "top", "Candidates taken from the top of --overview", a.top),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("", "nints", "Subintegrations per cube (1..256)", a.nints),
      val_n("", "nsub", "Subbands per cube (1..nchans; capped at nchans)", a.nsub),
      val_n("", "nbins", "Phase bins per cube (2..256)", a.nbins),
      val_n("", "fold_nsamps", "Samples folded (0 = the largest power of two that fits every candidate)",
            fold_nsamps),
      val_n("", "limit", "At most this many candidates from the top of the list", a.limit),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup fold-cube extension - subint x subband x phase cubes of candidates", nullptr,
                  exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.candfilename.empty() == a.overviewfilename.empty()) {
    std::cerr << "Error: give exactly one of --candfile and --overview" << std::endl;
    return false;
  }
  if (a.nints < 1 || a.nints > 256) {
    std::cerr << "Error: --nints must be in 1..256" << std::endl;
    return false;
  }
  if (a.nbins < 2 || a.nbins > 256) {
    std::cerr << "Error: --nbins must be in 2..256" << std::endl;
    return false;
  }
  if (a.nsub < 1) {
    std::cerr << "Error: --nsub must be at least 1" << std::endl;
    return false;
  }
  if (fold_nsamps < 0) {
    std::cerr << "Error: --fold_nsamps must be non-negative" << std::endl;
    return false;
  }
  a.fold_nsamps = static_cast<uint64_t>(fold_nsamps);
  if (a.top < 1 || a.limit < 0) {
    std::cerr << "Error: --top must be at least 1 and --limit non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_burst_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_burstcube.bursts", std::gmtime(&t));
  return std::string(buf);
}

bool parse_burst_cmdline(BurstCubeCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_burst_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_s("", "spfile", "Candidates: an spsearch output (S/N, sample, width and DM columns)", a.spfilename),
      val_s("", "candfile", "Candidates: one 'sample width dm [snr]' per line, '#' comments", a.candfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("", "ntime", "Time bins per cutout (1..1024)", a.ntime),
      val_n("", "nsub", "Subbands of the waterfall (1..nchans; capped at nchans)", a.nsub),
      val_n("", "ndm", "DM rows of the DM-time plane (1..1024)", a.ndm),
      val_n("", "tscrunch", "Samples per time bin (0 = half the candidate's width, at least 1; at most 4096)",
            a.tscrunch),
      val_n("", "dm_half_range", "DM rows span the candidate's DM -/+ this (0 = the DM itself: rows span 0..2 DM)",
            a.dm_half_range),
      val_n("", "limit", "At most this many candidates from the top of the list", a.limit),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup burst-cutout extension - dedispersed waterfall and DM-time plane per pulse",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.spfilename.empty() == a.candfilename.empty()) {
    std::cerr << "Error: give exactly one of --spfile and --candfile" << std::endl;
    return false;
  }
  if (a.ntime < 1 || a.ntime > 1024) {
    std::cerr << "Error: --ntime must be in 1..1024" << std::endl;
    return false;
  }
  if (a.ndm < 1 || a.ndm > 1024) {
    std::cerr << "Error: --ndm must be in 1..1024" << std::endl;
    return false;
  }
  if (a.nsub < 1) {
    std::cerr << "Error: --nsub must be at least 1" << std::endl;
    return false;
  }
  if (a.tscrunch < 0 || a.tscrunch > 4096) {
    std::cerr << "Error: --tscrunch must be in 0..4096" << std::endl;
    return false;
  }
  if (!(a.dm_half_range >= 0) || a.limit < 0) {
    std::cerr << "Error: --dm_half_range and --limit must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_opt_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_cubeopt.opt", std::gmtime(&t));
  return std::string(buf);
}

bool parse_opt_cmdline(CubeOptCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_opt_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "Fold cubes to search (a foldcube output)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_n("", "ndm", "DM trials (1..256); row ndm / 2 is the candidate's DM", a.ndm),
      val_n("", "dm_half_range", "DM trials span the candidate's DM -/+ this (0 = the DM itself: 0..2 DM)",
            a.dm_half_range),
      val_n("", "np", "Period trials (odd, 1..257)", a.np),
      val_n("", "p_step", "Period step: bins of drift across the fold", a.p_step),
      val_n("", "npd", "Acceleration trials (odd, 1..129)", a.npd),
      val_n("", "pd_step", "Acceleration step: bins of curvature at the middle of the fold", a.pd_step),
      val_n("", "limit", "At most this many candidates from the top of the file", a.limit),
      sw("v", "verbose", "verbose mode: one line per candidate", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup cube-optimiser extension - DM, period and acceleration search on fold cubes",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.ndm < 1 || a.ndm > 256) {
    std::cerr << "Error: --ndm must be in 1..256" << std::endl;
    return false;
  }
  if (a.np < 1 || a.np > 257 || a.np % 2 == 0) {
    std::cerr << "Error: --np must be odd and in 1..257" << std::endl;
    return false;
  }
  if (a.npd < 1 || a.npd > 129 || a.npd % 2 == 0) {
    std::cerr << "Error: --npd must be odd and in 1..129" << std::endl;
    return false;
  }
  if (!(a.p_step >= 0) || !(a.pd_step >= 0) || !(a.dm_half_range >= 0) || a.limit < 0 || !(a.p_step < 1e6) ||
      !(a.pd_step < 1e6) || !(a.dm_half_range < 1e9f)) {
    std::cerr << "Error: --p_step, --pd_step, --dm_half_range and --limit must be finite and non-negative"
              << std::endl;
    return false;
  }
  return true;
}

std::string default_bopt_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_burstopt.bopt", std::gmtime(&t));
  return std::string(buf);
}

bool parse_bopt_cmdline(BurstOptCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_bopt_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "Burst cutouts to search (a burstcube output)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_n("", "nfine", "Fine DM rows around the candidate's DM (odd, 1..257)", a.nfine),
      val_n("", "fine_half_range", "Fine DM rows span the candidate's DM -/+ this (0 = the spacing of two coarse rows)",
            a.fine_half_range),
      val_n("", "limit", "At most this many candidates from the top of the file", a.limit),
      sw("v", "verbose", "verbose mode: one line per candidate", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup burst-optimiser extension - DM, width and time search on burst cutouts",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.nfine < 1 || a.nfine > 257 || a.nfine % 2 == 0) {
    std::cerr << "Error: --nfine must be odd and in 1..257" << std::endl;
    return false;
  }
  if (!(a.fine_half_range >= 0) || !(a.fine_half_range < 1e9) || a.limit < 0) {
    std::cerr << "Error: --fine_half_range and --limit must be finite and non-negative" << std::endl;
    return false;
  }
  return true;
}

bool parse_rfi_cmdline(RfiCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The cleaned filterbank (header bytes copied verbatim)", a.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_s("", "mask_out", "RFI mask output filename", a.maskfilename),
      val_s("", "kill_out", "Output killfile: the input mask plus every channel flagged whole", a.killoutfilename),
      val_n("", "rfi_block", "Block length in samples (a multiple of 256 in [256, 65536])", a.rfi_block),
      val_n("", "rfi_thresh", "Flagging threshold in robust sigmas (1.4826 MAD)", a.rfi_thresh),
      val_n("", "rfi_chan_frac", "Flag a channel whole above this flagged share of its blocks", a.rfi_chan_frac),
      val_n("", "rfi_block_frac", "Flag a block whole above this flagged share of its live channels",
            a.rfi_block_frac),
      sw("", "zero_dm", "Subtract the band mean of the unflagged channels from every sample", a.zero_dm),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup RFI excision - block-statistics mask and zero-DM filter", nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.rfi_block < 256 || a.rfi_block > 65536 || a.rfi_block % 256 != 0) {
    std::cerr << "Error: --rfi_block must be a multiple of 256 in [256, 65536]" << std::endl;
    return false;
  }
  if (!(a.rfi_thresh >= 0) || !(a.rfi_chan_frac >= 0) || !(a.rfi_block_frac >= 0)) {
    std::cerr << "Error: --rfi_thresh, --rfi_chan_frac and --rfi_block_frac must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_scrunch_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_filscrunch.fil", std::gmtime(&t));
  return std::string(buf);
}

bool parse_scrunch_cmdline(ScrunchCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_scrunch_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The scrunched filterbank (8 bits)", a.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("", "dm", "DM the channels of a subband are aligned to before they are added", a.dm),
      val_n("", "nsub", "Output channels; must divide nchans (0 = nchans: no subbanding)", a.nsub),
      val_n("", "tscrunch", "Input samples added per output sample (1..256)", a.tscrunch),
      val_n("", "sigma_out", "Noise sigma of a typical subband in the 8-bit output", a.sigma_out),
      val_s("", "kill_out", "Output killfile: one line per subband, 0 = not live", a.killoutfilename),
      sw("", "plan", "Print 'dm_lo dm_hi tscrunch' per tier over [0, --dm_end] and exit", a.plan),
      val_n("", "dm_end", "Last DM of the plan (--plan only)", a.dm_end),
      sw("v", "verbose", "verbose mode: print the offsets, the scale and the live count", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup filscrunch extension - subband and time-scrunch a filterbank", nullptr,
                  exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (!(a.dm >= 0) || !(a.dm < 1e9f)) {
    std::cerr << "Error: --dm must be finite and non-negative" << std::endl;
    return false;
  }
  if (a.nsub < 0) {
    std::cerr << "Error: --nsub must be at least 1 (0 = nchans)" << std::endl;
    return false;
  }
  if (a.tscrunch < 1 || a.tscrunch > 256) {
    std::cerr << "Error: --tscrunch must be in 1..256" << std::endl;
    return false;
  }
  if (!(a.sigma_out > 0) || !(a.sigma_out < 1e9)) {
    std::cerr << "Error: --sigma_out must be positive" << std::endl;
    return false;
  }
  if (a.plan && !(a.dm_end >= 0)) {
    std::cerr << "Error: --plan needs a non-negative --dm_end" << std::endl;
    return false;
  }
  return true;
}

std::string default_digi_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_fildigi.fil", std::gmtime(&t));
  return std::string(buf);
}

bool parse_digi_cmdline(DigiCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_digi_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil of 8, 16 or 32 bits, either band order)", a.infilename, true),
      val_s("o", "outfilename", "The digitised filterbank (8 bits, descending frequency)", a.outfilename),
      val_s("k", "killfile", "Channel mask file (input channel order)", a.killfilename),
      val_s("", "kill_out", "Output killfile (output channel order): 0 = killed or dead", a.killoutfilename),
      val_n("", "sigma_out", "Noise sigma of a channel in the 8-bit output", a.sigma_out),
      val_s("", "scale", "channel: one gain per channel (flattens the bandpass); file: one gain for all", a.scale),
      val_n("", "rescale_blocks", "Blocks of 4096 samples per rescaling interval (0 = one for the file)",
            a.rescale_blocks),
      sw("v", "verbose", "verbose mode: print nbad, nclip, the live count and the range of gains", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup fildigi extension - digitise a 8/16/32-bit filterbank to 8 bits", nullptr,
                  exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (!(a.sigma_out > 0) || !(a.sigma_out < 1e9)) {
    std::cerr << "Error: --sigma_out must be positive" << std::endl;
    return false;
  }
  if (a.scale != "channel" && a.scale != "file") {
    std::cerr << "Error: --scale must be channel or file" << std::endl;
    return false;
  }
  if (a.rescale_blocks < 0) {
    std::cerr << "Error: --rescale_blocks must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_inject_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_filinject.fil", std::gmtime(&t));
  return std::string(buf);
}

bool parse_inject_cmdline(InjectCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_inject_output_filename();
  std::string seed = "0";
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil of 1, 2, 4 or 8 bits)", a.infilename, true),
      val_s("o", "outfilename", "The filterbank with the signals added (same width and header)", a.outfilename),
      val_s("", "injfile", "Signals: 'pulsar period_s dm amp [duty acc phase alpha]' or 'burst time_s dm amp "
                           "[width_s alpha]' per line",
            a.injfilename, true),
      val_s("k", "killfile", "Channel mask file: killed channels are left untouched", a.killfilename),
      val_s("", "seed", "Seed of the dither (a non-negative integer)", seed),
      val_s("", "units", "sigma: amp in units of each channel's noise sigma; level: in raw levels", a.units),
      sw("", "no_smear", "Do not widen the pulses by the intra-channel DM smearing", a.no_smear),
      val_s("", "truth_out", "Truth file: one line per signal with npulses, peak level and expected S/N",
            a.truthfilename),
      sw("v", "verbose", "verbose mode: print nclip, the live count and the touched samples per signal", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup filinject extension - inject dispersed pulsars and bursts into a filterbank",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  bool digits = !seed.empty() && seed.size() <= 19;
  for (char c : seed) digits = digits && std::isdigit(static_cast<unsigned char>(c));
  if (!digits) {
    std::cerr << "Error: --seed must be a non-negative integer below 10^19" << std::endl;
    return false;
  }
  a.seed = std::stoull(seed);
  if (a.units != "sigma" && a.units != "level") {
    std::cerr << "Error: --units must be sigma or level" << std::endl;
    return false;
  }
  return true;
}

std::string default_jerk_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_jerksearch.output", std::gmtime(&t));
  return std::string(buf);
}

// a float that may be inf or nan: the refusal names it (make_jerk_setup), not the parser
static Spec val_f(const char* l, const char* help, float& dst) {
  return Spec{"", l, help, false, false,
              [&dst](const std::string& v) {
                char* end = nullptr;
                dst = std::strtof(v.c_str(), &end);
                return end != v.c_str() && *end == '\0';
              },
              nullptr};
}

bool parse_jerk_cmdline(JerkCmdLineOptions& j, const std::vector<std::string>& argv, bool* exit_now) {
  j.outfilename = default_jerk_output_filename();
  CmdLineOptions& a = j.search;
  a.max_num_threads = 1;
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", j.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_s("z", "zapfile", "Birdie list file", a.zapfilename),
      val_n("t", "num_threads", "The number of GPUs to use: only 1 (one device; no multi-rank runs, no checkpoints)",
            a.max_num_threads),
      val_n("", "limit", "upper limit on number of candidates to write out", a.limit),
      val_u("", "fft_size", "Transform size to use (defaults to lower power of two)", a.size),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      val_n("", "acc_start", "First acceleration to resample to", a.acc_start),
      val_n("", "acc_end", "Last acceleration to resample to", a.acc_end),
      val_n("", "acc_tol", "Acceleration smearing tolerance (1.11=10%)", a.acc_tol),
      val_n("", "acc_pulse_width", "Minimum pulse width for which acc_tol is valid", a.acc_pulse_width),
      val_f("jerk_start", "First jerk to resample to (m/s^3)", j.jerk_start),
      val_f("jerk_end", "Last jerk to resample to (m/s^3)", j.jerk_end),
      val_f("jerk_tol", "Jerk smearing tolerance (1.11=10%)", j.jerk_tol),
      val_f("jerk_step", "Jerk step in m/s^3 (0 = from the plan)", j.jerk_step),
      val_n("n", "nharmonics", "Number of harmonic sums to perform", a.nharmonics),
      val_n("", "npdmp", "Number of candidates to fold and pdmp", a.npdmp),
      val_n("m", "min_snr", "The minimum S/N for a candidate", a.min_snr),
      val_n("", "min_freq", "Lowest Fourier freqency to consider", a.min_freq),
      val_n("", "max_freq", "Highest Fourier freqency to consider", a.max_freq),
      val_s("", "accel_convention", "Acceleration-plan unit convention: legacy (default, golden) | reference",
            a.accel_convention),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup jerksearch extension - jerk trials around the acceleration search (one device)",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.max_num_threads != 1) {
    std::cerr << "Error: jerksearch runs on one device (-t 1); multi-GPU runs and checkpoints are not supported"
              << std::endl;
    return false;
  }
  if (a.npdmp < 0 || a.limit < 0) {
    std::cerr << "Error: --npdmp and --limit must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_orbit_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_orbsearch.output", std::gmtime(&t));
  return std::string(buf);
}

// a double that may be inf or nan: the refusal names it (make_orbit_setup), not the parser
static Spec val_d(const char* l, const char* help, double& dst) {
  return Spec{"", l, help, false, false,
              [&dst](const std::string& v) {
                char* end = nullptr;
                dst = std::strtod(v.c_str(), &end);
                return end != v.c_str() && *end == '\0';
              },
              nullptr};
}

bool parse_orbit_cmdline(OrbitCmdLineOptions& o, const std::vector<std::string>& argv, bool* exit_now) {
  o.outfilename = default_orbit_output_filename();
  CmdLineOptions& a = o.search;
  a.max_num_threads = 1;
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", o.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_s("z", "zapfile", "Birdie list file", a.zapfilename),
      val_n("t", "num_threads", "The number of GPUs to use: only 1 (one device; no multi-rank runs, no checkpoints)",
            a.max_num_threads),
      val_n("", "limit", "upper limit on number of candidates to write out", a.limit),
      val_u("", "fft_size", "Transform size to use (defaults to lower power of two)", a.size),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      val_n("", "acc_start", "First acceleration to resample to", a.acc_start),
      val_n("", "acc_end", "Last acceleration to resample to", a.acc_end),
      val_n("", "acc_tol", "Acceleration smearing tolerance (1.11=10%)", a.acc_tol),
      val_n("", "acc_pulse_width", "Minimum pulse width for which acc_tol is valid", a.acc_pulse_width),
      val_s("", "bankfile", "Template bank: lines `pb_s a1_ls phase` (# starts a comment)", o.bankfile),
      val_d("pb_start", "Grid: first orbital period (s)", o.pb_start),
      val_d("pb_end", "Grid: last orbital period (s)", o.pb_end),
      val_n("", "npb", "Grid: orbital periods, geometric from pb_start to pb_end", o.npb),
      val_d("a1_start", "Grid: first projected semi-major axis a sin i / c (light-seconds)", o.a1_start),
      val_d("a1_end", "Grid: last projected semi-major axis (light-seconds)", o.a1_end),
      val_n("", "na1", "Grid: semi-major axes, linear from a1_start to a1_end", o.na1),
      val_n("", "nphase", "Grid: orbital phases, k / nphase turns", o.nphase),
      val_n("n", "nharmonics", "Number of harmonic sums to perform", a.nharmonics),
      val_n("", "npdmp", "Number of candidates to fold and pdmp", a.npdmp),
      val_n("m", "min_snr", "The minimum S/N for a candidate", a.min_snr),
      val_n("", "min_freq", "Lowest Fourier freqency to consider", a.min_freq),
      val_n("", "max_freq", "Highest Fourier freqency to consider", a.max_freq),
      val_s("", "accel_convention", "Acceleration-plan unit convention: legacy (default, golden) | reference",
            a.accel_convention),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv,
                  "Peasoup orbsearch extension - circular-orbit templates around the acceleration search (one device)",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.max_num_threads != 1) {
    std::cerr << "Error: orbsearch runs on one device (-t 1); multi-GPU runs and checkpoints are not supported"
              << std::endl;
    return false;
  }
  if (a.npdmp < 0 || a.limit < 0) {
    std::cerr << "Error: --npdmp and --limit must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_oopt_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_orbopt.oopt", std::gmtime(&t));
  return std::string(buf);
}

bool parse_oopt_cmdline(OrbOptCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_oopt_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("c", "candfile", "Candidates: lines `period_s dm acc pb_s a1_ls phase` (an orbsearch output)",
            a.candfilename, true),
      val_s("o", "outfilename", "The output filename", a.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_n("t", "num_threads", "The number of GPUs to use: only 1 (one device)", a.max_num_threads),
      val_u("", "fft_size", "Span the candidates were found with (defaults to lower power of two)", a.size),
      val_n("", "nbins", "Phase bins (2..256)", a.nbins),
      val_n("", "nints", "Subintegrations (1..64; nints * nbins <= 16384)", a.nints),
      val_n("", "npb", "Orbital periods of the local grid (odd)", a.npb),
      val_n("", "na1", "Semi-major axes of the local grid (odd)", a.na1),
      val_n("", "nphase", "Orbital phases of the local grid (odd)", a.nphase),
      val_d("pb_step", "Step in orbital period, s (0 = about half a phase bin)", a.pb_step),
      val_d("a1_step", "Step in a sin i / c, light-seconds (0 = about half a phase bin)", a.a1_step),
      val_d("phase_step", "Step in orbital phase, turns (0 = about half a phase bin)", a.phase_step),
      val_n("", "np", "Period-drift trials (odd, 1..257)", a.np),
      val_d("p_step", "Bins of drift across the fold per trial", a.p_step),
      val_n("", "limit", "At most this many candidates from the top of the file", a.limit),
      sw("v", "verbose", "verbose mode: one line per candidate", a.verbose),
  };
  if (!run_parser(specs, argv,
                  "Peasoup orbopt extension - refine orbit candidates by folding on a local template grid (one device)",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.max_num_threads != 1) {
    std::cerr << "Error: orbopt runs on one device (-t 1); multi-GPU runs are not supported" << std::endl;
    return false;
  }
  if (a.limit < 0) {
    std::cerr << "Error: --limit must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_sb_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_sbsearch.output", std::gmtime(&t));
  return std::string(buf);
}

bool parse_sb_cmdline(SbCmdLineOptions& o, const std::vector<std::string>& argv, bool* exit_now) {
  o.outfilename = default_sb_output_filename();
  CmdLineOptions& a = o.search;
  a.max_num_threads = 1;
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (.fil)", a.infilename, true),
      val_s("o", "outfilename", "The output filename", o.outfilename),
      val_s("k", "killfile", "Channel mask file", a.killfilename),
      val_s("z", "zapfile", "Birdie list file", a.zapfilename),
      val_n("t", "num_threads", "The number of GPUs to use: only 1 (one device; no multi-rank runs, no checkpoints)",
            a.max_num_threads),
      val_n("", "limit", "upper limit on number of candidates to write out", a.limit),
      val_u("", "fft_size", "Transform size to use (defaults to lower power of two)", a.size),
      val_n("", "dm_start", "First DM to dedisperse to", a.dm_start),
      val_n("", "dm_end", "Last DM to dedisperse to", a.dm_end),
      val_n("", "dm_tol", "DM smearing tolerance (1.11=10%)", a.dm_tol),
      val_n("", "dm_pulse_width", "Minimum pulse width for which dm_tol is valid", a.dm_pulse_width),
      val_f("min_freq", "Lowest Fourier freqency to consider", a.min_freq),
      val_f("max_freq", "Highest Fourier freqency to consider", a.max_freq),
      val_f("min_power", "The minimum secondary power S for an event", o.min_power),
      val_n("", "m_min", "Smallest segment size, M = 2^m_min bins (5..13)", o.m_min),
      val_n("", "m_max", "Largest segment size, M = 2^m_max bins (5..13)", o.m_max),
      val_n("", "j_min", "Lowest bin of the secondary spectrum searched", o.j_min),
      val_f("clip", "Powers above this many band means are lowered to it", o.clip),
      val_s("", "dedisp_kernel", "Dedispersion kernel: auto | mfma | valu | direct | packed2", a.dedisp_kernel),
      sw("v", "verbose", "verbose mode", a.verbose),
  };
  if (!run_parser(specs, argv,
                  "Peasoup sbsearch extension - sideband (phase-modulation) search for short orbits (one device)",
                  nullptr, exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (a.max_num_threads != 1) {
    std::cerr << "Error: sbsearch runs on one device (-t 1); multi-GPU runs and checkpoints are not supported"
              << std::endl;
    return false;
  }
  if (a.limit < 0) {
    std::cerr << "Error: --limit must be non-negative" << std::endl;
    return false;
  }
  return true;
}

std::string default_fits_output_filename() {
  char buf[128];
  std::time_t t = std::time(nullptr);
  std::strftime(buf, sizeof(buf), "%Y-%m-%d-%H:%M_fits2fil.fil", std::gmtime(&t));
  return std::string(buf);
}

bool parse_fits_cmdline(FitsCmdLineOptions& a, const std::vector<std::string>& argv, bool* exit_now) {
  a.outfilename = default_fits_output_filename();
  std::vector<Spec> specs = {
      val_s("i", "inputfile", "File to process (search-mode PSRFITS of 1, 2, 4, 8 or 16 bits)", a.infilename, true),
      val_s("o", "outfilename", "The filterbank written (8 bits, descending frequency)", a.outfilename),
      val_s("k", "killfile", "Channel mask file (input channel order)", a.killfilename),
      val_s("", "kill_out", "Output killfile (output channel order): 0 = killed or dead", a.killoutfilename),
      val_n("", "sigma_out", "Noise sigma of a channel in the 8-bit output", a.sigma_out),
      val_s("", "scale", "channel: one gain per channel (flattens the bandpass); file: one gain for all", a.scale),
      val_n("", "rescale_blocks", "Blocks of 4096 samples per rescaling interval (0 = one for the file)",
            a.rescale_blocks),
      val_s("", "pol", "auto (AABB: sum of 0 and 1; IQUV: 0) or the index of the one polarisation to take", a.pol),
      sw("", "no_scales", "Take DAT_SCL as 1", a.no_scales),
      sw("", "no_offsets", "Take DAT_OFFS as 0", a.no_offsets),
      sw("", "no_weights", "Take DAT_WTS as 1", a.no_weights),
      val_n("", "telescope_id", "telescope_id written (default: from TELESCOP)", a.telescope_id),
      val_n("", "machine_id", "machine_id written", a.machine_id),
      sw("v", "verbose", "verbose mode: print rows, dropped slots, polarisations, z, nbad, nclip, live count, gains",
         a.verbose),
  };
  if (!run_parser(specs, argv, "Peasoup fits2fil extension - search-mode PSRFITS to an 8-bit filterbank", nullptr,
                  exit_now))
    return false;
  if (exit_now && *exit_now) return true;
  if (!(a.sigma_out > 0) || !(a.sigma_out < 1e9)) {
    std::cerr << "Error: --sigma_out must be positive" << std::endl;
    return false;
  }
  if (a.scale != "channel" && a.scale != "file") {
    std::cerr << "Error: --scale must be channel or file" << std::endl;
    return false;
  }
  if (a.rescale_blocks < 0) {
    std::cerr << "Error: --rescale_blocks must be non-negative" << std::endl;
    return false;
  }
  bool pol_ok = a.pol == "auto" || (!a.pol.empty() && a.pol.size() <= 2);
  if (a.pol != "auto")
    for (char c : a.pol) pol_ok = pol_ok && std::isdigit(static_cast<unsigned char>(c));
  if (!pol_ok) {
    std::cerr << "Error: --pol must be auto or a polarisation index" << std::endl;
    return false;
  }
  if (a.telescope_id < -1 || a.machine_id < 0) {
    std::cerr << "Error: --telescope_id and --machine_id must be non-negative" << std::endl;
    return false;
  }
  return true;
}

}  // namespace psoup
