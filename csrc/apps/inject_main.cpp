// `filinject`: add dispersed pulsars and single bursts to a SIGPROC filterbank
// of 1, 2, 4 or 8 bits and write one of the same width (psoup/inject.hpp).
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/inject.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  InjectCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_inject_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    InjectRun run = run_inject_pipeline(args);
    if (args.verbose) {
      const InjectResult& r = run.result;
      std::cout << "filinject: " << r.nsamps << " samples x " << r.nchans << " channels, " << run.signals.size()
                << " signals, nclip " << r.nclip << ", " << r.nlive << " of " << r.nchans << " channels live, "
                << r.chunks << " chunk(s) (" << run.timers["total"] << " s)" << std::endl;
      for (size_t i = 0; i < run.signals.size(); ++i)
        std::cout << "  signal " << i << " (" << (run.signals[i].kind == InjectKind::Burst ? "burst" : "pulsar")
                  << "): " << r.touched[i] << " samples touched, " << r.truth[i].npulses << " pulses, peak "
                  << r.truth[i].peak << " levels, expected S/N " << r.truth[i].snr << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "filinject: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
