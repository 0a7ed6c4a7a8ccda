// `fildigi`: digitise a SIGPROC filterbank of 8, 16 or 32 bits and either band
// order into an 8-bit, descending-frequency file (psoup/digi.hpp).
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/digi.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  DigiCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_digi_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    DigiRun run = run_digi_pipeline(args);
    if (args.verbose) {
      const DigiResult& r = run.result;
      uint64_t nbad = 0;
      for (uint64_t b : r.nbad) nbad += b;
      std::cout << "fildigi: " << r.nsamps << " samples x " << r.nchans << " channels, nbad " << nbad << ", nclip "
                << r.nclip << ", " << r.scale.nlive << " of " << r.nchans << " channels live, gains "
                << r.scale.gain_min << " to " << r.scale.gain_max << " (" << run.timers["total"] << " s)" << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "fildigi: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
