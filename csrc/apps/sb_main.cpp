// `sbsearch`: the sideband (phase-modulation) search for orbits shorter than
// the observation: short FFTs of the normalised powers of each whitened
// spectrum (psoup/sideband.hpp).  One device.
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/sideband.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  SbCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_sb_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    SbRun run = run_sb_pipeline(args);
    write_sb_output(args, run.setup, run.candidates);
    if (args.search.verbose)
      std::cout << "sbsearch: " << run.candidates.size() << " candidates from " << run.events << " events of "
                << run.setup.search.dm_list.size() << " DM trials to " << args.outfilename << " ("
                << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "sbsearch: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
