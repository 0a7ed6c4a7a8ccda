// `burstcube`: cuts the dedispersed waterfall and the DM-time plane around
// each single-pulse candidate out of the filterbank, an extension beyond the
// reference (psoup/burstcube.hpp).
#include <iostream>

#include "psoup/burstcube.hpp"
#include "psoup/common.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  BurstCubeCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_burst_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    BurstRun run = run_burst_pipeline(args);
    if (args.verbose)
      std::cout << "Burst cutouts: " << run.candidates.size() << " candidates x (" << run.header.nsub << " subbands + "
                << run.header.ndm << " DM rows) x " << run.header.ntime << " time bins -> " << args.outfilename << " ("
                << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "burstcube: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
