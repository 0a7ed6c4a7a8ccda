// `orbopt`: refines orbsearch candidates by folding their dedispersed rows on a
// dense local grid of circular-orbit templates (psoup/orbopt.hpp).  One device.
#include <cstdio>
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/orbopt.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  OrbOptCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_oopt_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    OrbOptRun run = run_orbopt_pipeline(args);
    if (args.verbose) {
      std::printf("# period opt_period dm acc pb opt_pb a1 opt_a1 phase opt_phase width snr snr_in flags\n");
      for (const OrbOptResult& r : run.results) std::printf("%s\n", oopt_verbose_line(r).c_str());
      std::cout << "orbopt: " << run.results.size() << " candidates x " << run.header.npb << " x " << run.header.na1
                << " x " << run.header.nphase << " templates x " << run.header.np << " drift trials -> "
                << args.outfilename << " (" << run.timers["total"] << " s)" << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "orbopt: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
