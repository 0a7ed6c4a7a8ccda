// `orbsearch`: the acceleration search repeated over circular-orbit templates,
// each a dedispersed row re-indexed by the Roemer delay (psoup/orbit.hpp).  One
// device.
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/orbit.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  OrbitCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_orbit_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    OrbitRun run = run_orbit_pipeline(args);
    write_orbit_output(args, run.setup, run.candidates);
    if (args.search.verbose)
      std::cout << "orbsearch: " << run.candidates.size() << " candidates from " << run.template_trials
                << " DM-template trials (" << run.accel_trials << " acceleration trials) to " << args.outfilename
                << " (" << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "orbsearch: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
