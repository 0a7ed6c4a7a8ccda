// `jerksearch`: the acceleration search repeated over jerk trials, each a
// dedispersed row re-indexed by a cubic (psoup/jerk.hpp).  One device.
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/jerk.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  JerkCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_jerk_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    JerkRun run = run_jerk_pipeline(args);
    write_jerk_output(args, run.setup, run.candidates);
    if (args.search.verbose)
      std::cout << "jerksearch: " << run.candidates.size() << " candidates from " << run.jerk_trials
                << " DM-jerk trials (" << run.accel_trials << " acceleration trials) to " << args.outfilename << " ("
                << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "jerksearch: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
