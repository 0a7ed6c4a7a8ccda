// `spsearch`: single-pulse (transient) search over DM trials, an extension
// beyond the reference (psoup/singlepulse.hpp).
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/singlepulse.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  SpCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_sp_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    SpResult res = run_sp_pipeline(args);
    write_sp_output(args.outfilename, args, res);
    if (args.verbose)
      std::cout << "Single-pulse search: " << res.dm_list.size() << " DM trials, " << res.events << " events, "
                << res.candidates.size() << " candidates -> " << args.outfilename << " (" << res.timers["total"]
                << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "spsearch: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
