// `foldcube`: folds the filterbank into subint x subband x phase cubes for a
// list of periodicity candidates, an extension beyond the reference
// (psoup/foldcube.hpp).
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/foldcube.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  FoldCubeCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_cube_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    CubeRun run = run_cube_pipeline(args);
    if (args.verbose)
      std::cout << "Fold cubes: " << run.candidates.size() << " candidates x " << run.header.nints << " subints x "
                << run.header.nsub << " subbands x " << run.header.nbins << " bins over " << run.header.fold_nsamps
                << " samples -> " << args.outfilename << " (" << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "foldcube: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
