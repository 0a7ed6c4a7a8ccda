// `rficlean`: block-statistics RFI mask and zero-DM filter of a filterbank
// (psoup/rfi.hpp); writes the cleaned .fil, the mask file and a killfile.
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/rfi.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  RfiCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_rfi_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    RfiRun run = run_rfi_pipeline(args);
    if (args.verbose)
      std::cout << "RFI excision: " << run.mask.flagged_chans() << " of " << run.mask.nchans << " channels, "
                << run.mask.flagged_blocks() << " of " << run.mask.nblk << " blocks, " << run.mask.flagged_cells()
                << " of " << run.mask.cell.size() << " cells flagged (" << run.timers["total"] << " s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "rficlean: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
