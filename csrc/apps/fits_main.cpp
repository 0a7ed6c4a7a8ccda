// `fits2fil`: read one search-mode PSRFITS file into an 8-bit, descending-
// frequency SIGPROC filterbank (psoup/psrfits.hpp).
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/psrfits.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  FitsCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_fits_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    FitsRun run = run_fits_pipeline(args);
    if (args.verbose) {
      const FitsResult& f = run.result;
      const DigiResult& r = f.digi;
      uint64_t nbad = 0;
      for (uint64_t b : r.nbad) nbad += b;
      std::cout << "fits2fil: " << f.rows << " rows, " << f.ndropped << " dropped slots, polarisations " << f.pol_a;
      if (f.pol_b >= 0) std::cout << "+" << f.pol_b;
      std::cout << ", z " << f.z << ", " << r.nsamps << " samples x " << r.nchans << " channels, nbad " << nbad
                << ", nclip " << r.nclip << ", " << r.scale.nlive << " of " << r.nchans << " channels live, gains "
                << r.scale.gain_min << " to " << r.scale.gain_max << " (" << run.timers["total"] << " s)" << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "fits2fil: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
