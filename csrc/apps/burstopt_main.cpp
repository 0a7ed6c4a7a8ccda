// `burstopt`: searches DM rows, boxcar widths and start bins on the burst
// cutouts of `burstcube`, an extension beyond the reference
// (psoup/burstopt.hpp).
#include <cstdio>
#include <iostream>

#include "psoup/burstopt.hpp"
#include "psoup/common.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  BurstOptCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_bopt_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    BurstOptRun run = run_bopt_pipeline(args);
    if (args.verbose) {
      std::printf("# sample opt_sample width opt_width dm opt_dm snr snr_coarse snr_in snr_dm0 frac_pos\n");
      for (size_t i = 0; i < run.results.size(); ++i) {
        const BurstOptResult& r = run.results[i];
        const BurstOptInput& c = run.candidates[i];
        std::printf("%llu %lld %u %u %.6g %.6g %.3f %.3f %.3f %.3f %.3f\n", static_cast<unsigned long long>(c.sample),
                    static_cast<long long>(r.opt_sample), c.width, r.opt_width, c.dm, r.opt_dm, r.snr, r.snr_coarse,
                    r.snr_in, r.snr_dm0, r.frac_pos);
      }
      std::cout << "Burst optimiser: " << run.results.size() << " candidates x (" << run.header.ndm << " + "
                << run.header.nfine << ") rows -> " << args.outfilename << " (" << run.timers["total"] << " s)"
                << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "burstopt: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
