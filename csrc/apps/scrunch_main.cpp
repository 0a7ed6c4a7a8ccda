// `filscrunch`: subband and time-scrunch a filterbank into an 8-bit SIGPROC
// file (psoup/scrunch.hpp); with --plan, print the time-scrunch tiers over
// [0, --dm_end] from the header alone.
#include <cstdio>
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/scrunch.hpp"
#include "psoup/sigproc.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  ScrunchCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_scrunch_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    if (args.plan) {
      const SigprocHeader h = read_header_file(args.infilename);
      for (const ScrunchTier& t : scrunch_plan(h.tsamp, h.fch1, h.foff, h.nchans, args.dm_end))
        std::printf("%.6f %.6f %d\n", t.dm_lo, t.dm_hi, t.tscrunch);
      return 0;
    }
    ScrunchRun run = run_scrunch_pipeline(args);
    if (args.verbose) {
      const ScrunchScale& sc = run.result.scale;
      std::cout << "filscrunch: " << run.result.nout << " samples x " << run.result.nsub << " subbands, mul " << sc.mul
                << ", sigma_ref " << sc.sigma_ref << ", " << sc.nlive << " of " << run.result.nsub
                << " subbands live (" << run.timers["total"] << " s)\nM:";
      for (int32_t m : sc.M) std::cout << " " << m;
      std::cout << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "filscrunch: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
