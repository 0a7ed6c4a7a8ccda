// `cubeopt`: searches DM, period and acceleration trials on the fold cubes of
// `foldcube`, an extension beyond the reference (psoup/cubeopt.hpp).
#include <cstdio>
#include <iostream>

#include "psoup/common.hpp"
#include "psoup/cubeopt.hpp"

using namespace psoup;

int main(int argc, char** argv) {
  CubeOptCmdLineOptions args;
  bool exit_now = false;
  std::vector<std::string> av(argv, argv + argc);
  if (!parse_opt_cmdline(args, av, &exit_now)) return 1;
  if (exit_now) return 0;
  try {
    CubeOptRun run = run_opt_pipeline(args);
    if (args.verbose) {
      std::printf("# period opt_period dm opt_dm acc opt_acc width snr snr_in snr_dm0\n");
      for (size_t i = 0; i < run.results.size(); ++i) {
        const CubeOptResult& r = run.results[i];
        const CubeOptInput& c = run.candidates[i];
        std::printf("%.12g %.12g %.6g %.6g %.6g %.6g %u %.3f %.3f %.3f\n", c.period, r.opt_period, c.dm, r.opt_dm,
                    c.acc, r.opt_acc, r.opt_width, r.snr, r.snr_in, r.snr_dm0);
      }
      std::cout << "Cube optimiser: " << run.results.size() << " candidates x " << run.header.ndm << " x "
                << run.header.np << " x " << run.header.npd << " trials -> " << args.outfilename << " ("
                << run.timers["total"] << " s)" << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "cubeopt: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
