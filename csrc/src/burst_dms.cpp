// The DM rows of a candidate (psoup/burstcube.hpp), shared by the burst cutouts
// and cubeopt.  A translation unit of its own with no device code, so that
// host-only programs link it without the cutter.
#include <algorithm>

#include "psoup/burstcube.hpp"

namespace psoup {

std::vector<float> burst_dms(float dm, int ndm, float dm_half_range) {
  PSOUP_CHECK(ndm >= 1, "burst cube: ndm must be at least 1");
  const double d = static_cast<double>(dm);
  const double half = dm_half_range > 0 ? std::min(d, static_cast<double>(dm_half_range)) : d;
  const double step = 2.0 * half / ndm;
  std::vector<float> out(static_cast<size_t>(ndm));
  for (int j = 0; j < ndm; ++j)
    out[static_cast<size_t>(j)] = static_cast<float>(std::max(0.0, d + static_cast<double>(j - ndm / 2) * step));
  return out;
}

}  // namespace psoup
