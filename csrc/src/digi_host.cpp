// fildigi, host steps: parameters, the scale (steps 3 and 4), the band flip
// (step 6) and the header rewrite (step 7) of psoup/digi.hpp.  No device code
// here (the native unit tests link this file alone) and no FMA contraction:
// the double arithmetic is the definition's, operation by operation.
#include <algorithm>
#include <cmath>

#include "psoup/digi.hpp"

namespace psoup {

void digi_check_params(const DigiParams& p) {
  PSOUP_CHECK(std::isfinite(p.sigma_out) && p.sigma_out > 0, "digi: sigma_out must be positive");
  PSOUP_CHECK(p.rescale_blocks >= 0, "digi: rescale_blocks must be non-negative, got " << p.rescale_blocks);
  PSOUP_CHECK(p.scale == DigiScaleMode::Channel || p.scale == DigiScaleMode::File,
              "digi: scale must be channel or file");
}

kern::DigiType digi_check_header(int nbits, int is_signed, int nifs, double foff, int nchans) {
  PSOUP_CHECK(nbits == 8 || nbits == 16 || nbits == 32, "digi: nbits must be 8, 16 or 32, got " << nbits);
  PSOUP_CHECK(nifs == 1 || nifs == 0, "digi: nifs must be 1, got " << nifs);
  PSOUP_CHECK(std::isfinite(foff) && foff != 0, "digi: foff must not be zero");
  PSOUP_CHECK(nchans >= 1, "digi: no channels");
  if (nbits == 32) return kern::DigiType::F32;
  if (nbits == 16) return kern::DigiType::U16;
  return is_signed ? kern::DigiType::I8 : kern::DigiType::U8;
}

DigiParams digi_params_from(const DigiCmdLineOptions& a) {
  DigiParams p;
  p.sigma_out = a.sigma_out;
  PSOUP_CHECK(a.scale == "channel" || a.scale == "file", "digi: scale must be channel or file, got " << a.scale);
  p.scale = a.scale == "file" ? DigiScaleMode::File : DigiScaleMode::Channel;
  p.rescale_blocks = a.rescale_blocks;
  return p;
}

namespace {

// numpy.median: the mean of the two middle values for an even count
double median_of(std::vector<double> v) {
  const size_t n = v.size();
  std::sort(v.begin(), v.end());
  return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

}  // namespace

DigiScale digi_scale(const std::vector<uint32_t>& N, const std::vector<int64_t>& S1, const std::vector<uint64_t>& S2,
                     const std::vector<int32_t>& E, int nchans, uint64_t nblk, const std::vector<int>& killmask,
                     const DigiParams& p) {
  digi_check_params(p);
  PSOUP_CHECK(nchans >= 1 && nblk >= 1, "digi_scale: empty table");
  const size_t nc = static_cast<size_t>(nchans), nb = static_cast<size_t>(nblk);
  PSOUP_CHECK(N.size() == nc * nb && S1.size() == nc * nb && S2.size() == nc * nb && E.size() == nc * nb,
              "digi_scale: N, S1, S2 and E must be [nchans][nblk]");
  PSOUP_CHECK(killmask.empty() || killmask.size() == nc, "digi_scale: killmask size != nchans");
  const int J = p.rescale_blocks;
  DigiScale sc;
  sc.nint = digi_nint(nblk, J);
  const size_t ni = static_cast<size_t>(sc.nint);
  const size_t per = J > 0 ? static_cast<size_t>(J) : nb;  // blocks per interval
  sc.mean.assign(ni * nc, 0.0);
  sc.gain.assign(ni * nc, 0.0);
  sc.live.assign(ni * nc, 0);
  sc.alive.assign(nc, 0);
  std::vector<double> sig(ni * nc, 0.0);  // sqrt(med_v) of the live cells
  std::vector<double> m, v;
  for (size_t c = 0; c < nc; ++c) {
    const bool killed = !killmask.empty() && killmask[c] == 0;
    for (size_t j = 0; j < ni; ++j) {
      m.clear();
      v.clear();
      for (size_t b = j * per; b < std::min(nb, (j + 1) * per); ++b) {
        const size_t i = c * nb + b;
        const uint32_t n = N[i];
        if (n == 0) continue;
        PSOUP_CHECK(n <= static_cast<uint32_t>(kern::kDigiStatBlock), "digi_scale: N exceeds the block length");
        PSOUP_CHECK(E[i] >= -148 && E[i] <= 105, "digi_scale: E out of range");
        const __int128 s1 = S1[i];
        const unsigned __int128 lhs = static_cast<unsigned __int128>(n) * S2[i];
        const unsigned __int128 rhs = static_cast<unsigned __int128>(s1 * s1);
        PSOUP_CHECK(lhs >= rhs, "digi_scale: channel " << c << " block " << b << ": S1^2 exceeds N S2");
        const double dn = static_cast<double>(n);
        m.push_back(std::ldexp(static_cast<double>(S1[i]) / dn, E[i]));
        v.push_back(std::ldexp(static_cast<double>(lhs - rhs) / (dn * dn), 2 * E[i]));
      }
      if (m.empty()) continue;
      const double med_m = median_of(m), med_v = median_of(v);
      sc.mean[j * nc + c] = med_m;
      if (!killed && med_v > 0) {
        sc.live[j * nc + c] = 1;
        sc.alive[c] = 1;
        sig[j * nc + c] = std::sqrt(med_v);
      }
    }
  }
  for (size_t c = 0; c < nc; ++c) sc.nlive += sc.alive[c];
  PSOUP_CHECK(sc.nlive > 0, "digi: no live channel (every channel is killed, has no finite sample or has zero variance)");
  bool first = true;
  for (size_t j = 0; j < ni; ++j) {
    double file_gain = 0;
    if (p.scale == DigiScaleMode::File) {
      std::vector<double> s;
      for (size_t c = 0; c < nc; ++c)
        if (sc.live[j * nc + c]) s.push_back(sig[j * nc + c]);
      if (!s.empty()) file_gain = p.sigma_out / median_of(s);
    }
    for (size_t c = 0; c < nc; ++c) {
      const size_t i = j * nc + c;
      if (!sc.live[i]) {
        sc.mean[i] = 0.0;  // not used: the cell gives 128
        continue;
      }
      const double g = p.scale == DigiScaleMode::File ? file_gain : p.sigma_out / sig[i];
      sc.gain[i] = g;
      sc.gain_min = first ? g : std::min(sc.gain_min, g);
      sc.gain_max = first ? g : std::max(sc.gain_max, g);
      first = false;
    }
  }
  return sc;
}

DigiBand digi_band(double fch1, double foff, int nchans) {
  DigiBand b;
  b.flip = foff > 0;
  b.fch1 = b.flip ? fch1 + static_cast<double>(nchans - 1) * foff : fch1;
  b.foff = b.flip ? -foff : foff;
  return b;
}

SigprocHeader digi_header(const SigprocHeader& in) {
  SigprocHeader oh = in;
  const DigiBand b = digi_band(in.fch1, in.foff, in.nchans);
  oh.fch1 = b.fch1;
  oh.foff = b.foff;
  oh.nbits = 8;
  oh.signed_data = 0;
  auto& k = oh.keys_present;
  k.erase(std::remove(k.begin(), k.end(), std::string("signed")), k.end());
  if (std::find(k.begin(), k.end(), std::string("nsamples")) == k.end()) oh.nsamples = 0;
  return oh;
}

}  // namespace psoup
