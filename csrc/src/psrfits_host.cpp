// fits2fil, host steps: the FITS parser (cards, TFORM, column offsets, every
// structural refusal), rows and slots, the band, the polarisations, the output
// header and the mmap reader of psoup/psrfits.hpp.  No device code here (the
// native unit tests link this file alone) and no FMA contraction: the double
// arithmetic is the definition's, operation by operation.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "psoup/psrfits.hpp"

namespace psoup {

namespace {

constexpr uint64_t kBlock = 2880;
constexpr uint64_t kCard = 80;

std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && std::isspace(static_cast<unsigned char>(s[a]))) ++a;
  while (b > a && std::isspace(static_cast<unsigned char>(s[b - 1]))) --b;
  return s.substr(a, b - a);
}

std::string upper(std::string s) {
  for (char& c : s) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
  return s;
}

// A whole token as a double (D exponents allowed); false when it is not one.
bool parse_double(const std::string& text, double& out) {
  std::string s = trim(text);
  if (s.empty()) return false;
  for (char& c : s)
    if (c == 'D' || c == 'd') c = 'E';
  char* end = nullptr;
  const double v = std::strtod(s.c_str(), &end);
  if (end == s.c_str() || *end != '\0') return false;
  out = v;
  return true;
}

bool parse_int(const std::string& text, int64_t& out) {
  const std::string s = trim(text);
  if (s.empty()) return false;
  char* end = nullptr;
  const long long v = std::strtoll(s.c_str(), &end, 10);
  if (end == s.c_str() || *end != '\0') return false;
  out = v;
  return true;
}

// The value of one 80-character card (from column 11).
std::string card_value(const char* card) {
  const std::string v(card + 10, kCard - 10);
  size_t i = 0;
  while (i < v.size() && v[i] == ' ') ++i;
  if (i < v.size() && v[i] == '\'') {
    std::string out;
    for (++i; i < v.size(); ++i) {
      if (v[i] == '\'') {
        if (i + 1 < v.size() && v[i + 1] == '\'') {
          out.push_back('\'');
          ++i;
        } else {
          break;
        }
      } else {
        out.push_back(v[i]);
      }
    }
    while (!out.empty() && out.back() == ' ') out.pop_back();
    return out;
  }
  const size_t slash = v.find('/');
  return trim(slash == std::string::npos ? v : v.substr(0, slash));
}

// Reads the header at `off`; returns the offset of its data area.
uint64_t read_cards(const uint8_t* p, uint64_t n, uint64_t off, FitsCards& cards) {
  cards.kv.clear();
  for (uint64_t at = off;; at += kCard) {
    PSOUP_CHECK(at + kCard <= n, "fits: a header runs past the end of the file (no END card)");
    const char* card = reinterpret_cast<const char*>(p + at);
    const std::string key = trim(std::string(card, 8));
    if (key == "END") return off + (at + kCard - off + kBlock - 1) / kBlock * kBlock;
    if (key.empty() || key == "COMMENT" || key == "HISTORY" || card[8] != '=') continue;
    cards.kv.emplace_back(key, card_value(card));
  }
}

// NAXIS1 x NAXIS2 + PCOUNT, padded to a block.
uint64_t data_area(const FitsCards& c) {
  int64_t naxis = 0, n1 = 0, n2 = 1, pcount = 0;
  if (const std::string* s = c.find("NAXIS")) parse_int(*s, naxis);
  if (naxis <= 0) return 0;
  if (const std::string* s = c.find("NAXIS1")) parse_int(*s, n1);
  if (const std::string* s = c.find("NAXIS2")) parse_int(*s, n2);
  if (const std::string* s = c.find("PCOUNT")) parse_int(*s, pcount);
  PSOUP_CHECK(n1 >= 0 && n2 >= 0 && pcount >= 0 && n1 < (int64_t(1) << 31) && n2 < (int64_t(1) << 31) &&
                  pcount < (int64_t(1) << 50),
              "fits: an HDU has a bad NAXIS1, NAXIS2 or PCOUNT");
  const uint64_t bytes = static_cast<uint64_t>(n1) * static_cast<uint64_t>(n2) + static_cast<uint64_t>(pcount);
  return (bytes + kBlock - 1) / kBlock * kBlock;
}

int small_int(const FitsCards& c, const std::string& key, const char* hdu) {
  const int64_t v = c.integer(key, hdu);
  PSOUP_CHECK(v >= 0 && v <= (int64_t(1) << 30), "fits: " << key << " out of range: " << v);
  return static_cast<int>(v);
}

uint32_t be32(const uint8_t* p) {
  return (static_cast<uint32_t>(p[0]) << 24) | (static_cast<uint32_t>(p[1]) << 16) | (static_cast<uint32_t>(p[2]) << 8) |
         static_cast<uint32_t>(p[3]);
}
uint64_t be64(const uint8_t* p) { return (static_cast<uint64_t>(be32(p)) << 32) | be32(p + 4); }
float be_float(const uint8_t* p) {
  const uint32_t b = be32(p);
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
double be_double(const uint8_t* p) {
  const uint64_t b = be64(p);
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

}  // namespace

// ----------------------------------------------------------------- cards ----
const std::string* FitsCards::find(const std::string& key) const {
  for (const auto& e : kv)
    if (e.first == key) return &e.second;
  return nullptr;
}
std::string FitsCards::str(const std::string& key, const char* hdu) const {
  const std::string* s = find(key);
  PSOUP_CHECK(s != nullptr, "fits: missing key " << key << " in the " << hdu << " header");
  return *s;
}
double FitsCards::num(const std::string& key, const char* hdu) const {
  double v = 0;
  PSOUP_CHECK(parse_double(str(key, hdu), v), "fits: key " << key << " in the " << hdu << " header is not a number");
  return v;
}
int64_t FitsCards::integer(const std::string& key, const char* hdu) const {
  int64_t v = 0;
  PSOUP_CHECK(parse_int(str(key, hdu), v), "fits: key " << key << " in the " << hdu << " header is not an integer");
  return v;
}

FitsTform fits_tform(const std::string& text) {
  const std::string s = trim(text);
  size_t i = 0;
  uint64_t r = 0;
  while (i < s.size() && std::isdigit(static_cast<unsigned char>(s[i])) && i < 15) r = r * 10 + (s[i++] - '0');
  FitsTform f;
  f.repeat = i == 0 ? 1 : r;
  PSOUP_CHECK(i + 1 == s.size(), "fits: unsupported TFORM '" << s << "'");
  f.type = s[i];
  switch (f.type) {
    case 'B':
    case 'A': f.bytes = f.repeat; break;
    case 'I': f.bytes = 2 * f.repeat; break;
    case 'J':
    case 'E': f.bytes = 4 * f.repeat; break;
    case 'D': f.bytes = 8 * f.repeat; break;
    case 'X': f.bytes = (f.repeat + 7) / 8; break;
    default: PSOUP_THROW("fits: unsupported TFORM '" << s << "'");
  }
  return f;
}

// ---------------------------------------------------------------- parser ----
FitsLayout fits_parse(const uint8_t* p, uint64_t n) {
  FitsLayout lay;
  PSOUP_CHECK(p != nullptr && n >= kCard && std::memcmp(p, "SIMPLE  =", 9) == 0,
              "fits: not a FITS file (no SIMPLE = T)");
  uint64_t off = read_cards(p, n, 0, lay.primary);
  {
    const std::string* simple = lay.primary.find("SIMPLE");
    PSOUP_CHECK(simple != nullptr && *simple == "T", "fits: not a FITS file (no SIMPLE = T)");
    const std::string* mode = lay.primary.find("OBS_MODE");
    PSOUP_CHECK(mode != nullptr, "fits: missing key OBS_MODE in the primary header");
    PSOUP_CHECK(upper(trim(*mode)) == "SEARCH", "fits: OBS_MODE is '" << *mode << "', not SEARCH");
  }
  off += data_area(lay.primary);
  bool found = false;
  while (off < n) {
    FitsCards c;
    const uint64_t data = read_cards(p, n, off, c);
    const std::string* xt = c.find("XTENSION");
    const std::string* name = c.find("EXTNAME");
    if (xt != nullptr && trim(*xt) == "BINTABLE" && name != nullptr && trim(*name) == "SUBINT") {
      lay.subint = c;
      lay.table_off = data;
      found = true;
      break;
    }
    off = data + data_area(c);
  }
  PSOUP_CHECK(found, "fits: no SUBINT table");
  const FitsCards& s = lay.subint;
  const char* hdu = "SUBINT";
  lay.row_bytes = static_cast<uint64_t>(small_int(s, "NAXIS1", hdu));
  {
    const int64_t rows = s.integer("NAXIS2", hdu);
    PSOUP_CHECK(rows >= 0 && rows <= (int64_t(1) << 31), "fits: NAXIS2 out of range: " << rows);
    lay.nrows = static_cast<uint64_t>(rows);
  }
  const int tfields = small_int(s, "TFIELDS", hdu);
  PSOUP_CHECK(tfields >= 1 && tfields <= 999, "fits: TFIELDS out of range: " << tfields);
  lay.npol = small_int(s, "NPOL", hdu);
  lay.nbits = small_int(s, "NBITS", hdu);
  lay.nchan = small_int(s, "NCHAN", hdu);
  lay.nsblk = small_int(s, "NSBLK", hdu);
  lay.tbin = s.num("TBIN", hdu);
  lay.pol_type = trim(s.str("POL_TYPE", hdu));
  PSOUP_CHECK(lay.npol >= 1 && lay.npol <= 4, "fits: NPOL must be 1 to 4, got " << lay.npol);
  PSOUP_CHECK(lay.nchan >= 1 && lay.nchan <= (1 << 24), "fits: NCHAN out of range: " << lay.nchan);
  PSOUP_CHECK(lay.nsblk >= 1 && lay.nsblk <= (1 << 24), "fits: NSBLK out of range: " << lay.nsblk);
  PSOUP_CHECK(std::isfinite(lay.tbin) && lay.tbin > 0, "fits: TBIN must be positive");
  PSOUP_CHECK(lay.nbits == 1 || lay.nbits == 2 || lay.nbits == 4 || lay.nbits == 8 || lay.nbits == 16,
              "fits: NBITS must be 1, 2, 4, 8 or 16, got " << lay.nbits);
  PSOUP_CHECK((static_cast<uint64_t>(lay.nchan) * static_cast<uint64_t>(lay.nbits)) % 8 == 0,
              "fits: NCHAN x NBITS must be a multiple of 8, got " << lay.nchan << " x " << lay.nbits);
  if (const std::string* v = s.find("SIGNINT")) {
    int64_t k = 0;
    lay.signint = parse_int(*v, k) && k == 1 ? 1 : 0;
  }
  if (const std::string* v = s.find("CHAN_BW")) {
    double d = 0;
    if (parse_double(*v, d)) lay.chan_bw = d;
  }
  if (const std::string* v = s.find("ZERO_OFF")) {
    double d = 0;
    if (parse_double(*v, d)) {
      const float zf = std::fabs(static_cast<float>(d));
      if (std::isfinite(zf)) lay.z = static_cast<double>(zf);
    }
  }
  // the columns
  uint64_t at = 0;
  for (int i = 1; i <= tfields; ++i) {
    FitsColumn col;
    col.name = trim(s.str("TTYPE" + std::to_string(i), hdu));
    col.form = fits_tform(s.str("TFORM" + std::to_string(i), hdu));
    col.offset = at;
    at += col.form.bytes;
    PSOUP_CHECK(at <= (uint64_t(1) << 40), "fits: the columns are too large");
    const int idx = static_cast<int>(lay.columns.size());
    if (col.name == "OFFS_SUB") lay.c_offs_sub = idx;
    if (col.name == "DAT_FREQ") lay.c_dat_freq = idx;
    if (col.name == "DAT_WTS") lay.c_dat_wts = idx;
    if (col.name == "DAT_OFFS") lay.c_dat_offs = idx;
    if (col.name == "DAT_SCL") lay.c_dat_scl = idx;
    if (col.name == "DATA") lay.c_data = idx;
    lay.columns.push_back(col);
  }
  PSOUP_CHECK(at == lay.row_bytes,
              "fits: the column sizes add up to " << at << " bytes, NAXIS1 is " << lay.row_bytes);
  auto need = [&](int idx, const char* name) -> const FitsColumn& {
    PSOUP_CHECK(idx >= 0, "fits: missing column " << name);
    return lay.columns[static_cast<size_t>(idx)];
  };
  const uint64_t nchan = static_cast<uint64_t>(lay.nchan), npol = static_cast<uint64_t>(lay.npol);
  if (lay.c_offs_sub >= 0) {
    const FitsTform& f = lay.columns[static_cast<size_t>(lay.c_offs_sub)].form;
    PSOUP_CHECK(f.type == 'D' && f.repeat == 1, "fits: OFFS_SUB must be 1D");
  }
  {
    const FitsTform& f = need(lay.c_dat_freq, "DAT_FREQ").form;
    PSOUP_CHECK((f.type == 'E' || f.type == 'D') && f.repeat == nchan,
                "fits: DAT_FREQ has the wrong length or type (" << f.repeat << f.type << ", NCHAN " << nchan << ")");
  }
  {
    const FitsTform& f = need(lay.c_dat_wts, "DAT_WTS").form;
    PSOUP_CHECK(f.type == 'E' && f.repeat == nchan,
                "fits: DAT_WTS has the wrong length or type (" << f.repeat << f.type << ", NCHAN " << nchan << ")");
  }
  {
    const FitsTform& f = need(lay.c_dat_offs, "DAT_OFFS").form;
    PSOUP_CHECK(f.type == 'E' && f.repeat == npol * nchan, "fits: DAT_OFFS has the wrong length or type ("
                                                               << f.repeat << f.type << ", NPOL x NCHAN " << npol * nchan
                                                               << ")");
  }
  {
    const FitsTform& f = need(lay.c_dat_scl, "DAT_SCL").form;
    PSOUP_CHECK(f.type == 'E' && f.repeat == npol * nchan, "fits: DAT_SCL has the wrong length or type ("
                                                              << f.repeat << f.type << ", NPOL x NCHAN " << npol * nchan
                                                              << ")");
  }
  {
    const FitsTform& f = need(lay.c_data, "DATA").form;
    PSOUP_CHECK(f.type == 'B' || f.type == 'I', "fits: DATA must be of type B or I (32-bit float DATA is out of scope)");
    PSOUP_CHECK(f.bytes == lay.data_bytes(), "fits: the DATA column holds " << f.bytes << " bytes, NSBLK x NPOL x NCHAN x NBITS / 8 is "
                                                                            << lay.data_bytes());
  }
  PSOUP_CHECK(lay.nrows >= 1, "fits: NAXIS2 = 0: the SUBINT table has no rows");
  PSOUP_CHECK(lay.table_off <= n && lay.row_bytes * lay.nrows <= n - lay.table_off,
              "fits: the SUBINT table runs past the end of the file");
  return lay;
}

// ------------------------------------------------------------------ rows ----
FitsSlots fits_row_slots(const std::vector<double>& offs_sub, uint64_t nrows, int nsblk, double tbin) {
  PSOUP_CHECK(nrows >= 1 && nsblk >= 1 && tbin > 0, "fits: no rows");
  PSOUP_CHECK(offs_sub.empty() || offs_sub.size() == nrows, "fits: OFFS_SUB has the wrong length");
  FitsSlots out;
  const double row_s = static_cast<double>(nsblk) * tbin;
  const double half = (0.5 * static_cast<double>(nsblk)) * tbin;
  const bool zero = std::all_of(offs_sub.begin(), offs_sub.end(), [](double v) { return v == 0.0; });
  out.slot.resize(nrows);
  if (zero) {
    for (uint64_t i = 0; i < nrows; ++i) out.slot[i] = static_cast<int64_t>(i);
    out.offs_sub0 = half;
  } else {
    out.offs_sub0 = offs_sub[0] == 0.0 ? half : offs_sub[0];
    for (uint64_t i = 0; i < nrows; ++i) {
      PSOUP_CHECK(std::isfinite(offs_sub[i]), "fits: OFFS_SUB of row " << i << " is not finite");
      const double q = (offs_sub[i] - offs_sub[0]) / row_s;
      const double k = std::rint(q);
      PSOUP_CHECK(std::fabs(q - k) <= 1e-3, "fits: row " << i << " does not start on a whole row (OFFS_SUB is " << q
                                                            << " rows after the first; gaps that are not whole rows are "
                                                               "out of scope)");
      PSOUP_CHECK(k >= 0 && k <= 4.0e9, "fits: the row slots do not increase strictly at row " << i);
      out.slot[i] = static_cast<int64_t>(k);
      PSOUP_CHECK(i == 0 || out.slot[i] > out.slot[i - 1], "fits: the row slots do not increase strictly at row " << i);
    }
  }
  out.nslots = static_cast<uint64_t>(out.slot.back()) + 1;
  PSOUP_CHECK(out.nslots <= 2 * nrows, "fits: " << out.nslots << " row slots for " << nrows
                                                 << " rows: more than half the rows are dropped");
  out.nsamps = out.nslots * static_cast<uint64_t>(nsblk);
  PSOUP_CHECK(out.nsamps < (uint64_t(1) << 31), "fits: too many samples for a SIGPROC header (" << out.nsamps << ")");
  out.slot_row.assign(out.nslots, -1);
  for (uint64_t i = 0; i < nrows; ++i) out.slot_row[static_cast<size_t>(out.slot[i])] = static_cast<int32_t>(i);
  out.ndropped = out.nslots - nrows;
  return out;
}

// ------------------------------------------------------------------ band ----
FitsBand fits_band(const std::vector<double>& f, double chan_bw) {
  PSOUP_CHECK(!f.empty(), "fits: DAT_FREQ is empty");
  FitsBand b;
  const size_t n = f.size();
  b.fch1 = f[0];
  b.foff = n == 1 ? chan_bw : (f[n - 1] - f[0]) / static_cast<double>(n - 1);
  PSOUP_CHECK(std::isfinite(b.fch1) && std::isfinite(b.foff) && b.foff != 0, "fits: foff must not be zero");
  for (size_t c = 0; c < n; ++c) {
    const double want = b.fch1 + static_cast<double>(c) * b.foff;
    PSOUP_CHECK(std::fabs(f[c] - want) <= 0.01 * std::fabs(b.foff),
                "fits: DAT_FREQ is not evenly spaced at channel " << c << " (" << f[c] << " MHz, expected " << want << ")");
  }
  return b;
}

// ---------------------------------------------------------- polarisations ----
std::pair<int, int> fits_pols(int npol, const std::string& pol_type, int pol) {
  PSOUP_CHECK(npol >= 1, "fits: NPOL must be at least 1");
  if (pol >= 0) {
    PSOUP_CHECK(pol < npol, "fits: --pol " << pol << " is not below NPOL = " << npol);
    return {pol, -1};
  }
  if (npol == 1) return {0, -1};
  const std::string t = upper(trim(pol_type));
  if (t.rfind("AABB", 0) == 0) return {0, 1};
  if (t == "IQUV") return {0, -1};
  PSOUP_THROW("fits: POL_TYPE '" << pol_type << "' with NPOL = " << npol << " needs --pol P");
}

int fits_telescope_id(const std::string& telescop) {
  static const std::pair<const char*, int> table[] = {{"ARECIBO", 1}, {"OOTY", 2},        {"NANCAY", 3}, {"PARKES", 4},
                                                      {"JODRELL", 5}, {"GBT", 6},         {"GMRT", 7},   {"EFFELSBERG", 8},
                                                      {"LOFAR", 11},  {"VLA", 12},        {"MEERKAT", 64}};
  const std::string t = upper(trim(telescop));
  for (const auto& e : table)
    if (t == e.first) return e.second;
  return 0;
}

double fits_sexagesimal(const std::string& text) {
  std::string s = trim(text);
  if (s.empty()) return 0.0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    s = s.substr(1);
  }
  const size_t a = s.find(':');
  const size_t b = a == std::string::npos ? a : s.find(':', a + 1);
  if (b == std::string::npos) return 0.0;
  int64_t h = 0, m = 0;
  double sec = 0;
  if (!parse_int(s.substr(0, a), h) || !parse_int(s.substr(a + 1, b - a - 1), m) || !parse_double(s.substr(b + 1), sec))
    return 0.0;
  if (h < 0 || m < 0 || !(sec >= 0) || !std::isfinite(sec)) return 0.0;
  const double v = (static_cast<double>(h) * 10000.0 + static_cast<double>(m) * 100.0) + sec;
  return neg ? -v : v;
}

SigprocHeader fits_header(const FitsLayout& lay, const FitsSlots& slots, const FitsBand& band, const FitsOptions& opt,
                          const std::string& rawdatafile) {
  const FitsCards& p = lay.primary;
  SigprocHeader h;
  if (const std::string* s = p.find("SRC_NAME")) h.source_name = trim(*s);
  h.rawdatafile = rawdatafile;
  const std::string* tel = p.find("TELESCOP");
  h.telescope_id = opt.telescope_id >= 0 ? opt.telescope_id : fits_telescope_id(tel ? *tel : std::string());
  h.machine_id = opt.machine_id;
  h.data_type = 1;
  if (const std::string* s = p.find("RA")) h.src_raj = fits_sexagesimal(*s);
  if (const std::string* s = p.find("DEC")) h.src_dej = fits_sexagesimal(*s);
  const double imjd = static_cast<double>(p.integer("STT_IMJD", "primary"));
  const double smjd = p.num("STT_SMJD", "primary");
  const double soffs = p.num("STT_OFFS", "primary");
  const double half = (0.5 * static_cast<double>(lay.nsblk)) * lay.tbin;
  const double secs = ((smjd + soffs) + slots.offs_sub0) - half;
  h.tstart = imjd + secs / 86400.0;
  h.tsamp = lay.tbin;
  const DigiBand b = digi_band(band.fch1, band.foff, lay.nchan);
  h.fch1 = b.fch1;
  h.foff = b.foff;
  h.nchans = lay.nchan;
  h.nbits = 8;
  h.nifs = 1;
  h.nsamples = static_cast<int>(slots.nsamps);
  h.barycentric = 0;
  h.keys_present = {"telescope_id", "machine_id", "barycentric", "src_raj", "src_dej", "tstart", "nsamples"};
  if (const std::string* s = p.find("BEAM_ID")) {
    int64_t v = 0;
    if (parse_int(*s, v) && v >= -2147483647 && v <= 2147483647) {
      h.ibeam = static_cast<int>(v);
      h.keys_present.push_back("ibeam");
    }
  }
  return h;
}

FitsOptions fits_options_from(const FitsCmdLineOptions& a) {
  FitsOptions o;
  if (a.pol != "auto") {
    int64_t v = -1;
    PSOUP_CHECK(parse_int(a.pol, v) && v >= 0 && v < 64, "fits: --pol must be auto or a polarisation index, got " << a.pol);
    o.pol = static_cast<int>(v);
  }
  o.no_scales = a.no_scales;
  o.no_offsets = a.no_offsets;
  o.no_weights = a.no_weights;
  o.telescope_id = a.telescope_id;
  o.machine_id = a.machine_id;
  return o;
}

DigiParams fits_digi_params_from(const FitsCmdLineOptions& a) {
  DigiCmdLineOptions d;
  d.sigma_out = a.sigma_out;
  d.scale = a.scale;
  d.rescale_blocks = a.rescale_blocks;
  return digi_params_from(d);
}

// ---------------------------------------------------------------- reader ----
void PsrfitsFile::init(const uint8_t* p, uint64_t n) {
  base_ = p;
  size_ = n;
  lay_ = fits_parse(p, n);
  std::vector<double> offs;
  if (lay_.c_offs_sub >= 0) {
    offs.resize(lay_.nrows);
    for (uint64_t r = 0; r < lay_.nrows; ++r) read_doubles(r, lay_.c_offs_sub, 1, &offs[r]);
  }
  slots_ = fits_row_slots(offs, lay_.nrows, lay_.nsblk, lay_.tbin);
  std::vector<double> f(static_cast<size_t>(lay_.nchan));
  read_doubles(0, lay_.c_dat_freq, f.size(), f.data());
  band_ = fits_band(f, lay_.chan_bw);
}

PsrfitsFile PsrfitsFile::from_memory(const uint8_t* p, uint64_t n) {
  PsrfitsFile f;
  f.init(p, n);
  return f;
}

PsrfitsFile PsrfitsFile::from_file(const std::string& filename) {
  int fd = ::open(filename.c_str(), O_RDONLY);
  if (fd < 0) PSOUP_THROW("cannot open " << filename);
  struct stat st;
  if (fstat(fd, &st) != 0) {
    ::close(fd);
    PSOUP_THROW("cannot stat " << filename);
  }
  const uint64_t size = static_cast<uint64_t>(st.st_size);
  if (size == 0) {
    ::close(fd);
    PSOUP_THROW("fits: not a FITS file (no SIMPLE = T): " << filename << " is empty");
  }
  void* map = ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (map == MAP_FAILED) PSOUP_THROW("mmap failed for " << filename);
  ::madvise(map, size, MADV_SEQUENTIAL);
  PsrfitsFile f;
  f.owner_ = std::shared_ptr<void>(map, [size](void* q) { ::munmap(q, size); });
  f.init(static_cast<const uint8_t*>(map), size);
  return f;
}

void PsrfitsFile::read_floats(uint64_t r, int col, size_t n, float* dst) const {
  const FitsColumn& c = lay_.columns[static_cast<size_t>(col)];
  PSOUP_CHECK(r < lay_.nrows && c.form.type == 'E' && c.form.repeat >= n, "fits: bad float column read");
  const uint8_t* p = row(r) + c.offset;
  for (size_t i = 0; i < n; ++i) dst[i] = be_float(p + 4 * i);
}

void PsrfitsFile::read_doubles(uint64_t r, int col, size_t n, double* dst) const {
  const FitsColumn& c = lay_.columns[static_cast<size_t>(col)];
  PSOUP_CHECK(r < lay_.nrows && (c.form.type == 'E' || c.form.type == 'D') && c.form.repeat >= n,
              "fits: bad double column read");
  const uint8_t* p = row(r) + c.offset;
  for (size_t i = 0; i < n; ++i)
    dst[i] = c.form.type == 'D' ? be_double(p + 8 * i) : static_cast<double>(be_float(p + 4 * i));
}

}  // namespace psoup
