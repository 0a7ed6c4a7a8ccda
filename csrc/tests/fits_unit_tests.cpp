// Host unit tests of fits2fil's host steps (psoup/psrfits.hpp): the parser over
// an in-memory file truncated at every block boundary and in mid-card, TFORM
// and the column offsets, the structural refusals, rows and slots, the band,
// the RA / DEC conversion, the telescope table and the header.  No GPU.  Exit
// status 0 = all passed.
#include <cmath>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "psoup/psrfits.hpp"

using namespace psoup;

static int g_failed = 0;
#define EXPECT(cond)                                                            \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond << std::endl;      \
      ++g_failed;                                                               \
    }                                                                           \
  } while (0)

namespace {

template <class F>
bool throws_with(F&& f, const std::string& what) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

using Cards = std::vector<std::pair<std::string, std::string>>;

std::string card(const std::string& key, const std::string& value) {
  std::string c = key;
  c.resize(8, ' ');
  c += "= " + value;
  c.resize(80, ' ');
  return c;
}
std::string quoted(const std::string& s) { return "'" + s + "'"; }

void put_header(std::vector<uint8_t>& f, const Cards& cards) {
  std::string h;
  for (const auto& c : cards) h += card(c.first, c.second);
  std::string end = "END";
  end.resize(80, ' ');
  h += end;
  h.resize((h.size() + 2879) / 2880 * 2880, ' ');
  f.insert(f.end(), h.begin(), h.end());
}
void pad_block(std::vector<uint8_t>& f) { f.resize((f.size() + 2879) / 2880 * 2880, 0); }

void put_be(std::vector<uint8_t>& f, const void* v, size_t n) {
  const uint8_t* p = static_cast<const uint8_t*>(v);
  for (size_t i = 0; i < n; ++i) f.push_back(p[n - 1 - i]);
}

struct Spec {
  int nchan = 8, npol = 2, nbits = 8, nsblk = 4, nrows = 3;
  std::string obs_mode = "SEARCH";
  int naxis1_extra = 0;
  bool with_subint = true;
  std::string data_form;  // default: the right size
};

// primary + a HISTORY table with PCOUNT > 0 + SUBINT (OFFS_SUB 1D, DAT_FREQ nE, DAT_WTS, DAT_OFFS, DAT_SCL, DATA)
std::vector<uint8_t> make_file(const Spec& s) {
  std::vector<uint8_t> f;
  put_header(f, {{"SIMPLE", "T"}, {"BITPIX", "8"}, {"NAXIS", "0"}, {"OBS_MODE", quoted(s.obs_mode)},
                 {"TELESCOP", quoted("Parkes  ")}, {"SRC_NAME", quoted("J0000-00")}, {"RA", quoted("12:34:56.7")},
                 {"DEC", quoted("-01:02:03.4")}, {"STT_IMJD", "55000"}, {"STT_SMJD", "100"}, {"STT_OFFS", "0.25"},
                 {"BEAM_ID", quoted("3")}});
  put_header(f, {{"XTENSION", quoted("BINTABLE")}, {"BITPIX", "8"}, {"NAXIS", "2"}, {"NAXIS1", "10"}, {"NAXIS2", "7"},
                 {"PCOUNT", "33"}, {"GCOUNT", "1"}, {"TFIELDS", "1"}, {"TTYPE1", quoted("X")}, {"TFORM1", quoted("10A")},
                 {"EXTNAME", quoted("HISTORY")}});
  f.resize(f.size() + 103, 7);
  pad_block(f);
  if (!s.with_subint) return f;
  const int nd = s.nsblk * s.npol * s.nchan * s.nbits / 8;
  const int row = 8 + 4 * s.nchan + 4 * s.nchan + 2 * 4 * s.npol * s.nchan + nd;
  put_header(f, {{"XTENSION", quoted("BINTABLE")}, {"BITPIX", "8"}, {"NAXIS", "2"},
                 {"NAXIS1", std::to_string(row + s.naxis1_extra)}, {"NAXIS2", std::to_string(s.nrows)}, {"PCOUNT", "0"},
                 {"GCOUNT", "1"}, {"TFIELDS", "6"}, {"TTYPE1", quoted("OFFS_SUB")}, {"TFORM1", quoted("1D")},
                 {"TTYPE2", quoted("DAT_FREQ")}, {"TFORM2", quoted(std::to_string(s.nchan) + "E")},
                 {"TTYPE3", quoted("DAT_WTS")}, {"TFORM3", quoted(std::to_string(s.nchan) + "E")},
                 {"TTYPE4", quoted("DAT_OFFS")}, {"TFORM4", quoted(std::to_string(s.npol * s.nchan) + "E")},
                 {"TTYPE5", quoted("DAT_SCL")}, {"TFORM5", quoted(std::to_string(s.npol * s.nchan) + "E")},
                 {"TTYPE6", quoted("DATA")},
                 {"TFORM6", quoted(s.data_form.empty() ? std::to_string(nd) + "B" : s.data_form)},
                 {"EXTNAME", quoted("SUBINT")}, {"NPOL", std::to_string(s.npol)}, {"POL_TYPE", quoted("AABB")},
                 {"TBIN", "1.0E-3"}, {"NBITS", std::to_string(s.nbits)}, {"NCHAN", std::to_string(s.nchan)},
                 {"NSBLK", std::to_string(s.nsblk)}, {"ZERO_OFF", "-1.5"}, {"SIGNINT", "0"}, {"CHAN_BW", "0.5"}});
  for (int r = 0; r < s.nrows; ++r) {
    const double offs = (0.5 + r) * s.nsblk * 1e-3;
    put_be(f, &offs, 8);
    for (int c = 0; c < s.nchan; ++c) {
      const float fr = 1200.0f + 0.5f * c;
      put_be(f, &fr, 4);
    }
    for (int c = 0; c < s.nchan; ++c) {
      const float w = 1.0f;
      put_be(f, &w, 4);
    }
    for (int i = 0; i < s.npol * s.nchan; ++i) {
      const float o = 0.25f * i;
      put_be(f, &o, 4);
    }
    for (int i = 0; i < s.npol * s.nchan; ++i) {
      const float sc = 1.0f + i;
      put_be(f, &sc, 4);
    }
    for (int i = 0; i < nd + s.naxis1_extra; ++i) f.push_back(static_cast<uint8_t>(i + r));
  }
  pad_block(f);
  return f;
}

void test_parser() {
  const std::vector<uint8_t> f = make_file(Spec());
  const FitsLayout l = fits_parse(f.data(), f.size());
  EXPECT(l.nrows == 3 && l.nchan == 8 && l.npol == 2 && l.nbits == 8 && l.nsblk == 4 && l.signint == 0);
  EXPECT(l.z == 1.5 && l.tbin == 1e-3 && l.chan_bw == 0.5 && l.pol_type == "AABB");
  EXPECT(l.table_off == 3 * 2880 + 2880 && l.row_bytes == 8 + 32 + 32 + 64 + 64 + 64);
  EXPECT(l.columns.size() == 6 && l.columns[5].name == "DATA" && l.columns[5].offset == 200 && l.c_data == 5);
  EXPECT(l.columns[1].offset == 8 && l.columns[2].offset == 40 && l.columns[3].offset == 72 && l.columns[4].offset == 136);
  EXPECT(l.primary.str("TELESCOP", "primary") == "Parkes");
  const PsrfitsFile pf = PsrfitsFile::from_memory(f.data(), f.size());
  EXPECT(pf.slots().nslots == 3 && pf.slots().ndropped == 0 && pf.band().fch1 == 1200.0 && pf.band().foff == 0.5);
  EXPECT(pf.row_data(1)[0] == 1 && pf.row_data(2)[3] == 5);
  float scl[16];
  pf.read_floats(2, l.c_dat_scl, 16, scl);
  EXPECT(scl[0] == 1.0f && scl[15] == 16.0f);
  FitsOptions opt;
  const SigprocHeader h = fits_header(l, pf.slots(), pf.band(), opt, "a.fits");
  EXPECT(h.telescope_id == 4 && h.ibeam == 3 && h.nchans == 8 && h.nbits == 8 && h.nsamples == 12 && h.nifs == 1);
  EXPECT(h.fch1 == 1203.5 && h.foff == -0.5 && h.source_name == "J0000-00" && h.rawdatafile == "a.fits");
  EXPECT(h.src_raj == 123456.7 && h.src_dej == -10203.4 && h.tsamp == 1e-3);
  EXPECT(h.tstart == 55000.0 + (((100.0 + 0.25) + 0.5 * 4 * 1e-3) - (0.5 * 4) * 1e-3) / 86400.0);

  // truncated at every block boundary, in mid-card and at every 997th byte: a named refusal, never a read past n
  int refused = 0;
  for (size_t n = 0; n < l.table_off + l.row_bytes * l.nrows; ++n) {
    if (!(n % 2880 == 0 || n % 2880 == 1000 || n % 997 == 0)) continue;
    std::vector<uint8_t> cut(f.begin(), f.begin() + n);  // its own allocation: a sanitizer sees a read past n
    EXPECT(throws_with([&] { PsrfitsFile::from_memory(cut.data(), cut.size()); }, "fits:"));
    ++refused;
  }
  EXPECT(refused > 10);
  {
    // the table's padding may be missing; one byte less of the last row is refused
    const size_t end = l.table_off + l.row_bytes * l.nrows;
    std::vector<uint8_t> cut(f.begin(), f.begin() + end);
    EXPECT(fits_parse(cut.data(), cut.size()).nrows == 3);
    cut.pop_back();
    EXPECT(throws_with([&] { fits_parse(cut.data(), cut.size()); }, "runs past the end of the file"));
  }
  EXPECT(throws_with([&] { fits_parse(f.data() + 1, f.size() - 1); }, "not a FITS file"));
  Spec s;
  s.obs_mode = "PSR";
  std::vector<uint8_t> g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "not SEARCH"));
  s = Spec();
  s.with_subint = false;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "no SUBINT table"));
  s = Spec();
  s.naxis1_extra = 1;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "NAXIS1 is 265"));
  s = Spec();
  s.nbits = 3;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "NBITS must be 1, 2, 4, 8 or 16"));
  s = Spec();
  s.nbits = 2;
  s.nchan = 6;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "multiple of 8"));
  s = Spec();
  s.data_form = "63B";
  s.naxis1_extra = -1;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "DATA column holds 63 bytes"));
  s = Spec();
  s.nrows = 0;
  g = make_file(s);
  EXPECT(throws_with([&] { fits_parse(g.data(), g.size()); }, "NAXIS2 = 0"));
}

void test_tform() {
  EXPECT(fits_tform("1D").bytes == 8 && fits_tform("D").repeat == 1 && fits_tform("D").bytes == 8);
  EXPECT(fits_tform("4096E").bytes == 16384 && fits_tform("3I").bytes == 6 && fits_tform("2J").bytes == 8);
  EXPECT(fits_tform("24A").bytes == 24 && fits_tform("9X").bytes == 2 && fits_tform("8X").bytes == 1);
  EXPECT(fits_tform(" 16B ").bytes == 16 && fits_tform("16B").type == 'B');
  EXPECT(throws_with([] { fits_tform("1PE(5)"); }, "unsupported TFORM"));
  EXPECT(throws_with([] { fits_tform("4Q"); }, "unsupported TFORM"));
  EXPECT(throws_with([] { fits_tform(""); }, "unsupported TFORM"));
}

void test_slots() {
  const double row = 512 * 64e-6;
  FitsSlots s = fits_row_slots({}, 4, 512, 64e-6);
  EXPECT(s.nslots == 4 && s.nsamps == 2048 && s.ndropped == 0 && s.offs_sub0 == (0.5 * 512) * 64e-6);
  s = fits_row_slots({0, 0, 0}, 3, 512, 64e-6);
  EXPECT(s.nslots == 3 && s.slot[2] == 2);
  s = fits_row_slots({10.5 * row, 11.5 * row, 13.5 * row, 14.5 * row + 2e-4 * row}, 4, 512, 64e-6);
  EXPECT(s.nslots == 5 && s.ndropped == 1 && s.slot_row[2] == -1 && s.slot_row[3] == 2 && s.slot_row[4] == 3);
  EXPECT(s.offs_sub0 == 10.5 * row);
  EXPECT(throws_with([&] { fits_row_slots({0.5 * row, 1.7 * row}, 2, 512, 64e-6); }, "whole row"));
  EXPECT(throws_with([&] { fits_row_slots({0.5 * row, 0.5 * row}, 2, 512, 64e-6); }, "increase strictly"));
  EXPECT(throws_with([&] { fits_row_slots({1.5 * row, 0.5 * row}, 2, 512, 64e-6); }, "increase strictly"));
  EXPECT(throws_with([&] { fits_row_slots({0.5 * row, 4.5 * row}, 2, 512, 64e-6); }, "more than half the rows are dropped"));
  EXPECT(fits_row_slots({0.5 * row, 3.5 * row}, 2, 512, 64e-6).nslots == 4);
  EXPECT(throws_with([&] { fits_row_slots({}, 1 << 20, 4096, 64e-6); }, "too many samples"));
  EXPECT(throws_with([&] { fits_row_slots({0.5}, 2, 512, 64e-6); }, "wrong length"));
}

void test_band_pols_header_fields() {
  FitsBand b = fits_band({1200.0, 1200.5, 1201.0, 1201.5}, 0.0);
  EXPECT(b.fch1 == 1200.0 && b.foff == 0.5);
  b = fits_band({1500.0, 1499.0, 1498.0}, 0.0);
  EXPECT(b.fch1 == 1500.0 && b.foff == -1.0);
  b = fits_band({1400.0}, -2.0);
  EXPECT(b.foff == -2.0);
  EXPECT(throws_with([] { fits_band({1400.0}, 0.0); }, "foff must not be zero"));
  EXPECT(throws_with([] { fits_band({1400.0, 1400.0}, 1.0); }, "foff must not be zero"));
  EXPECT(throws_with([] { fits_band({1200.0, 1200.52, 1201.0}, 0.0); }, "not evenly spaced"));
  EXPECT(fits_band({1200.0, 1200.504, 1201.0}, 0.0).foff == 0.5);

  EXPECT(fits_pols(1, "AA+BB", -1) == std::make_pair(0, -1));
  EXPECT(fits_pols(2, "aabb", -1) == std::make_pair(0, 1));
  EXPECT(fits_pols(4, "AABBCRCI", -1) == std::make_pair(0, 1));
  EXPECT(fits_pols(4, "IQUV", -1) == std::make_pair(0, -1));
  EXPECT(fits_pols(4, "AABBCRCI", 3) == std::make_pair(3, -1));
  EXPECT(throws_with([] { fits_pols(2, "XXYY", -1); }, "needs --pol"));
  EXPECT(throws_with([] { fits_pols(2, "AABB", 2); }, "not below NPOL"));

  EXPECT(fits_telescope_id("Arecibo") == 1 && fits_telescope_id("ooty") == 2 && fits_telescope_id("NANCAY") == 3);
  EXPECT(fits_telescope_id(" PARKES ") == 4 && fits_telescope_id("Jodrell") == 5 && fits_telescope_id("gbt") == 6);
  EXPECT(fits_telescope_id("GMRT") == 7 && fits_telescope_id("Effelsberg") == 8 && fits_telescope_id("LOFAR") == 11);
  EXPECT(fits_telescope_id("VLA") == 12 && fits_telescope_id("MeerKAT") == 64 && fits_telescope_id("FAST") == 0);
  EXPECT(fits_telescope_id("") == 0);

  EXPECT(fits_sexagesimal("12:34:56.7") == 123456.7 && fits_sexagesimal("-01:02:03.4") == -10203.4);
  EXPECT(fits_sexagesimal("+45:00:00") == 450000.0 && fits_sexagesimal("00:00:01.25") == 1.25);
  EXPECT(fits_sexagesimal("-00:00:30") == -30.0 && fits_sexagesimal("") == 0.0 && fits_sexagesimal("12h") == 0.0);
  EXPECT(fits_sexagesimal("a:b:c") == 0.0);

  FitsCmdLineOptions a;
  a.pol = "3";
  a.no_offsets = true;
  a.machine_id = 9;
  const FitsOptions o = fits_options_from(a);
  EXPECT(o.pol == 3 && o.no_offsets && !o.no_scales && o.machine_id == 9 && o.telescope_id == -1);
  a.pol = "x";
  EXPECT(throws_with([&] { fits_options_from(a); }, "--pol must be auto"));
}

}  // namespace

int main() {
  test_parser();
  test_tform();
  test_slots();
  test_band_pols_header_fields();
  std::cout << (g_failed == 0 ? "all fits unit tests passed, " : "FAILURES: ") << g_failed << " failed" << std::endl;
  return g_failed == 0 ? 0 : 1;
}
