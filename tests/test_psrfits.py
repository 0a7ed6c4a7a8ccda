"""fits2fil (csrc/include/psoup/psrfits.hpp; an extension beyond the reference):
read one search-mode PSRFITS file into the 8-bit, descending-frequency
filterbank the other tools read.

CPU: the NumPy writer / reader round trip against the native parser, TFORM and
column offsets, every refusal by its message, identities of the NumPy oracle,
the contraction guard of the decode test's input, option parsing and the native
host unit tests with their sanitizer builds.  GPU (test_psrfits_gpu.py): the
kernel and the whole tool must EQUAL the oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import psrfits as pf
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils.sigproc import read_header

L = C.digi_stat_block()
NAN = 0x7FC00000

# ------------------------------------------------------- the decode cases ----
KINDS = [(1, False), (2, False), (4, False), (8, False), (8, True), (16, False), (16, True)]
NCHANS = (8, 24, 72, 136, 1, 6, 520)       # 1 and 6 where NCHAN x NBITS is a multiple of 8; 520: two workgroups
NSBLKS = (1, 37, 512)
POLS = [(1, "AA+BB", -1), (2, "AABB", -1), (4, "AABBCRCI", -1), (4, "IQUV", -1), (4, "AABBCRCI", 3)]
SLOT_ROW = [0, 1, -1, 2, 3, 4]             # 5 rows, slot 2 dropped
Z = 1.5


def raw_range(nbits, signed):
    if nbits < 8 or not signed:
        return 0, (1 << nbits) - 1
    return -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1


def full_mantissa(rng, shape, lo=-3, hi=3):
    """float32 values with random mantissas, signs and exponents in [lo, hi)."""
    m = rng.integers(0, 1 << 23, shape).astype(np.uint32)
    e = rng.integers(127 + lo, 127 + hi, shape).astype(np.uint32)
    s = rng.integers(0, 2, shape).astype(np.uint32)
    return ((s << 31) | (e << 23) | m).view(np.float32)


@functools.lru_cache(maxsize=None)
def decode_case(nbits, signed, nchan, npol, nsblk):
    """(raw, scl, offs, wts) of 5 rows with the special cells of the sweep: a zero weight, an infinite scale, a
    cell that overflows float32 and a cell whose result is subnormal in float32."""
    rng = np.random.default_rng(nbits * 1000 + nchan * 10 + npol + nsblk + (5 if signed else 0))
    lo, hi = raw_range(nbits, signed)
    raw = rng.integers(lo, hi + 1, (5, nsblk, npol, nchan)).astype(np.int32)
    scl = full_mantissa(rng, (5, npol, nchan))
    offs = full_mantissa(rng, (5, npol, nchan), -2, 6)
    wts = np.abs(full_mantissa(rng, (5, nchan), -1, 1))
    c1 = 1 % nchan
    wts[0, 0] = 0.0
    wts[2, c1] = -0.0
    scl[1, :, 0] = np.inf
    scl[3, :, 0] = 3e38
    offs[3, :, 0] = 0.0
    wts[3, 0] = 1.0
    scl[4, :, 0] = (np.arange(npol) + 1) * np.float32(1e-44)   # subnormal scales, subnormal results
    offs[4, :, 0] = 0.0
    wts[4, 0] = 1.0
    for a in (raw, scl, offs, wts):
        a.setflags(write=False)
    return raw, scl, offs, wts


def decode_shapes(nbits):
    return [(nchan, npol, ptype, pol, nsblk) for nchan in NCHANS if (nchan * nbits) % 8 == 0
            for npol, ptype, pol in POLS for nsblk in NSBLKS if nchan != 520 or nsblk == 37]


@functools.lru_cache(maxsize=None)
def contraction_case():
    """8-bit data with z = float32(1/3): raw - z has 33 significant bits, so its product with a 24-bit scale is not
    exact in double (with z = 1.5 it always is, and no contraction could show).  Offsets that cancel the product for
    the samples at the level 100 leave the product's rounding error as the leading bits of the result."""
    rng = np.random.default_rng(77)
    nsblk, npol, nchan = 256, 2, 72
    raw = rng.integers(0, 256, (5, nsblk, npol, nchan)).astype(np.int32)
    raw[:, ::2] = 100
    scl = full_mantissa(rng, (5, npol, nchan))
    z = np.float32(1.0) / np.float32(3.0)
    offs = (-((100.0 - np.float64(z)) * scl.astype(np.float64))).astype(np.float32)
    keep = rng.random((5, npol, nchan)) < 0.25
    offs = np.where(keep, full_mantissa(rng, (5, npol, nchan), -2, 6), offs)
    wts = np.abs(full_mantissa(rng, (5, nchan), -1, 1))
    return raw, scl, offs, wts, float(z)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------ the whole-tool case ----
@functools.lru_cache(maxsize=None)
def tool_case():
    """9 slots of NSBLK = 1000 samples (a file holds whole rows, so 9000 samples stand for the 2 x 4096 + 300 asked
    for: two whole statistics blocks and a short one, with rows that cross the blocks), 72 channels, 4 bits, AABB,
    ascending band, per-row scales that undo a gain drift, one dropped row and one zero-weight channel.  Returns
    (file bytes, raw samples, kwargs of the writer)."""
    rng = np.random.default_rng(2024)
    nchan, nsblk, nrows = 72, 1000, 8
    slots = np.array([0, 1, 2, 3, 5, 6, 7, 8])                  # slot 4 dropped: 9 slots
    gain = (1.0 + 0.1 * np.arange(nrows))[:, None, None] * np.ones((1, 2, nchan))    # the recorded level drifts down
    true = rng.normal(0.0, 2.4, (nrows, nsblk, 2, nchan))
    raw = np.clip(np.rint(true / gain[:, None] + 7.5), 0, 15).astype(np.int32)
    scl = gain.astype(np.float32)
    offs = (-7.5 * gain + np.arange(nchan)[None, None, :]).astype(np.float32)
    wts = np.ones((nrows, nchan), np.float32)
    wts[:, 9] = 0.0
    wts[2, 11] = 0.0                                            # zero in one row only: NaN there, the channel lives
    tbin = 1e-3
    kw = dict(nbits=4, tbin=tbin, freq=1200.0 + 0.5 * np.arange(nchan), scl=scl, offs=offs, wts=wts,
              offs_sub=(slots + 0.5) * nsblk * tbin + 3.0, zero_off=0.0,
              primary={"TELESCOP": "GBT", "SRC_NAME": "J1234+56", "RA": "12:34:56.78", "DEC": "-05:06:07.8",
                       "STT_IMJD": 58000, "STT_SMJD": 3600, "STT_OFFS": 0.125, "BEAM_ID": "2"})
    return pf.psrfits_bytes(raw, **kw), raw, kw


TOOL_NSAMPS = 9 * 1000


# ------------------------------------------------------------------- CPU ----
def _small(**kw):
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, (3, 4, 2, 8)).astype(np.int32)
    args = dict(nbits=8, tbin=1e-3, freq=1500.0 - 0.5 * np.arange(8))
    args.update(kw)
    return raw, pf.psrfits_bytes(raw, **args)


def _arr(b):
    return np.frombuffer(b, np.uint8)


def test_fits_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_fits_cmdline(["fits2fil", "-i", "x.fits"])
    assert ok and not exit_now and a.infilename == "x.fits"
    assert (a.sigma_out, a.scale, a.rescale_blocks, a.pol, a.verbose) == (16.0, "channel", 0, "auto", False)
    assert (a.no_scales, a.no_offsets, a.no_weights, a.telescope_id, a.machine_id) == (False, False, False, -1, 0)
    assert a.outfilename.endswith("_fits2fil.fil") and len(a.outfilename) == len("2026-01-01-00:00_fits2fil.fil")
    ok, _, a = C.parse_fits_cmdline(["fits2fil", "-i", "y.fits", "-o", "o.fil", "-k", "k.txt", "--kill_out", "ko.txt",
                                     "--sigma_out", "12.5", "--scale", "file", "--rescale_blocks", "8", "--pol", "1",
                                     "--no_scales", "--no_offsets", "--no_weights", "--telescope_id", "6",
                                     "--machine_id", "11", "-v"])
    assert ok and (a.outfilename, a.killfilename, a.killoutfilename) == ("o.fil", "k.txt", "ko.txt")
    assert (a.sigma_out, a.scale, a.rescale_blocks, a.pol, a.verbose) == (12.5, "file", 8, "1", True)
    o = C.fits_options_from(a)
    assert (o.pol, o.no_scales, o.no_offsets, o.no_weights, o.telescope_id, o.machine_id) == (1, True, True, True, 6, 11)
    p = C.fits_digi_params_from(a)
    assert (p.sigma_out, p.scale, p.rescale_blocks) == (12.5, "file", 8)
    assert C.parse_fits_cmdline(["fits2fil", "-h"])[:2] == (True, True)
    for extra in (["--sigma_out", "0"], ["--scale", "both"], ["--rescale_blocks", "-1"], ["--pol", "x"],
                  ["--machine_id", "-3"], ["--nsub", "4"]):
        assert not C.parse_fits_cmdline(["fits2fil", "-i", "x.fits"] + extra)[0]
    assert not C.parse_fits_cmdline(["fits2fil", "--sigma_out", "3"])[0]    # -i is required


def test_writer_reader_round_trip_with_foreign_hdus_and_column_order():
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 16, (3, 5, 2, 6)).astype(np.int32)
    scl = rng.normal(1, 0.1, (3, 2, 6)).astype(np.float32)
    offs = rng.normal(0, 3, (3, 2, 6)).astype(np.float32)
    wts = rng.random((3, 6)).astype(np.float32)
    history = pf.bintable_hdu("HISTORY", [("DATE_PRO", "24A", ["2020-01-01", "2020-01-02"]),
                                          ("NSUB", "1J", np.array([3, 4]))])
    heap = pf.bintable_hdu("POLYCO", [("NSPAN", "1I", np.array([7])), ("FLAGS", "9X", np.zeros((1, 2), np.uint8))],
                           heap=b"\x05" * 4001)                  # PCOUNT > 0, more than a block
    order = ["DATA", "TSUBINT", "DAT_SCL", "DAT_WTS", "OFFS_SUB", "DAT_OFFS", "LST_SUB", "DAT_FREQ"]
    extra = [("TSUBINT", "D", np.full(3, 5e-3)), ("LST_SUB", "1E", np.arange(3.0))]
    b = pf.psrfits_bytes(raw, 4, 1e-3, 1400.0 + 2.0 * np.arange(6), scl=scl, offs=offs, wts=wts, column_order=order,
                         extra_columns=extra, hdus_before=[history, heap], freq_form="D", zero_off=-2.5, signint=0)
    assert len(b) % 2880 == 0
    f = pf.read_psrfits(b)
    n = C.fits_parse(_arr(b))
    # column offsets against a hand-computed table: DATA 5*2*6*4/8 = 30 B, D 8, 12E 48, 6E 24, D 8, 12E 48, E 4, 6D 48
    hand = [("DATA", "B", 30, 0, 30), ("TSUBINT", "D", 1, 30, 8), ("DAT_SCL", "E", 12, 38, 48),
            ("DAT_WTS", "E", 6, 86, 24), ("OFFS_SUB", "D", 1, 110, 8), ("DAT_OFFS", "E", 12, 118, 48),
            ("LST_SUB", "E", 1, 166, 4), ("DAT_FREQ", "D", 6, 170, 48)]
    assert f["columns"] == hand == [tuple(c) for c in n["columns"]]
    assert f["row_bytes"] == 218 == n["row_bytes"] and f["nrows"] == 3 == n["nrows"]
    # primary 1 block, HISTORY 1 + 1, POLYCO 1 + 2 (4 B of table and the heap), the SUBINT header (37 cards) 2
    assert f["table_off"] == n["table_off"] == 2880 * (1 + 2 + 3 + 2)
    for k in ("npol", "nbits", "nchan", "nsblk", "signint", "tbin", "z", "pol_type", "chan_bw"):
        assert f[k] == n[k], k
    assert (f["npol"], f["nbits"], f["nchan"], f["nsblk"], f["z"], f["pol_type"]) == (2, 4, 6, 5, 2.5, "AABB")
    assert n["primary"]["TELESCOP"] == "Parkes" == f["primary"]["TELESCOP"] and n["subint"]["EXTNAME"] == "SUBINT"
    assert np.array_equal(bits(f["DAT_SCL"]), bits(scl)) and np.array_equal(bits(f["DAT_OFFS"]), bits(offs))
    assert np.array_equal(bits(f["DAT_WTS"]), bits(wts)) and np.array_equal(f["DAT_FREQ"][1], 1400.0 + 2.0 * np.arange(6))
    assert np.array_equal(f["OFFS_SUB"], (np.arange(3) + 0.5) * 5e-3)
    assert np.array_equal(pf.unpack_samples(f["DATA"], 4).reshape(raw.shape), raw)
    # TFORM with and without a repeat count
    for s, want in (("1D", (1, "D", 8)), ("D", (1, "D", 8)), ("E", (1, "E", 4)), ("4096E", (4096, "E", 16384)),
                    ("3I", (3, "I", 6)), ("J", (1, "J", 4)), ("24A", (24, "A", 24)), ("9X", (9, "X", 2)),
                    ("16B", (16, "B", 16))):
        assert pf.parse_tform(s) == want == tuple(C.fits_tform(s)), s
    for bad in ("1PE(5)", "4Q", ""):
        with pytest.raises(ValueError, match="unsupported TFORM"):
            pf.parse_tform(bad)
        with pytest.raises(C.NativeError, match="unsupported TFORM"):
            C.fits_tform(bad)
    # the whole validation, natively: slots, band, polarisations and header
    i = C.fits_inspect(_arr(b), C.FitsOptions(), "x.sf")
    assert i["slots"]["nslots"] == 3 and i["band"] == (1400.0, 2.0) and tuple(i["pols"]) == (0, 1)
    assert (i["header"]["fch1"], i["header"]["foff"], i["header"]["nsamples"]) == (1410.0, -2.0, 15)


REFUSALS = [
    ("not FITS", lambda: b"HEADER_START" + bytes(4000), "not a FITS file"),
    ("fold mode", lambda: _small(primary={"OBS_MODE": "PSR"})[1], "not SEARCH"),
    ("no OBS_MODE", lambda: _small(primary={"OBS_MODE": None})[1], "missing key OBS_MODE"),
    ("no SUBINT", lambda: _small()[1][:2880] + pf.bintable_hdu("HISTORY", [("A", "1J", np.arange(2))]), "no SUBINT table"),
    ("missing key", lambda: _small(subint={"NSBLK": None})[1], "missing key NSBLK"),
    ("missing TBIN", lambda: _small(subint={"TBIN": None})[1], "missing key TBIN"),
    ("missing primary key", lambda: _small(primary={"STT_IMJD": None})[1], "missing key STT_IMJD"),
    ("missing column", lambda: _small(column_order=["OFFS_SUB", "DAT_FREQ", "DAT_OFFS", "DAT_SCL", "DATA"])[1],
     "missing column DAT_WTS"),
    ("no DATA", lambda: _small(column_order=["DAT_FREQ", "DAT_WTS", "DAT_OFFS", "DAT_SCL"])[1], "missing column DATA"),
    ("NBITS", lambda: _small(subint={"NBITS": 3})[1], "NBITS must be 1, 2, 4, 8 or 16"),
    ("NBITS 32", lambda: _small(subint={"NBITS": 32})[1], "NBITS must be 1, 2, 4, 8 or 16"),
    ("bits per sample", lambda: pf.psrfits_bytes(np.zeros((2, 4, 1, 8), np.int32), 4, 1e-3, np.arange(8.0) + 1,
                                                 subint={"NCHAN": 7}), "NCHAN x NBITS must be a multiple of 8"),
    ("DATA size", lambda: _small(subint={"NSBLK": 5})[1], "DATA column holds 64 bytes"),
    ("float DATA", lambda: _small(data_form="16E")[1], "DATA must be of type B or I"),
    ("DAT_WTS length", lambda: _small(subint={"NCHAN": 16, "NSBLK": 2})[1], "DAT_FREQ has the wrong length"),
    ("DAT_SCL length", lambda: _small(subint={"NPOL": 1, "NSBLK": 8})[1], "DAT_OFFS has the wrong length"),
    ("NAXIS1", lambda: _small(naxis1_extra=1)[1], "add up to 264 bytes, NAXIS1 is 265"),
    ("truncated in the table", lambda: _small()[1][:2 * 2880 + 300], "runs past the end of the file"),
    ("truncated in a header", lambda: _small()[1][:2880 + 800], "header runs past the end"),
    ("NAXIS2 = 0", lambda: _small(subint={})[1].replace(pf._card("NAXIS2", 3), pf._card("NAXIS2", 0)), "NAXIS2 = 0"),
    ("fractional gap", lambda: _small(offs_sub=[0.002, 0.0085, 0.010])[1], "whole row"),
    ("rows out of order", lambda: _small(offs_sub=[0.002, 0.010, 0.006])[1], "increase strictly"),
    ("too many dropped", lambda: _small(offs_sub=[0.002, 0.006, 0.030])[1], "more than half the rows are dropped"),
    ("uneven band", lambda: _small(freq=[1500, 1499.5, 1499, 1498.5, 1498, 1497.5, 1497, 1496.4])[1],
     "not evenly spaced"),
    ("foff = 0", lambda: _small(freq=np.full(8, 1400.0))[1], "foff must not be zero"),
    ("pol type", lambda: _small(pol_type="XXYY")[1], "needs --pol"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_every_refusal_by_its_message(case):
    _, make, msg = case
    b = make()
    with pytest.raises(C.NativeError, match=msg):
        C.fits_inspect(_arr(b), C.FitsOptions(), "")
    if msg not in ("missing key STT_IMJD",):                     # the oracle reads that key only for the header
        with pytest.raises(ValueError):
            ref.fits_filterbank(b)


def test_refusals_of_options_and_sizes(tmp_path):
    _, b = _small()
    with pytest.raises(C.NativeError, match="not below NPOL"):
        C.fits_inspect(_arr(b), C.FitsOptions(pol=2), "")
    assert tuple(C.fits_inspect(_arr(_small(pol_type="XXYY")[1]), C.FitsOptions(pol=1), "")["pols"]) == (1, -1)
    with pytest.raises(C.NativeError, match="too many samples"):
        C.fits_row_slots([], 1 << 20, 4096, 64e-6)
    assert C.fits_row_slots([], 1 << 19, 4095, 64e-6)["nsamps"] == (1 << 19) * 4095
    a = C.FitsCmdLineOptions()
    a.pol = "x"
    with pytest.raises(C.NativeError, match="--pol must be auto"):
        C.fits_options_from(a)
    a = C.FitsCmdLineOptions()
    a.sigma_out = -1.0
    with pytest.raises(C.NativeError, match="sigma_out must be positive"):
        C.digi_check_params(C.fits_digi_params_from(a))
    # a file the command line cannot read says so by name and writes nothing
    r = subprocess.run([os.path.join(REPO, "bin", "fits2fil"), "-i", str(tmp_path / "none.fits"), "-o",
                        str(tmp_path / "never.fil")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "cannot open" in r.stderr and not os.path.exists(str(tmp_path / "never.fil"))


def test_oracle_unpacking_and_identities():
    one = np.ones((1, 1, 8), np.float32)
    w = np.ones((1, 8), np.float32)
    # 8 bits, scale 1, offset 0, weight 1, z = 0: the integers
    raw = np.arange(40, dtype=np.int32).reshape(1, 5, 1, 8) * 6
    x = ref.fits_decode(raw, one, 0 * one, w, [0], (0, -1))
    assert np.array_equal(x, raw.reshape(5, 8).astype(np.float32))
    # first sample in the top bits, on hand-written bytes
    assert pf.unpack_samples(np.array([0b10110001], np.uint8), 1).tolist() == [1, 0, 1, 1, 0, 0, 0, 1]
    assert pf.unpack_samples(np.array([0b11100100], np.uint8), 2).tolist() == [3, 2, 1, 0]
    assert pf.unpack_samples(np.array([0xA5, 0x0F], np.uint8), 4).tolist() == [10, 5, 0, 15]
    assert pf.pack_samples(np.array([[1, 0, 1, 1, 0, 0, 0, 1]]), 1).tolist() == [0b10110001]
    assert pf.pack_samples(np.array([[3, 2, 1, 0]]), 2).tolist() == [0b11100100]
    assert pf.pack_samples(np.array([[10, 5, 0, 15]]), 4).tolist() == [0xA5, 0x0F]
    # 16 bits big-endian, signed and unsigned; 8 bits two's complement
    b16 = np.array([0x01, 0x02, 0xFF, 0xFE, 0x80, 0x00], np.uint8)
    assert pf.unpack_samples(b16, 16).tolist() == [258, 65534, 32768]
    assert pf.unpack_samples(b16, 16, True).tolist() == [258, -2, -32768]
    assert pf.pack_samples(np.array([[258, -2, -32768]]), 16).tolist() == b16.tolist()
    assert pf.unpack_samples(np.array([0x7F, 0x80, 0xFF], np.uint8), 8, True).tolist() == [127, -128, -1]
    assert pf.unpack_samples(np.array([0x7F, 0x80, 0xFF], np.uint8), 8).tolist() == [127, 128, 255]
    # polarisations
    raw = np.random.default_rng(0).integers(0, 200, (2, 3, 4, 8)).astype(np.int32)
    s4, o4, w2 = np.ones((2, 4, 8), np.float32), np.zeros((2, 4, 8), np.float32), np.ones((2, 8), np.float32)
    dec = lambda pols, **kw: ref.fits_decode(raw, s4, o4, w2, kw.pop("slots", [0, 1]), pols, **kw)   # noqa: E731
    assert np.array_equal(dec(ref.fits_pols(4, "AABBCRCI")), (raw[:, :, 0] + raw[:, :, 1]).reshape(6, 8))
    assert np.array_equal(dec(ref.fits_pols(4, "IQUV")), raw[:, :, 0].reshape(6, 8))
    assert np.array_equal(dec(ref.fits_pols(4, "aabb ", 1)), raw[:, :, 1].reshape(6, 8))
    assert ref.fits_pols(1, "AA+BB") == (0, -1) == tuple(C.fits_pols(1, "AA+BB")) and ref.fits_pols(2, "AABB") == (0, 1)
    assert np.array_equal(dec((0, -1), z=1.5), raw[:, :, 0].reshape(6, 8) - 1.5)
    # a zero weight and a dropped slot: the NaN pattern; t0 / count cut anywhere
    w0 = w2.copy()
    w0[1, 3] = 0.0
    x = ref.fits_decode(raw, s4, o4, w0, [0, -1, 1], (0, 1))
    assert x.shape == (9, 8) and (bits(x[3:6]) == NAN).all() and (bits(x[6:, 3]) == NAN).all()
    assert np.isfinite(x[:3]).all() and np.isfinite(np.delete(x[6:], 3, axis=1)).all()
    assert np.array_equal(bits(ref.fits_decode(raw, s4, o4, w0, [0, -1, 1], (0, 1), t0=2, count=6)), bits(x[2:8]))


def test_oracle_whole_tool_nan_cells_header_and_band(tmp_path):
    b, raw, kw = tool_case()
    out = str(tmp_path / "o.fil")
    res = ref.fits_filterbank(b, out, kill_out=str(tmp_path / "k.txt"), rawdatafile="obs.sf")
    x, y = res["x"], res["y"]
    assert x.shape == (TOOL_NSAMPS, 72) == y.shape and res["flip"] and res["slots"]["ndropped"] == 1
    # the dropped slot 4, the dead channel 9 and channel 11 in row 2 are NaN, give 128 and are counted
    assert (bits(x[4000:5000]) == NAN).all() and (bits(x[:, 9]) == NAN).all() and (bits(x[2000:3000, 11]) == NAN).all()
    assert (y[4000:5000] == 128).all() and (y[:, 71 - 9] == 128).all() and (y[2000:3000, 71 - 11] == 128).all()
    assert res["nbad"][9] == TOOL_NSAMPS and res["nbad"][11] == 2000 and res["nbad"][0] == 1000
    assert res["killmask"][71 - 9] == 0 and sum(res["killmask"]) == 71
    assert open(tmp_path / "k.txt").read().split()[71 - 9] == "0"
    # the per-row scales undo the drift: every live channel at mean 128, sigma 16
    live = np.delete(y[np.r_[0:4000, 5000:9000]].astype(float), [71 - 9, 71 - 11], axis=1)
    assert np.abs(live.mean(axis=0) - 128).max() < 1.0 and np.abs(live.std(axis=0) - 16).max() < 1.5
    h = read_header(out)
    assert open(out, "rb").read() == res["header_bytes"] + y.tobytes() and not os.path.exists(out + ".tmp")
    assert (h["nchans"], h["nbits"], h["nifs"], h["nsamples"], h["data_type"]) == (72, 8, 1, TOOL_NSAMPS, 1)
    assert (h["fch1"], h["foff"], h["tsamp"]) == (1200.0 + 71 * 0.5, -0.5, 1e-3)
    assert (h["telescope_id"], h["machine_id"], h["ibeam"], h["barycentric"]) == (6, 0, 2, 0)
    assert (h["source_name"], h["rawdatafile"]) == ("J1234+56", "obs.sf")
    assert h["src_raj"] == (12 * 10000.0 + 34 * 100.0) + 56.78 and h["src_dej"] == -((5 * 10000.0 + 6 * 100.0) + 7.8)
    assert h["tstart"] == 58000 + (((3600 + 0.125) + (0.5 * 1000 * 1e-3 + 3.0)) - (0.5 * 1000) * 1e-3) / 86400.0
    assert abs(h["tstart"] - (58000 + 3603.125 / 86400)) < 1e-12
    # ... and the native header is the same bytes
    i = C.fits_inspect(_arr(b), C.FitsOptions(), "obs.sf")
    assert i["header"]["bytes"] == res["header_bytes"]
    # a descending band is not flipped; without OFFS_SUB the first row starts at STT
    raw2, b2 = _small(offs_sub=False, primary={"TELESCOP": "unknown", "STT_SMJD": 10, "BEAM_ID": "x"})
    r2 = ref.fits_filterbank(b2, telescope_id=-1, machine_id=7)
    assert not r2["flip"] and (r2["header"]["fch1"], r2["header"]["foff"]) == (1500.0, -0.5)
    assert r2["header"]["tstart"] == 55000 + (((10.0 + 0.0) + 0.002) - 0.002) / 86400.0 and "ibeam" not in r2["header"]["_present"]
    assert (r2["header"]["telescope_id"], r2["header"]["machine_id"]) == (0, 7)
    i2 = C.fits_inspect(_arr(b2), C.FitsOptions(machine_id=7), "")
    assert i2["header"]["bytes"] == r2["header_bytes"]
    for name, tid in list(ref.FITS_TELESCOPES.items()) + [("FAST", 0), ("", 0)]:
        assert C.fits_telescope_id(name.title()) == tid
    for s in ("12:34:56.7", "-01:02:03.4", "+45:00:00", "-00:00:30", "", "12h", "1:2"):
        assert C.fits_sexagesimal(s) == ref.fits_sexagesimal(s), s
    assert ref.fits_sexagesimal("-01:02:03.4") == -10203.4


def test_contraction_guard():
    """The decode test's input would expose a contracted FMA: on at least one cell the float32 result of the defined
    two-rounding evaluation differs from a fused one (emulated in the 64-bit mantissa of np.longdouble, where the
    33-bit x 24-bit product is exact)."""
    assert np.finfo(np.longdouble).nmant >= 63
    raw, scl, offs, wts, z = contraction_case()
    d = raw[:, :, 0, :].astype(np.float64) - z
    s, o = scl[:, None, 0, :].astype(np.float64), offs[:, None, 0, :].astype(np.float64)
    two = ((d * s) + o).astype(np.float32)
    fused = (d.astype(np.longdouble) * s.astype(np.longdouble) + o.astype(np.longdouble)).astype(np.float64).astype(np.float32)
    assert (bits(two) != bits(fused)).sum() > 0
    # ... and the oracle is the two-rounding one
    x = ref.fits_decode(raw, scl, offs, np.ones_like(wts), [0, 1, 2, 3, 4], (0, -1), z)
    assert np.array_equal(bits(x), bits(two.reshape(-1, raw.shape[3])))
    # with z = 1.5 the product is exact in double: no input could tell
    r2, s2, o2, _ = decode_case(16, False, 72, 2, 37)
    d2 = r2[:, :, 0, :].astype(np.float64) - 1.5
    exact = d2.astype(np.longdouble) * s2[:, None, 0, :].astype(np.longdouble)
    assert np.array_equal((d2 * s2[:, None, 0, :].astype(np.float64)).astype(np.longdouble), exact)


def test_decode_sweep_covers_what_it_claims():
    seen = set()
    for nbits, signed in KINDS:
        for nchan, npol, ptype, pol, nsblk in decode_shapes(nbits):
            seen.add((nchan % 8 != 0, nchan > 64 * 8, npol, ref.fits_pols(npol, ptype, pol), nsblk))
        raw, scl, offs, wts = decode_case(nbits, signed, 8, 2, 37)
        x = ref.fits_decode(raw, scl, offs, wts, SLOT_ROW, (0, 1), Z)
        assert (bits(x[2 * 37:3 * 37]) == NAN).all() and (bits(x[:37, 0]) == NAN).all()       # dropped, zero weight
        assert not np.isfinite(x[37:2 * 37, 0]).any()                                         # infinite scale
        assert np.isinf(x[4 * 37:5 * 37, 0]).any()                                            # overflow
        sub = x[5 * 37:, 0]
        assert ((np.abs(sub) < np.finfo(np.float32).tiny) & (sub != 0)).any()                 # subnormal results
    assert {s[0] for s in seen} == {True, False} == {s[1] for s in seen} and {s[3] for s in seen} == {(0, -1), (0, 1), (3, -1)}
    assert [n for n in NCHANS if (n * 1) % 8 == 0] == [8, 24, 72, 136, 520] and 6 in [n for n in NCHANS if (n * 4) % 8 == 0]
    assert 1 in [n for n in NCHANS if (n * 8) % 8 == 0] and 1 not in [n for n in NCHANS if (n * 4) % 8 == 0]


def _run_native(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    return r


def test_native_unit_tests():
    _run_native(os.path.join(REPO, "bin", "psoup_fits_unit_tests"))


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_host_sanitizers(san):
    """A stand-alone host binary built with the sanitizer, run in the inherited environment."""
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_fits_unit_tests")
    r = _run_native(os.path.join(REPO, "bin", f"psoup_fits_unit_tests_{san}"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
