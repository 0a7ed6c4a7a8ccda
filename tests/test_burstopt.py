"""burstopt (csrc/include/psoup/burstopt.hpp; an extension beyond the
reference): a search over DM rows, boxcar widths and start bins on burst
cutouts.  The CPU half: option parsing, the C++ host steps against the NumPy
oracle (exact, doubles bit for bit), the refusals, identities of the oracle,
recovery of an injected burst on the oracle, a zero-DM impulse, a narrow-band
burst, the result file (Python and native writers byte-identical), the DM
panel and the host unit tests with their sanitizer builds.  The GPU half is
tests/test_burstopt_gpu.py."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.outputs import BurstOptFile, write_bopt_file
from peasoup_amd.utils.plotting import burst_dm_curve_panel

TSAMP = 64e-6
SEARCH_KEYS = ("best_val", "best_idx", "curve", "curve_bin")


def test_bopt_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_bopt_cmdline(["burstopt", "-i", "c.bursts"])
    assert ok and not exit_now and a.infilename == "c.bursts"
    assert (a.nfine, a.fine_half_range, a.limit) == (65, 0.0, 1000) and not a.verbose
    assert a.outfilename.endswith("_burstopt.bopt") and len(a.outfilename) == len("2026-01-01-00:00_burstopt.bopt")
    ok, _, a = C.parse_bopt_cmdline(["burstopt", "-i", "y.bursts", "-o", "out.bopt", "--nfine", "17",
                                     "--fine_half_range", "2.5", "--limit", "7", "-v"])
    assert ok and (a.outfilename, a.nfine, a.fine_half_range, a.limit, a.verbose) == ("out.bopt", 17, 2.5, 7, True)
    ok, exit_now, _ = C.parse_bopt_cmdline(["burstopt", "-h"])
    assert ok and exit_now


@pytest.mark.parametrize("extra", [["--nfine", "64"], ["--nfine", "0"], ["--nfine", "259"], ["--nfine", "-3"],
                                   ["--fine_half_range", "-1"], ["--limit", "-1"]])
def test_bopt_cmdline_errors(extra):
    assert not C.parse_bopt_cmdline(["burstopt", "-i", "c.bursts"] + extra)[0]
    assert not C.parse_bopt_cmdline(["burstopt"] + extra)[0]  # -i is required
    assert not C.parse_bopt_cmdline(["burstopt"])[0]


def make_cutout(ntime, nsub, ndm, seed, dm=55.5, f=4, holes=False, dead_sub=(), dead_dm=(), level=1000, spread=100):
    """A random cutout with burstcube's keys: unequal hits, a pulse in the middle, optionally empty bins, subbands
    without any hit (killed) and DM rows without any hit."""
    rng = np.random.default_rng(seed)
    nact = rng.integers(1, 5, nsub).astype(np.int32)
    ds_hits = (f * nact[:, None] * np.ones((1, ntime), np.int64)).astype(np.int32)
    dmt_hits = np.full((ndm, ntime), f * int(nact.sum()), np.int32)
    if holes:
        ds_hits[:, :2] //= 2                 # short bins at the edge of the file
        ds_hits[0, ntime - 3:] = 0           # empty off-pulse bins
        ds_hits[nsub - 1, ntime // 2] = 0    # an empty on-pulse bin
        dmt_hits[:, 0] = 0
        dmt_hits[ndm - 1, ntime // 3:] //= 3
    for s in dead_sub:
        ds_hits[s] = 0
        nact[s] = 0
    for j in dead_dm:
        dmt_hits[j] = 0
    rate = rng.integers(level - spread, level + spread, (nsub, ntime)).astype(np.int64)
    rate[:, ntime // 2 - 1:ntime // 2 + 1] += 3 * spread
    ds_sums = rate * ds_hits // 7
    rate = rng.integers(level - spread, level + spread, (ndm, ntime)).astype(np.int64)
    rate[ndm // 2, ntime // 2 - 1:ntime // 2 + 1] += 3 * spread
    dmt_sums = rate * dmt_hits // 7
    return {"sample": 5000 + seed, "width": 2 * f, "tscrunch": f, "t0": 5000 + seed + f - (ntime // 2) * f,
            "dm": float(np.float32(dm)), "snr": 9.5, "dms": ref.burst_dms(dm, ndm), "nactive": nact,
            "ds_sums": ds_sums.astype(np.int32), "ds_hits": ds_hits, "dmt_sums": dmt_sums.astype(np.int32),
            "dmt_hits": dmt_hits}


def assert_same_record(got, exp):
    assert set(exp) <= set(got), set(exp) - set(got)
    for k, e in exp.items():
        if isinstance(e, np.ndarray):
            g = np.asarray(got[k])
            assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), k
        else:
            assert got[k] == e, (k, got[k], e)


def _geom(ntime, nsub, ndm, nchans=64):
    return C.BurstOptGeom(ntime, nsub, ndm, nchans, TSAMP, 1510.0, -1.09)


# ntime, nsub, ndm, nfine, fine_half_range, cutout options
HOST_CASES = {
    "full_hits": (32, 5, 6, 9, 0.0, dict()),
    "empty_bins_and_rows": (33, 7, 5, 5, 0.0, dict(holes=True, dead_dm=(1,))),
    "killed_subband": (16, 4, 4, 3, 2.5, dict(dead_sub=(2,))),
    "dm_zero": (24, 3, 4, 5, 0.0, dict(dm=0.0)),
    "one_dm_row": (40, 6, 1, 7, 0.0, dict(holes=True)),
    "one_fine_row": (8, 2, 3, 1, 0.0, dict()),
}


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_host_steps_equal_the_oracle(name):
    ntime, nsub, ndm, nfine, half, opts = HOST_CASES[name]
    cand = make_cutout(ntime, nsub, ndm, seed=ntime, **opts)
    g, grid = _geom(ntime, nsub, ndm), C.BurstOptGrid(nfine, half)
    delays = np.asarray(C.generate_delay_table(64, TSAMP, 1510.0, -1.09), dtype=np.float32)
    got = C.burst_opt_prepare(0, g, cand)
    exp = ref.burst_opt_prepare(cand)
    assert_same_record(got, exp)  # v, mbar_ds and mbar_dmt bit for bit
    assert exp["v"] > 0 and exp["d_ds"].any() and exp["d_dmt"].any()
    if name == "full_hits":
        # with full hits q == sums: d is the sums less their off-pulse floor mean
        off = np.r_[0:ntime // 4, ntime - ntime // 4:ntime]
        s = cand["ds_sums"].astype(np.int64)
        assert np.array_equal(exp["d_ds"], s - (s[:, off].sum(axis=1) // len(off))[:, None])
    if name == "killed_subband":
        assert exp["cnt_ds"][2] == 0 and not exp["d_ds"][2].any() and exp["moff_ds"][2] == 0
    if name == "empty_bins_and_rows":
        assert exp["cnt_dmt"][1] == 0 and exp["mbar_dmt"][1] == 0.0 and not exp["d_dmt"][1].any()
        assert exp["cnt_ds"][0] == 2 * (ntime // 4) - 3 and not exp["d_ds"][0, ntime - 3:].any()
        assert exp["d_dmt"][0, 0] == 0 and exp["d_ds"][nsub - 1, ntime // 2] == 0
    sh = C.burst_opt_shifts(g, grid, cand["dm"], cand["tscrunch"], cand["dms"], [float(x) for x in delays])
    esh = ref.burst_opt_shifts(ntime, nsub, 64, cand["dm"], cand["tscrunch"], cand["dms"], delays, nfine, half)
    for k in ("dmf", "sf"):
        assert sh[k].dtype == esh[k].dtype and sh[k].shape == esh[k].shape and np.array_equal(sh[k], esh[k]), k
    # the fine row nfine / 2 is the candidate's DM and has all-zero shifts
    assert esh["dmf"][nfine // 2] == np.float32(cand["dm"]) and not esh["sf"][nfine // 2].any()
    assert np.abs(esh["sf"]).max() <= ntime and np.all(esh["dmf"] >= 0)
    if name in ("dm_zero", "one_dm_row", "one_fine_row"):
        assert not esh["sf"].any()  # no DM to step over
    else:
        assert esh["sf"].any() and np.all(np.diff(esh["dmf"]) > 0)
    if name == "killed_subband":
        assert esh["dmf"][-1] == np.float32(float(np.float32(55.5)) + 2.5)
    found = ref.burst_opt_search(exp["d_ds"], exp["d_dmt"], esh["sf"])
    host = C.burst_opt_search_host(g, exp["d_ds"], exp["d_dmt"], esh["sf"])
    for k in SEARCH_KEYS:
        assert host[k].dtype == np.int32 and np.array_equal(host[k], found[k]), k
    rec = C.burst_opt_finish(g, grid, cand, exp, esh, found)
    erec = ref.burst_opt_finish(cand, exp, esh, found)
    assert_same_record(rec, erec)  # every S/N bit for bit
    assert (erec["flags"] == 0) == (float(cand["dms"][0]) == 0.0)
    assert erec["snr"] > 0 and 0.0 <= erec["frac_pos"] <= 1.0
    assert erec["opt_sample"] == cand["t0"] + erec["opt_bin"] * cand["tscrunch"]


def test_refusals_name_the_candidate():
    def both(c, ntime, nsub=3, ndm=2, what=""):
        with pytest.raises(C.NativeError, match="candidate 4 .*" + what):
            C.burst_opt_prepare(4, _geom(ntime, nsub, ndm), c)
        with pytest.raises(ValueError, match="candidate 4 .*" + what):
            ref.burst_opt_prepare(c, 4)

    both(make_cutout(7, 3, 2, seed=1), 7, what="below 8")
    cand = make_cutout(16, 3, 2, seed=2)
    ref.burst_opt_prepare(cand, 4)
    both(dict(cand, ds_hits=np.zeros_like(cand["ds_hits"])), 16, what="live")
    # hits in the on-pulse bins alone: still no live row
    on = cand["ds_hits"].copy()
    on[:, :4] = on[:, 12:] = 0
    both(dict(cand, ds_hits=on), 16, what="live")
    # one sample stands in for ten: q = 2^31 - 1 scaled by Href / hits does not fit int32
    bad = dict(cand, ds_sums=cand["ds_sums"].copy(), ds_hits=cand["ds_hits"].copy())
    bad["ds_hits"][1, 8], bad["ds_sums"][1, 8] = 1, 2 ** 31 - 1
    both(bad, 16, what="int32")
    # d fits, but max|d_ds| x 3 live subbands x 8 >= 2^31
    # (with equal hits q == sums, and bin 8 is on-pulse: the baseline B of the row does not move)
    lim = -(-2 ** 31 // (3 * 8))
    B = int(cand["ds_sums"][1, 8]) - int(ref.burst_opt_prepare(cand)["d_ds"][1, 8])
    bad = dict(cand, ds_sums=cand["ds_sums"].copy())
    bad["ds_sums"][1, 8] = lim + B
    both(bad, 16, what="waterfall")
    bad["ds_sums"][1, 8] = lim + B - 1  # one below the bound passes
    assert ref.burst_opt_prepare(bad, 4)["d_ds"][1, 8] == lim - 1
    assert C.burst_opt_prepare(4, _geom(16, 3, 2), bad)["d_ds"][1, 8] == lim - 1
    bad = dict(cand, dmt_sums=cand["dmt_sums"].copy())
    bad["dmt_sums"][0, 8] = 2 ** 31 - 1
    both(bad, 16, what="DM-time")
    both(dict(cand, dm=-1.0), 16)


def test_oracle_identities():
    ntime, nsub, ndm, nfine = 32, 4, 5, 7
    rng = np.random.default_rng(3)
    d_ds = rng.integers(-500, 500, (nsub, ntime)).astype(np.int32)
    d_dmt = rng.integers(-500, 500, (ndm, ntime)).astype(np.int32)
    sf = rng.integers(-3, 4, (nfine, nsub)).astype(np.int32)
    sf[nfine // 2] = 0
    f = ref.burst_opt_search(d_ds, d_dmt, sf)
    nw = ref.burst_opt_nwidths(ntime)
    assert nw == 5 and [ref.burst_opt_nwidths(n) for n in (8, 9, 63, 64, 65, 1000, 1024)] == [3, 3, 5, 6, 6, 9, 10]
    assert np.array_equal(ref.burst_opt_profile(d_ds, sf[nfine // 2]), d_ds.astype(np.int64).sum(axis=0))
    P = np.concatenate([d_dmt.astype(np.int64), np.stack([ref.burst_opt_profile(d_ds, r) for r in sf])])
    for kw in range(nw):
        w = 1 << kw
        for r in range(ndm + nfine):
            boxes = [int(P[r, k:k + w].sum()) for k in range(ntime - w + 1)]  # not circular
            assert f["curve"][kw, r] == max(boxes) and f["curve_bin"][kw, r] == boxes.index(max(boxes))
        for plane, rows in ((0, slice(0, ndm)), (1, slice(ndm, None))):
            assert f["best_val"][plane, kw] == f["curve"][kw, rows].max()
            r = int(np.argmax(f["curve"][kw, rows]))
            assert f["best_idx"][plane, kw] == r * ntime + f["curve_bin"][kw, rows][r]
    # band.sum() is the fine optimum's box sum when no shifted term falls outside the window
    cand = make_cutout(ntime, nsub, ndm, seed=5)
    prep = ref.burst_opt_prepare(cand)
    delays = ref.delay_table(64, TSAMP, 1510.0, -1.09)
    sh = ref.burst_opt_shifts(ntime, nsub, 64, cand["dm"], 4, cand["dms"], delays, nfine)
    found = ref.burst_opt_search(prep["d_ds"], prep["d_dmt"], sh["sf"])
    rec = ref.burst_opt_finish(cand, prep, sh, found)
    w, kf, k = rec["opt_width"] // 4, rec["opt_kf"], rec["opt_bin"]
    assert k + sh["sf"][kf].min() >= 0 and k + w - 1 + sh["sf"][kf].max() < ntime
    assert int(rec["band"].sum()) == int(found["best_val"][1, int(np.log2(w))]) == int(rec["profile"][k:k + w].sum())
    # all-negative planes: the maxima are the least negative boxes, ties to the smallest index
    neg = ref.burst_opt_search(np.full((nsub, ntime), -2, np.int32), np.full((ndm, ntime), -7, np.int32), sf * 0)
    assert np.array_equal(neg["best_val"], np.outer([-7, -2 * nsub], 2 ** np.arange(nw)))
    assert not neg["best_idx"].any() and not neg["curve_bin"].any()


# 64 channels of 8 bits; a burst at DM 100 (a sweep of 277 samples over the band), a zero-DM impulse and a burst
# that exists in eight of the channels only (two of 16 subbands)
R_N = 1 << 15
R_DM, R_WIDTH = 100.0, 16
R_BURST = synthetic.BurstSpec(time=0.8, dm=R_DM, width=R_WIDTH * TSAMP, amplitude=1.0)
R_IMPULSE = synthetic.RfiSpec(kind="impulse", time=1.4, duration=16 * TSAMP, amplitude=1.5)
R_NARROW = [synthetic.RfiSpec(kind="cell", channel=c, time=0.3, duration=64 * TSAMP, amplitude=1.5) for c in range(8, 16)]


@functools.lru_cache(maxsize=None)
def recovery():
    """values, header, delays and the oracle's records of the three candidates."""
    hdr = synthetic.make_header(nchans=64, nbits=8, tsamp=TSAMP)
    delays = ref.delay_table(64, TSAMP, hdr["fch1"], hdr["foff"])
    vals = synthetic.generate(R_N, hdr, (), seed=41, bursts=[R_BURST], rfi=[R_IMPULSE] + R_NARROW)
    header = {"nchans": 64, "tsamp": TSAMP, "fch1": hdr["fch1"], "foff": hdr["foff"]}
    # (sample, width, dm, tscrunch, nsub): the burst at a DM 4 too high, the impulse as the search finds it at its
    # lowest DM trial (smeared over the sweep of DM 50), the narrow-band burst at a low DM
    specs = {"burst": (int(0.8 / TSAMP) - 8, 16, 104.0, 4, 8),
             "impulse": (int(1.4 / TSAMP) - 100, 64, 50.0, 8, 8),
             "narrow": (int(0.3 / TSAMP) - 9, 64, 20.0, 4, 16)}
    out = {}
    for name, (sample, width, dm, f, nsub) in specs.items():
        cut = ref.burst_cube(vals, sample, width, dm, delays, 64, nsub, 32, tscrunch=f)
        cut.update(sample=sample, width=width, dm=float(np.float32(dm)), snr=0.0)
        out[name] = (cut, ref.burst_optimise(cut, header, delays, nfine=65))
    return vals, header, delays, out


def test_recovery_on_the_oracle():
    _, _, delays, out = recovery()
    cut, rec = out["burst"]
    print({k: rec[k] for k in ("opt_dm", "opt_width", "opt_sample", "snr", "snr_coarse", "snr_in", "snr_dm0", "frac_pos",
                               "coarse_dm", "opt_kf")})
    fine_step = (float(cut["dms"][16]) - float(cut["dms"][15])) / 32
    bin_dm = cut["tscrunch"] / float(delays[-1])  # the DM that sweeps one bin over the band
    assert abs(float(rec["dmf"][1]) - float(rec["dmf"][0]) - fine_step) < 1e-4
    assert abs(rec["opt_dm"] - R_DM) <= fine_step + bin_dm
    assert abs(cut["dm"] - R_DM) > fine_step + bin_dm and rec["opt_kf"] < 32  # it was off, and the search moved down
    assert rec["flags"] == 0 and rec["snr"] > rec["snr_dm0"] and rec["snr"] >= rec["snr_in"] > 10
    assert rec["frac_pos"] >= 0.9
    assert R_WIDTH / 2 <= rec["opt_width"] <= 2 * R_WIDTH
    # the refined arrival: the box holds the pulse's peak in the top channel
    assert rec["opt_sample"] - 4 <= 0.8 / TSAMP <= rec["opt_sample"] + rec["opt_width"] + 4


def test_a_zero_dm_impulse_peaks_at_dm_zero():
    _, _, _, out = recovery()
    cut, rec = out["impulse"]
    assert rec["flags"] == 0 and cut["dms"][0] == 0.0
    assert rec["snr_dm0"] >= rec["snr_in"] and rec["snr_dm0"] > 10
    assert rec["coarse_dm"] < cut["dm"] / 2


def test_a_narrow_band_burst_has_a_low_frac_pos():
    _, _, _, out = recovery()
    cut, rec = out["narrow"]
    assert rec["snr"] > 8
    # two of 16 subbands hold the burst; the others are positive or not by chance
    assert rec["frac_pos"] <= 0.75 and rec["band"].argmax() in (2, 3)
    assert out["burst"][1]["frac_pos"] - rec["frac_pos"] >= 0.25


def hand_record(seed=0, nw=3, ndm=4, nfine=3, nsub=5, ntime=8):
    rng = np.random.default_rng(seed)
    i32 = lambda *shape: rng.integers(-1000, 1000, shape).astype(np.int32)  # noqa: E731
    return {"sample": (1 << 33) + 7, "width": 12, "tscrunch": 6, "t0": -17, "dm": 12.25, "cand_snr": 9.5, "snr": 17.5,
            "snr_coarse": 16.25, "snr_in": 11.25, "snr_dm0": 3.0, "frac_pos": 0.875, "v": 2.5e6, "mbar_ds": -1.5,
            "opt_sample": -(1 << 35), "opt_dm": 13.5, "coarse_dm": 18.375, "opt_width": 24, "opt_kf": 2, "opt_bin": 5,
            "coarse_row": 3, "coarse_width": 6, "coarse_bin": 4, "flags": 0,
            "dms": np.linspace(0, 24.5, ndm).astype(np.float32), "dmf": np.linspace(11, 13.5, nfine).astype(np.float32),
            "mbar_dmt": rng.normal(size=ndm), "best_val": i32(2, nw), "best_idx": i32(2, nw),
            "curve": i32(nw, ndm + nfine), "curve_bin": i32(nw, ndm + nfine), "band": i32(nsub), "profile": i32(ntime)}


BOPT_HDR = {"ntime": 8, "nsub": 5, "ndm": 4, "nchans": 12, "nbits": 8, "nfine": 3, "nw": 3, "nsamps": (1 << 33) + 5,
            "tsamp": 64e-6, "fch1": 1510.0, "foff": -1.09, "fine_half_range": 1.25}


def test_bopt_file_roundtrip_and_layout(tmp_path):
    recs = [hand_record(1), dict(hand_record(2), flags=1, snr_dm0=0.0)]
    path = str(tmp_path / "a.bopt")
    write_bopt_file(path, BOPT_HDR, recs)
    assert not os.path.exists(path + ".tmp")
    raw = open(path, "rb").read()
    r0 = recs[0]
    hand = b"PSBOPT01" + struct.pack("<8I", 2, 8, 5, 4, 12, 8, 3, 3) + struct.pack("<Q", (1 << 33) + 5)
    hand += struct.pack("<4d", 64e-6, 1510.0, -1.09, 1.25)
    assert len(hand) == 80 and raw[:80] == hand
    body = struct.pack("<QIIqff", (1 << 33) + 7, 12, 6, -17, 12.25, 9.5)
    body += struct.pack("<7d", 17.5, 16.25, 11.25, 3.0, 0.875, 2.5e6, -1.5)
    body += struct.pack("<qff", -(1 << 35), 13.5, 18.375) + struct.pack("<8I", 24, 2, 5, 3, 6, 4, 0, 0)
    assert len(body) == 136
    for k, dt in (("dms", "<f4"), ("dmf", "<f4"), ("mbar_dmt", "<f8"), ("best_val", "<i4"), ("best_idx", "<i4"),
                  ("curve", "<i4"), ("curve_bin", "<i4"), ("band", "<i4"), ("profile", "<i4")):
        body += np.ascontiguousarray(r0[k], dtype=dt).tobytes()
    assert len(body) == 136 + 4 * 4 + 4 * 3 + 8 * 4 + 4 * (6 + 6 + 21 + 21 + 5 + 8)
    assert raw[80:80 + len(body)] == body and len(raw) == 80 + 2 * len(body)
    f = BurstOptFile(path)
    assert len(f) == 2 and f.header == dict(BOPT_HDR, ncand=2)
    for i, r in enumerate(recs):
        assert_same_record(f.candidate(i), r)
    with pytest.raises(IndexError):
        f.candidate(2)
    h = C.BoptFileHeader()
    for k, v in dict(BOPT_HDR, ncand=2).items():
        setattr(h, k, v)
    native = str(tmp_path / "b.bopt")
    C.write_bopt_file(native, h, recs)
    assert open(native, "rb").read() == raw and not os.path.exists(native + ".tmp")
    open(path, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        BurstOptFile(path)
    open(path, "wb").write(b"PSOPT001" + raw[8:])
    with pytest.raises(ValueError):
        BurstOptFile(path)


def test_dm_curve_panel_on_a_hand_built_record():
    rec = hand_record(3)
    rec.update(v=16.0, mbar_ds=1.0, mbar_dmt=np.array([0.0, 2.0, 0.0, 0.0]))
    rec["curve"] = np.zeros((3, 7), np.int32)
    rec["curve"][1, 1] = 100  # coarse row 1 at width 2
    rec["curve"][2, 6] = 60   # fine row 2 at width 4
    dms, coarse, dmf, fine = burst_dm_curve_panel(rec)
    assert dms.dtype == np.float64 and np.array_equal(dms, rec["dms"].astype(np.float64))
    assert np.array_equal(dmf, rec["dmf"].astype(np.float64)) and coarse.shape == (4,) and fine.shape == (3,)
    assert coarse[1] == pytest.approx((100 - 2 * 2.0) / np.sqrt(16.0 * 2)) and int(np.argmax(coarse)) == 1
    assert fine[2] == pytest.approx((60 - 4 * 1.0) / np.sqrt(16.0 * 4)) and int(np.argmax(fine)) == 2
    assert coarse[0] == 0.0 and fine[0] == pytest.approx(-1.0 / 4.0)  # width 1: (0 - 1) / sqrt(16)
    flat = burst_dm_curve_panel(dict(rec, v=0.0))
    assert not flat[1].any() and not flat[3].any()
    # on a real record the panel's maxima are the record's S/N
    _, _, _, out = recovery()
    r = out["burst"][1]
    _, coarse, _, fine = burst_dm_curve_panel(r)
    assert fine.max() == pytest.approx(r["snr"], rel=1e-12) and coarse.max() == pytest.approx(r["snr_coarse"], rel=1e-12)
    assert coarse[16] == pytest.approx(r["snr_in"], rel=1e-12) and coarse[0] == pytest.approx(r["snr_dm0"], rel=1e-12)


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_native_unit_tests():
    assert "passed" in run([os.path.join(REPO, "bin", "psoup_bopt_unit_tests")]).stdout


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_host_sanitizers(san):
    """A stand-alone host binary built with the sanitizer, run in the inherited environment."""
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_bopt_unit_tests")
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = run([os.path.join(REPO, "bin", f"psoup_bopt_unit_tests_{san}")], env=env)
    assert "passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
