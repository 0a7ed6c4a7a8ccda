"""cubeopt (csrc/include/psoup/cubeopt.hpp; an extension beyond the reference):
a search over DM, period-drift and acceleration-drift trials on fold cubes.

CPU: option parsing, the C++ host steps against the NumPy oracle (exact), the
refusals, identities of the oracle, recovery of a mis-folded pulsar on the
oracle (which fixes the signs of the three conversions), the result file
(Python and native writers byte-identical), the two plot panels, the plot tool
and the host unit tests with their sanitizer builds.  GPU: the kernel's integer
outputs must EQUAL the oracle's over a sweep of shapes, ties, batching,
validation, the recovery record and the two entry points."""
import functools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_CANDS, GOLDEN_XML, REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.outputs import FoldOptFile, write_cube_file, write_opt_file
from peasoup_amd.utils.plotting import CandidatePlotter, dm_curve_panel, p_pdot_panel

SEARCH_KEYS = ("best_val", "best_idx", "dmcurve", "ppd", "centre")


# ------------------------------------------------------------------- CPU ----
def test_opt_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_opt_cmdline(["cubeopt", "-i", "c.cubes"])
    assert ok and not exit_now and a.infilename == "c.cubes"
    assert (a.ndm, a.dm_half_range, a.np, a.p_step, a.npd, a.pd_step, a.limit) == (64, 0.0, 65, 1.0, 33, 1.0, 1000)
    assert not a.verbose and a.outfilename.endswith("_cubeopt.opt")
    assert len(a.outfilename) == len("2026-01-01-00:00_cubeopt.opt")
    ok, _, a = C.parse_opt_cmdline(["cubeopt", "-i", "y.cubes", "-o", "out.opt", "--ndm", "16", "--dm_half_range", "12.5",
                                    "--np", "17", "--p_step", "0.5", "--npd", "9", "--pd_step", "2", "--limit", "7",
                                    "-v"])
    assert ok and a.outfilename == "out.opt" and (a.ndm, a.dm_half_range, a.np, a.p_step) == (16, 12.5, 17, 0.5)
    assert (a.npd, a.pd_step, a.limit) == (9, 2.0, 7) and a.verbose
    ok, exit_now, _ = C.parse_opt_cmdline(["cubeopt", "-h"])
    assert ok and exit_now


@pytest.mark.parametrize("extra", [["--np", "64"], ["--np", "259"], ["--npd", "4"], ["--npd", "131"], ["--ndm", "0"],
                                   ["--ndm", "257"], ["--p_step", "-1"], ["--limit", "-1"]])
def test_opt_cmdline_errors(extra):
    assert not C.parse_opt_cmdline(["cubeopt", "-i", "c.cubes"] + extra)[0]
    assert not C.parse_opt_cmdline(["cubeopt"] + extra)[0]  # -i is required
    assert not C.parse_opt_cmdline(["cubeopt"])[0]


def _random_cube(nints, nsub, nbins, seed, dead=()):
    rng = np.random.default_rng(seed)
    hits = rng.integers(5, 60, (nints, nbins)).astype(np.int32)  # unequal hits
    nact = rng.integers(1, 9, nsub).astype(np.int32)
    nact[list(dead)] = 0
    rate = rng.integers(900, 1100, (nints, nsub, nbins)).astype(np.int64)
    rate[:, :, nbins // 3] += 300  # a pulse: Mtot is not 0 after the floor divisions
    sums = rate * hits[:, None, :] * nact[None, :, None] // 7
    return {"period": 0.0123 * (1 + seed), "dm": 55.5 + seed, "acc": -3.25 * seed, "nactive": nact, "hits": hits,
            "sums": sums}


def _geom(nints, nsub, nbins, nchans=64, n=1 << 16, tsamp=320e-6, fch1=1510.0, foff=-1.09):
    return C.CubeOptGeom(nints, nsub, nbins, nchans, n, tsamp, fch1, foff)


def _assert_same_search(got, exp):
    for k in SEARCH_KEYS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == np.int32 and g.shape == e.shape and np.array_equal(g, e), k


def _assert_same_record(got, exp):
    assert set(exp) <= set(got)
    for k, e in exp.items():
        if isinstance(e, np.ndarray):
            g = np.asarray(got[k])
            assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), k
        else:
            assert got[k] == e, (k, got[k], e)


HOST_CASES = [(3, 5, 16, 4, 5, 3, 1.0, 1.0, 0.0), (16, 8, 64, 6, 7, 5, 0.5, 0.5, 10.0), (2, 7, 50, 3, 3, 3, 2.0, 1.5, 0.0)]


@pytest.mark.parametrize("case", HOST_CASES)
def test_host_steps_equal_the_oracle(case):
    nints, nsub, nbins, ndm, np_, npd, p_step, pd_step, half = case
    cube = _random_cube(nints, nsub, nbins, seed=nints, dead=(1,))
    g, grid = _geom(nints, nsub, nbins), C.CubeOptGrid(ndm, half, np_, p_step, npd, pd_step)
    delays = np.asarray(C.generate_delay_table(64, 320e-6, 1510.0, -1.09), dtype=np.float32)
    got = C.cube_opt_prepare(0, g, grid, cube["period"], cube["dm"], cube["acc"], cube["nactive"], cube["hits"],
                             cube["sums"])
    exp = ref.cube_opt_prepare(cube["sums"], cube["hits"], cube["nactive"], ndm, np_, npd)
    assert got["d"].dtype == np.int32 and np.array_equal(got["d"], exp["d"])
    assert (got["mtot"], got["v2"], got["v"]) == (exp["mtot"], exp["v2"], exp["v"])
    assert exp["mtot"] != 0 and np.all(exp["d"][:, 1] == 0) and exp["d"].any()
    sh = C.cube_opt_shifts(g, grid, cube["period"], cube["dm"], [float(x) for x in delays])
    esh = ref.cube_opt_shifts(nints, nsub, nbins, 64, 320e-6, cube["period"], cube["dm"], delays, ndm, np_, npd, half,
                              p_step, pd_step)
    for k in ("dms", "sdm", "st"):
        assert sh[k].dtype == esh[k].dtype and np.array_equal(sh[k], esh[k]), k
    assert np.array_equal(esh["dms"], C.burst_dms(cube["dm"], ndm, half))
    assert esh["sdm"].min() >= 0 and esh["sdm"].max() < nbins and esh["sdm"].any()
    assert esh["st"].min() >= 0 and esh["st"].max() < nbins and not esh["st"][np_ // 2, npd // 2].any()
    found = ref.cube_opt_search(exp["d"], esh["sdm"], esh["st"])
    _assert_same_search(C.cube_opt_search_host(g, grid, exp["d"], esh["sdm"], esh["st"]), found)
    rec = C.cube_opt_finish(g, grid, cube["period"], cube["acc"], exp["d"], exp["mtot"], exp["v2"], esh["dms"],
                            esh["sdm"], esh["st"], found)
    _assert_same_record(rec, ref.cube_opt_finish(exp, esh, found, cube["period"], cube["acc"], 320e-6, 1 << 16,
                                                 p_step, pd_step))
    assert (rec["flags"] == 0) == (half == 0.0 and ndm % 2 == 0)


def test_refusals_name_the_candidate():
    g, grid = _geom(3, 5, 16), C.CubeOptGrid(4, 0.0, 5, 1.0, 3, 1.0)
    cube = _random_cube(3, 5, 16, seed=2)

    def both(c, geom=g, gr=grid):
        with pytest.raises(C.NativeError, match="candidate 4 "):
            C.cube_opt_prepare(4, geom, gr, c["period"], c["dm"], c["acc"], c["nactive"], c["hits"], c["sums"])
        with pytest.raises(ValueError, match="candidate 4 "):
            ref.cube_opt_prepare(c["sums"], c["hits"], c["nactive"], gr.ndm, gr.np, gr.npd, 4, c["period"])

    bad = dict(cube, hits=cube["hits"].copy())
    bad["hits"][1, 7] = 0
    both(bad)
    bad = dict(cube, sums=cube["sums"].copy())
    bad["sums"][0, 0, 0] = 1 << 40  # d does not fit int32
    both(bad)
    bad["sums"][0, 0, 0] = 1 << 61  # 2 sums Href does not fit 63 bits
    both(bad)
    bad = dict(cube, sums=cube["sums"] * 4000)  # max|d| nints nsub nbins / 2 >= 2^31
    both(bad)
    both(dict(cube, period=0.0))
    big = _random_cube(65, 1, 256, seed=3)  # nints * nbins > 16384
    both(big, _geom(65, 1, 256))
    wide = _random_cube(1, 1, 256, seed=4)  # 256 * 257 * 129 * 256 trial bins >= 2^31
    both(wide, _geom(1, 1, 256), C.CubeOptGrid(256, 0.0, 257, 1.0, 129, 1.0))


def _tables(nints, nsub, nbins, ndm, np_, npd, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, nbins, (ndm, nsub)).astype(np.int32),
            rng.integers(0, nbins, (np_, npd, nints)).astype(np.int32))


def test_oracle_identities():
    nints, nsub, nbins, ndm, np_, npd = 4, 3, 16, 4, 5, 3
    sdm, st = _tables(nints, nsub, nbins, ndm, np_, npd, seed=1)
    # a delta pulse rotated by the tables of one trial is found at exactly that trial and bin
    kd, kp, kpd, bin_ = 2, 3, 1, 11
    d = np.zeros((nints, nsub, nbins), dtype=np.int32)
    for i in range(nints):
        for s in range(nsub):
            d[i, s, (bin_ + st[kp, kpd, i] + sdm[kd, s]) % nbins] += 9
    f = ref.cube_opt_search(d, sdm, st)
    assert f["best_val"][0] == 9 * nints * nsub
    assert f["best_idx"][0] == ((kd * np_ + kp) * npd + kpd) * nbins + bin_
    assert f["dmcurve"][0, kd] == f["best_val"][0] and f["ppd"][0, kp, kpd] == f["best_val"][0]
    assert np.array_equal(ref.cube_opt_profile(d.astype(np.int64), sdm[kd], st[kp, kpd]),
                          np.eye(nbins, dtype=np.int64)[bin_] * 9 * nints * nsub)
    # wider boxes hold the pulse too, and first at the bin w - 1 before it
    for k in range(1, ref.cube_opt_nwidths(nbins)):
        assert f["best_val"][k] == f["best_val"][0]
    # an all-equal cube: every trial and bin ties, the smallest index wins
    f = ref.cube_opt_search(np.full((nints, nsub, nbins), 3, np.int32), sdm, st)
    assert np.array_equal(f["best_idx"], np.zeros(4, np.int32))
    assert np.array_equal(f["best_val"], 3 * nints * nsub * 2 ** np.arange(4))
    assert np.array_equal(f["centre"], f["best_val"])
    assert [ref.cube_opt_nwidths(n) for n in (2, 3, 4, 50, 64, 256)] == [1, 1, 2, 5, 6, 8]


# The recovery setup of test_foldcube.py (64 channels of 8 bits, n = 2^16, a pulsar at DM 200), folded at DM
# 180, at a period that drifts 3 bins over the fold and at an acceleration that bends it by 2 bins.
R_TSAMP = 320e-6
R_N = 1 << 16
R_PERIOD = R_N * R_TSAMP / 210.0
R_DM, R_FOLD_DM = 200.0, 180.0
R_NINTS, R_NSUB, R_NBINS = 16, 8, 64
R_GRID = dict(ndm=16, np_=17, npd=9)


@functools.lru_cache(maxsize=None)
def _recovery():
    hdr = synthetic.make_header(nchans=64, nbits=8, tsamp=R_TSAMP)
    delays = ref.delay_table(64, R_TSAMP, hdr["fch1"], hdr["foff"])
    nsamps = R_N + int(ref.dm_offsets([260.0], delays).max()) + 8
    vals = synthetic.generate(nsamps, hdr, [synthetic.PulsarSpec(period=R_PERIOD, dm=R_DM, duty=0.05, amplitude=1.0)],
                              seed=21)
    ts = float(np.float32(R_TSAMP))
    T = R_N * ts
    period = 1.0 / (1.0 / R_PERIOD + 3.0 / (R_NBINS * T))
    acc_step = 8 * ref.C_LIGHT * period / (R_NBINS * ts * ts * R_N * R_N)
    acc = float(np.float32(2.0 * acc_step))
    sums, hits, nact = ref.fold_cube(vals, ref.dm_offsets([R_FOLD_DM], delays)[0], period,
                                     ref.accel_factor(acc, R_TSAMP), R_TSAMP, R_N, R_NINTS, R_NSUB, R_NBINS)
    cand = {"period": period, "dm": R_FOLD_DM, "acc": acc, "sums": sums, "hits": hits, "nactive": nact}
    header = {"nints": R_NINTS, "nsub": R_NSUB, "nbins": R_NBINS, "nchans": 64, "nbits": 8, "fold_nsamps": R_N,
              "tsamp": R_TSAMP, "fch1": hdr["fch1"], "foff": hdr["foff"]}
    rec = ref.cube_optimise(cand, header, delays, **R_GRID)
    return cand, header, delays, rec, acc_step


def test_recovery_on_the_oracle():
    cand, header, _, rec, acc_step = _recovery()
    print({k: rec[k] for k in ("opt_dm", "opt_period", "opt_acc", "snr", "snr_in", "snr_dm0", "opt_width", "opt_kd",
                               "opt_kp", "opt_kpd")})
    dm_step = 2.0 * R_FOLD_DM / R_GRID["ndm"]
    T = R_N * float(np.float32(R_TSAMP))
    p_step = abs(1.0 / (1.0 / cand["period"] - 1.0 / (R_NBINS * T)) - cand["period"])
    assert abs(rec["opt_dm"] - R_DM) <= dm_step
    # the fold DM is itself within one step: the search must move off row ndm / 2, to the row nearest the truth
    assert rec["opt_kd"] == int(np.argmin(np.abs(rec["dms"].astype(np.float64) - R_DM))) != R_GRID["ndm"] // 2
    assert abs(rec["opt_period"] - R_PERIOD) <= p_step
    assert abs(rec["opt_acc"] - 0.0) <= acc_step  # the pulsar is not accelerated
    assert rec["snr"] > rec["snr_in"] and rec["snr"] > rec["snr_dm0"] and rec["flags"] == 0
    assert abs(cand["period"] - R_PERIOD) > 2 * p_step and abs(cand["acc"]) > 1.5 * acc_step  # it was off


def _hand_record(seed=0, nw=4, ndm=4, np_=5, npd=3, nbins=16):
    rng = np.random.default_rng(seed)
    i32 = lambda *shape: rng.integers(-1000, 1000, shape).astype(np.int32)  # noqa: E731
    return {"period": 0.123456789012345, "dm": 12.25, "acc": -3.5, "snr": 17.5, "snr_in": 11.25, "snr_dm0": 3.0,
            "opt_period": 0.1234, "opt_acc": -1.5, "opt_dm": 13.5, "opt_width": 4, "opt_bin": 9, "opt_kd": 3,
            "opt_kp": 1, "opt_kpd": 2, "flags": 0, "mtot": -(1 << 40), "v": 2.5e6,
            "dms": np.linspace(0, 24.5, ndm).astype(np.float32), "best_val": i32(nw), "best_idx": i32(nw),
            "centre": i32(nw), "dmcurve": i32(nw, ndm), "ppd": i32(nw, np_, npd), "profile": i32(nbins)}


OPT_HDR = {"nints": 3, "nsub": 5, "nbins": 16, "nchans": 12, "ndm": 4, "np": 5, "npd": 3, "nw": 4,
           "fold_nsamps": (1 << 33) + 5, "tsamp": 64e-6, "fch1": 1510.0, "foff": -1.09, "p_step": 0.5, "pd_step": 2.0,
           "dm_half_range": 12.5}


def test_opt_file_roundtrip_and_layout(tmp_path):
    recs = [_hand_record(1), dict(_hand_record(2), flags=1, snr_dm0=0.0)]
    path = str(tmp_path / "a.opt")
    write_opt_file(path, OPT_HDR, recs)
    assert not os.path.exists(path + ".tmp")
    raw = open(path, "rb").read()
    assert raw[0:8] == b"PSOPT001"
    assert struct.unpack_from("<10I", raw, 8) == (2, 3, 5, 16, 12, 4, 5, 3, 4, 0)
    assert struct.unpack_from("<Q", raw, 48) == ((1 << 33) + 5,)
    assert struct.unpack_from("<6d", raw, 56) == (64e-6, 1510.0, -1.09, 0.5, 2.0, 12.5)
    assert struct.unpack_from("<dff", raw, 104) == (0.123456789012345, 12.25, -3.5)
    assert struct.unpack_from("<5d", raw, 120) == (17.5, 11.25, 3.0, 0.1234, -1.5)
    assert struct.unpack_from("<f7I", raw, 160) == (13.5, 4, 9, 3, 1, 2, 0, 0)
    assert struct.unpack_from("<qd", raw, 192) == (-(1 << 40), 2.5e6)
    assert struct.unpack_from("<4f", raw, 208) == tuple(float(x) for x in recs[0]["dms"])
    rec = 104 + 4 * (4 + 3 * 4 + 4 * 4 + 4 * 15 + 16)
    assert len(raw) == 104 + 2 * rec
    f = FoldOptFile(path)
    assert len(f) == 2 and f.header == dict(OPT_HDR, ncand=2)
    for i, r in enumerate(recs):
        _assert_same_record(f.candidate(i), r)
    with pytest.raises(IndexError):
        f.candidate(2)
    h = C.OptFileHeader()
    for k, v in dict(OPT_HDR, ncand=2).items():
        setattr(h, k, v)
    native = str(tmp_path / "b.opt")
    C.write_opt_file(native, h, recs)
    assert open(native, "rb").read() == raw and not os.path.exists(native + ".tmp")
    open(path, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        FoldOptFile(path)


def _panel_record():
    """4 widths x 4 DM rows x (5 x 3) trials over 16 bins: the S/N peaks at DM row 3 and trial (1, 2) at width 2."""
    rec = _hand_record(3)
    rec.update(mtot=0, v=16.0)
    rec["dmcurve"] = np.zeros((4, 4), np.int32)
    rec["dmcurve"][1, 3] = 100
    rec["ppd"] = np.zeros((4, 5, 3), np.int32)
    rec["ppd"][1, 1, 2] = 100
    return rec


def test_panels_on_a_hand_built_record():
    rec = _panel_record()
    dms, snr = dm_curve_panel(rec)
    assert dms.dtype == np.float64 and np.array_equal(dms, rec["dms"].astype(np.float64))
    assert snr.shape == (4,) and int(np.argmax(snr)) == 3
    assert snr[3] == pytest.approx(100.0 / np.sqrt(16.0 * 2 * (1 - 2 / 16))) and np.all(snr[:3] == 0)
    pp = p_pdot_panel(rec)
    assert pp.shape == (3, 5) and np.unravel_index(np.argmax(pp), pp.shape) == (2, 1)
    assert pp[2, 1] == pytest.approx(snr[3]) and np.count_nonzero(pp) == 1
    assert np.all(p_pdot_panel(dict(rec, v=0.0)) == 0)


def test_plot_tool_with_opt(tmp_path):
    shutil.copy(GOLDEN_XML, tmp_path / "overview.xml")
    shutil.copy(GOLDEN_CANDS, tmp_path / "candidates.peasoup")
    rec = _panel_record()
    opt = str(tmp_path / "c.opt")
    write_opt_file(opt, OPT_HDR, [rec, rec])
    cube = _random_cube(3, 5, 16, seed=1)
    cubes = str(tmp_path / "c.cubes")
    write_cube_file(cubes, {k: OPT_HDR[k] for k in ("nints", "nsub", "nbins", "nchans", "fold_nsamps", "tsamp", "fch1",
                                                    "foff")} | {"nbits": 8}, [cube, cube])
    pl = CandidatePlotter(str(tmp_path), cubes=cubes, opt=opt)
    pl._plt = None
    with np.load(pl.plot_cand(1, str(tmp_path / "with.npz"))) as z:
        assert np.array_equal(z["opt_dm_snr"], dm_curve_panel(rec)[1])
        assert np.array_equal(z["opt_p_pdot"], p_pdot_panel(rec)) and "freq_phase" in z.files
        with_keys = set(z.files)
    plain = CandidatePlotter(str(tmp_path), cubes=cubes)
    plain._plt = None
    with np.load(plain.plot_cand(1, str(tmp_path / "without.npz"))) as z:
        assert with_keys - set(z.files) == {"opt_dms", "opt_dm_snr", "opt_p_pdot"}
    out = str(tmp_path / "cand1.png")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "peasoup_plot_cand.py"), str(tmp_path), "1",
                        "--cubes", cubes, "--opt", opt, "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    written = r.stdout.strip().splitlines()[-1]
    assert os.path.getsize(written) > 0
    if written.endswith(".npz"):
        with np.load(written) as z:
            assert "opt_p_pdot" in z.files and "time_phase" in z.files


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_native_unit_tests():
    assert "passed" in _run([os.path.join(REPO, "bin", "psoup_opt_unit_tests")]).stdout


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_host_sanitizers(san):
    """A stand-alone host binary built with the sanitizer, run in the inherited environment."""
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_opt_unit_tests")
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = _run([os.path.join(REPO, "bin", f"psoup_opt_unit_tests_{san}")], env=env)
    assert "passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------- GPU ----
# nints, nsub, nbins, ndm, np, npd
SHAPES = [(1, 1, 2, 1, 1, 1), (3, 7, 50, 5, 3, 3), (16, 8, 64, 4, 5, 3), (5, 3, 256, 2, 3, 1), (64, 2, 256, 1, 3, 3),
          (16, 32, 64, 3, 7, 5)]


@functools.lru_cache(maxsize=None)
def _shape_case(i):
    nints, nsub, nbins, ndm, np_, npd = SHAPES[i]
    rng = np.random.default_rng(40 + i)
    d = rng.integers(-5000, 5000, (nints, nsub, nbins)).astype(np.int32)
    d.flat[0], d.flat[-1] = -1234, 4321  # both signs, in the two-element cube too
    sdm, st = _tables(nints, nsub, nbins, ndm, np_, npd, seed=50 + i)
    return d, sdm, st, ref.cube_opt_search(d, sdm, st)


def _gpu_search(d, sdm, st, **kw):
    import torch

    from peasoup_amd import ops

    out = ops.cube_search(torch.from_numpy(np.ascontiguousarray(d)), torch.from_numpy(np.ascontiguousarray(sdm)),
                          torch.from_numpy(np.ascontiguousarray(st)), **kw)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in out)
    return dict(zip(SEARCH_KEYS, out))


def _assert_gpu_equals(got, exp, cand=0):
    for k in SEARCH_KEYS:
        g = got[k][cand].cpu().numpy()
        assert g.shape == exp[k].shape and np.array_equal(g, exp[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_cube_search_equals_oracle(i):
    import torch

    d, sdm, st, exp = _shape_case(i)
    assert d.min() < 0 < d.max()
    got = _gpu_search(d[None], sdm[None], st[None])
    _assert_gpu_equals(got, exp)
    again = _gpu_search(d[None], sdm[None], st[None])
    assert all(torch.equal(got[k], again[k]) for k in SEARCH_KEYS)


@pytest.mark.gpu
def test_ties_go_to_the_smaller_index():
    nints, nsub, nbins, ndm, np_, npd = 3, 2, 50, 3, 5, 3
    sdm, st = _tables(nints, nsub, nbins, ndm, np_, npd, seed=7)
    zero = np.zeros((nints, nsub, nbins), np.int32)
    got = _gpu_search(zero[None], sdm[None], st[None])
    assert not got["best_idx"].any() and not got["best_val"].any()
    # one positive sample: every trial reaches the same maximum, at a bin of its own
    one = zero.copy()
    one[1, 1, 17] = 5
    exp = ref.cube_opt_search(one, sdm, st)
    assert exp["best_val"][0] == 5 and (exp["ppd"][0] == 5).all()
    _assert_gpu_equals(_gpu_search(one[None], sdm[None], st[None]), exp)
    # two equal maxima planted at two different trials
    two = zero.copy()
    for kd, kp, kpd, b in ((2, 1, 0, 40), (1, 4, 2, 3)):
        for i in range(nints):
            for s in range(nsub):
                two[i, s, (b + st[kp, kpd, i] + sdm[kd, s]) % nbins] += 7
    exp = ref.cube_opt_search(two, sdm, st)
    got = _gpu_search(two[None], sdm[None], st[None])
    _assert_gpu_equals(got, exp)
    assert int(got["best_idx"][0, 0]) <= ((1 * np_ + 4) * npd + 2) * nbins + 3


@pytest.mark.gpu
def test_batch_equals_one_at_a_time_and_keeps_order():
    nints, nsub, nbins, ndm, np_, npd = 16, 8, 64, 4, 5, 3
    rng = np.random.default_rng(9)
    d = rng.integers(-3000, 3000, (5, nints, nsub, nbins)).astype(np.int32)
    tabs = [_tables(nints, nsub, nbins, ndm, np_, npd, seed=60 + c) for c in range(5)]
    sdm, st = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    exp = [ref.cube_opt_search(d[c], sdm[c], st[c]) for c in range(5)]
    both = _gpu_search(d, sdm, st)
    for c in range(5):
        _assert_gpu_equals(both, exp[c], c)
        _assert_gpu_equals(_gpu_search(d[c:c + 1], sdm[c:c + 1], st[c:c + 1]), exp[c])
    # a budget of two candidates: three launches, input order kept
    g, grid = C.CubeOptGeom(nints, nsub, nbins), C.CubeOptGrid(ndm, 0.0, np_, 1.0, npd, 1.0)
    per = C.CubeOptimiser(g, grid).bytes_per_candidate
    opt = C.CubeOptimiser(g, grid, 0, 2 * per + 8)
    assert opt.batch_size == 2
    res = opt.search(d, sdm, st)
    assert opt.batches == 3 and len(res) == 5
    for c in range(5):
        _assert_same_search(res[c], exp[c])


@pytest.mark.gpu
def test_bad_candidates_are_named_and_nothing_is_launched():
    cand, header, delays, _, _ = _recovery()
    g = _geom(R_NINTS, R_NSUB, R_NBINS, 64, R_N, R_TSAMP, header["fch1"], header["foff"])
    opt = C.CubeOptimiser(g, C.CubeOptGrid(4, 0.0, 5, 1.0, 3, 1.0))
    good = dict(cand)
    zero_hit = dict(cand, hits=cand["hits"].copy())
    zero_hit["hits"][3, 3] = 0
    for bad in (zero_hit, dict(cand, period=-1.0), dict(cand, sums=cand["sums"] * 100000)):
        with pytest.raises(C.NativeError, match="candidate 2 "):
            opt.optimise([good, good, bad], [float(x) for x in delays])
    sdm, st = _tables(R_NINTS, R_NSUB, R_NBINS, 4, 5, 3, seed=1)
    d = np.zeros((2, R_NINTS, R_NSUB, R_NBINS), np.int32)
    st2 = np.stack([st, st])
    st2[1, 2, 1, 5] = R_NBINS  # one shift outside [0, nbins)
    with pytest.raises(C.NativeError, match="candidate 1 "):
        opt.search(d, np.stack([sdm, sdm]), st2)
    assert opt.batches == 0
    import torch

    from peasoup_amd import ops

    with pytest.raises(ValueError, match="candidate 1 "):
        ops.cube_search(torch.from_numpy(d), torch.from_numpy(np.stack([sdm, sdm])), torch.from_numpy(st2))


@pytest.mark.gpu
def test_recovery_on_the_device():
    from peasoup_amd import ops

    cand, header, delays, rec, _ = _recovery()
    got = ops.cube_optimise([cand], header, delays=delays, **R_GRID)
    assert len(got) == 1
    _assert_same_record(got[0], rec)


@pytest.mark.gpu
def test_cli_and_module_write_identical_files(tmp_path):
    fil = os.path.join(REPO, "tests", "data", "tutorial.fil")
    candf = tmp_path / "cands.txt"
    candf.write_text("0.25 30.0 0.0\n0.125 28.5 1.5\n")
    cubes = str(tmp_path / "t.cubes")
    _run([os.path.join(REPO, "bin", "foldcube"), "-i", fil, "--candfile", str(candf), "-o", cubes, "--nsub", "8"])
    flags = ["-i", cubes, "--ndm", "8", "--np", "9", "--npd", "5", "--p_step", "0.5"]
    a, b = str(tmp_path / "native.opt"), str(tmp_path / "module.opt")
    r = _run([os.path.join(REPO, "bin", "cubeopt")] + flags + ["-o", a, "-v"])
    assert len([ln for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]) == 2
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "opt"] + flags + ["-o", b], env=env, cwd=REPO)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = FoldOptFile(a)
    src = C.read_cube_file(cubes)
    geom = src["geom"]
    assert len(f) == 2 and (f.header["ndm"], f.header["np"], f.header["npd"], f.header["p_step"]) == (8, 9, 5, 0.5)
    header = {"nchans": geom.nchans, "tsamp": geom.tsamp, "fold_nsamps": geom.fold_nsamps}
    delays = np.asarray(C.generate_delay_table(geom.nchans, geom.tsamp, geom.fch1, geom.foff), dtype=np.float32)
    for i, c in enumerate(src["candidates"]):
        _assert_same_record(f.candidate(i), ref.cube_optimise(c, header, delays, 8, 9, 5, p_step=0.5))
    assert len(C.read_cube_file(cubes, 1)["candidates"]) == 1
