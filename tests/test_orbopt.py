"""orbopt without a GPU: the native host transcriptions against the NumPy oracle
(fold, hits, moments, drift table, search, finish) on orbopt_cases, the grid (its
defaults, the collapse at a1 = 0, the sign fold, the centre), the writer's bytes
and the reader, every refusal by name, the command line, the CMake lists and the
native host unit tests."""
import os
import re
import subprocess

import numpy as np
import pytest

import orbopt_cases as cc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import outputs, plotting
from peasoup_amd.utils import reference as ref

TS = cc.TS


# ------------------------------------------------------ fold, hits, search ----
@pytest.mark.parametrize("n,pad", cc.SHAPES)
def test_host_fold_and_hits_equal_oracle(n, pad):
    """The host transcription against the oracle.  At 17 samples every (nints, nbins) runs all 60 templates; at 4101
    every (nints, nbins) runs one template group in turn; at 65539 only the four corner (nints, nbins) run, one group
    each.  The cut only shortens CPU time (the transcription evaluates every shift again, 65539 x K per call):
    test_orbopt_gpu.py runs every combination with every template on the kernel."""
    x, tpl, y = cc.shape_case(n, pad)
    groups = cc.group_bounds(len(tpl))
    # the long shape takes the four corner combinations only: the host transcription evaluates every shift again
    combos = cc.combos(n) if n < 60000 else [cc.combos(n)[i] for i in (0, 3, 8, 11)]
    for ci, (nints, nbins, Gs) in enumerate(combos):
        k0, k1 = groups[ci % len(groups)] if n > 4000 else (0, len(tpl))
        want = cc.want_fold(y, k0, k1, n, Gs, nints, nbins)
        for c in range(3):
            got = C.orbopt_fold_host(x[c], n, Gs[c], tpl[k0:k1], nints, nbins)
            assert got.dtype == np.int32 and got.shape == (k1 - k0, nints, nbins)
            np.testing.assert_array_equal(got, want[c], err_msg=f"nints {nints} nbins {nbins} row {c}")
            hits = C.oopt_hits(Gs[c], n, nints, nbins)
            np.testing.assert_array_equal(hits, ref.orbopt_hits(n, Gs[c], nints, nbins))
            assert hits.sum() == n and got.astype(np.int64).sum() == y[c, k0:k1].astype(np.int64).sum()
    # the oracle's own fold is the plain fold of its resampled rows
    nints, nbins, Gs = cc.combos(n)[5]
    np.testing.assert_array_equal(ref.orbopt_fold(x[1], n, Gs[1], tpl[:7], nints, nbins),
                                  cc.want_fold(y, 0, 7, n, Gs, nints, nbins)[1])
    np.testing.assert_array_equal(ref.orbopt_fold_plain(y[1, 3], n, Gs[1], nints, nbins),
                                  cc.want_fold(y, 3, 4, n, Gs, nints, nbins)[1, 0])
    if n == 17:  # 16 subints over 17 samples: one holds two samples; over 5 samples most are empty
        assert (C.oopt_hits(Gs[0], 17, 16, 2).sum(axis=1) > 0).all()
        assert (C.oopt_hits(Gs[0], 5, 16, 2).sum(axis=1) == 0).sum() == 11


def test_moments_and_drift_table_equal_oracle():
    rng = np.random.default_rng(2)
    for n in (1, 17, 4101):
        x = rng.integers(0, 256, n + 5, dtype=np.uint8)
        assert tuple(C.oopt_moments(0, x, n)) == ref.orbopt_moments(x, n)
    big = np.full(1 << 24, 128, dtype=np.uint8)
    with pytest.raises(RuntimeError, match=r"candidate 4: max\(m, 255 - m\) \* n >= 2\^31"):
        C.oopt_moments(4, big, 1 << 24)
    with pytest.raises(ValueError, match=r"candidate 4: max\(m, 255 - m\) \* n >= 2\^31"):
        ref.orbopt_moments(big, 1 << 24, 4)
    assert tuple(C.oopt_moments(0, big, (1 << 24) - 1)) == ref.orbopt_moments(big, (1 << 24) - 1)
    for nints, nbins, np_, step in ((16, 64, 33, 1.0), (3, 7, 5, 0.5), (64, 256, 257, 1.0), (1, 2, 1, 1.0), (4, 16, 9, 3.7)):
        p = C.OrbOptParams(nbins=nbins, nints=nints, np=np_, p_step=step)
        st = C.oopt_drift_table(p)
        np.testing.assert_array_equal(st, ref.orbopt_drift_table(nints, nbins, np_, step))
        assert st.min() >= 0 and st.max() < nbins and not st[np_ // 2].any()


SEARCH_CASES = [("bound", 3, 4, 16, 5), ("equal", 3, 4, 16, 5), ("bound", 5, 3, 7, 9), ("equal", 2, 1, 2, 1),
                ("bound", 2, 16, 64, 33)]


@pytest.mark.parametrize("kind,K,nints,nbins,np_", SEARCH_CASES)
def test_host_search_and_finish_equal_oracle(kind, K, nints, nbins, np_):
    fold, hits, m = cc.search_planes(kind, K, nints, nbins, seed=K + nbins)
    st = ref.orbopt_drift_table(nints, nbins, np_, 1.0)
    want = ref.orbopt_search(fold, hits, m, st)
    got = C.orbopt_search_host(fold, hits, m, st)
    for key in ("best_val", "best_idx", "centre", "tcurve", "msum"):
        assert got[key].dtype == want[key].dtype
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    if kind == "equal":
        assert not got["best_idx"].any()
    else:
        wmax = 1 << (len(got["best_val"]) - 1)
        assert got["best_val"][-1] == ((2 ** 31 - 1) // (nints * wmax)) * nints * wmax > 2 ** 30


def test_finish_equals_oracle():
    """The whole chain on a short row: the native host steps, put together here, against reference.orbit_optimise."""
    n = 4101
    x = cc.shape_case(4101, 37)[0][0]
    for k, cand in enumerate([(64.3 * TS, 12.5, 0.0, 1500 * TS, 3.0 * TS, 0.37), (20.7 * TS, 3.0, 1.0e6, 900 * TS, 0.0, 0.6),
                              (64.3 * TS, 12.5, 0.0, 1500 * TS, 0.2 * TS, 0.9)]):
        kw = dict(nbins=16, nints=4, npb=3, na1=5, nphase=3, np_=5)
        want = ref.orbit_optimise(x, cand, n, TS, k=k, **kw)
        p = C.OrbOptParams(nbins=16, nints=4, npb=3, na1=5, nphase=3, np=5)
        g = C.oopt_grid(k, p, cand, n, TS)
        m, v1 = C.oopt_moments(k, x, n)
        hits = C.oopt_hits(g["G"], n, 4, 16)
        fold = C.orbopt_fold_host(x, n, g["G"], g["quant"], 4, 16)
        found = C.orbopt_search_host(fold, hits, m, C.oopt_drift_table(p))
        got = C.oopt_finish(p, cand, n, TS, m, v1, hits, found, fold[int(want["opt_k"])])
        cc_compare(got, want)
        assert got["flags"] & 2 == (2 if k == 1 else 0)


def cc_compare(got, want):
    """Field by field: the scalars bit for bit, the arrays element for element."""
    for key in ("period", "dm", "acc", "pb", "a1", "phase", "npb", "na1", "nphase", "dpb", "da1", "dph", "snr", "snr_in",
                "opt_period", "opt_pb", "opt_a1", "opt_phase", "opt_width", "opt_bin", "opt_k", "opt_l", "flags", "m", "v1"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("best_val", "best_idx", "centre", "tcurve", "msum", "hits", "fold", "profile"):
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg=key)


# -------------------------------------------------------------------- grid ----
def test_grid_defaults_collapse_sign_fold_and_centre():
    n, P = 1 << 17, 0.0101
    cand = (P, 20.0, 0.0, 63.0, 0.0088, 0.72)
    p = C.OrbOptParams()
    g, w = C.oopt_grid(0, p, cand, n, TS), ref.orbopt_grid(cand, n, TS)
    for key in ("npb", "na1", "nphase", "dpb", "da1", "dph", "G", "templates", "quant"):
        assert g[key] == w[key], key
    T = n * TS
    assert g["da1"] == P / (2.0 * 64) and g["dph"] == min(1 / 16, P / ((4 * np.pi) * 0.0088 * 64))
    assert g["dpb"] == min(63.0 / 16, (63.0 * 63.0 * P) / ((4 * np.pi) * 0.0088 * T * 64))
    assert len(g["templates"]) == 729 and g["templates"][729 // 2] == (63.0, 0.0088, 0.72)
    assert g["quant"][364] == ref.orbit_quantise(63.0, 0.0088, 0.72, TS)
    assert g["templates"][365] == (63.0, 0.0088, 0.72 + g["dph"]) and g["templates"][364 + 81][0] == 63.0 + g["dpb"]
    # each default step moves a pulse by about half a bin: a1 by da1 shifts the delay by at most 2 da1 = P / nbins
    assert abs(2 * g["da1"] / (P / 64) - 1) < 1e-12
    # user steps
    pu = C.OrbOptParams(pb_step=0.5, a1_step=1e-4, phase_step=0.01, npb=3, na1=3, nphase=3)
    gu = C.oopt_grid(0, pu, cand, n, TS)
    assert (gu["dpb"], gu["da1"], gu["dph"]) == (0.5, 1e-4, 0.01) and gu["templates"][13] == (63.0, 0.0088, 0.72)
    assert gu == ref.orbopt_grid(cand, n, TS, 64, 3, 3, 3, 0.5, 1e-4, 0.01)
    # a1 = 0: one pb and one phase
    z = C.oopt_grid(0, p, (P, 20.0, 0.0, 63.0, 0.0, 0.25), n, TS)
    assert (z["npb"], z["na1"], z["nphase"], z["dpb"], z["dph"]) == (1, 9, 1, 0.0, 0.0) and len(z["templates"]) == 9
    assert z == ref.orbopt_grid((P, 20.0, 0.0, 63.0, 0.0, 0.25), n, TS) and z["templates"][4] == (63.0, 0.0, 0.25)
    # the sign fold: the lower half of the a1 axis is |a1| at ph + 0.5 ...
    assert z["templates"][3] == (63.0, z["da1"], 0.75) and z["templates"][5] == (63.0, z["da1"], 0.25)
    # ... which is the same delay: a1 = -x at ph and x at ph + 0.5 give identical planes
    x = cc.shape_case(4101, 37)[0][2]
    pb, a = 1500 * TS, 7.3 * TS
    neg = C.oopt_grid(0, C.OrbOptParams(npb=1, na1=1, nphase=1), (64.3 * TS, 0.0, 0.0, pb, -a, 0.2), 4101, TS)
    pos = C.oopt_grid(0, C.OrbOptParams(npb=1, na1=1, nphase=1), (64.3 * TS, 0.0, 0.0, pb, a, 0.7), 4101, TS)
    assert neg["templates"] == pos["templates"] == [(pb, a, 0.7)] and neg["quant"] == pos["quant"]
    planes = [C.orbopt_fold_host(x, 4101, g2["G"], g2["quant"], 3, 16) for g2 in (neg, pos)]
    np.testing.assert_array_equal(planes[0], planes[1])
    s = ref.orbit_shift(4101, pos["quant"][0])
    i = np.arange(4101) * TS
    want = -7.3 * (np.sin(2 * np.pi * (i / pb + 0.2)) - np.sin(2 * np.pi * 0.2))   # the delay of a1 = -a at ph = 0.2
    assert np.max(np.abs(s - want)) < 0.5 + 1e-2


def test_recovery_figures_of_the_cpu_oracle():
    """The two S/N the GPU recovery test's midpoint rule is built on, from the CPU oracle alone: at the injected
    template and at the off-grid starting one (1 x 1 x 1 grids, 33 drift trials)."""
    row, n = cc.recovery_row()
    one = dict(npb=1, na1=1, nphase=1)
    truth = ref.orbit_optimise(row, (cc.P0, cc.DM0, 0.0) + cc.TRUTH, n, TS, **one)
    start = ref.orbit_optimise(row, (cc.P0, cc.DM0, 0.0) + cc.START, n, TS, **one)
    print(f"n {n}: S/N at the injected template {truth['snr']!r}, at the starting template {start['snr']!r}")
    assert abs(truth["snr"] / cc.SNR_TRUTH - 1) < 1e-9 and abs(start["snr"] / cc.SNR_START - 1) < 1e-9
    assert truth["snr"] > 3 * start["snr"] and truth["flags"] == start["flags"] == 0


# --------------------------------------------------------- writer, reader ----
def _records():
    n = 4101
    x = cc.shape_case(4101, 37)[0][1]
    kw = dict(nbins=16, nints=4, npb=3, na1=3, nphase=3, np_=5)
    recs = [ref.orbit_optimise(x, (64.3 * TS, 12.5, 0.5, 1500 * TS, 3.0 * TS, 0.37), n, TS, **kw),
            ref.orbit_optimise(x, (20.7 * TS, 3.0, 0.0, 900 * TS, 0.0, 0.6), n, TS, **kw)]
    header = dict(nints=4, nbins=16, npb=3, na1=3, nphase=3, np=5, nw=ref.cube_opt_nwidths(16), n=n, tsamp=TS, p_step=1.0)
    return header, recs


def test_writer_bytes_and_reader_round_trip(tmp_path):
    header, recs = _records()
    assert (recs[0]["npb"], recs[0]["nphase"]) == (3, 3) and (recs[1]["npb"], recs[1]["nphase"]) == (1, 1)
    a, b = str(tmp_path / "py.oopt"), str(tmp_path / "native.oopt")
    outputs.write_orbopt_file(a, header, recs)
    C.write_orbopt_file(b, header, recs)
    with open(a, "rb") as f, open(b, "rb") as g:
        ba, bb = f.read(), g.read()
    assert ba == bb and ba[:8] == b"PSOOPT01" and not os.path.exists(a + ".tmp") and not os.path.exists(b + ".tmp")
    nw = header["nw"]
    assert len(ba) == 64 + sum(160 + 4 * (3 * nw + nw * K) + 8 * K + 4 * (64 + 64 + 16) for K in (27, 3))
    f = outputs.OrbOptFile(a)
    assert len(f) == 2 and f.header == dict(header, ncand=2)
    for i, r in enumerate(recs):
        cc_compare(f.candidate(i), r)
    with open(a, "wb") as g:
        g.write(ba[:-3])
    with pytest.raises(ValueError, match="truncated"):
        outputs.OrbOptFile(a)
    with pytest.raises(RuntimeError, match="wrong shape"):
        C.write_orbopt_file(b, header, [dict(recs[0], profile=recs[0]["profile"][:5])])
    with pytest.raises(ValueError, match="wrong shape"):
        outputs.write_orbopt_file(a, header, [dict(recs[0], profile=recs[0]["profile"][:5])])
    slices = plotting.orbit_surface_panel(recs[0])
    assert slices[0].shape == (3, 3) and slices[1].shape == (3, 3)
    k = recs[0]["opt_k"]
    assert slices[0][(k // 3) % 3, k // 9] == slices[1][(k // 3) % 3, k % 3] == max(slices[0].max(), slices[1].max())
    assert abs(slices[0].max() - recs[0]["snr"]) < 1e-9
    assert C.oopt_verbose_line(recs[0]).split()[-1] == str(recs[0]["flags"])


# ----------------------------------------------------------------- refusals ----
def _args(fil, cand, extra):
    ok, _, a = C.parse_oopt_cmdline(["orbopt", "-i", fil, "-c", cand] + [str(e) for e in extra])
    assert ok
    return a


def test_every_refusal_is_raised_by_name(tmp_path):
    """The module's driver refuses before it touches a device, so this runs without one; the binary's side is in
    test_orbopt_gpu.py on the same cases."""
    from peasoup_amd.models.orbopt import run_orbit_optimise

    fil, _ = cc.small_file(tmp_path)
    for i, (text, extra, what) in enumerate(cc.refusal_cases(tmp_path)):
        cand = str(tmp_path / f"c{i}.txt")
        if text is not None:
            with open(cand, "w") as f:
                f.write(text)
        with pytest.raises(RuntimeError, match=re.escape(what)):
            run_orbit_optimise(_args(fil, cand, extra + ["-o", str(tmp_path / "never.oopt")]))
    assert not os.path.exists(str(tmp_path / "never.oopt"))
    a = _args(fil, str(tmp_path / "c0.txt"), [])
    a.max_num_threads = 2
    with pytest.raises(RuntimeError, match="one device"):
        run_orbit_optimise(a)
    # n > 2^26, from the header alone
    import orbit_cases as oc

    with open(str(tmp_path / "good.txt"), "w") as f:
        f.write("0.0123 0 0 40 0.004 0.3\n")
    with pytest.raises(RuntimeError, match="longer than 2\\^26"):
        run_orbit_optimise(_args(oc.big_file(tmp_path), str(tmp_path / "good.txt"), ["--fft_size", 1 << 27]))
    # the oracle refuses the same things
    for cand, what in (((1e-4, 1.0, 0.0, 40.0, 0.004, 0.3), "below 2 tsamp"), ((0.01, -1.0, 0.0, 40.0, 0.004, 0.3), "negative DM"),
                       ((0.01, 1.0, 0.0, 0.01, 0.004, 0.3), "pb < 64 tsamp"), ((0.01, 1.0, 0.0, 100.0, 20.0, 0.0), "0.9 samples")):
        with pytest.raises(ValueError, match=what):
            ref.orbopt_grid(cand, 4096, TS, k=3)
    with pytest.raises(ValueError, match="an even count"):
        ref.orbopt_check_params(npb=2)
    assert ref.orbopt_parse_candidates(cc.CAND_TEXT) == C.oopt_parse_candidates(cc.CAND_TEXT)
    assert C.oopt_dm_list(C.oopt_parse_candidates(cc.CAND_TEXT)) == [3.0, 12.5]
    with pytest.raises(ValueError, match="candidate line 3 is malformed"):
        ref.orbopt_parse_candidates("# c\n\n1 2 3 4 5\n")


# ---------------------------------------------------------------------- CLI ----
def test_cli_parsing():
    ok, exit_now, a = C.parse_oopt_cmdline(["orbopt", "-i", "x.fil", "-c", "c.txt"])
    assert ok and not exit_now
    assert (a.nbins, a.nints, a.npb, a.na1, a.nphase, a.np, a.p_step, a.limit, a.size) == (64, 16, 9, 9, 9, 33, 1.0, 100, 0)
    assert (a.pb_step, a.a1_step, a.phase_step, a.verbose, a.max_num_threads) == (0.0, 0.0, 0.0, False, 1)
    assert re.fullmatch(r"\d{4}-\d\d-\d\d-\d\d:\d\d_orbopt\.oopt", a.outfilename)
    ok, _, b = C.parse_oopt_cmdline(["orbopt", "-i", "x.fil", "-c", "c.txt", "-o", "o", "-k", "k", "--nbins", "7", "--nints",
                                     "3", "--npb", "5", "--na1", "3", "--nphase", "1", "--np", "17", "--p_step", "0.5",
                                     "--pb_step", "0.25", "--a1_step", "1e-4", "--phase_step=0.01", "--limit", "4",
                                     "--fft_size", "65536", "-v"])
    assert ok and (b.outfilename, b.killfilename, b.nbins, b.nints, b.npb, b.na1, b.nphase, b.np) == ("o", "k", 7, 3, 5, 3, 1, 17)
    assert (b.p_step, b.pb_step, b.a1_step, b.phase_step, b.limit, b.size, b.verbose) == (0.5, 0.25, 1e-4, 0.01, 4, 65536, True)
    p = C.oopt_params_of(b)
    assert (p.nbins, p.nints, p.npb, p.np, p.pb_step) == (7, 3, 5, 17, 0.25)
    assert not C.parse_oopt_cmdline(["orbopt", "-i", "x.fil"])[0]
    assert not C.parse_oopt_cmdline(["orbopt", "-i", "x.fil", "-c", "c", "-t", "2"])[0]      # one device
    assert not C.parse_oopt_cmdline(["orbopt", "-i", "x.fil", "-c", "c", "--limit", "-1"])[0]
    assert not C.parse_oopt_cmdline(["orbopt", "-i", "x.fil", "-c", "c", "--p_step", "1x"])[0]
    assert C.parse_oopt_cmdline(["orbopt", "--help"])[1]


def test_numerics_id_does_not_depend_on_the_orbopt_sources():
    with open(os.path.join(REPO, "CMakeLists.txt")) as f:
        cm = f.read()
    num = re.search(r"set\(PSOUP_NUMERICS_SOURCES \$\{PSOUP_HIP_SOURCES\}([^)]*)\)", cm).group(1)
    hip = re.search(r"set\(PSOUP_HIP_SOURCES\s+([^)]*)\)", cm).group(1)
    assert "orbopt" not in num and "orbopt" not in hip
    assert 'EXCLUDE REGEX "/orbopt\\\\.hpp$"' in cm
    oopt = re.search(r"set\(PSOUP_OOPT_SOURCES\s+([^)]*)\)", cm).group(1).split()
    assert oopt == ["csrc/src/orbopt_host.cpp", "csrc/src/orbopt.cpp", "csrc/kernels/orbopt.hip"]
    assert re.search(r"set_source_files_properties\(csrc/src/orbopt_host\.cpp csrc/src/orbopt\.cpp csrc/kernels/orbopt\.hip\s+"
                     r"PROPERTIES COMPILE_OPTIONS -ffp-contract=off\)", cm)


# ------------------------------------------------- native host unit tests ----
def test_native_orbopt_unit_tests():
    r = subprocess.run([os.path.join(REPO, "bin", "psoup_orbopt_unit_tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
