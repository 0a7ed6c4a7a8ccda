"""sbsearch without a GPU: the float64 oracle against the analytic comb and
against numpy.fft.rfft directly, the native host steps (geometry, clustering,
the transcriptions of both kernels) against the oracle, every refusal by name,
the option parser, the end-to-end case on the NumPy-dedispersed row and the
host unit-test binary, plain and under ASan / UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sideband_cases as sc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref


# ------------------------------------------------------------------ oracle ----
@pytest.mark.parametrize("m", range(5, 14))
def test_oracle_on_the_analytic_comb(m):
    M = 1 << m
    P, cases = sc.comb_rows(m)
    k_hi = sc.COMB_K_LO + sc.COMB_BAND
    for r, (seg, j0) in enumerate(cases):
        o = ref.sideband_search(P[r], sc.COMB_K_LO, k_hi, m, m, 2, 32.0, 30.0)[m]
        want = sc.COMB_A ** 2 * M / 4.0
        assert o["best_j"][seg] == j0
        assert abs(o["best_S"][seg] - want) <= 1e-5 * want  # the float32 rounding of P
        # the neighbour that shares half of the comb sees a quarter of its energy leak; nobody else anything
        far = [s for s in range(len(o["best_S"])) if abs(s - seg) > 1]
        assert np.all(o["best_S"][far] < 1e-9)


def test_oracle_against_rfft_directly():
    rng = np.random.default_rng(5)
    k_lo, k_hi = 9, 9 + 700
    P = rng.exponential(1.0, 720).astype(np.float32)
    P[100] = 50.0
    for m, clip in ((5, 32.0), (8, 32.0), (9, 4.0)):
        M = 1 << m
        S, norm = ref.sideband_spectra(P, k_lo, k_hi, m, clip)
        assert S.shape == (ref.sideband_nseg(700, m), M // 2)
        for s in (0, S.shape[0] - 1):
            x = np.minimum(P[k_lo + s * M // 2:k_lo + s * M // 2 + M].astype(np.float64), clip) - 1.0
            F = np.fft.rfft(x)
            assert np.allclose(S[s], np.abs(F[:M // 2]) ** 2 / M, rtol=1e-12, atol=1e-12)
            assert np.isclose(norm[s], np.sqrt((x * x).sum()))
        o = ref.sideband_search(P, k_lo, k_hi, m, m, 3, clip, 0.0)[m]
        assert np.array_equal(o["best_j"], np.argmax(S[:, 3:], axis=1) + 3)
        assert np.all(o["gap"] >= 0) and np.all(o["bound"] > 0)
    # the lowest j wins a tie; a flat segment is all zeros
    o = ref.sideband_search(np.ones(64, dtype=np.float32), 0, 64, 5, 6, 2, 32.0, 0.0)
    assert list(o[5]["best_j"]) == [2, 2, 2] and list(o[6]["best_j"]) == [2] and np.all(o[5]["best_S"] == 0)
    assert [e[:4] for e in o["events"]] == [(0, 5, 0, 2), (0, 5, 1, 2), (0, 5, 2, 2), (0, 6, 0, 2)]


def test_oracle_power_and_its_order():
    rng = np.random.default_rng(6)
    nb = 9000
    X = (rng.normal(size=nb) + 1j * rng.normal(size=nb)).astype(np.complex64)
    zap = np.zeros(nb, dtype=bool)
    zap[300:320] = True
    k_lo, k_hi = 11, 11 + 8192 + 301
    mu, P = ref.sideband_power(X, k_lo, k_hi, zap)
    p = X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2
    keep = ~zap[k_lo:k_hi]
    want = float(np.sum(p[k_lo:k_hi][keep])) / int(keep.sum())
    assert abs(mu - want) <= 1e-12 * want
    assert np.all(P[:k_lo] == 0) and np.all(P[k_hi:] == 0) and np.all(P[300:320] == 1.0)
    assert np.array_equal(P[k_lo:300], (p[k_lo:300] / mu).astype(np.float32))
    # the native transcription: the same sum in the same order, bit for bit
    words = np.packbits(np.concatenate([zap, np.zeros(24, bool)]).reshape(-1, 32), axis=1, bitorder="little")
    mu_h, P_h = C.sb_power_host(X[None, :], [int(w) for w in words.view("<u4").reshape(-1)], k_lo, k_hi)
    assert mu_h[0] == mu and np.array_equal(P_h[0], P)
    with pytest.raises(ValueError, match="no unzapped bin"):
        ref.sideband_power(X, 300, 320, zap)


# ---------------------------------------------------------- native host steps ----
def test_geometry_at_the_band_edges():
    for m in range(5, 14):
        M = 1 << m
        for band, want in ((M - 1, 0), (M, 1), (M + M // 2 - 1, 1), (M + M // 2, 2)):
            assert C.sb_nseg(band, m) == want == ref.sideband_nseg(band, m)
            g = C.sb_band_geometry(7, 7 + band, m, m)
            assert g.nseg == [want] and g.nwin == (2 if (m, want) == (13, 2) else min(want, 1)) and g.seg_stride == want
    g = C.sb_geometry(0.1, 1100.0, 1 << 17, 1e-3)
    w = ref.sideband_geometry(0.1, 1100.0, 1 << 17, 1e-3)
    assert (g.tobs, g.k_lo, g.k_hi) == (w["tobs"], w["k_lo"], w["k_hi"]) == (sc.e2e_tobs(), 14, 65536)
    assert g.nseg == [w["nseg"][m] for m in range(5, 14)]
    g = C.sb_geometry(10.0, 120.0, 1 << 17, 1e-3, 6, 9)
    w = ref.sideband_geometry(10.0, 120.0, 1 << 17, 1e-3, 6, 9)
    assert (g.k_lo, g.k_hi, g.nseg) == (w["k_lo"], w["k_hi"], [w["nseg"][m] for m in range(6, 10)])
    assert g.k_lo == 1311 and g.k_hi == 15728
    # the windows (hop 4096) own every segment and hold it whole
    g = C.sb_band_geometry(sc.K_LO, sc.K_HI)
    for m, n in zip(range(5, 14), g.nseg):
        M = 1 << m
        owned = 1 if m == 13 else sc.WINDOW // M
        last = (n - 1) * (M // 2)
        win = (n - 1) // owned
        assert win < g.nwin and win * sc.HOP <= last and last + M <= win * sc.HOP + sc.WINDOW
    assert g.nwin == 8


def test_host_transcription_against_the_oracle():
    """The native host transcription of sb_search (the kernel's arithmetic, one thread after the other) on the GPU
    test's own input: within the derived bound of the oracle, and the oracle alone shows that at most 1% of the
    segments are too close to call."""
    P, oracle = sc.all_sizes()
    bs, bj, ev = C.sb_search_host(np.array(P), sc.K_LO, sc.K_HI, 5, 13, 2, 32.0, 30.0, 0)
    g = C.sb_band_geometry(sc.K_LO, sc.K_HI)
    total, amb = sc.compare_dense(bs, bj, oracle, g.nseg, what="host")
    assert total == 3 * sum(g.nseg) and amb <= 0.01 * total, (amb, total)
    for m, n in zip(range(5, 14), g.nseg):
        assert np.all(np.isnan(bs[:, m - 5, n:])) and np.all(bj[:, m - 5, n:] == -1)
    sure, border = sc.split_events(oracle, 30.0)
    sc.check_events(ev, sure, border, complete=True)


def test_host_transcription_beside_a_bright_bin():
    """One bin of 10^6: clipped, and with the clip off, where a quiet segment must not ride a transform with it."""
    P, o32, obig = sc.clip_case()
    k_lo, k_hi = sc.CLIP_K_LO, sc.CLIP_K_LO + sc.CLIP_BAND
    g = C.sb_band_geometry(k_lo, k_hi)
    for clip, o in ((32.0, o32), (1.0e9, obig)):
        bs, bj, ev = C.sb_search_host(np.array(P), k_lo, k_hi, 5, 13, 2, clip, 30.0, 0)
        sc.compare_dense(bs, bj, [o], g.nseg, what=f"host clip {clip}")
        sure, border = sc.split_events([o], 30.0)
        sc.check_events(ev, sure, border, complete=True)


def _ev(dm, m, seg, j, S):
    return (dm, m, seg, j, float(np.float32(S)))


CLUSTER_CASES = {
    "third harmonic at the next size, other DMs": [_ev(2, 11, 24, 384, 40), _ev(1, 10, 48, 64, 53), _ev(3, 10, 49, 64, 35),
                                                   _ev(0, 10, 48, 65, 31)],
    "overlap at the limit": [_ev(0, 10, 10, 64, 50), _ev(0, 10, 12, 64, 40)],
    "no overlap": [_ev(0, 10, 10, 64, 50), _ev(0, 10, 13, 64, 40)],
    "overlap across sizes": [_ev(0, 13, 0, 512, 50), _ev(0, 5, 511, 2, 40), _ev(0, 5, 513, 2, 39)],
    "tolerance in": [_ev(0, 12, 0, 400, 50), _ev(0, 12, 0, 402, 40), _ev(0, 12, 0, 201, 39), _ev(0, 12, 0, 1204, 38)],
    "tolerance out": [_ev(0, 12, 0, 400, 50), _ev(0, 12, 0, 403, 40), _ev(0, 12, 0, 1001, 39), _ev(0, 12, 0, 337, 38)],
    "ties": [_ev(5, 10, 3, 64, 40), _ev(4, 10, 3, 64, 40), _ev(4, 9, 6, 32, 40), _ev(4, 9, 5, 32, 40)],
    "first accepted candidate": [_ev(0, 10, 0, 100, 60), _ev(0, 10, 0, 107, 50), _ev(0, 10, 0, 214, 45),
                                 _ev(7, 10, 1, 321, 44)],
    "nothing": [],
}
for _r in range(1, 6):
    CLUSTER_CASES[f"r = {_r} up"] = [_ev(0, 12, 0, 40, 50), _ev(1, 12, 0, 40 * _r, 40)]
    CLUSTER_CASES[f"r = {_r} down"] = [_ev(0, 12, 0, 40 * _r, 50), _ev(1, 12, 0, 40, 40)]


@pytest.mark.parametrize("name", sorted(CLUSTER_CASES))
def test_cluster_binding_against_the_reference(name):
    ev = CLUSTER_CASES[name]
    got = C.sb_cluster(ev)
    want = ref.sideband_cluster(ev)
    assert [(tuple(e), n, lo, hi) for e, n, lo, hi in got] == want
    assert sum(n for _, n, _, _ in got) == len(ev)


def test_cluster_by_hand():
    n = {k: len(C.sb_cluster(v)) for k, v in CLUSTER_CASES.items()}
    assert n["third harmonic at the next size, other DMs"] == 1 and n["overlap at the limit"] == 1
    assert n["no overlap"] == 2 and n["tolerance in"] == 1 and n["tolerance out"] == 4 and n["ties"] == 1
    assert n["overlap across sizes"] == 2
    for r in range(1, 6):
        assert n[f"r = {r} up"] == n[f"r = {r} down"] == (1 if r <= 4 else 2), r
    (e, members, lo, hi), = C.sb_cluster(CLUSTER_CASES["third harmonic at the next size, other DMs"])
    assert e[:4] == (1, 10, 48, 64) and (members, lo, hi) == (4, 0, 3)
    (e, members, lo, hi), = C.sb_cluster(CLUSTER_CASES["ties"])
    assert e[:4] == (4, 9, 5, 32) and (members, lo, hi) == (4, 4, 5)
    a, b = C.sb_cluster(CLUSTER_CASES["first accepted candidate"])
    assert (a[0][3], a[1], b[0][3], b[1], b[2], b[3]) == (100, 1, 107, 3, 0, 7)


# ------------------------------------------------------------------ refusals ----
REFUSALS = [
    (dict(fft_size=(1 << 26) + 2), "above 2^26"),
    (dict(m_lo=4), "m_min is below 5"),
    (dict(m_hi=14), "m_max is above 13"),
    (dict(m_lo=9, m_hi=8), "m_min is above m_max"),
    (dict(j_min=0), "j_min is outside"),
    (dict(j_min=16), "j_min is outside"),
    (dict(m_lo=7, j_min=64), "j_min is outside"),
    (dict(clip=1.0), "clip must be above 1"),
    (dict(clip=0.5), "clip must be above 1"),
    (dict(clip=float("inf")), "non-finite"),
    (dict(clip=float("nan")), "non-finite"),
    (dict(min_power=float("nan")), "non-finite"),
    (dict(min_freq=float("nan")), "non-finite"),
    (dict(max_freq=float("inf")), "non-finite"),
    (dict(min_freq=10.0, max_freq=10.2), "shorter than 2^m_min"),
    (dict(min_freq=10.0, max_freq=11.0, m_lo=8), "shorter than 2^m_min"),
]


@pytest.mark.parametrize("change,what", REFUSALS)
def test_every_refusal_by_name(change, what):
    kw = dict(min_freq=0.1, max_freq=1100.0, fft_size=1 << 17, tsamp=1e-3)
    C.sb_check(**kw)
    C.sb_check(**dict(kw, j_min=15))
    C.sb_check(**dict(kw, m_lo=7, j_min=63))
    C.sb_check(**dict(kw, min_freq=10.0, max_freq=10.3))
    kw.update(change)
    with pytest.raises(RuntimeError, match=what.replace("^", r"\^")):
        C.sb_check(**kw)


def test_setup_refusals_from_the_header(tmp_path):
    fil = sc.empty_file(tmp_path)

    def setup(*extra):
        ok, _, args = C.parse_sb_cmdline(["sbsearch", "-i", fil, "--fft_size", str(sc.NS)] + [str(e) for e in extra])
        assert ok
        return args

    s = C.sb_setup(setup(*sc.E2E_DM_OPTS))
    assert len(s.dm_list) == 4 and s.geom.k_lo == 14 and s.geom.k_hi == 65536 and s.unzapped == 65522
    assert (s.m_lo, s.m_hi, s.j_min, s.clip, s.min_power) == (5, 13, 2, 32.0, 30.0)
    for extra, what in (((("--m_min", 4)), "m_min is below 5"), (("--m_max", 14), "m_max is above 13"),
                        (("--m_min", 9, "--m_max", 8), "m_min is above m_max"), (("--j_min", 0), "j_min is outside"),
                        (("--j_min", 16), "j_min is outside"), (("--clip", 1), "clip must be above 1"),
                        (("--clip", "inf"), "non-finite"), (("--min_power", "nan"), "non-finite"),
                        (("--min_freq", "nan"), "non-finite"),
                        (("--min_freq", 10, "--max_freq", 10.2), "shorter than 2^m_min")):
        with pytest.raises(RuntimeError, match=what.replace("^", r"\^")):
            C.sb_setup(setup(*extra))
    args = setup()
    args.search.max_num_threads = 2
    with pytest.raises(RuntimeError, match="one device"):
        C.sb_setup(args)
    big = sc.big_file(tmp_path)
    ok, _, args = C.parse_sb_cmdline(["sbsearch", "-i", big, "--dm_start", "0", "--dm_end", "0", "--fft_size", str(1 << 27)])
    with pytest.raises(RuntimeError, match=r"above 2\^26"):
        C.sb_setup(args)
    # a zap list that covers the band
    z = tmp_path / "zap.txt"
    z.write_text("250 260\n")
    with pytest.raises(RuntimeError, match="no unzapped bin"):
        C.sb_setup(setup("-z", str(z)))
    z.write_text("50 1\n")
    s = C.sb_setup(setup("-z", str(z)))
    assert 0 < s.geom.k_hi - s.geom.k_lo - s.unzapped < 300


def test_option_parser():
    ok, exit_now, a = C.parse_sb_cmdline(["sbsearch", "-i", "x.fil"])
    assert ok and not exit_now
    assert (a.min_power, a.m_min, a.m_max, a.j_min, a.clip) == (30.0, 5, 13, 2, 32.0)
    s = a.search
    assert (s.max_num_threads, s.limit, s.dm_start, s.dm_end, s.size) == (1, 1000, 0.0, 100.0, 0)
    assert abs(s.min_freq - 0.1) < 1e-7 and s.max_freq == 1100.0 and abs(s.dm_tol - 1.1) < 1e-6 and s.dm_pulse_width == 64.0
    assert a.outfilename.endswith("_sbsearch.output") and s.dedisp_kernel == "auto" and not s.verbose
    ok, _, b = C.parse_sb_cmdline("sbsearch -i x.fil -o o.txt -k k.txt -z z.txt --dm_start 1 --dm_end 9 --dm_tol 1.2 "
                                  "--dm_pulse_width 40 --min_freq 2 --max_freq 300 --fft_size 65536 --limit 5 "
                                  "--dedisp_kernel direct -v --min_power 12 --m_min 6 --m_max 11 --j_min 3 --clip 100 "
                                  "-t 1".split())
    assert ok and (b.min_power, b.m_min, b.m_max, b.j_min, b.clip, b.outfilename) == (12.0, 6, 11, 3, 100.0, "o.txt")
    s = b.search
    assert (s.killfilename, s.zapfilename, s.dm_start, s.dm_end, s.dm_pulse_width) == ("k.txt", "z.txt", 1.0, 9.0, 40.0)
    assert (s.min_freq, s.max_freq, s.size, s.limit, s.dedisp_kernel, s.verbose) == (2.0, 300.0, 65536, 5, "direct", True)
    assert not C.parse_sb_cmdline(["sbsearch", "-i", "x.fil", "-t", "2"])[0]
    assert not C.parse_sb_cmdline(["sbsearch"])[0]
    assert not C.parse_sb_cmdline(["sbsearch", "-i", "x.fil", "--acc_start", "1"])[0]
    assert not C.parse_sb_cmdline(["sbsearch", "-i", "x.fil", "--limit", "-1"])[0]
    assert C.parse_sb_cmdline(["sbsearch", "-h"])[1]


# ---------------------------------------------------------------- end to end ----
def test_the_injected_orbit_on_the_numpy_dedispersed_row(tmp_path):
    """What the GPU end-to-end test rests on, confirmed without one: the oracle on the NumPy-dedispersed, NumPy-
    whitened row of the injected DM has power >= 30 at M = 1024 with pb recovered exactly, and its strongest event
    holds 50 Hz; the neighbouring DM trials have nothing that strong."""
    ok, _, args = C.parse_sb_cmdline(["sbsearch", "-i", sc.empty_file(tmp_path), "--fft_size", str(sc.NS)] + sc.E2E_DM_OPTS)
    s = C.sb_setup(args)
    dms = list(s.dm_list)
    assert len(dms) == 4
    hdr = sc.e2e_header()
    v = sc.e2e_values(dms)
    rows = ref.dedisperse(v, ref.dm_offsets(dms, ref.delay_table(16, hdr["tsamp"], hdr["fch1"], hdr["foff"])), 8)
    T = sc.e2e_tobs()
    best = []
    for d in range(4):
        D = ref.whiten64(rows[d], sc.NS, s.tsamp)[0].astype(np.complex64)
        _, P = ref.sideband_power(D, s.geom.k_lo, s.geom.k_hi)
        o = ref.sideband_search(P, s.geom.k_lo, s.geom.k_hi, dm_idx=d)
        best.append(max(o["events"], key=lambda e: e[4]) if o["events"] else None)
        if d == sc.E2E_DM_IDX:
            k = int(np.argmax(o[10]["best_S"]))
            assert o[10]["best_S"][k] >= 30.0 and o[10]["best_j"][k] == 64
            assert 64 * T / 1024 == T / 16
    top = best[sc.E2E_DM_IDX]
    assert top is not None and all(b is None or b[4] < top[4] - 3.0 for d, b in enumerate(best) if d != sc.E2E_DM_IDX)
    _, m, seg, j, S = top
    M = 1 << m
    assert abs(j * T / M - T / 16) <= T / M
    c = s.geom.k_lo + seg * M // 2 + M // 2
    assert (c - M // 2) / T <= sc.F0 <= (c + M // 2) / T


# ----------------------------------------------------------- native unit tests ----
def test_native_unit_tests_run_clean():
    r = subprocess.run([os.path.join(REPO, "bin", "psoup_sideband_unit_tests")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_a_host_sanitizer(san):
    """The stand-alone host program, built with -fsanitize through the build driver's --sanitize route."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "peasoup_amd", "_build.py"), "--sanitize", san, "--target",
                        "psoup_sideband_unit_tests"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, "bin", f"psoup_sideband_unit_tests_{san}")], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout and "runtime error" not in r.stderr
