"""sbsearch on the GPU: sb_power and sb_search against the float64 oracle
(utils.reference.sideband_*) within the derived bound (sideband_cases.py) at
the smallest shapes that reach every path; the event records and their
overflow; SidebandSearcher's re-run; an injected short orbit recovered end to
end, the binary and the module writing the same lines; refusals by name."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import sideband_cases as sc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref

pytestmark = pytest.mark.gpu


def _search(P, k_lo, k_hi, **kw):
    import torch

    from peasoup_amd import ops

    res = ops.sideband_search(torch.from_numpy(np.array(P, dtype=np.float32)).cuda(), k_lo, k_hi, **kw)
    if "best_S" in res:
        res["best_S"] = res["best_S"].cpu().numpy()
        res["best_j"] = res["best_j"].cpu().numpy()
    return res


# ---------------------------------------------------------------- sb_power ----
def test_power_against_the_oracle():
    """Two rows, a band of one full range and a partial one from an odd k_lo, a zap list inside and outside the band;
    NaN outside the band in the output buffer stays NaN.  mu within 1e-12, P within 4 ulp."""
    import torch

    from peasoup_amd import ops

    rng = np.random.default_rng(8)
    nb = 9001
    X = (rng.normal(size=(2, nb)) + 1j * rng.normal(size=(2, nb))).astype(np.complex64)
    zap = np.zeros(nb, dtype=bool)
    zap[[3, 300, 301, 302, 8600]] = True
    k_lo, k_hi = 11, 11 + 4096 + 4000
    for z in (None, zap):
        out = torch.full((2, 9004), float("nan"), dtype=torch.float32, device="cuda")
        mu, P = ops.sideband_power(torch.from_numpy(X).cuda(), k_lo, k_hi, z, out=out)
        mu, P = mu.cpu().numpy(), P.cpu().numpy()
        assert np.all(np.isnan(P[:, :k_lo])) and np.all(np.isnan(P[:, k_hi:]))
        for r in range(2):
            wmu, wP = ref.sideband_power(X[r], k_lo, k_hi, z)
            assert abs(mu[r] - wmu) <= 1e-12 * wmu, (mu[r], wmu)
            got, want = P[r, k_lo:k_hi], wP[k_lo:k_hi]
            assert np.all(np.abs(got.astype(np.float64) - want) <= 4 * np.spacing(want).astype(np.float64))
            if z is not None:
                assert np.all(got[np.nonzero(z[k_lo:k_hi])[0]] == 1.0)


# --------------------------------------------------------------- every size ----
def test_every_size_against_the_oracle():
    P, oracle = sc.all_sizes()
    assert np.all(np.isnan(P[:, :sc.K_LO])) and np.all(np.isnan(P[:, sc.K_HI:])) and sc.STRIDE % 4 == 0
    res = _search(P, sc.K_LO, sc.K_HI)
    total, amb = sc.compare_dense(res["best_S"], res["best_j"], oracle, res["nseg"], what="gpu")
    assert total == 3 * sum(res["nseg"]) and amb <= 0.01 * total, (amb, total)
    sure, border = sc.split_events(oracle, 30.0)
    assert len(sure) <= res["count"] <= len(sure) + len(border)
    sc.check_events(res["events"].tolist(), sure, border, complete=True)


# ------------------------------------------------------------ planted combs ----
@pytest.mark.parametrize("m", range(5, 14))
def test_planted_combs(m):
    M = 1 << m
    P, cases = sc.comb_rows(m)
    k_lo, k_hi = sc.COMB_K_LO, sc.COMB_K_LO + sc.COMB_BAND
    res = _search(P, k_lo, k_hi, m_lo=m, m_hi=m, min_power=1.0)
    want = sc.COMB_A ** 2 * M / 4.0
    for r, (seg, j0) in enumerate(cases):
        S, norm = ref.sideband_spectra(P[r], k_lo, k_hi, m)
        bound = ref.sideband_bound(S[seg, j0], norm[seg:seg + 1], m)[0]
        print(m, seg, j0, res["best_S"][r, 0, seg], S[seg, j0], bound)
        assert res["best_j"][r, 0, seg] == j0
        assert abs(res["best_S"][r, 0, seg] - S[seg, j0]) <= bound
        assert abs(S[seg, j0] - want) <= 1e-5 * want
        ev = [e for e in res["events"].tolist() if e[0] == r and e[2] == seg]
        assert len(ev) == 1 and ev[0][3] == j0 and ev[0][1] == m


# -------------------------------------------------------------------- edges ----
@pytest.mark.parametrize("m", [5, 9, 13])
def test_a_band_of_exactly_one_segment_and_one_bin_less(m):
    M = 1 << m
    P = sc.noise_rows(2, M + 12, 6, 6 + M, 20 + m)
    o = [ref.sideband_search(P[r], 6, 6 + M, m, m, 2, 32.0, 0.0, r) for r in range(2)]
    res = _search(P, 6, 6 + M, m_lo=m, m_hi=m, min_power=0.0)
    assert res["nseg"] == [1] and res["count"] == 2
    sc.compare_dense(res["best_S"], res["best_j"], o, res["nseg"], m, m)
    # M - 1 bins: no segment, nothing launched, every guard and every payload word untouched
    res = _search(P, 6, 6 + M - 1, m_lo=m, m_hi=m, min_power=0.0)
    assert res["nseg"] == [0] and res["count"] == 0 and len(res["events"]) == 0
    assert np.all(np.isnan(res["best_S"])) and np.all(res["best_j"] == 0x7FC0DEAD)


def test_one_admissible_j():
    P = sc.noise_rows(1, 200, 5, 5 + 150, 31)
    res = _search(P, 5, 155, m_lo=5, m_hi=6, j_min=15, min_power=0.0)
    assert np.all(res["best_j"][0, 0, :res["nseg"][0]] == 15)
    o = ref.sideband_search(P[0], 5, 155, 5, 6, 15, 32.0, 0.0)
    sc.compare_dense(res["best_S"], res["best_j"], [o], res["nseg"], 5, 6)


# --------------------------------------------------------------------- clip ----
def test_clip_keeps_one_bright_bin_from_lifting_every_size():
    P, o32, obig = sc.clip_case()
    k_lo, k_hi = sc.CLIP_K_LO, sc.CLIP_K_LO + sc.CLIP_BAND
    # the oracle alone: nothing at M >= 128 with the clip; with it off, every size covering the bin fires
    assert not [e for e in o32["events"] if e[1] >= sc.CLIP_QUIET_M_LO]
    for m in range(5, 14):
        cover = sc.covering(m, k_lo, sc.CLIP_BIN, len(obig[m]["best_S"]))
        assert cover and all(obig[m]["best_S"][s] >= 30.0 for s in cover)
    res = _search(P, k_lo, k_hi, clip=32.0)
    sc.compare_dense(res["best_S"], res["best_j"], [o32], res["nseg"], what="clip 32")
    assert not [e for e in res["events"].tolist() if e[1] >= sc.CLIP_QUIET_M_LO]
    sure, border = sc.split_events([o32], 30.0)
    sc.check_events(res["events"].tolist(), sure, border, complete=True)
    res = _search(P, k_lo, k_hi, clip=1.0e9)
    sc.compare_dense(res["best_S"], res["best_j"], [obig], res["nseg"], what="clip off")
    got = {(e[1], e[2]) for e in res["events"].tolist()}
    for m in range(5, 14):
        assert all((m, s) in got for s in sc.covering(m, k_lo, sc.CLIP_BIN, res["nseg"][m - 5]))


# ------------------------------------------------------------------ records ----
def test_records_past_the_capacity():
    P, _ = sc.all_sizes()
    oracle = [ref.sideband_search(P[r], sc.K_LO, sc.K_HI, 5, 13, 2, 32.0, 3.0, r) for r in range(3)]
    sure, border = sc.split_events(oracle, 3.0)
    res = _search(P, sc.K_LO, sc.K_HI, min_power=3.0, capacity=64, dense=False, dm0=0)
    assert len(sure) > 64 and len(sure) <= res["count"] <= len(sure) + len(border)
    assert len(res["events"]) == 64  # (the ops check the poison behind the buffer and past the count)
    sc.check_events(res["events"].tolist(), sure, border, complete=False)
    full = _search(P, sc.K_LO, sc.K_HI, min_power=3.0, capacity=res["count"], dense=False)
    assert full["count"] == res["count"] == len(full["events"])
    sc.check_events(full["events"].tolist(), sure, border, complete=True)
    # dm0 is added to the row
    one = _search(P[:1], sc.K_LO, sc.K_HI, m_lo=13, m_hi=13, min_power=0.0, dm0=7, dense=False)
    assert one["count"] == one["nseg"][0] and set(one["events"]["dm_idx"].tolist()) == {7}


# --------------------------------------------------------------- end to end ----
@functools.lru_cache(maxsize=None)
def _e2e(tmp):
    ok, _, args = C.parse_sb_cmdline(["sbsearch", "-i", sc.empty_file(tmp), "--fft_size", str(sc.NS)] + sc.E2E_DM_OPTS)
    dms = list(C.sb_setup(args).dm_list)
    assert len(dms) == 4
    return sc.e2e_file(tmp, dms), ["--fft_size", str(sc.NS)] + sc.E2E_DM_OPTS


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _e2e(str(tmp_path_factory.mktemp("sideband_e2e")))


def _args(path, opts):
    ok, _, args = C.parse_sb_cmdline(["sbsearch", "-i", path] + [str(o) for o in opts])
    assert ok
    return args


def test_searcher_reruns_a_chunk_that_overflowed(e2e):
    """min_power 3 and a buffer of 64 events: the searcher runs the chunk again and returns exactly the oracle's event
    set of its own float32 P rows."""
    import torch

    path, opts = e2e
    args = _args(path, opts + ["--min_power", 3])
    setup = C.sb_setup(args)
    fb = C.Filterbank.from_file(path)
    packed = torch.from_numpy(fb.data().copy()).cuda()
    stream = C.GpuStream()
    torch.cuda.synchronize()
    dfb = C.DeviceFilterbank(setup.geometry, stream.handle)
    dfb.load_packed_device(packed.data_ptr())
    stream.synchronize()
    ss = C.SidebandSearcher(setup, dfb, stream.handle, 64)
    events = ss.search()
    assert ss.reruns >= 1 and len(events) > 64
    P, mu = ss.power_rows(0, 4)
    g = setup.geom
    assert np.all(mu > 0) and np.all(P[:, :g.k_lo] == 0) and abs(P[:, g.k_lo:g.k_hi].mean() - 1.0) < 1e-3
    oracle = [ref.sideband_search(P[d], g.k_lo, g.k_hi, 5, 13, 2, 32.0, 3.0, d) for d in range(4)]
    sure, border = sc.split_events(oracle, 3.0)
    sc.check_events(events, sure, border, complete=True)
    assert events == sorted(events, key=lambda e: e[:3])
    assert events == ss.search()  # and again, now without a re-run
    del ss, dfb


def test_an_injected_short_orbit_is_recovered(e2e, tmp_path):
    from peasoup_amd.models.sideband import run_sideband_search

    path, opts = e2e
    out = str(tmp_path / "sb.out")
    res = run_sideband_search(_args(path, opts + ["-o", out]))
    assert res.candidates, "no candidate"
    T = sc.e2e_tobs()
    top = res.candidates[0]
    dm_idx, m, seg, j, S = top.event
    M = 1 << m
    freq, half, pb, pb_res = C.sb_event_values(res.setup.geom, top.event)
    print("top", top.event, freq, half, pb, pb_res, top.members, top.dm_lo, top.dm_hi)
    assert S >= 30.0 and abs(pb - 8.192) <= T / M + 1e-9 and pb_res == T / M
    assert freq - half <= sc.F0 <= freq + half
    assert dm_idx == sc.E2E_DM_IDX and top.dm_lo <= dm_idx <= top.dm_hi
    lines = sc.cand_lines(out)
    assert len(lines) == len(res.candidates) and float(lines[0].split()[2]) == pytest.approx(pb, abs=1e-8)
    assert all(float(a.split()[4]) >= float(b.split()[4]) for a, b in zip(lines, lines[1:]))


def test_native_and_python_drivers_write_the_same_lines(e2e, tmp_path):
    path, opts = e2e
    o1, o2 = str(tmp_path / "native.out"), str(tmp_path / "module.out")
    extra = [str(o) for o in opts] + ["--min_power", "20", "--limit", "40"]
    r = subprocess.run([os.path.join(REPO, "bin", "sbsearch"), "-i", path, "-o", o1] + extra, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "sb", "-i", path, "-o", o2] + extra, capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    l1, l2 = sc.cand_lines(o1), sc.cand_lines(o2)
    assert l1 and l1 == l2 and len(l1) <= 40
    assert len(l1[0].split()) == 12
    with open(o1) as f:
        head = [ln for ln in f.read().splitlines() if ln.startswith("#")]
    assert any("M 1024 segments" in ln for ln in head) and any("min_power 20" in ln for ln in head)


def test_refusals_reach_the_user_by_name(e2e, tmp_path):
    path, opts = e2e
    for extra, what in ((["--m_min", 4], "m_min is below 5"), (["--clip", 1], "clip must be above 1"),
                        (["--min_freq", 10, "--max_freq", 10.2], "shorter than 2^m_min"), (["-t", 2], "one device")):
        r = subprocess.run([os.path.join(REPO, "bin", "sbsearch"), "-i", path, "-o", str(tmp_path / "no.out")] +
                           [str(o) for o in opts + extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and what in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "no.out"))
