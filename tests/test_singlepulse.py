"""Single-pulse (transient) search: boxcar matched filter over the DM trials
(csrc/include/psoup/singlepulse.hpp; an extension beyond the reference).

CPU: option parsing, width ladder, clustering against a literal Python
transcription, and the synthetic generator's regression pin.  GPU: the fused
kernel's block maxima and records against a float64 NumPy oracle written from
the definition, capacity overflow, degenerate rows, batching, and the
pipelines (native, CLI, two ranks) on an injected dispersed burst."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = 4096
WMAX = 4096
T = C.SP_TILE
TOL = dict(rtol=1e-3, atol=1e-3)  # as test_ffa_planes_match_numpy: boxcar S/N against the float64 oracle


# ------------------------------------------------------------------- CPU ----
def test_sp_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_sp_cmdline(["spsearch", "-i", "x.fil"])
    assert ok and not exit_now and a.infilename == "x.fil"
    assert a.max_num_threads == 14 and (a.dm_start, a.dm_end) == (0.0, 100.0)
    assert a.dm_tol == pytest.approx(1.10) and a.dm_pulse_width == 64.0
    assert not a.verbose and not a.progress_bar and a.killfilename == ""
    assert a.min_snr == 6.5 and a.boxcar_max == 4096 and a.baseline == 2.0 and a.limit == 1000
    assert a.dedisp_kernel == "auto"
    assert a.outfilename.endswith("_spsearch.output")
    assert len(a.outfilename) == len("2026-01-01-00:00_spsearch.output")
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", "y.fil", "-o", "out.txt", "-k", "kill.txt", "-t", "2",
                                   "--dm_start", "5", "--dm_end", "50", "--dm_tol", "1.2", "--dm_pulse_width", "40",
                                   "-vp", "--min_snr", "8", "--boxcar_max", "512", "--baseline", "0.5",
                                   "--limit", "10", "--dedisp_kernel", "valu"])
    assert ok and a.outfilename == "out.txt" and a.killfilename == "kill.txt" and a.max_num_threads == 2
    assert (a.dm_start, a.dm_end) == (5.0, 50.0) and a.dm_tol == pytest.approx(1.2) and a.dm_pulse_width == 40.0
    assert a.verbose and a.progress_bar and a.min_snr == 8.0 and a.boxcar_max == 512 and a.baseline == 0.5
    assert a.limit == 10 and a.dedisp_kernel == "valu"
    p = C.sp_params_from(a, 1e-3)
    assert (p.tsamp, p.min_snr, p.boxcar_max, p.baseline_s) == (1e-3, 8.0, 512, 0.5)
    ok, _, _ = C.parse_sp_cmdline(["spsearch"])  # -i is required
    assert not ok


def test_sp_widths():
    assert C.sp_widths(5000, 4096) == [1 << k for k in range(12)]
    assert C.sp_widths(70001, 4096) == [1 << k for k in range(13)]
    assert C.sp_widths(100, 4096) == [1, 2, 4, 8, 16, 32]
    for n, w in [(5000, 4096), (70001, 4096), (100, 4096), (12287, 100)]:
        assert C.sp_widths(n, w) == ref.sp_widths(n, w)


def _assert_clusters_equal(events, dm_list, band_delay, tsamp):
    got = C.sp_cluster([C.SpEvent(*e) for e in events], dm_list, band_delay, tsamp)
    exp = ref.sp_cluster_ref(events, dm_list, band_delay, tsamp)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert (g.sample, g.width, g.dm_idx, g.members) == (e["sample"], e["width"], e["dm_idx"], e["members"])
        assert (g.first_sample, g.last_sample, g.dm_idx_lo, g.dm_idx_hi) == (
            e["first_sample"], e["last_sample"], e["dm_idx_lo"], e["dm_idx_hi"])
        assert g.snr == np.float32(e["snr"]) and g.time_s == e["time_s"] and g.dm == np.float32(e["dm"])
    assert [g.snr for g in got] == sorted((g.snr for g in got), reverse=True)
    return got


def test_sp_cluster_hand_written():
    dm_list = [float(np.float32(2.5 * i)) for i in range(9)]  # 0, 2.5, ... 20
    tsamp, band_delay = 1e-3, 4e-3  # 4 samples of delay across the band per unit DM
    # burst A: strongest at DM index 4, width 8, seen at 5 DMs displaced by at
    # most |dDM| * 4 samples (2.5 -> 10, 5 -> 20); events are (sample, k, snr, dm_idx)
    a = [(10000, 3, 20.0, 4), (10009, 3, 15.0, 3), (9991, 3, 14.0, 5), (10019, 4, 11.0, 2), (9975, 4, 10.0, 6)]
    # one event just outside A's window at the same DM: |t - t0| = 9 > (8 + 8) / 2
    outside = [(10009, 3, 9.0, 4)]
    # burst B at another time, two widths
    b = [(50000, 5, 12.0, 1), (50010, 4, 9.5, 1)]
    got = _assert_clusters_equal(a + outside + b, dm_list, band_delay, tsamp)
    assert [(g.sample, g.members) for g in got] == [(10000, 5), (50000, 2), (10009, 1)]
    assert (got[0].dm_idx_lo, got[0].dm_idx_hi, got[0].first_sample, got[0].last_sample) == (2, 6, 9975, 10034)
    # exactly on the window's edge (|t - t0| = 8) it is absorbed
    got = _assert_clusters_equal(a + [(10008, 3, 9.0, 4)], dm_list, band_delay, tsamp)
    assert [(g.sample, g.members) for g in got] == [(10000, 6)]


def test_sp_cluster_random_events():
    rng = np.random.default_rng(2024)
    dm_list = [float(x) for x in np.linspace(0, 60, 40).astype(np.float32)]
    ev = [(int(rng.integers(0, 30000)), int(rng.integers(0, 9)), float(np.float32(rng.uniform(6.5, 12))),
           int(rng.integers(0, 40))) for _ in range(2000)]
    ev += ev[:20]  # exact duplicates: ties in every key
    got = _assert_clusters_equal(ev, dm_list, 2.3e-3, 1e-3)
    assert 1 < len(got) < len(ev) and sum(g.members for g in got) == len(ev)


def test_synthetic_without_bursts_is_unchanged():
    """SHA-256 of generate()/packed() computed on the commit before bursts=() existed."""
    hdr = synthetic.make_header(nchans=16, nbits=2, tsamp=1e-3)
    psr = [synthetic.PulsarSpec(period=0.25, dm=20.0, duty=0.05, amplitude=0.8, accel=3.0)]
    a = synthetic.generate(70000, hdr, psr, seed=7)
    assert hashlib.sha256(a.tobytes()).hexdigest() == \
        "74b870f97f407e81176b9306d0908e9a00097527008085667b54b4bc98f84f91"
    assert np.array_equal(a, synthetic.generate(70000, hdr, psr, seed=7, bursts=()))
    assert hashlib.sha256(synthetic.packed(5000, hdr, (), 3).tobytes()).hexdigest() == \
        "9049ce6f75a9fb56d16752499187a337ddf6a9ce730b85c85e822ac447865a92"
    burst = synthetic.BurstSpec(time=30.0, dm=10.0, width=0.01, amplitude=2.0)
    b = synthetic.generate(70000, hdr, psr, seed=7, bursts=[burst])
    changed = np.nonzero((a != b).any(axis=1))[0]
    assert len(changed) and 29950 < changed.min() and changed.max() < 30150  # the same noise, one pulse added


# ------------------------------------------------------------------- GPU ----
def _params(thresh=6.5, capacity=1 << 16):
    p = C.SpParams()
    p.tsamp, p.min_snr, p.boxcar_max, p.baseline_samples, p.capacity = 1e-3, thresh, WMAX, BASELINE, capacity
    return p


@functools.lru_cache(maxsize=None)
def _rows(ndm, n, pulses=False):
    """Seeded noise rows rint(N(100, 6)) + a linear ramp, clipped to uint8, in
    rows of stride > n whose padding is 255 (a read past n would show)."""
    rng = np.random.default_rng(1000 * ndm + n)
    stride = (n + 3) // 4 * 4 + 8
    rows = np.full((ndm, stride), 255, dtype=np.uint8)
    ramp = 10.0 * np.arange(n) / n
    for d in range(ndm):
        x = rng.normal(100.0, 6.0, n) + ramp * (d + 1) / ndm
        if pulses and d != 1:
            # top-hat pulses of 1, 37 and 1500 samples; the 37-sample one
            # straddles the boundary between the kernel's tiles 1 and 2
            x[1234 + d] += 60.0
            x[2 * T - 18:2 * T + 19] += 10.0
            x[40000:41500] += 2.0
        rows[d, :n] = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(ndm, n, pulses=False):
    """Per DM: (widths, snr_k arrays, block maxima) of the float64 oracle."""
    rows = _rows(ndm, n, pulses)
    widths = ref.sp_widths(n, WMAX)
    out = []
    for d in range(ndm):
        snr = ref.sp_boxcar_snr(rows[d, :n], BASELINE, widths)
        out.append((widths, snr, ref.sp_block_maxima(snr)))
    return out


def _tuples(events):
    return [e.astuple() for e in events]


SHAPES = [(1, 5000), (3, 70001), (2, T + 1), (2, T + WMAX - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("ndm,n", SHAPES)
def test_sp_dense_block_maxima_match_oracle(ndm, n):
    rows = _rows(ndm, n)
    events, reruns, best, arg = C.sp_search_rows(rows, n, _params(thresh=1e30), dense=True)
    assert events == [] and reruns == 0
    nblk = (n + 63) // 64
    widths = ref.sp_widths(n, WMAX)
    assert best.shape == arg.shape == (ndm, len(widths), nblk)
    assert np.isfinite(best).all()
    for d, (_, snr, maxima) in enumerate(_oracle(ndm, n)):
        for k, w in enumerate(widths):
            mx, _ = maxima[k]
            nb = len(mx)  # blocks with a valid start, the last one partial
            assert nb == (n - w + 1 + 63) // 64
            np.testing.assert_allclose(best[d, k, :nb], mx, err_msg=f"dm {d} width {w}", **TOL)
            a = arg[d, k, :nb].astype(np.int64)
            assert np.array_equal(a // 64, np.arange(nb)) and (a + w <= n).all()
            # tie-tolerant: the oracle's S/N at the kernel's argmax is the oracle's block maximum
            np.testing.assert_allclose(snr[k][a], mx, err_msg=f"argmax dm {d} width {w}", **TOL)
            assert (best[d, k, nb:] == 0).all() and (arg[d, k, nb:] == 0xFFFFFFFF).all()


def _threshold_from_oracle(oracle):
    """Midpoint of the widest gap between consecutive sorted oracle block
    maxima in [4.5, 5.5]: no oracle value lies within tolerance of it."""
    vals = np.sort(np.concatenate([mx for (_, _, maxima) in oracle for (mx, _) in maxima]))
    vals = vals[(vals >= 4.5) & (vals <= 5.5)]
    assert len(vals) >= 2
    gaps = np.diff(vals)
    i = int(np.argmax(gaps))
    assert gaps[i] > 0.02, gaps[i]
    return float(0.5 * (vals[i] + vals[i + 1]))


PULSE_SHAPE = (3, 70001)


def _expected_records(oracle, thresh):
    exp = {}
    for d, (widths, _, maxima) in enumerate(oracle):
        for k in range(len(widths)):
            mx, _ = maxima[k]
            for b in np.nonzero(mx >= thresh)[0]:
                exp[(d, k, int(b))] = mx[b]
    return exp


@pytest.mark.gpu
def test_sp_records_equal_thresholded_oracle():
    ndm, n = PULSE_SHAPE
    oracle = _oracle(ndm, n, True)
    thresh = _threshold_from_oracle(oracle)
    exp = _expected_records(oracle, thresh)
    # the injected pulses are found at their own widths
    assert max(exp[k] for k in exp if k[:2] == (0, 0)) > 8 and max(exp[k] for k in exp if k[:2] == (2, 5)) > 8
    assert (0, 5, (2 * T - 18) // 64) in exp or (0, 5, (2 * T - 18) // 64 - 1) in exp  # across the tile boundary
    events, reruns, _, _ = C.sp_search_rows(_rows(ndm, n, True), n, _params(thresh=thresh), dense=False)
    got = _tuples(events)
    assert got == sorted(got, key=lambda t: t[:3])
    keys = [(d, k, s // 64) for (d, k, s, _) in got]
    assert len(set(keys)) == len(keys) and set(keys) == set(exp)
    for (d, k, s, snr) in got:
        np.testing.assert_allclose(snr, exp[(d, k, s // 64)], **TOL)
        assert s + (1 << k) <= n
    assert not any(d == 1 and snr > 8 for (d, _, _, snr) in got)  # the row without pulses


@pytest.mark.gpu
def test_sp_capacity_overflow_reruns_to_the_same_events():
    ndm, n = PULSE_SHAPE
    thresh = _threshold_from_oracle(_oracle(ndm, n, True))
    rows = _rows(ndm, n, True)
    big, reruns_big, _, _ = C.sp_search_rows(rows, n, _params(thresh, capacity=1 << 16), dense=False)
    small, reruns_small, _, _ = C.sp_search_rows(rows, n, _params(thresh, capacity=8), dense=False)
    assert len(big) > 8 and reruns_big == 0 and reruns_small >= 1
    assert _tuples(small) == _tuples(big)


@pytest.mark.gpu
def test_sp_constant_row_gives_no_events_and_no_nan():
    n = T + 1
    rows = np.array(_rows(2, n))
    rows[0, :n] = 77  # sigma == 0
    thresh = 3.5
    events, _, best, arg = C.sp_search_rows(rows, n, _params(thresh), dense=True)
    assert np.isfinite(best).all() and (best[0] == 0).all()
    got = _tuples(events)
    assert got and all(d == 1 for (d, _, _, _) in got)
    alone, _, best1, _ = C.sp_search_rows(rows[1:], n, _params(thresh), dense=True, dm_idx0=1)
    assert _tuples(alone) == got and np.array_equal(best1[0], best[1])


@pytest.mark.gpu
def test_sp_batch_equals_single_rows():
    ndm, n = 5, T + 1
    rows = _rows(ndm, n)
    p = _params(thresh=3.5)
    batch, _, _, _ = C.sp_search_rows(rows, n, p, dense=False)
    single = []
    for d in range(ndm):
        ev, _, _, _ = C.sp_search_rows(rows[d:d + 1], n, p, dense=False, dm_idx0=d)
        single += _tuples(ev)
    assert len(single) > 50 and _tuples(batch) == single  # bit for bit, S/N included


@pytest.mark.gpu
def test_sp_torch_op_matches_driver():
    import torch

    from peasoup_amd import ops

    ndm, n = 2, T + 1
    rows = _rows(ndm, n)
    ev, _, best, arg = C.sp_search_rows(rows, n, _params(3.5), dense=True)
    tev, tbest, targ = ops.single_pulse_search(torch.from_numpy(np.array(rows)).cuda(), n, _params(3.5), dense=True)
    assert _tuples(tev) == _tuples(ev) and np.array_equal(tbest.cpu().numpy(), best)
    assert np.array_equal(targ.cpu().numpy(), np.where(arg == 0xFFFFFFFF, -1, arg.astype(np.int64)))
    with pytest.raises(ValueError):
        ops.single_pulse_search(torch.from_numpy(np.array(rows)), n, _params(3.5))  # no CPU fallback


BURST = synthetic.BurstSpec(time=40.0, dm=25.0, width=8e-3, amplitude=1.5)


def _burst_file(tmp_path, bursts, seed):
    hdr = synthetic.make_header(nchans=64, nbits=2, tsamp=1e-3, fch1=1510.0, foff=-1.09)
    path = str(tmp_path / f"sp{seed}.fil")
    synthetic.write(path, 1 << 17, hdr, [], seed=seed, bursts=bursts)
    return path


def _lines(path):
    return [ln for ln in open(path) if not ln.startswith("#")]


@pytest.mark.gpu
def test_sp_pipeline_finds_injected_burst(tmp_path):
    """64 channels, 2 bits, tsamp 1 ms, 2^17 samples, one burst at 40 s and DM
    25 (FWHM 8 ms, amplitude 1.5 sigma per channel), seed 21.  The float64
    oracle on reference.dedisperse's trial at the DM nearest 25 (baseline 2 s)
    gives S/N 23.09 at width 8, start sample 39996 (6 DM trials, the nearest
    to 25 is index 2, DM 20.31): far above the default threshold of 6.5."""
    path = _burst_file(tmp_path, [BURST], seed=21)
    out = str(tmp_path / "sp.txt")
    flags = ["-i", path, "--dm_start", "0", "--dm_end", "50", "-t", "1"]
    ok, _, a = C.parse_sp_cmdline(["spsearch"] + flags + ["-o", out])
    assert ok
    res = C.run_sp_pipeline(a)
    assert res.candidates, "no single-pulse candidates"
    best = res.candidates[0]
    assert abs(best.time_s - BURST.time) / 1e-3 <= best.width + 2
    dms = np.asarray(res.dm_list)
    assert abs(best.dm_idx - int(np.argmin(np.abs(dms - BURST.dm)))) <= 1
    assert best.members > 1 and best.snr > 6.5
    assert best.dm_idx_lo <= best.dm_idx <= best.dm_idx_hi and best.first_sample <= best.sample <= best.last_sample
    C.write_sp_output(out, a, res)
    lines = _lines(out)
    assert len(lines) == len(res.candidates)
    f = lines[0].split()
    assert float(f[0]) == pytest.approx(best.snr, abs=1e-3) and int(f[1]) == best.sample
    assert float(f[2]) == pytest.approx(best.time_s, abs=1e-8) and int(f[3]) == best.width
    assert int(f[4]) == best.dm_idx and int(f[6]) == best.members
    assert (int(f[7]), int(f[8]), int(f[9]), int(f[10])) == (best.first_sample, best.last_sample, best.dm_idx_lo,
                                                             best.dm_idx_hi)
    # the native CLI writes the same first line
    cli_out = str(tmp_path / "cli.txt")
    r = subprocess.run([os.path.join(REPO, "bin", "spsearch")] + flags + ["-o", cli_out], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert _lines(cli_out)[0] == lines[0]


@pytest.mark.gpu
def test_sp_pipeline_noise_only_gives_no_candidates(tmp_path):
    """Seed 22: the float64 oracle's largest block maximum over every DM trial
    of 0..50 is 4.77 (baseline 2 s, widths 1..4096)."""
    path = _burst_file(tmp_path, [], seed=22)
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", path, "--dm_end", "50", "-t", "1", "--min_snr", "8"])
    assert ok
    res = C.run_sp_pipeline(a)
    assert res.candidates == [] and res.events == 0 and len(res.dm_list) > 1


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
def test_sp_two_rank_search_equals_native_pipeline(tmp_path):
    """DM-sharded search (2 ranks, gloo transport, one GPU) + gather +
    cross-DM clustering == the native thread-per-GPU pipeline's candidates."""
    import sys

    path = _burst_file(tmp_path, [BURST], seed=21)
    flags = ["-i", path, "--dm_end", "50", "-t", "1", "--min_snr", "6"]
    script = (
        "import os,sys; sys.path.insert(0, %r)\n"
        "from peasoup_amd.parallel import dist as pdist\n"
        "pdist.init(backend='gloo')\n"
        "from peasoup_amd import __main__ as m\n"
        "raise SystemExit(m.main(['x', 'sps'] + sys.argv[1:]))\n" % REPO)
    f = tmp_path / "run.py"
    f.write_text(script)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    out = str(tmp_path / "dist.txt")
    procs = [subprocess.Popen([sys.executable, str(f)] + flags + ["-o", out], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-3000:]
    native = str(tmp_path / "native.txt")
    ok, _, a = C.parse_sp_cmdline(["spsearch"] + flags + ["-o", native])
    res = C.run_sp_pipeline(a)
    C.write_sp_output(native, a, res)
    assert len(res.candidates) > 0 and _lines(out) == _lines(native)
