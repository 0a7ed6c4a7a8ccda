"""jerksearch without a GPU: the oracle's own properties, the host steps through
the bindings against the oracle (plan, gather, distillation), every refusal by
name, the command line, the unchanged generator and numerics id, and the native
host unit tests plain and under ASan / UBSan."""
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import write_filterbank
from peasoup_amd.utils.synthetic import PulsarSpec

C_LIGHT = 299792458.0
S3 = 12.0 * math.sqrt(3.0)


def _rows(nrows, stride, seed):
    return np.random.default_rng(seed).integers(0, 256, (nrows, stride), dtype=np.uint8)


# ------------------------------------------------------------ the oracle ----
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4101, 65539])
def test_oracle_identity_and_fixed_points(n):
    x = _rows(1, n + 37, n)[0]
    for jf in (0.0, 0.4 * S3 / n ** 3, -0.4 * S3 / n ** 3):
        i = np.arange(n, dtype=np.float64)
        g = ((i * (i - n // 2)) * (i - n)) * jf
        assert np.max(np.abs(g)) < 0.5
        np.testing.assert_array_equal(ref.jerk_resample(x, n, jf), x)
    # y = x at 0, h and n - 1 whenever |g| < 0.5 there: always at 0 and h (g = 0), and at n - 1 up to half the
    # driver's refusal limit (|g(n - 1)| < |jf| n^2 / 2); beyond it the last sample may move by one
    for jf in (0.9 / n ** 2, -0.9 / n ** 2, 1.8 / n ** 2, -1.8 / n ** 2, 40.0 * S3 / n ** 3):
        if abs(jf) * n * n / 2 > 0.9:
            continue
        s = ref.jerk_shift(n, jf)
        y = ref.jerk_resample(x, n, jf)
        last = abs(float(n - 1) * float(n - 1 - n // 2) * jf)
        assert last < 0.5 or abs(jf) * n * n / 2 > 0.45
        for i, g in ((0, 0.0), (n // 2, 0.0), (n - 1, last)):
            if g < 0.5:
                assert s[i] == 0 and y[i] == x[i]
        np.testing.assert_array_equal(y[n:], x[n:])


@pytest.mark.parametrize("n", [16, 17, 4101, 65539, 1 << 20])
def test_oracle_shift_bound(n):
    """max|s| <= ceil(|jf| n^3 / (12 sqrt 3)) + 1.  n^3 / (12 sqrt 3) is the extremum of i (i - n/2)(i - n); for odd
    n the middle root is h = (n - 1) / 2 and the cubic differs by i (i - n) / 2, at most n^2 / 8.  So the bound
    holds for every factor when n is even, and for odd n when |jf| n^2 / 8 < 1 - which the driver's refusal rule
    |jf| n^2 / 2 <= 0.9 guarantees; the bound with the n^2 / 8 term holds always."""
    for m in (0.4, 3.0, 40.0, 1000.0):
        for jf in (m * S3 / n ** 3, -m * S3 / n ** 3):
            s = ref.jerk_shift(n, jf)
            assert s.dtype == np.int64
            assert np.max(np.abs(s)) <= math.ceil(abs(jf) * (n ** 3 / S3 + n * n / 8.0)) + 1
            if n % 2 == 0 or abs(jf) * n * n / 2 <= 0.9:
                assert np.max(np.abs(s)) <= math.ceil(abs(jf) * n ** 3 / S3) + 1
    for jf in (1.8 / n ** 2, -1.8 / n ** 2):  # the largest factors the driver admits
        assert np.max(np.abs(ref.jerk_shift(n, jf))) <= math.ceil(abs(jf) * n ** 3 / S3) + 1


def test_oracle_half_to_even_and_clamps():
    n = 4096
    s = ref.jerk_shift(n, 0.0625)
    assert s[2] == 2 * 2046 * 4094 // 16 and s[2] % 2 == 0      # 1047064.5 -> the even neighbour
    assert 2 * 2046 * 4094 % 16 == 8
    x = _rows(1, n, 1)[0]
    y = ref.jerk_resample(x, n, 0.0625)
    assert y[1000] == x[n - 1] and y[3000] == x[0]
    assert ref.jerk_factor(0.0, 64e-6) == 0.0
    jf = ref.jerk_factor(0.1, 64e-6)
    assert jf == ((float(np.float32(0.1)) * float(np.float32(64e-6))) * float(np.float32(64e-6))) / (6 * C_LIGHT)
    assert C.jerk_factor(0.1, 64e-6) == jf
    assert C.jerk_freq_factor(2.5, 1 << 20, 64e-6) == ref.jerk_freq_factor(2.5, 1 << 20, 64e-6)


# ------------------------------------------------- the host transcription ----
@pytest.mark.parametrize("pad", [0, 37])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4101, 65539])
def test_host_gather_equals_oracle(n, pad):
    nrow = n + pad
    x = _rows(3, (nrow + 255) // 256 * 256, n + pad)
    jf = [s * m * S3 / float(n) ** 3 for m in (0.0, 0.4, 3.0, 40.0, 1000.0) for s in (1.0, -1.0)]
    y = C.jerk_resample_host(x, nrow, n, np.array(jf), nrow + 5)
    assert y.shape == (3, len(jf), nrow + 5) and np.all(y[:, :, nrow:] == 0)
    for r in range(3):
        for k, f in enumerate(jf):
            np.testing.assert_array_equal(y[r, k, :nrow], ref.jerk_resample(x[r, :nrow], n, f))
            assert [C.jerk_shift(i, n, f) for i in (0, n // 3, n - 1)] == ref.jerk_shift(n, f)[[0, n // 3, n - 1]].tolist()


def test_host_gather_exact_halves():
    x = _rows(2, 4096, 4)
    y = C.jerk_resample_host(x, 4096, 4096, np.array([0.0625, -0.0625]))
    for r in range(2):
        for k, f in enumerate((0.0625, -0.0625)):
            np.testing.assert_array_equal(y[r, k], ref.jerk_resample(x[r], 4096, f))


# ----------------------------------------------------------------- plan ----
PLAN = dict(tol=1.1, step=0.0, pulse_width=64.0, n=1 << 23, tsamp=64e-6, cfreq=1400.0, bw=-0.5)


def _plan(lo, hi, **kw):
    a = dict(PLAN, **kw)
    return C.JerkPlan(lo, hi, a["tol"], a["step"], a["pulse_width"], a["n"], a["tsamp"], a["cfreq"], a["bw"])


def _oracle_plan(lo, hi, dm, **kw):
    a = dict(PLAN, **kw)
    return ref.jerk_plan(lo, hi, a["tol"], a["step"], a["pulse_width"], a["n"], a["tsamp"], a["cfreq"], a["bw"], dm)


@pytest.mark.parametrize("lo,hi,kw", [(-1.0, 1.0, {}), (-0.3, 2.0, {}), (0.3, 1.0, {}), (-2.0, -0.4, {}),
                                      (0.0, 1.25, dict(step=0.25)), (-1.0, 1.0, dict(n=1 << 22, cfreq=350.0, bw=-0.39)),
                                      (0.7, 0.7, {}), (0.0, 0.0, {})])
def test_plan_equals_oracle(lo, hi, kw):
    for dm in (0.0, 30.0, 900.0):
        got = np.asarray(_plan(lo, hi, **kw).generate(dm), dtype=np.float32)
        want = _oracle_plan(lo, hi, dm, **kw)
        np.testing.assert_array_equal(got, want)
        assert (0.0 in got) == (lo <= 0.0 <= hi)
        assert got[0] >= np.float32(lo) and got[-1] <= np.float32(hi)
        if lo == hi:
            assert got.tolist() == [float(np.float32(lo))]
        elif len(got) > 1:
            st = _plan(lo, hi, **kw).step(dm)
            assert got[0] - st < lo and got[-1] + st > hi
            np.testing.assert_allclose(np.diff(got.astype(np.float64)), st, rtol=1e-5)


def test_plan_step_is_the_definition():
    p = _plan(-1.0, 1.0)
    T = float(1 << 23) * float(np.float32(64e-6))
    for dm in (0.0, 500.0):
        w = p.width(dm)
        assert w == ref.jerk_width(dm, 64.0, 64e-6, 1400.0, -0.5)
        t = float(np.float32(1.1))
        assert p.step(dm) == ((2.0 * w) * math.sqrt(t * t - 1.0)) * ((72.0 * math.sqrt(3.0)) * C_LIGHT) / ((T * T) * T)
    # the same width the acceleration plan steps with
    ap = C.AccelPlan(-5.0, 5.0, 1.1, 64.0, 1 << 23, 64e-6, 1400.0, -0.5)
    tobs = float(np.float32(np.float32(1 << 23) * np.float32(64e-6)))
    w_from_acc = ap.step(500.0) * tobs * tobs / (2.0 * 24.0 * C_LIGHT * math.sqrt(t * t - 1.0))
    assert abs(w_from_acc / p.width(500.0) - 1) < 1e-6


# ------------------------------------------------------------- refusals ----
def _fil(tmp_path, nsamps=4096, name="small.fil", **kw):
    path = str(tmp_path / name)
    hdr = synthetic.make_header(nchans=8, nbits=8, tsamp=64e-6, **kw)
    synthetic.write(path, nsamps, hdr, (), seed=0)
    return path


def _args(path, extra):
    ok, _, a = C.parse_jerk_cmdline(["jerksearch", "-i", path] + [str(e) for e in extra])
    assert ok
    return a


def test_every_refusal_is_raised_by_name(tmp_path):
    path = _fil(tmp_path)
    dm = ["--dm_start", 0, "--dm_end", 0]
    ok = C.jerk_setup(_args(path, dm + ["--jerk_start", -1, "--jerk_end", 1, "--jerk_step", 0.5]))
    assert ok.jerks == [[-1.0, -0.5, 0.0, 0.5, 1.0]] and ok.span == min(ok.nrow, ok.fft_size) and ok.total_trials == 5
    with pytest.raises(RuntimeError, match="jerk_start > jerk_end"):
        C.jerk_setup(_args(path, dm + ["--jerk_start", 2, "--jerk_end", 1]))
    for flag in ("--jerk_start", "--jerk_end", "--jerk_tol", "--jerk_step"):
        for bad in ("inf", "-inf", "nan"):
            with pytest.raises(RuntimeError, match="non-finite"):
                C.jerk_setup(_args(path, dm + [flag, bad]))
    with pytest.raises(RuntimeError, match="more than 4096 jerk trials"):
        C.jerk_setup(_args(path, dm + ["--jerk_end", 4096, "--jerk_step", 1]))
    assert len(C.jerk_setup(_args(path, dm + ["--jerk_end", 4095, "--jerk_step", 1])).jerks[0]) == 4096
    # |jf| n^2 / 2 > 0.9: jerk > 1.8 * 6c / (n tsamp)^2
    n = ok.span
    edge = 1.8 * 6 * C_LIGHT / (n * float(np.float32(64e-6))) ** 2
    C.jerk_setup(_args(path, dm + ["--jerk_start", repr(0.99 * edge), "--jerk_end", repr(0.99 * edge)]))
    with pytest.raises(RuntimeError, match="0.9 samples per sample"):
        C.jerk_setup(_args(path, dm + ["--jerk_start", repr(1.01 * edge), "--jerk_end", repr(1.01 * edge)]))
    with pytest.raises(RuntimeError, match="0.9 samples per sample"):
        C.jerk_setup(_args(path, dm + ["--jerk_start", repr(-1.01 * edge), "--jerk_end", 0, "--jerk_step",
                                       repr(1.01 * edge)]))
    with pytest.raises(RuntimeError, match="no trial"):
        C.jerk_setup(_args(path, dm + ["--jerk_start", 0.1, "--jerk_end", 0.2, "--jerk_step", 1]))
    # n > 2^26, from the header alone (the data block of this file is sparse and never read)
    big = str(tmp_path / "big.fil")
    hdr = synthetic.make_header(nchans=8, nbits=1, tsamp=64e-6)
    hdr["nsamples"] = (1 << 26) + 4096
    write_filterbank(big, hdr, np.zeros((0, 8), dtype=np.uint8))
    with open(big, "r+b") as f:
        f.truncate(os.path.getsize(big) + hdr["nsamples"])
    with pytest.raises(RuntimeError, match="longer than 2\\^26"):
        C.jerk_setup(_args(big, dm + ["--fft_size", 1 << 27]))
    assert C.jerk_setup(_args(big, dm + ["--fft_size", 1 << 26])).span == 1 << 26
    # the checks themselves
    with pytest.raises(RuntimeError, match="longer than 2\\^26"):
        C.jerk_check((1 << 26) + 1, np.zeros(1))
    with pytest.raises(RuntimeError, match="non-finite"):
        C.jerk_check(1024, np.array([np.inf]))
    with pytest.raises(ValueError, match="0.9 samples"):
        ref.jerk_check(1024, [1.81 / 1024 ** 2])
    with pytest.raises(ValueError, match="jerk_start > jerk_end"):
        _oracle_plan(1.0, -1.0, 0.0)
    with pytest.raises(ValueError, match="more than 4096"):
        _oracle_plan(0.0, 4096.0, 0.0, step=1.0)


# --------------------------------------------------------- distillation ----
def _hand_made():
    """(freq, acc, snr, jerk, nh).  0 and 1 differ only in jerk; 2 is outside the plain tolerance of 0 but inside
    the one widened by its jerk difference; 3 lies as far off at the same jerk and survives; 4 and 5 are a pair
    outside the widened tolerance that must both survive; 6 is related through the acceleration sweep; 7 equals 4
    in S/N (the sort is stable)."""
    tobs = float(np.float32(536.870912))
    return [(100.0, 0.0, 50.0, 0.0, 0), (100.0, 0.0, 40.0, 1.0, 1), (100.02, 0.0, 30.0, 4.0, 0),
            (100.02, 0.0, 29.0, 0.0, 0), (200.0, 0.0, 20.0, 0.0, 2), (200.1, 0.0, 19.0, 2.0, 0),
            (100.0 - 100.0 * 5.0 * tobs / C_LIGHT * 0.5, 5.0, 10.0, 0.0, 0), (300.0, -3.0, 20.0, 0.5, 3)]


@pytest.mark.parametrize("keep", [True, False])
def test_jerk_distill_equals_oracle(keep):
    tobs, T, tol = 536.870912, 536.870912, 1e-4
    rows = _hand_made()
    native = C.jerk_distill([C.JerkCandidate(C.Candidate(10.0, 3, a, nh, s, f), j) for f, a, s, j, nh in rows], tobs, T,
                            tol, keep)
    oracle = ref.jerk_distill([(ref.Cand(10.0, 3, ref.f32(a), nh, ref.f32(s), ref.f32(f)), ref.f32(j))
                               for f, a, s, j, nh in rows], tobs, T, tol, keep)
    assert len(native) == len(oracle) == 5
    for g, (w, wj) in zip(native, oracle):
        assert (g.cand.freq, g.cand.acc, g.cand.snr, g.cand.nh, g.jerk) == (w.freq, w.acc, w.snr, w.nh, wj)
        assert [(c.freq, c.snr) for c in g.cand.assoc] == [(c.freq, c.snr) for c in w.assoc]
    snrs = [g.cand.snr for g in native]
    assert snrs == [50.0, 29.0, 20.0, 20.0, 19.0]
    assert [g.cand.nh for g in native][2:4] == [2, 3]                 # equal S/N: input order
    assert (native[4].jerk, native[2].jerk) == (2.0, 0.0)             # the pair outside the widened tolerance
    assert len(native[0].cand.assoc) == (3 if keep else 0)


def test_jerk_distill_with_one_trial_is_the_acceleration_distiller():
    rng = np.random.default_rng(3)
    tobs, tol = float(np.float32(41.9)), 1e-4
    cands = [C.Candidate(20.0, 0, float(rng.choice([-50.0, 0.0, 50.0])), int(rng.integers(0, 4)),
                         float(np.float32(rng.uniform(9, 40))), float(np.float32(rng.choice([50.0, 50.001, 77.0, 99.0])
                                                                                  * rng.choice([1.0, 1.00005]))))
             for _ in range(60)]
    first = C.AccelerationDistiller(tobs, tol, True).distill(cands)
    assert 2 < len(first) < 60
    again = C.jerk_distill([C.JerkCandidate(c, 1.5) for c in first], tobs, 40.0, tol, True)
    assert [(g.cand.freq, g.cand.acc, g.cand.snr, g.cand.nh, g.cand.count_assoc()) for g in again] == \
           [(c.freq, c.acc, c.snr, c.nh, c.count_assoc()) for c in first]


def test_global_distill_carries_the_jerk_through_the_distillers(tmp_path):
    """jerk_global_distill sends the wrapped candidates through the existing DM and harmonic distillers and the
    scorer, which reorder and nest whole candidates; the wrapper's index rides in Candidate.opt_period (unused until
    a fold) and is cleared afterwards.  Pinned here: the survivors are exactly global_distill_and_score's on the
    bare candidates, each with the jerk it came in with, and no opt_period is left behind, nested ones included."""
    path = _fil(tmp_path, nsamps=8192)
    args = _args(path, ["--dm_start", 0, "--dm_end", 60, "--dm_tol", 1.3, "--jerk_start", -1, "--jerk_end", 1,
                        "--jerk_step", 0.5])
    setup = C.jerk_setup(args)
    dms = setup.dm_list
    assert len(dms) >= 4
    rng = np.random.default_rng(11)
    rows = []
    for d in range(len(dms)):
        for f in (40.0, 40.0005, 80.0, 77.7, 123.4 + d, 13.3333):      # harmonics, DM repeats and loners
            rows.append((float(np.float32(dms[d])), d, float(rng.choice([-5.0, 0.0, 5.0])), int(rng.integers(0, 4)),
                         float(np.float32(rng.uniform(9, 60))), float(np.float32(f))))
    # a jerk that is a function of the candidate, so that a mix-up shows
    jerk_of = {(r[1], r[4], r[5]): float(np.float32(0.25 * (k % 9) - 1.0)) for k, r in enumerate(rows)}
    assert len(jerk_of) == len(rows)
    wrapped = [C.JerkCandidate(C.Candidate(*r), jerk_of[(r[1], r[4], r[5])]) for r in rows]
    got = C.jerk_global_distill(wrapped, args, setup)
    hdr = C.read_header(path)
    want = C.global_distill_and_score([C.Candidate(*r) for r in rows], args.search, hdr)
    assert 2 < len(got) < len(rows) and len(got) == len(want)
    nested = 0

    def clean(c):
        return c.opt_period == 0.0 and all(clean(a) for a in c.assoc)

    for g, w in zip(got, want):
        assert (g.cand.dm_idx, g.cand.snr, g.cand.freq, g.cand.acc, g.cand.nh) == (w.dm_idx, w.snr, w.freq, w.acc, w.nh)
        assert g.cand.count_assoc() == w.count_assoc()
        assert (g.cand.is_adjacent, g.cand.is_physical, g.cand.ddm_count_ratio) == \
               (w.is_adjacent, w.is_physical, w.ddm_count_ratio)
        assert g.jerk == jerk_of[(g.cand.dm_idx, g.cand.snr, g.cand.freq)]
        assert clean(g.cand)
        nested += g.cand.count_assoc()
    assert nested > 0 and len({g.jerk for g in got}) > 2


# ------------------------------------------------------------------- CLI ----
def test_cli_parsing():
    ok, exit_now, a = C.parse_jerk_cmdline(["jerksearch", "-i", "x.fil"])
    assert ok and not exit_now
    assert (a.jerk_start, a.jerk_end, a.jerk_step) == (0.0, 0.0, 0.0) and a.jerk_tol == float(np.float32(1.1))
    ok, _, p = C.parse_cmdline(["peasoup", "-i", "x.fil"])
    for f in ("dm_start", "dm_end", "dm_tol", "dm_pulse_width", "acc_start", "acc_end", "acc_tol", "acc_pulse_width",
              "nharmonics", "min_snr", "min_freq", "max_freq", "size", "npdmp", "limit", "dedisp_kernel",
              "accel_convention", "verbose", "killfilename", "zapfilename"):
        assert getattr(a.search, f) == getattr(p, f), f
    assert re.fullmatch(r"\d{4}-\d\d-\d\d-\d\d:\d\d_jerksearch\.output", a.outfilename)
    ok, _, b = C.parse_jerk_cmdline(
        ["jerksearch", "-i", "x.fil", "-o", "o.txt", "-k", "k", "-z", "z", "--dm_start", "1", "--dm_end", "2", "--dm_tol",
         "1.2", "--dm_pulse_width", "40", "--acc_start", "-5", "--acc_end", "5", "--acc_tol", "1.3",
         "--acc_pulse_width", "32", "-n", "3", "-m", "7", "--min_freq", "1", "--max_freq", "900", "--fft_size", "65536",
         "--npdmp", "4", "--limit", "10", "--dedisp_kernel", "valu", "--accel_convention", "reference", "-v",
         "--jerk_start", "-2.5", "--jerk_end=3", "--jerk_tol", "1.2", "--jerk_step", "0.5"])
    assert ok and b.outfilename == "o.txt" and (b.jerk_start, b.jerk_end, b.jerk_step) == (-2.5, 3.0, 0.5)
    s = b.search
    assert (s.killfilename, s.zapfilename, s.dm_start, s.dm_end, s.acc_start, s.acc_end, s.nharmonics, s.min_snr,
            s.min_freq, s.max_freq, s.size, s.npdmp, s.limit, s.dedisp_kernel, s.accel_convention, s.verbose) == \
           ("k", "z", 1.0, 2.0, -5.0, 5.0, 3, 7.0, 1.0, 900.0, 65536, 4, 10, "valu", "reference", True)
    assert not C.parse_jerk_cmdline(["jerksearch"])[0]
    assert not C.parse_jerk_cmdline(["jerksearch", "-i", "x.fil", "--jerk_end", "1x"])[0]
    assert not C.parse_jerk_cmdline(["jerksearch", "-i", "x.fil", "-t", "2"])[0]              # one device
    assert not C.parse_jerk_cmdline(["jerksearch", "-i", "x.fil", "--checkpoint_dir", "c"])[0]  # no checkpoints
    assert C.parse_jerk_cmdline(["jerksearch", "--help"])[1]


def test_output_text(tmp_path):
    path = _fil(tmp_path)
    args = _args(path, ["--dm_start", 0, "--dm_end", 0, "--jerk_start", -1, "--jerk_end", 1, "--jerk_step", 0.5, "-o",
                        str(tmp_path / "o.txt")])
    setup = C.jerk_setup(args)
    c = C.Candidate(0.0, 0, 2.5, 2, 12.5, 100.0)
    c.folded_snr = 14.0
    text = C.jerk_output_text(args, setup, [C.JerkCandidate(c, 1.0), C.JerkCandidate(C.Candidate(0.0, 0, 0.0, 0, 11.0, 50.0), 0.0)])
    head = [ln for ln in text.splitlines() if ln.startswith("#")]
    rows = [ln.split() for ln in text.splitlines() if not ln.startswith("#")]
    assert head[-1] == "# period_s dm acc jerk freq nh snr folded_snr dm_idx"
    assert any("jerk_start -1 jerk_end 1" in ln for ln in head) and any(": 5 -1 1" in ln for ln in head)
    assert any("mid-span" in ln for ln in head) and any("1 + jerk T^2 / (12 c)" in ln for ln in head)
    k = ref.jerk_freq_factor(1.0, setup.span, 64e-6)
    assert float(rows[0][4]) == pytest.approx(100.0 / k, rel=1e-11) and float(rows[0][0]) == pytest.approx(k / 100.0, rel=1e-11)
    assert [float(v) for v in rows[0][1:4]] == [0.0, 2.5, 1.0] and rows[0][5:] == ["2", "12.5", "14", "0"]
    assert [float(v) for v in rows[1][:5]] == [0.02, 0.0, 0.0, 0.0, 50.0]
    C.write_jerk_output(args, setup, [])
    assert os.path.exists(args.outfilename) and not os.path.exists(args.outfilename + ".tmp")


# ------------------------------------------------- what must not change ----
def test_generator_is_unchanged_at_zero_jerk():
    """PulsarSpec(jerk=0) and a PulsarSpec built without the field give the bytes the parent's generator gave: the
    same expression runs (the parent's phase line, kept verbatim for jerk == 0)."""
    hdr = synthetic.make_header(nchans=16, nbits=8, tsamp=256e-6)
    base = dict(period=0.0101, dm=20.0, duty=0.05, amplitude=0.8, accel=35.0, phase=0.3)
    without = synthetic.generate(20000, hdr, [PulsarSpec(**base)], seed=7)
    with_zero = synthetic.generate(20000, hdr, [PulsarSpec(jerk=0.0, **base)], seed=7)
    np.testing.assert_array_equal(without, with_zero)
    assert [f.name for f in dataclasses.fields(PulsarSpec)][-1] == "jerk" and PulsarSpec().jerk == 0.0
    # the parent's expression, written out
    rng = np.random.default_rng(7)
    x = rng.standard_normal((20000, 16)).astype(np.float32)
    freqs = hdr["fch1"] + hdr["foff"] * np.arange(16)
    te = (np.arange(20000, dtype=np.float64) * hdr["tsamp"])[:, None] - \
        (4.15e3 * 20.0 * (1.0 / freqs ** 2 - 1.0 / hdr["fch1"] ** 2))[None, :]
    ph = (te - 35.0 * te * te / (2 * C_LIGHT)) / 0.0101 + 0.3
    ph = ph - np.floor(ph)
    x += 0.8 * np.exp(-0.5 * (np.minimum(ph, 1.0 - ph) / (0.05 / 2.3548)) ** 2).astype(np.float32)
    np.testing.assert_array_equal(without, np.clip(np.rint(127.5 + 63.75 * x), 0, 255).astype(np.uint8))
    # and the jerk term does something: the phase differs by jerk te^3 / (6 c P)
    jerked = synthetic.generate(20000, hdr, [PulsarSpec(jerk=5e5, **base)], seed=7)
    assert np.any(jerked != without)


def _numerics_id(include=()):
    """cmake/numerics_id.cmake over the sources CMakeLists.txt lists for it; ``include`` names excluded headers to
    hash all the same."""
    import glob
    import hashlib

    with open(os.path.join(REPO, "CMakeLists.txt")) as f:
        cm = f.read()
    hip = re.search(r"set\(PSOUP_HIP_SOURCES\s+([^)]*)\)", cm).group(1).split()
    num = re.search(r"set\(PSOUP_NUMERICS_SOURCES \$\{PSOUP_HIP_SOURCES\}([^)]*)\)", cm).group(1).split()
    skip = set(re.findall(r'EXCLUDE REGEX "/(\w+)\\\\\.hpp\$"', cm)) - set(include)
    heads = sorted(h for pat in ("csrc/kernels/*.hpp", "csrc/include/psoup/*.hpp")
                   for h in glob.glob(os.path.join(REPO, pat))
                   if os.path.basename(h)[:-4] not in skip or pat.startswith("csrc/kernels"))
    acc = ""
    for src in [os.path.join(REPO, x) for x in hip + num] + heads:
        with open(src, "rb") as f:
            acc += hashlib.sha256(f.read()).hexdigest()
    return hashlib.sha256(acc.encode()).hexdigest()[:16], hip + num, skip


def test_numerics_id_does_not_depend_on_the_jerk_sources():
    """The id in the generated header is the hash of the numerics sources alone: no jerk file is among them and
    jerk.hpp is excluded from the header glob, so the id is what the parent commit's build gives (recorded in
    profiles/jerk/SUMMARY.md) and earlier checkpoint spills stay resumable."""
    gen = os.path.join(REPO, "build", "gen", "psoup_numerics_id.hpp")
    if not os.path.exists(gen):
        from peasoup_amd import _build

        _build.build()
    with open(gen) as f:
        ids = re.findall(r'#define PSOUP_NUMERICS_ID "([0-9a-f]{16})"', f.read())
    want, sources, skip = _numerics_id()
    assert ids == [want]
    assert "jerk" in skip and not any("jerk" in s for s in sources)
    # were jerk.hpp inside the glob, the id would differ: the exclusion is what keeps it
    assert _numerics_id(include=("jerk",))[0] != want


# ------------------------------------------------- native host unit tests ----
def _run_native(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    return r


def test_native_jerk_unit_tests():
    _run_native(os.path.join(REPO, "bin", "psoup_jerk_unit_tests"))


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_jerk_unit_tests_under_host_sanitizers(san):
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_jerk_unit_tests")
    r = _run_native(os.path.join(REPO, "bin", f"psoup_jerk_unit_tests_{san}"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
