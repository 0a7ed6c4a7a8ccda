"""orbsearch without a GPU: the sine table against the oracle's, the host steps
through the bindings against the oracle (quantisation, shift, gather, bank,
grid, distillation), every refusal by name, the command line, the generator's
orbit and the native host unit tests."""
import hashlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import orbit_cases as oc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.synthetic import PulsarSpec

TS = oc.TS


# ------------------------------------------------------------ sine table ----
def test_sine_table_equals_oracle():
    got, want = np.asarray(C.orbit_sine_table()), ref.orbit_sine_table()
    assert got.dtype == np.int32 and got.shape == (4097,)
    np.testing.assert_array_equal(got, want)
    assert got[1024] == 1 << 30 and got[3072] == -(1 << 30) and got[0] == got[2048] == got[4096] == 0
    np.testing.assert_array_equal(got[2048::-1], got[:2049])
    np.testing.assert_array_equal(got[2048:], -got[:2049])
    # NumPy's own double sine gives the same table (it may differ from the C library's in the last bit of a double,
    # never in the Q30 rounding), and the table is pinned so that it cannot drift between machines
    j = np.arange(1025, dtype=np.float64)
    np.testing.assert_array_equal(np.rint(np.ldexp(np.sin(j * (np.pi / 2048)), 30)).astype(np.int32), got[:1025])
    assert got[1] == 1647099 and got[512] == 759250125
    assert hashlib.sha256(got.astype("<i4").tobytes()).hexdigest()[:16] == TABLE_SHA


TABLE_SHA = "f8448633b4e69328"


# ------------------------------------------------- quantisation and shift ----
EDGE_PHASES = [0.0, 0.25, 0.75, 1.0 - 2.0 ** -60, -1e-20, 1.0 - 2.0 ** -53, -0.25, 7.5, -3.37]


def test_quantise_and_shift_equal_oracle():
    rng = np.random.default_rng(1)
    cases = [(float(10 ** rng.uniform(-1.5, 5)), float(rng.uniform(0, 2) * 10 ** rng.uniform(-4, 0)),
              float(rng.uniform(-3, 3))) for _ in range(200)]
    cases += [(3600.0, 1.5, ph) for ph in EDGE_PHASES]
    cases += [(64.0 * TS, 0.01, 0.37), (1e9, (1073741823.0 / 256.0) * TS, 0.1)]
    for pb, a1, ph in cases:
        q = tuple(C.orbit_quantise(pb, a1, ph, TS))
        assert q == ref.orbit_quantise(pb, a1, ph, TS), (pb, a1, ph)
        assert 0 <= q[0] <= 1 << 58 and 0 <= q[1] < 1 << 64 and 0 <= q[2] < 1 << 30
        np.testing.assert_array_equal(np.asarray(C.orbit_shifts(q, 3000)), ref.orbit_shift(3000, q))
        assert C.orbit_shift(q, 2999) == ref.orbit_shift(3000, q)[2999] and C.orbit_shift(q, 0) == 0
    assert C.orbit_quantise(64.0 * TS, 0.0, 0.0, TS) == (1 << 58, 0, 0)
    assert C.orbit_quantise(1e9, (1073741823.0 / 256.0) * TS, 0.0, TS)[2] == (1 << 30) - 1
    assert [C.orbit_quantise(3600.0, 0.0, ph, TS)[1] for ph in EDGE_PHASES[:5]] == [0, 1 << 62, 3 << 62, 0, 0]
    assert C.orbit_quantise(3600.0, 0.0, 1.0 - 2.0 ** -53, TS)[1] == (1 << 64) - 2048
    from peasoup_amd import ops

    assert ops.orbit_quantise([(3600.0, 1.5, 0.25)], 320e-6) == [ref.orbit_quantise(3600.0, 1.5, 0.25, TS)]


def test_shift_is_the_roemer_delay_in_samples():
    """s(i) is within half a sample (and the table's 1e-6) of a1 / tsamp [sin 2 pi (i tsamp / pb + ph) - sin 2 pi ph]."""
    n, pb, amp, ph = 65539, 30000.0, 40.0, 0.37
    s = ref.orbit_shift(n, oc.quant(pb, amp, ph))
    i = np.arange(n, dtype=np.float64)
    want = amp * (np.sin(2 * np.pi * (i / pb + ph)) - np.sin(2 * np.pi * ph))
    assert s.dtype == np.int64 and np.max(np.abs(s - want)) < 0.5 + 1e-3
    # a1 = 0 is the identity at any phase; 0.4 samples is where |sin - sin 2 pi ph| stays below 1.25, as from phase 0
    assert np.all(ref.orbit_shift(n, oc.quant(pb, 0.0, ph)) == 0) and np.all(ref.orbit_shift(n, oc.quant(pb, 0.4, 0.0)) == 0)
    assert np.any(ref.orbit_shift(n, oc.quant(pb, 0.4, ph)) != 0)


# ------------------------------------------------- the host transcription ----
@pytest.mark.parametrize("n,pad", oc.SHAPES)
def test_host_gather_equals_oracle(n, pad):
    nrow = n + pad
    x = oc.rows(3, (nrow + 255) // 256 * 256, n + pad)
    for tpl in oc.groups(oc.templates(n)):
        y = C.orbit_resample_host(x, nrow, n, tpl, nrow + 5)
        assert y.shape == (3, len(tpl), nrow + 5) and np.all(y[:, :, nrow:] == 0)
        oc.check_rows(y[:, :, :nrow], x, nrow, n, tpl)


def test_host_gather_special_cases():
    q, i0 = oc.turning_case()
    x = oc.rows(2, 65539, 3)
    oc.check_rows(C.orbit_resample_host(x, 65539, 65539, [q]), x, 65539, 65539, [q])
    qc = oc.clamp_case()
    x = oc.rows(2, 4096, 4)
    oc.check_rows(C.orbit_resample_host(x, 4096, 4096, [qc]), x, 4096, 4096, [qc])
    qh, hits = oc.exact_half_case()
    x = oc.rows(2, 8192, 5)
    oc.check_rows(C.orbit_resample_host(x, 8192, 8192, [qh]), x, 8192, 8192, [qh])
    with pytest.raises(RuntimeError, match="span"):
        C.orbit_resample_host(x, 8192, 9000, [qh])
    with pytest.raises(RuntimeError, match="templates per launch"):
        C.orbit_resample_host(x, 8192, 8192, [])
    with pytest.raises(RuntimeError, match="Aq >= 2\\^30"):
        C.orbit_resample_host(x, 8192, 8192, [(1, 0, 1 << 30)])
    with pytest.raises(RuntimeError, match="pb < 64 tsamp"):
        C.orbit_resample_host(x, 8192, 8192, [((1 << 58) + 1, 0, 0)])


# -------------------------------------------------------- bank and grid ----
BANK = """# pb_s a1_ls phase
3600 1.5 0.25

  7200.5\t0 0.5 a fourth column # and a comment
   # only a comment
1e3 2e-3 -0.125"""


def test_bank_parser_equals_oracle():
    got = C.orbit_parse_bank(BANK)
    assert got == ref.orbit_parse_bank(BANK) == [(3600.0, 1.5, 0.25), (7200.5, 0.0, 0.5), (1000.0, 0.002, -0.125)]
    assert C.orbit_parse_bank("# nothing\n\n") == ref.orbit_parse_bank("# nothing\n\n") == []
    for text, ln in (("3600 1 0\n3600 1\n", 2), ("3600 1 0\n\n# c\n3600 x 0\n", 4), ("3600 1.0.0 0", 1)):
        with pytest.raises(RuntimeError, match=f"bank line {ln} is malformed"):
            C.orbit_parse_bank(text)
        with pytest.raises(ValueError, match=f"bank line {ln} is malformed"):
            ref.orbit_parse_bank(text)


def test_grid_order_equals_oracle():
    args = (40.0, 90.0, 3, 0.0, 0.0144, 4, 4)
    got = C.orbit_grid(*args)
    assert got == ref.orbit_grid(*args) and len(got) == 48
    # pb slowest, phase fastest
    assert [t[2] for t in got[:5]] == [0.0, 0.25, 0.5, 0.75, 0.0]
    assert [t[1] for t in got[:16:4]] == [0.0, 0.0144 * (1.0 / 3.0), 0.0144 * (2.0 / 3.0), 0.0144]
    assert [t[0] for t in got[::16]] == [40.0, 60.0, 90.0]      # geometric: sqrt(40 * 90) = 60
    assert C.orbit_grid(50.0, 60.0, 1, 0.1, 0.2, 1, 1) == ref.orbit_grid(50.0, 60.0, 1, 0.1, 0.2, 1, 1) == [(50.0, 0.1, 0.0)]
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = (float(rng.uniform(10, 100)), float(rng.uniform(100, 1e4)), int(rng.integers(1, 9)), float(rng.uniform(0, 1)),
             float(rng.uniform(1, 3)), int(rng.integers(1, 9)), int(rng.integers(1, 9)))
        assert C.orbit_grid(*a) == ref.orbit_grid(*a)
    for bad in ((1.0, 2.0, 0, 0.0, 1.0, 1, 1), (1.0, 2.0, 1, 0.0, 1.0, 1, -1)):
        with pytest.raises(RuntimeError, match="at least 1"):
            C.orbit_grid(*bad)
        with pytest.raises(ValueError, match="at least 1"):
            ref.orbit_grid(*bad)
    with pytest.raises(RuntimeError, match="more than 2\\^20 templates"):
        C.orbit_grid(1.0, 2.0, 1025, 0.0, 1.0, 1024, 1)


# --------------------------------------------------------- distillation ----
def _same(native, oracle):
    assert len(native) == len(oracle)
    for g, (w, wt) in zip(native, oracle):
        assert (g.cand.freq, g.cand.snr, g.cand.nh, g.tmpl) == (w.freq, w.snr, w.nh, wt)
        assert [(c.freq, c.snr) for c in g.cand.assoc] == [(c.freq, c.snr) for c in w.assoc]


@pytest.mark.parametrize("keep", [True, False])
def test_orbit_distill_equals_oracle(keep):
    beta = [0.0, 1e-3, 5e-3]
    # (freq, snr, template, nh): see csrc/tests/orbit_unit_tests.cpp for the hand-made list
    rows = [(100.0, 50.0, 0, 0), (100.005, 45.0, 0, 0), (100.1, 40.0, 1, 0), (100.2, 30.0, 1, 1), (100.7, 20.0, 2, 0),
            (300.0, 30.0, 2, 2)]
    native = C.orbit_distill([C.OrbitCandidate(C.Candidate(10.0, 3, 0.0, nh, s, f), t) for f, s, t, nh in rows], beta,
                             1e-4, keep)
    oracle = ref.orbit_distill([(ref.Cand(10.0, 3, 0.0, nh, ref.f32(s), ref.f32(f)), t) for f, s, t, nh in rows], beta,
                               1e-4, keep)
    _same(native, oracle)
    assert [g.cand.snr for g in native] == [50.0, 45.0, 30.0, 30.0] and [g.cand.nh for g in native][2:] == [1, 2]
    assert [len(g.cand.assoc) for g in native] == ([1, 1, 1, 0] if keep else [0, 0, 0, 0])


def test_orbit_distill_random_lists_equal_the_plain_scan():
    """The native distiller looks candidates up through a frequency-sorted index; the oracle is the plain scan."""
    rng = np.random.default_rng(9)
    bank = ref.orbit_grid(40.0, 4000.0, 5, 0.0, 0.05, 4, 2)
    beta = [ref.orbit_beta(pb, a1) for pb, a1, _ in bank]
    assert beta == [C.orbit_beta(pb, a1) for pb, a1, _ in bank] and max(beta) < 0.01
    for trial in range(4):
        rows = []
        for _ in range(400):
            f = float(np.float32(rng.choice([50.0, 50.3, 77.0, 99.0, 99.05]) * (1 + rng.normal(0, 2e-3))))
            rows.append((f, float(np.float32(rng.choice([10.0, 12.5, rng.uniform(9, 40)]))), int(rng.integers(0, 40)),
                         int(rng.integers(0, 4))))
        native = C.orbit_distill([C.OrbitCandidate(C.Candidate(10.0, 3, 0.0, nh, s, f), t) for f, s, t, nh in rows],
                                 beta, 1e-4, True)
        oracle = ref.orbit_distill([(ref.Cand(10.0, 3, 0.0, nh, s, f), t) for f, s, t, nh in rows], beta, 1e-4, True)
        assert 5 < len(native) < 400
        _same(native, oracle)


def test_orbit_distill_with_one_template_changes_nothing():
    rng = np.random.default_rng(3)
    cands = [C.OrbitCandidate(C.Candidate(20.0, 0, 0.0, int(rng.integers(0, 4)), float(np.float32(rng.uniform(9, 40))),
                                          float(np.float32(rng.choice([50.0, 50.001, 77.0])))), 0) for _ in range(60)]
    out = C.orbit_distill(cands, [0.01], 1e-4, True)
    order = sorted(range(60), key=lambda i: -cands[i].cand.snr)
    assert [(g.cand.freq, g.cand.snr, g.cand.nh, g.cand.count_assoc()) for g in out] == \
           [(cands[i].cand.freq, cands[i].cand.snr, cands[i].cand.nh, 0) for i in order]


# ------------------------------------------------------------- refusals ----
def _fil(tmp_path, nsamps=4096, name="small.fil"):
    path = str(tmp_path / name)
    hdr = synthetic.make_header(nchans=8, nbits=8, tsamp=320e-6)
    synthetic.write(path, nsamps, hdr, (), seed=0)
    return path


def _args(path, extra):
    ok, _, a = C.parse_orbit_cmdline(["orbsearch", "-i", path] + [str(e) for e in extra])
    assert ok
    return a


def test_every_refusal_is_raised_by_name(tmp_path):
    path = _fil(tmp_path)
    dm = ["--dm_start", 0, "--dm_end", 0]
    ok = C.orbit_setup(_args(path, dm + ["--bankfile", oc.bank_file(tmp_path, BANK, "ok.txt")]))
    assert ok.bank == ref.orbit_parse_bank(BANK) and ok.span == min(ok.nrow, ok.fft_size)
    assert ok.quant == [ref.orbit_quantise(pb, a1, ph, TS) for pb, a1, ph in ok.bank]
    assert ok.beta == [ref.orbit_beta(pb, a1) for pb, a1, _ in ok.bank]
    grid = C.orbit_setup(_args(path, dm + ["--pb_start", 40, "--pb_end", 90, "--npb", 3, "--a1_end", 0.0144, "--na1", 4,
                                           "--nphase", 4]))
    assert grid.bank == ref.orbit_grid(40.0, 90.0, 3, 0.0, 0.0144, 4, 4)
    for extra, what in oc.refusal_cases(tmp_path):
        with pytest.raises(RuntimeError, match=re.escape(what)):
            C.orbit_setup(_args(path, dm + extra))
    # the limits themselves
    C.orbit_setup(_args(path, dm + ["--bankfile", oc.bank_file(tmp_path, f"{64 * TS!r} 0 0\n100 {0.89 * 100 / (2 * math.pi)!r} 0\n",
                                                        "edge.txt")]))
    with pytest.raises(RuntimeError, match="0.9 samples per sample"):
        C.orbit_setup(_args(path, dm + ["--bankfile", oc.bank_file(tmp_path, f"100 {0.91 * 100 / (2 * math.pi)!r} 0\n", "e2.txt")]))
    # -t other than 1: the parser refuses it, and the setup does for options made by hand
    assert not C.parse_orbit_cmdline(["orbsearch", "-i", path, "-t", "2"])[0]
    a = _args(path, dm + ["--bankfile", oc.bank_file(tmp_path, "100 0 0\n", "one.txt")])
    a.search.max_num_threads = 2
    with pytest.raises(RuntimeError, match="one device"):
        C.orbit_setup(a)
    # n > 2^26
    big = oc.big_file(tmp_path)
    one = ["--bankfile", oc.bank_file(tmp_path, "100 0 0\n", "one.txt")]
    with pytest.raises(RuntimeError, match="longer than 2\\^26"):
        C.orbit_setup(_args(big, dm + one + ["--fft_size", 1 << 27]))
    assert C.orbit_setup(_args(big, dm + one + ["--fft_size", 1 << 26])).span == 1 << 26
    # the checks themselves, and the oracle's
    with pytest.raises(RuntimeError, match="longer than 2\\^26"):
        C.orbit_check((1 << 26) + 1, [(100.0, 0.0, 0.0)], TS)
    with pytest.raises(RuntimeError, match="empty bank"):
        C.orbit_check(1024, [], TS)
    for bank, what in (([(100.0, 0.0, float("nan"))], "non-finite"), ([(0.01, 0.0, 0.0)], "pb < 64 tsamp"),
                       ([(100.0, -1.0, 0.0)], "a1 < 0"), ([(1e9, 2000.0, 0.0)], "Aq >= 2\\^30"),
                       ([(100.0, 20.0, 0.0)], "0.9 samples"), ([], "empty bank")):
        with pytest.raises(ValueError, match=what):
            ref.orbit_check(1024, bank, TS)


# ------------------------------------------------------------------- CLI ----
def test_cli_parsing():
    ok, exit_now, a = C.parse_orbit_cmdline(["orbsearch", "-i", "x.fil"])
    assert ok and not exit_now
    assert (a.bankfile, a.npb, a.na1, a.nphase, a.pb_start, a.pb_end, a.a1_start, a.a1_end) == ("", 0, 0, 0, 0.0, 0.0, 0.0, 0.0)
    ok, _, p = C.parse_cmdline(["peasoup", "-i", "x.fil"])
    for f in ("dm_start", "dm_end", "dm_tol", "dm_pulse_width", "acc_start", "acc_end", "acc_tol", "acc_pulse_width",
              "nharmonics", "min_snr", "min_freq", "max_freq", "size", "npdmp", "limit", "dedisp_kernel",
              "accel_convention", "verbose", "killfilename", "zapfilename"):
        assert getattr(a.search, f) == getattr(p, f), f
    assert re.fullmatch(r"\d{4}-\d\d-\d\d-\d\d:\d\d_orbsearch\.output", a.outfilename)
    ok, _, b = C.parse_orbit_cmdline(
        ["orbsearch", "-i", "x.fil", "-o", "o.txt", "-k", "k", "-z", "z", "--dm_start", "1", "--dm_end", "2",
         "--acc_start", "-5", "--acc_end", "5", "-n", "3", "-m", "7", "--fft_size", "65536", "--npdmp", "4", "--limit",
         "10", "--dedisp_kernel", "valu", "-v", "--pb_start", "3600.25", "--pb_end=7200", "--npb", "3", "--a1_start",
         "0.5", "--a1_end", "1.5", "--na1", "2", "--nphase", "4", "--bankfile", "b.txt"])
    assert ok and (b.outfilename, b.bankfile) == ("o.txt", "b.txt")
    assert (b.pb_start, b.pb_end, b.npb, b.a1_start, b.a1_end, b.na1, b.nphase) == (3600.25, 7200.0, 3, 0.5, 1.5, 2, 4)
    s = b.search
    assert (s.killfilename, s.zapfilename, s.dm_start, s.dm_end, s.acc_start, s.acc_end, s.nharmonics, s.min_snr, s.size,
            s.npdmp, s.limit, s.dedisp_kernel, s.verbose) == ("k", "z", 1.0, 2.0, -5.0, 5.0, 3, 7.0, 65536, 4, 10, "valu", True)
    assert not C.parse_orbit_cmdline(["orbsearch"])[0]
    assert not C.parse_orbit_cmdline(["orbsearch", "-i", "x.fil", "--pb_end", "1x"])[0]
    assert not C.parse_orbit_cmdline(["orbsearch", "-i", "x.fil", "-t", "2"])[0]              # one device
    assert not C.parse_orbit_cmdline(["orbsearch", "-i", "x.fil", "--checkpoint_dir", "c"])[0]  # no checkpoints
    assert C.parse_orbit_cmdline(["orbsearch", "--help"])[1]


def test_output_text(tmp_path):
    path = _fil(tmp_path)
    args = _args(path, ["--dm_start", 0, "--dm_end", 0, "--bankfile", oc.bank_file(tmp_path, BANK), "-o", str(tmp_path / "o.txt")])
    setup = C.orbit_setup(args)
    c = C.Candidate(0.0, 0, 2.5, 2, 12.5, 100.0)
    c.folded_snr = 14.0
    text = C.orbit_output_text(args, setup, [C.OrbitCandidate(c, 1), C.OrbitCandidate(C.Candidate(0.0, 0, 0.0, 0, 11.0, 50.0), 2)])
    head = [ln for ln in text.splitlines() if ln.startswith("#")]
    rows = [ln.split() for ln in text.splitlines() if not ln.startswith("#")]
    assert head[-1] == "# period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx"
    assert any(ln.startswith("# templates 3 ") for ln in head) and any("bankfile " + args.bankfile in ln for ln in head)
    assert any("npb 0" in ln and "nphase 0" in ln for ln in head) and any("intrinsic" in ln for ln in head)
    assert [float(v) for v in rows[0]] == [0.01, 0.0, 2.5, 7200.5, 0.0, 0.5, 100.0, 2.0, 12.5, 14.0, 0.0]
    assert [float(v) for v in rows[1][:7]] == [0.02, 0.0, 0.0, 1000.0, 0.002, -0.125, 50.0]
    with pytest.raises(RuntimeError, match="outside the bank"):
        C.orbit_output_text(args, setup, [C.OrbitCandidate(c, 3)])
    C.write_orbit_output(args, setup, [])
    assert os.path.exists(args.outfilename) and not os.path.exists(args.outfilename + ".tmp")


# ----------------------------------------------------------- the generator ----
def _profile(series, period, nbins=32):
    ph = np.arange(len(series), dtype=np.float64) * TS / period
    b = np.floor((ph - np.floor(ph)) * nbins).astype(np.int64)
    return np.bincount(b, weights=series, minlength=nbins) / np.maximum(np.bincount(b, minlength=nbins), 1)


def test_generator_with_an_orbit():
    """The noise-free series of a pulsar on an orbit (the generator's output minus its output without the pulsar: the
    same noise draws, so what is left is the pulse train to within a count of rounding), re-indexed by the oracle at
    the true template and folded at P, against the same without the orbit: the peak-to-mean ratios agree within 5 %.
    The pulse is 0.1 P = 3.2 samples wide (sigma 1.34): a nearest-neighbour re-index adds a boxcar of one sample,
    variance 1/12, which lowers the peak of that Gaussian by 2.3 %; at a period of 31.6 samples and 32 bins the
    fold itself is the same for both."""
    ns, P = 1 << 17, 0.0101
    hdr = synthetic.make_header(nchans=2, nbits=8, tsamp=320e-6)
    orbit = (60.0, 30.0 * TS, 0.75)
    base = dict(period=P, dm=0.0, duty=0.1, amplitude=0.3)
    noise = synthetic.generate(ns, hdr, [], seed=2).astype(np.float64).sum(axis=1)
    plain = synthetic.generate(ns, hdr, [PulsarSpec(**base)], seed=2).astype(np.float64).sum(axis=1) - noise
    orb = synthetic.generate(ns, hdr, [PulsarSpec(orbit=orbit, **base)], seed=2).astype(np.float64).sum(axis=1) - noise
    q = ref.orbit_quantise(*orbit, TS)
    assert 29 <= np.max(np.abs(ref.orbit_shift(ns, q))) <= 60
    ratio = lambda s: (lambda p: p.max() / p.mean())(_profile(s, P))  # noqa: E731
    r_plain, r_orb, r_back = ratio(plain), ratio(orb), ratio(ref.orbit_resample(orb, ns, q))
    print(f"peak / mean: orbit-free {r_plain:.4f}, on the orbit {r_orb:.4f}, resampled at the true template {r_back:.4f}")
    assert r_plain > 5.0 and r_orb < 0.5 * r_plain        # the orbit smears the fold
    assert abs(r_back / r_plain - 1.0) < 0.05
    # None and a1 = 0 are the orbit-free generator
    zero = synthetic.generate(20000, hdr, [PulsarSpec(orbit=(60.0, 0.0, 0.3), **base)], seed=2)
    np.testing.assert_array_equal(zero, synthetic.generate(20000, hdr, [PulsarSpec(**base)], seed=2))
    assert PulsarSpec().orbit is None


def test_numerics_id_does_not_depend_on_the_orbit_sources():
    with open(os.path.join(REPO, "CMakeLists.txt")) as f:
        cm = f.read()
    num = re.search(r"set\(PSOUP_NUMERICS_SOURCES \$\{PSOUP_HIP_SOURCES\}([^)]*)\)", cm).group(1)
    hip = re.search(r"set\(PSOUP_HIP_SOURCES\s+([^)]*)\)", cm).group(1)
    assert "orbit" not in num and "orbit" not in hip
    assert 'EXCLUDE REGEX "/orbit\\\\.hpp$"' in cm


# ------------------------------------------------- native host unit tests ----
def test_native_orbit_unit_tests():
    r = subprocess.run([os.path.join(REPO, "bin", "psoup_orbit_unit_tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
