"""filinject (csrc/include/psoup/inject.hpp) without a GPU: the dither's
statistics from the oracle alone, the hash on hand-computed values, option
parsing, the injection file's parser and every refusal by name, the host tables
and the truth numbers through the bindings against the NumPy oracle, identities
of the oracle, and the native host unit tests with their sanitizer builds."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.synthetic import BurstSpec, PulsarSpec

L = C.inject_stat_block()


def _header(nchans=16, nbits=8, **kw):
    return synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=256e-6, **kw)


def _signals(sigs):
    from peasoup_amd.ops.core import _inject_signals

    return _inject_signals(sigs)


# ---------------------------------------------------------------- dither ----
def test_dither_statistics_of_the_oracle():
    """A constant E = 2^29 (a quarter of a level) over 2^20 samples of one channel: every add is 0 or 1 and their
    sum lies within six binomial sigma of N / 4."""
    n = 1 << 20
    t = np.arange(n, dtype=np.uint64)
    add = (np.uint64(1 << 29) + ref.inject_draws(0, 0, t)) >> np.uint64(31)
    assert set(np.unique(add).tolist()) <= {0, 1}
    assert abs(int(add.sum()) - n // 4) <= 6 * np.sqrt(n * 0.25 * 0.75)
    # the draws are 31 bits, so E = 0 adds nothing and E = 2^31 adds exactly one
    d = ref.inject_draws(3, 5, t[:4096])
    assert int(d.max()) < (1 << 31)
    assert np.all((np.uint64(1 << 31) + d) >> np.uint64(31) == 1)


def test_hash_on_hand_computed_values():
    """splitmix64's first three outputs from state 0 are the draws of seeds 0, 1 and 2 at c = t = 0 (the state
    advances by the golden constant once per seed); one more value worked by hand from the definition."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for seed, w in enumerate(want):
        assert ref.inject_hash(seed, 0, 0) == w
        assert C.inject_hash(seed, 0, 0) == w
    m = (1 << 64) - 1
    z = (8 * 0x9E3779B97F4A7C15 + ((3 << 40) | 12345)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    assert ref.inject_hash(7, 3, 12345) == z == C.inject_hash(7, 3, 12345)
    t = np.array([0, 1, 12345, (1 << 40) - 1], dtype=np.uint64)
    assert ref.inject_draws(7, 3, t).tolist() == [ref.inject_hash(7, 3, int(x)) >> 33 for x in t]


# ----------------------------------------------------------------- parse ----
def test_inject_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_inject_cmdline(["filinject", "-i", "x.fil", "--injfile", "s.inj"])
    assert ok and not exit_now and a.infilename == "x.fil" and a.injfilename == "s.inj"
    assert a.outfilename.endswith("_filinject.fil") and a.seed == 0 and a.units == "sigma"
    assert not a.no_smear and not a.verbose and a.killfilename == "" and a.truthfilename == ""
    ok, _, a = C.parse_inject_cmdline(["filinject", "-i", "x.fil", "--injfile", "s.inj", "-o", "y.fil", "-k", "k.txt",
                                       "--seed", "18446744073709551", "--units", "level", "--no_smear", "--truth_out",
                                       "t.txt", "-v"])
    assert ok and (a.outfilename, a.killfilename, a.truthfilename) == ("y.fil", "k.txt", "t.txt")
    assert a.seed == 18446744073709551 and a.units == "level" and a.no_smear and a.verbose


@pytest.mark.parametrize("extra", [["--seed", "-1"], ["--seed", "1.5"], ["--units", "jansky"], ["--nsub", "4"]])
def test_inject_cmdline_errors(extra):
    assert not C.parse_inject_cmdline(["filinject", "-i", "x.fil", "--injfile", "s.inj"] + extra)[0]
    assert not C.parse_inject_cmdline(["filinject", "-i", "x.fil"])[0]             # --injfile is required
    assert not C.parse_inject_cmdline(["filinject", "--injfile", "s.inj"])[0]      # -i is required


INJ_TEXT = """# two pulsars and two bursts
pulsar 0.05 30 0.3            # the defaults

pulsar 0.0123 100 1 0.1 150 0.3 -1.5
burst 1.0 200 5
   burst 0.5 10 2 0.003 2
"""


def test_injfile_parser_defaults_and_comments(tmp_path):
    s = C.inject_parse(INJ_TEXT)
    assert [x.kind for x in s] == ["pulsar", "pulsar", "burst", "burst"]
    assert (s[0].t, s[0].dm, s[0].amp, s[0].width, s[0].acc, s[0].phase, s[0].alpha) == (0.05, 30, 0.3, 0.05, 0, 0, 0)
    assert (s[1].width, s[1].acc, s[1].phase, s[1].alpha) == (0.1, 150, 0.3, -1.5)
    assert (s[2].t, s[2].dm, s[2].amp, s[2].width, s[2].alpha) == (1.0, 200, 5, 0.005, 0)
    assert (s[3].width, s[3].alpha) == (0.003, 2)
    p = tmp_path / "s.inj"
    p.write_text(INJ_TEXT)
    assert len(C.inject_read_file(str(p))) == 4
    o = ref.inject_parse(INJ_TEXT)
    assert o == [PulsarSpec(0.05, 30, 0.05, 0.3, 0, 0, 0), PulsarSpec(0.0123, 100, 0.1, 1, 150, 0.3, -1.5),
                 BurstSpec(1.0, 200, 0.005, 5, 0), BurstSpec(0.5, 10, 0.003, 2, 2)]


REFUSALS = [
    ("# nothing\n", "no signal"),
    ("quasar 1 2 3\n", "unknown kind"),
    ("pulsar 1 2\n", "needs at least"),
    ("pulsar 1 2 3 4 5 6 7 8\n", "too many columns"),
    ("burst 1 2 3 4 5 6\n", "too many columns"),
    ("pulsar 1 2 3x\n", "cannot read"),
    ("pulsar 1 2 -3\n", "amp must not be negative"),
    ("burst 1 2 -0.1\n", "amp must not be negative"),
    ("pulsar 0 2 3\n", "period must be positive"),
    ("pulsar -1 2 3\n", "period must be positive"),
    ("pulsar 1 2 3 0\n", "duty must be positive"),
    ("pulsar 1 2 3 1.01\n", "duty must not exceed 1"),
    ("burst 1 2 3 0\n", "width must be positive"),
    ("burst 1 2 3 -1\n", "width must be positive"),
    ("burst 1 -2 3\n", "dm must not be negative"),
    ("burst 1 2 nan\n", "not finite"),
    ("burst 1 2 3\n" * 65, "more than 64 signals"),
]


@pytest.mark.parametrize("text,what", REFUSALS, ids=[f"{i}-{w[1].replace(' ', '-')}" for i, w in enumerate(REFUSALS)])
def test_every_refusal_is_named_without_a_gpu(text, what):
    with pytest.raises(C.NativeError, match=what):
        C.inject_parse(text)
    with pytest.raises(ValueError, match=what):
        ref.inject_parse(text)


def test_more_refusals_are_named_without_a_gpu():
    with pytest.raises(C.NativeError, match="cannot open the injection file"):
        C.inject_read_file("/nonexistent/s.inj")
    with pytest.raises(C.NativeError, match="nbits must be 1, 2, 4 or 8"):
        C.inject_check_geometry(16, 16, 100, 1e-3, 1500.0, -1.0)
    with pytest.raises(C.NativeError, match="shorter than one sample"):
        C.inject_check_geometry(16, 8, 0, 1e-3, 1500.0, -1.0)
    with pytest.raises(C.NativeError, match="foff must not be zero"):
        C.inject_check_geometry(16, 8, 100, 1e-3, 1500.0, 0.0)
    with pytest.raises(C.NativeError, match="multiple of 8"):
        C.inject_check_geometry(3, 2, 100, 1e-3, 1500.0, -1.0)
    hdr = _header()
    big = _signals([BurstSpec(time=1.0, dm=10, amplitude=300)])      # 300 levels
    with pytest.raises(C.NativeError, match=r"A_q >= 2\^24"):
        C.inject_tables(big, 16, 8, 1000, hdr["tsamp"], hdr["fch1"], hdr["foff"], np.ones(16), False)
    with pytest.raises(ValueError, match=r"A_q >= 2\^24"):
        ref.inject_tables([BurstSpec(time=1.0, dm=10, amplitude=300)], hdr, np.ones(16), False)
    # the Injector validates before it touches a device: no GPU is needed to be refused
    data = np.zeros(16 * 100, dtype=np.uint8)
    with pytest.raises(C.NativeError, match="duty must not exceed 1"):
        C.Injector(data, 16, 8, 100, hdr["tsamp"], hdr["fch1"], hdr["foff"],
                   _signals([PulsarSpec(duty=2.0)]), [])
    with pytest.raises(C.NativeError, match="killmask size"):
        C.Injector(data, 16, 8, 100, hdr["tsamp"], hdr["fch1"], hdr["foff"], _signals([PulsarSpec()]), [1, 1])
    with pytest.raises(C.NativeError, match="smaller than the data block"):
        C.Injector(data, 16, 8, 101, hdr["tsamp"], hdr["fch1"], hdr["foff"], _signals([PulsarSpec()]), [])


# ---------------------------------------------------------------- tables ----
T_SIGNALS = [PulsarSpec(period=0.05, dm=30, amplitude=0.3),
             PulsarSpec(period=0.0123, dm=100, amplitude=1.0, duty=0.1, accel=150.0, phase=0.3),
             BurstSpec(time=1.0, dm=200, width=3e-3, amplitude=5.0),
             BurstSpec(time=-0.2, dm=0.0, width=1e-3, amplitude=0.0)]
T_ALPHA = [PulsarSpec(period=0.02, dm=50, amplitude=0.7, alpha=-1.5), BurstSpec(time=0.3, dm=80, amplitude=3.0, alpha=2.2)]


@pytest.mark.parametrize("smear", [True, False])
@pytest.mark.parametrize("foff", [-1.09, 0.5])
def test_host_tables_equal_the_oracle(smear, foff):
    from peasoup_amd import ops

    hdr = _header(fch1=1510.0 if foff < 0 else 1200.0, foff=foff)
    unit = np.linspace(0.0, 20.0, 16)         # channel 0 is dead
    a = ops.inject_tables(T_SIGNALS, hdr, 10000, unit, smear)
    b = ref.inject_tables(T_SIGNALS, hdr, unit, smear)
    for k in ("sigc", "delay", "inv_w", "w", "T", "A_q"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["nlive"] == b["nlive"] == 15 and not a["A_q"][:, 0].any() and not a["A_q"][3].any()
    assert a["delay"].dtype == np.float64 and a["A_q"].dtype == np.uint32 and a["T"].dtype == np.uint16
    # the delays are the search's: DM times the dedisperser's float table
    D = ref.delay_table(16, hdr["tsamp"], hdr["fch1"], hdr["foff"]).astype(np.float64)
    np.testing.assert_array_equal(a["delay"][2], 200.0 * D)
    a = ops.inject_tables(T_ALPHA, hdr, 10000, unit, smear)
    b = ref.inject_tables(T_ALPHA, hdr, unit, smear)
    for k in ("sigc", "delay", "inv_w", "w"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.abs(a["A_q"].astype(np.int64) - b["A_q"].astype(np.int64)).max() <= 1      # pow
    mid = a["A_q"][1].astype(np.float64) / unit.clip(1e-9)
    assert (mid[1] > mid[15]) == (foff < 0)             # alpha > 0: brighter at the higher frequency


def test_profile_table():
    T = C.inject_profile_table()
    np.testing.assert_array_equal(T, ref.inject_profile_table())
    assert T.shape == (1537,) and T[0] == 32768 and T[256] == 19875 and T[1536] == 0 and np.all(np.diff(T.astype(int)) <= 0)


def test_sigma_equals_the_oracle():
    rng = np.random.default_rng(5)
    for nsamps in (100, L, 3 * L + 17, 4 * L):
        x = np.clip(np.rint(rng.normal(100, [[1.0], [7.5], [30.0], [0.0]], (4, nsamps))), 0, 255).astype(np.uint8)
        x[1, : L // 2] = 255                              # one block is interference: the median ignores it
        S1, S2 = ref.rfi_block_sums(x, L)
        s = ref.inject_sigma(S1, S2, nsamps)
        np.testing.assert_array_equal(C.inject_sigma(S1, S2, nsamps), s)
        assert s[3] == 0.0 and abs(s[0] - 1.04) < 0.2 and abs(s[2] - 30) < 3
        if nsamps >= 3 * L:
            assert abs(s[1] - 7.5) < 0.5
    one = np.full((1, 10), 7, dtype=np.uint8)
    one[0, ::2] = 11
    assert ref.inject_sigma(*ref.rfi_block_sums(one, L), 10)[0] == 2.0


def test_truth_numbers_equal_the_oracle():
    hdr = _header()
    nsamps = 20000
    sigma = np.linspace(0.0, 20.0, 16)
    kill = [1] * 16
    kill[7] = 0
    unit = ref.inject_unit(sigma, kill, 16)
    sigs = T_SIGNALS + T_ALPHA
    tab = ref.inject_tables(sigs, hdr, unit, True)
    want = ref.inject_truth(sigs, tab, hdr, nsamps, unit, sigma)
    got = C.inject_truth(_signals(sigs), 16, 8, nsamps, hdr["tsamp"], hdr["fch1"], hdr["foff"], unit, sigma, True)
    for g, w in zip(got, want):
        assert g[0] == w[0]
        assert g[1] == pytest.approx(w[1], rel=1e-9) and g[2] == pytest.approx(w[2], rel=1e-9)
    assert want[0][0] == 103 and want[2][0] == 1 and want[3] == (0, 0.0, 0.0)      # 19999 x 256 us / 50 ms = 102.4
    # level units: no sigma, no S/N; the peak is the amplitude itself without smearing
    unit1 = ref.inject_unit(None, kill, 16)
    tab = ref.inject_tables(sigs, hdr, unit1, False)
    lv = ref.inject_truth(sigs, tab, hdr, nsamps, unit1, None)
    assert lv[2][1] == 5.0 and lv[2][2] == 0.0
    got = C.inject_truth(_signals(sigs), 16, 8, nsamps, hdr["tsamp"], hdr["fch1"], hdr["foff"], unit1, [], False)
    assert got[2] == (1, 5.0, 0.0)
    text = C.inject_truth_text(_signals(sigs), want, "sigma", 3)
    lines = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert len(lines) == 6 and lines[0].split()[:4] == ["pulsar", "0.050000000000000003", "30", "0.29999999999999999"]
    assert lines[2].split()[0] == "burst" and float(lines[2].split()[-1]) == pytest.approx(want[2][2], rel=1e-15)


# ---------------------------------------------------------------- oracle ----
def test_oracle_identities():
    """The expected value is what was asked for: at amp = 0.25 level the mean of out - in over many samples is the
    profile itself; chunks with their t0 give the bytes of one call; amp 0 and dead channels change nothing."""
    hdr = _header(nchans=8, nbits=2)
    n = 1 << 15
    x = synthetic.generate(n, hdr, (), seed=4).T.copy()
    x[3] = 1                                                 # a dead channel
    unit = np.ones(8)
    unit[3] = 0
    sig = [PulsarSpec(period=0.0031, dm=20.0, amplitude=0.25, duty=0.2), BurstSpec(time=2.0, dm=50, amplitude=0.5)]
    tab = ref.inject_tables(sig, hdr, unit, True)
    out, nclip, touched = ref.inject_apply(x, tab, 2, seed=9)
    assert np.array_equal(out[3], x[3]) and np.all(out >= x) and np.all(out.astype(int) - x <= 1)
    parts = [ref.inject_apply(x[:, a:b], tab, 2, seed=9, t0=a) for a, b in ((0, 5000), (5000, 5001), (5001, n))]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), out)
    assert sum(p[1] for p in parts) == nclip and np.array_equal(sum(p[2] for p in parts), touched)
    # channel 0, where nothing clips: sum of the adds against the sum of E
    room = x[0] < 3
    E, _ = ref.inject_expected(tab, 0, np.arange(n, dtype=np.uint64))
    want = float(E[room].sum()) / 2.0 ** 31
    got = float((out[0].astype(int) - x[0])[room].sum())
    assert want > 500 and abs(got - want) <= 6 * np.sqrt(want)          # a sum of Bernoulli draws: variance < mean
    zero, nz, _ = ref.inject_apply(x, ref.inject_tables([PulsarSpec(amplitude=0.0)], hdr, unit, True), 2, seed=9)
    assert np.array_equal(zero, x) and nz == 0
    other, _, _ = ref.inject_apply(x, tab, 2, seed=10)
    assert not np.array_equal(other, out)


def test_spec_dataclasses_gain_alpha_only():
    assert PulsarSpec().alpha == 0.0 and BurstSpec().alpha == 0.0
    assert PulsarSpec(0.1, 2.0, 0.3, 4.0, 5.0, 0.6) == PulsarSpec(period=0.1, dm=2.0, duty=0.3, amplitude=4.0, accel=5.0,
                                                                  phase=0.6, alpha=0.0)
    assert BurstSpec(1.0, 2.0, 3.0, 4.0) == BurstSpec(time=1.0, dm=2.0, width=3.0, amplitude=4.0, alpha=0.0)


# ---------------------------------------------------------------- native ----
def _run_native(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "inject unit tests passed" in r.stdout
    return r


def test_native_unit_tests():
    _run_native(os.path.join(REPO, "bin", "psoup_inject_unit_tests"))


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_host_sanitizers(san):
    """A stand-alone host binary built with the sanitizer, run in the inherited environment."""
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_inject_unit_tests")
    r = _run_native(os.path.join(REPO, "bin", f"psoup_inject_unit_tests_{san}"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
