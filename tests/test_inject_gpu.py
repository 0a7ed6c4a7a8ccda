"""filinject on the GPU: the kernel's output must EQUAL the NumPy oracle's
(utils.reference.inject_apply / inject_filterbank) at the smallest shapes that
reach each edge; the binary, the module and the oracle write identical files;
the search tools find what was injected."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import header_bytes, pack_samples, read_header
from peasoup_amd.utils.synthetic import BurstSpec, PulsarSpec

pytestmark = pytest.mark.gpu

TILE = C.inject_tile()
L = C.inject_stat_block()
TSAMP = 256e-6


def _header(nchans=8, nbits=8):
    return synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=TSAMP)


def _noise(nsamps, hdr, seed=1):
    """Raw samples [nchans, nsamps]."""
    return np.ascontiguousarray(synthetic.generate(nsamps, hdr, (), seed=seed).T)


def _kernel(x, tab, nbits, seed=0, t0=0):
    """The inject op on raw samples x [nchans, nsamps]: (out raw uint8, nclip, touched).  The rows are padded to a
    stride that is a multiple of 16 with a guard value that must come back unchanged."""
    import torch

    from peasoup_amd import ops

    nchans, nsamps = x.shape
    bias = 128 if nbits == 8 else 0
    stride = (nsamps + 15) // 16 * 16 + 16
    rows = np.full((nchans, stride), 77 - bias, dtype=np.int16)
    rows[:, :nsamps] = x.astype(np.int16) - bias
    d = torch.from_numpy(rows.astype(np.int8)).cuda()
    _, nclip, touched = ops.inject(d, nsamps, nbits, tab, seed=seed, t0=t0, bias=bias)
    torch.cuda.synchronize()
    y = d.cpu().numpy().astype(np.int16) + bias
    assert np.all(y[:, nsamps:] == 77), "the kernel wrote past the end of a row"
    return y[:, :nsamps].astype(np.uint8), nclip, touched


def _check(x, tab, nbits, seed=0, t0=0):
    want, wclip, wtouch = ref.inject_apply(x, tab, nbits, seed, t0)
    got, nclip, touched = _kernel(x, tab, nbits, seed, t0)
    np.testing.assert_array_equal(got, want)
    assert nclip == wclip
    np.testing.assert_array_equal(np.asarray(touched, dtype=np.uint64), wtouch)
    return got


# ------------------------------------------------------- tails and tiles ----
@pytest.mark.parametrize("nsamps", [15, 16, 17, TILE - 1, TILE + 17])
def test_tails_and_tiles(nsamps):
    hdr = _header()
    x = _noise(nsamps, hdr)
    tab = ref.inject_tables([PulsarSpec(period=37.3 * TSAMP, dm=12.0, amplitude=2.6, duty=0.2)], hdr, np.ones(8))
    got = _check(x, tab, 8, seed=3)
    assert not np.array_equal(got, x)
    _check(x, tab, 8, seed=3, t0=5 * L)                     # the same rows as a later chunk of the file


# ----------------------------------------------------------- every width ----
W_SIGNALS = [PulsarSpec(period=0.0171, dm=40.0, amplitude=0.4, duty=0.1, phase=0.2),
             BurstSpec(time=0.6, dm=90.0, width=4e-3, amplitude=1.5)]


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_every_width_through_unpack_inject_pack(tmp_path, nbits):
    from peasoup_amd import ops

    hdr = _header(64, nbits)
    fil = str(tmp_path / "in.fil")
    synthetic.write(fil, 5000, hdr, (), seed=nbits)
    want = ref.inject_filterbank(fil, None, W_SIGNALS, seed=11)
    h = read_header(fil)
    packed = np.fromfile(fil, dtype=np.uint8, offset=h["size"])
    y, res = ops.inject_filterbank_bytes(packed, h, 5000, W_SIGNALS, seed=11)
    np.testing.assert_array_equal(y, want["packed"])
    assert res["nclip"] == want["nclip"] and res["chunks"] == 1
    np.testing.assert_array_equal(res["touched"], want["touched"])
    np.testing.assert_array_equal(res["sigma"], want["sigma"])
    assert not np.array_equal(y, packed)


# ------------------------------------------------------------ skip paths ----
def test_skip_one_burst_in_the_middle_of_four_tiles():
    hdr = _header()
    n = 4 * TILE
    x = _noise(n, hdr)
    b = BurstSpec(time=2 * TILE * TSAMP, dm=25.0, width=2e-3, amplitude=30.0)
    tab = ref.inject_tables([b], hdr, np.ones(8))
    got = _check(x, tab, 8)
    t = np.arange(n, dtype=np.float64)
    for c in range(8):
        half = 1536.5 / tab["inv_w"][0, c]
        outside = np.abs(t - tab["delay"][0, c] - tab["sigc"][0, 1]) >= half
        assert np.array_equal(got[c][outside], x[c][outside]) and not np.array_equal(got[c], x[c])
        assert outside[:TILE].all() and outside[3 * TILE:].all()          # whole tiles go untouched


@pytest.mark.parametrize("time,changed", [(-1.0, False), (5.0, False), (-0.002, True), (2 * TILE * TSAMP + 0.002, True)],
                         ids=["before-the-start", "after-the-end", "straddles-the-start", "straddles-the-end"])
def test_skip_bursts_at_and_beyond_the_ends(time, changed):
    hdr = _header()
    x = _noise(2 * TILE, hdr)
    b = BurstSpec(time=time, dm=0.0, width=5e-3, amplitude=30.0)
    tab = ref.inject_tables([b], hdr, np.ones(8))
    got = _check(x, tab, 8)
    assert np.array_equal(got, x) != changed


# --------------------------------------------------------------- overlap ----
def test_overlap_one_draw_for_the_summed_expectation():
    hdr = _header()
    n = TILE + 300
    x = _noise(n, hdr)
    sig = [PulsarSpec(period=0.011, dm=5.0, amplitude=3.3, duty=0.5), PulsarSpec(period=0.0173, dm=9.0, amplitude=2.1,
                                                                                 duty=0.4, phase=0.4),
           BurstSpec(time=0.5 * n * TSAMP, dm=3.0, width=0.1, amplitude=7.7)]
    tab = ref.inject_tables(sig, hdr, np.ones(8))
    E = [ref.inject_expected(ref.inject_tables([s], hdr, np.ones(8)), 2, np.arange(n, dtype=np.uint64))[0] for s in sig]
    assert np.count_nonzero((E[0] > 0) & (E[1] > 0) & (E[2] > 0)) > 100          # all three on the same samples
    _check(x, tab, 8, seed=1)


# -------------------------------------------------------------- clipping ----
def test_clipping_at_300_levels():
    """--units level, amp = 300 on 8-bit data.  An A_q of 2^24 (256 levels) is refused, so the burst is one the
    intra-channel smearing of its DM lowers below that (fluence is conserved: the peak falls as the width grows);
    it still carries the noise past 255."""
    hdr = _header()
    x = _noise(TILE, hdr)
    b = BurstSpec(time=0.5 * TILE * TSAMP, dm=300.0, width=1e-3, amplitude=300.0)
    with pytest.raises(ValueError, match=r"A_q >= 2\^24"):
        ref.inject_tables([b], hdr, np.ones(8), smear=False)
    tab = ref.inject_tables([b], hdr, np.ones(8), smear=True)
    assert tab["A_q"].max() < (1 << 24) and tab["A_q"].min() > 100 * 65536
    want, wclip, _ = ref.inject_apply(x, tab, 8)
    got = _check(x, tab, 8)
    assert wclip > 8 and got.max() == 255 and np.count_nonzero(got == 255) >= wclip


# ------------------------------------------------ killed, dead, chunking ----
def _file(tmp_path, nsamps, nchans=16, nbits=8, seed=2, dead=None):
    hdr = _header(nchans, nbits)
    vals = synthetic.generate(nsamps, hdr, (), seed=seed)
    if dead is not None:
        vals[:, dead] = 3
    fil = str(tmp_path / "in.fil")
    hdr["nsamples"] = nsamps
    with open(fil, "wb") as f:
        f.write(header_bytes(hdr))
        f.write(pack_samples(vals, nbits).tobytes())
    h = read_header(fil)
    return fil, h, np.fromfile(fil, dtype=np.uint8, offset=h["size"]), vals


def test_killed_and_dead_channels_are_untouched(tmp_path):
    from peasoup_amd import ops

    fil, h, packed, vals = _file(tmp_path, 5000, dead=9)
    kill = [1] * 16
    kill[4] = 0
    sig = [PulsarSpec(period=0.01, dm=10.0, amplitude=1.0, duty=0.3)]
    want = ref.inject_filterbank(fil, None, sig, killmask=kill, seed=5)
    y, res = ops.inject_filterbank_bytes(packed, h, 5000, sig, killmask=kill, seed=5)
    np.testing.assert_array_equal(y, want["packed"])
    out = y.reshape(5000, 16)
    assert np.array_equal(out[:, 4], vals[:, 4]) and np.array_equal(out[:, 9], vals[:, 9])
    assert res["sigma"][9] == 0.0 and res["sigma"][4] > 0
    assert not res["A_q"][:, 4].any() and not res["A_q"][:, 9].any() and res["A_q"][:, 5].all() and res["nlive"] == 14
    assert not np.array_equal(out[:, 5], vals[:, 5])


@pytest.mark.parametrize("units", ["sigma", "level"])
def test_chunking_cannot_change_a_byte(tmp_path, units):
    from peasoup_amd import ops

    nsamps = 2 * L + 300
    fil, h, packed, _ = _file(tmp_path, nsamps, nbits=4)
    sig = [PulsarSpec(period=0.0123, dm=60.0, amplitude=0.5 if units == "sigma" else 1.5, duty=0.2),
           BurstSpec(time=(L + 10) * TSAMP, dm=20.0, amplitude=2.0)]
    want = ref.inject_filterbank(fil, None, sig, seed=8, units=units)
    one, r1 = ops.inject_filterbank_bytes(packed, h, nsamps, sig, seed=8, units=units)
    per = 16 * 4 // 8 + 16                                   # packed bytes and row bytes of one sample
    three, r3 = ops.inject_filterbank_bytes(packed, h, nsamps, sig, seed=8, units=units, budget_bytes=per * L)
    assert (r1["chunks"], r3["chunks"], r3["chunk_samples"]) == (1, 3, L)
    np.testing.assert_array_equal(one, want["packed"])
    np.testing.assert_array_equal(three, one)
    assert r1["nclip"] == r3["nclip"] == want["nclip"]
    np.testing.assert_array_equal(r3["touched"], want["touched"])
    np.testing.assert_array_equal(r1["touched"], want["touched"])
    if units == "sigma":
        np.testing.assert_array_equal(r3["sigma"], want["sigma"])


# ----------------------------------------------------------------- seeds ----
def test_seeds_and_zero_amplitude(tmp_path):
    from peasoup_amd import ops

    fil, h, packed, _ = _file(tmp_path, 3000, nbits=2)
    sig = [PulsarSpec(period=0.0123, dm=60.0, amplitude=0.3, duty=0.2)]
    a, _ = ops.inject_filterbank_bytes(packed, h, 3000, sig, seed=1)
    b, _ = ops.inject_filterbank_bytes(packed, h, 3000, sig, seed=1)
    c, _ = ops.inject_filterbank_bytes(packed, h, 3000, sig, seed=2)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, packed)
    z, rz = ops.inject_filterbank_bytes(packed, h, 3000, [PulsarSpec(amplitude=0.0), BurstSpec(amplitude=0.0)], seed=1)
    assert np.array_equal(z, packed) and rz["nclip"] == 0 and not rz["touched"].any()


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


INJ_TEXT = """# one pulsar, two bursts
pulsar 0.0123 60 0.5 0.2 25 0.1 -1
burst 0.4 20 2
burst 1.1 150 1.5 0.003 1.5
"""


@pytest.mark.parametrize("units", ["sigma", "level"])
def test_cli_module_and_oracle_write_identical_files(tmp_path, units):
    nsamps = 2 * L + 300
    fil, h, packed, _ = _file(tmp_path, nsamps, nbits=2, dead=3)
    kill = [1] * 16
    kill[5] = kill[6] = 0
    killf = tmp_path / "kill.txt"
    killf.write_text("".join(f"{k}\n" for k in kill))
    inj = tmp_path / "s.inj"
    inj.write_text(INJ_TEXT)
    flags = ["-i", fil, "--injfile", str(inj), "-k", str(killf), "--seed", "77", "--units", units]
    out = {k: (str(tmp_path / f"{k}.fil"), str(tmp_path / f"{k}.truth")) for k in ("native", "module", "oracle")}
    r = _run([os.path.join(REPO, "bin", "filinject")] + flags + ["-o", out["native"][0], "--truth_out",
                                                                   out["native"][1], "-v"])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "inject"] + flags + ["-o", out["module"][0], "--truth_out",
                                                                    out["module"][1]], env=env, cwd=REPO)
    res = ref.inject_filterbank(fil, out["oracle"][0], INJ_TEXT, killmask=kill, seed=77, units=units)
    a = open(out["native"][0], "rb").read()
    assert a == open(out["module"][0], "rb").read()
    assert a == open(out["oracle"][0], "rb").read()
    assert a[:h["size"]] == open(fil, "rb").read()[:h["size"]] and a[h["size"]:] != packed.tobytes()
    t = open(out["native"][1]).read()
    assert t == open(out["module"][1]).read()
    rows = [ln.split() for ln in t.splitlines() if not ln.startswith("#")]
    assert [r_[0] for r_ in rows] == ["pulsar", "burst", "burst"]
    for r_, w in zip(rows, res["truth"]):
        assert int(r_[-3]) == w[0]
        assert float(r_[-2]) == pytest.approx(w[1], rel=1e-9) and float(r_[-1]) == pytest.approx(w[2], rel=1e-9)
    nlive = 13 if units == "sigma" else 14                   # the dead channel has a unit in levels
    assert f"nclip {res['nclip']}, {nlive} of 16 channels live" in r.stdout
    assert f"signal 1 (burst): {int(res['touched'][1])} samples touched" in r.stdout
    assert C.Filterbank.from_file(out["native"][0]).nsamps == nsamps
    # a refusal reaches the command line by name and writes nothing
    inj.write_text("pulsar 0.01 10 1 1.5\n")
    bad = subprocess.run([os.path.join(REPO, "bin", "filinject"), "-i", fil, "--injfile", str(inj), "-o",
                          str(tmp_path / "bad.fil")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "duty must not exceed 1" in bad.stderr and not os.path.exists(str(tmp_path / "bad.fil"))


# ---------------------------------------------------------- acceleration ----
def test_acceleration_is_exact():
    """acc = 150 m/s^2 over 2^15 samples: the (af te) te term is where a contracted multiply-add would show."""
    hdr = _header()
    n = 1 << 15
    x = _noise(n, hdr)
    sig = [PulsarSpec(period=0.00237, dm=70.0, amplitude=2.0, duty=0.1, accel=150.0, phase=0.37)]
    tab = ref.inject_tables(sig, hdr, np.ones(8))
    _check(x, tab, 8, seed=6)
    _check(x[:, :TILE], tab, 8, seed=6, t0=(1 << 33) + 5)     # late in a long file: large te


# ------------------------------------------------------------ end to end ----
E_N = 1 << 17
E_SEED = 17
E_PSR = PulsarSpec(period=0.05, dm=30.0, amplitude=0.3)
E_BURST = BurstSpec(time=20.0, dm=40.0, width=5e-3, amplitude=1.2)
# |S/N(B) / S/N(A) - 1| of the pulsar, B injected and A generated: twice the deviation measured on the first run
# (S/N 89.174 against 90.013, ratio 0.99068; profiles/inject/SUMMARY.md).  Both values are deterministic.
E_SNR_BOUND = 2 * 0.00932


# The band: 64 channels of 2 MHz below 800 MHz, where a DM error of one unit sweeps 2.6 ms across the band, as much
# as the pulsar's 2.5 ms pulse, so neighbouring DM trials differ by more than the noise.  (At 1.5 GHz with 1.09 MHz
# channels the trials are 3.3 units apart and lose 0.6 ms, a quarter of the pulse: there even the generated file A
# comes back one trial off.)
@functools.lru_cache(maxsize=None)
def _e2e():
    hdr = synthetic.make_header(nchans=64, nbits=8, fch1=800.0, foff=-2.0, nsamples=E_N)
    return hdr, synthetic.generate(E_N, hdr, (), seed=E_SEED)


def _search(hdr, packed):
    import torch

    from peasoup_amd.models.search import RankSearcher

    ok, _, args = C.parse_cmdline(["peasoup", "-i", "synthetic", "--dm_start", "20", "--dm_end", "40", "--acc_start", "0",
                                   "--acc_end", "0", "-n", "4"])
    assert ok
    rs = RankSearcher(args, hdr, torch.from_numpy(packed).cuda(), E_N)
    cands = C.global_distill_and_score(rs.search(range(len(rs.dm_list))), args, rs.header)
    assert cands, "no candidates"
    return cands[0], np.asarray(rs.dm_list), rs


def test_search_finds_the_injected_pulsar():
    from peasoup_amd import ops

    hdr, noise = _e2e()
    A = pack_samples(synthetic.generate(E_N, hdr, [E_PSR], seed=E_SEED), 8)
    # synthetic.generate has no intra-channel smearing, which at DM 30 in this band would widen the pulse by half:
    # like for like, B is injected without it
    B, res = ops.inject_filterbank_bytes(pack_samples(noise, 8), hdr, E_N, [E_PSR], seed=1, smear=False)
    a, dms, _ = _search(hdr, A)
    b, _, rs = _search(hdr, B)
    bin_hz = 1.0 / (rs.fft_size * hdr["tsamp"])
    ratio = b.snr / a.snr
    print(f"\npulsar: A freq {a.freq:.6f} dm {a.dm:.3f} snr {a.snr:.3f}; B freq {b.freq:.6f} dm {b.dm:.3f} "
          f"snr {b.snr:.3f}; ratio {ratio:.5f}; truth snr {res['truth'][0][2]:.2f}; bin {bin_hz:.6f} Hz")
    assert abs(b.freq - 1.0 / E_PSR.period) <= bin_hz
    assert b.dm == pytest.approx(float(dms[np.argmin(np.abs(dms - E_PSR.dm))]))
    assert abs(ratio - 1.0) <= E_SNR_BOUND


def test_spsearch_finds_the_injected_burst(tmp_path):
    from peasoup_amd import ops

    hdr, noise = _e2e()
    B, _ = ops.inject_filterbank_bytes(pack_samples(noise, 8), hdr, E_N, [E_BURST], seed=1)
    fil, out = str(tmp_path / "b.fil"), str(tmp_path / "sp.txt")
    with open(fil, "wb") as f:
        f.write(header_bytes(hdr))
        f.write(B.tobytes())
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", fil, "--dm_start", "0", "--dm_end", "80", "-t", "1", "-o", out])
    assert ok
    res = C.run_sp_pipeline(a)
    assert res.candidates, "no single-pulse candidates"
    best = res.candidates[0]
    dms = np.asarray(res.dm_list)
    print(f"\nburst: time {best.time_s:.5f} dm {dms[best.dm_idx]:.3f} width {best.width} snr {best.snr:.2f}")
    assert abs(best.dm_idx - int(np.argmin(np.abs(dms - E_BURST.dm)))) <= 1
    assert abs(best.time_s - E_BURST.time) <= max(E_BURST.width, best.width * hdr["tsamp"])
