"""jerksearch on the GPU: the kernel's output must EQUAL the NumPy oracle's
(utils.reference.jerk_resample) at the smallest shapes that reach each path; a
jerk grid of {0} must return the plain search's candidates bit for bit; an
injected jerk must be recovered at its grid point; the binary and the module
write the same candidate lines; every refusal reaches the user by name."""
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
from peasoup_amd.utils.sigproc import write_filterbank
from peasoup_amd.utils.synthetic import PulsarSpec

pytestmark = pytest.mark.gpu

C_LIGHT = 299792458.0
LANE = C.JERK_LANE
GUARD = 64
S3 = 12.0 * np.sqrt(3.0)  # max|g| = |jf| n^3 / (12 sqrt 3) (n even; within a sample otherwise)


def _factors(n):
    """Jerk factors whose largest |g| is about 0, 0.4 (identity), 3, 40 and 1000, of both signs."""
    return [s * m * S3 / float(n) ** 3 for m in (0.0, 0.4, 3.0, 40.0, 1000.0) for s in ((1.0,) if m == 0 else (1.0, -1.0))]


def _run(x, nrow, n, jf, out_stride, offset=0, in_offset=0):
    """The op on host rows x [nrows, row_stride]: out [nrows, K, nrow].  The output is guarded by GUARD bytes on both
    sides and between rows (out_stride > nrow), and every guard byte must come back unchanged.  ``offset`` shifts the
    first output byte off its 16-byte alignment, ``in_offset`` the first input byte off its 4-byte alignment."""
    import torch

    from peasoup_amd import ops

    nrows, K = x.shape[0], len(jf)
    d = torch.from_numpy(x).cuda()
    if in_offset:
        raw = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
        d = raw[in_offset:in_offset + x.size].view(x.shape).copy_(d)
        assert d.data_ptr() % 4 == in_offset % 4 != 0
    total = nrows * K * out_stride
    buf = torch.full((GUARD + offset + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + offset:GUARD + offset + total].view(nrows, K, out_stride)
    ops.jerk_resample(d, n, (), 0.0, nrow=nrow, out=out, factors=jf)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + offset] == 0xA5) and np.all(h[GUARD + offset + total:] == 0xA5), "wrote outside the output"
    y = h[GUARD + offset:GUARD + offset + total].reshape(nrows, K, out_stride)
    assert np.all(y[:, :, nrow:] == 0xA5), "wrote past the end of a row"
    return y[:, :, :nrow]


def _check(x, nrow, n, jf, out_stride, offset=0, in_offset=0):
    got = _run(x, nrow, n, jf, out_stride, offset, in_offset)
    for r in range(x.shape[0]):
        for k, f in enumerate(jf):
            np.testing.assert_array_equal(got[r, k], ref.jerk_resample(x[r, :nrow], n, f), err_msg=f"row {r} factor {f}")
    return got


def _rows(nrows, row_stride, seed):
    return np.random.default_rng(seed).integers(0, 256, (nrows, row_stride), dtype=np.uint8)


# ------------------------------------------------------------------ kernel ----
@pytest.mark.parametrize("pad", [0, 37])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4101, 65539])
def test_kernel_equals_oracle(n, pad):
    nrow = n + pad
    stride = (nrow + 255) // 256 * 256
    x = _rows(3, stride, n + pad)
    jf = _factors(n)
    _check(x, nrow, n, jf[:1], stride)       # K = 1
    _check(x, nrow, n, jf[3:8], stride)      # K = 5: +-0.4 is skipped below, +-3, +-40, +1000
    _check(x, nrow, n, jf[1:3] + jf[8:], stride)  # +-0.4 (identity) and -1000
    ident = _run(x, nrow, n, jf[:3], stride)
    for k in range(3):
        np.testing.assert_array_equal(ident[:, k], x[:, :nrow])


@pytest.mark.parametrize("n,pad", [(17, 0), (4101, 37), (65539, 0)])
def test_kernel_strides_that_are_no_multiple_of_16(n, pad):
    """Rows that start off a 16-byte (and 4-byte) boundary: byte stores, and source windows of every alignment."""
    nrow = n + pad
    jf = _factors(n)[3:8]
    x = _rows(3, nrow + 3, 5 * n)            # row_stride = nrow + 3
    _check(x, nrow, n, jf, nrow + 5)         # out_stride = nrow + 5
    _check(x, nrow, n, jf, (nrow + 255) // 256 * 256, offset=7)  # aligned stride, base off by 7
    # an input base that is not 4-byte aligned: the kernel reads by bytes throughout
    for off in (1, 2, 3):
        _check(x, nrow, n, jf, (nrow + 255) // 256 * 256, in_offset=off)


def test_kernel_exact_halves_and_both_clamps():
    """n = 4096 with jf = 2^-4: g hits exact halves (p(2) = 2^3 1023 2047) and most indices clamp."""
    n = 4096
    s = ref.jerk_shift(n, 0.0625)
    i = np.arange(n)
    g = (i * (i - n // 2) * (i - n)).astype(np.float64) * 0.0625
    halves = np.nonzero(np.abs(g - np.floor(g)) == 0.5)[0]
    assert 2 in halves and len(halves) > 100 and np.all(s[halves] % 2 == 0)
    assert np.mean(i + s > n - 1) > 0.4 and np.mean(i + s < 0) > 0.4
    x = _rows(3, n, 11)
    _check(x, n, n, [0.0625, -0.0625], n)
    # a factor at which the exact halves are inside the row: p(2) / 2^24 = 0.99..., p(2) jf = x.5
    jf = 2.5 / float(2 * (2 - 2048) * (2 - 4096))
    assert ref.jerk_shift(n, jf)[2] == 2
    _check(x, n, n, [jf, -jf, 3 * jf], n)


def test_kernel_fast_path_is_not_taken_across_a_stationary_point():
    """n = 65539 at moderate factors (shifts of about 40): the lane spans that hold a stationary point of the cubic.
    The factors are placed so that g crosses a half between the lane's ends and the extremum inside it: the end
    shifts agree and the shift inside differs, so a fast path taken there would show."""
    n = 65539
    lo, hi = C.jerk_stationary(n)
    a, b = n / 2.0 - n / (2 * np.sqrt(3.0)), n / 2.0 + n / (2 * np.sqrt(3.0))
    assert abs(lo - a) < 2 and abs(hi - b) < 2
    i = np.arange(n, dtype=np.int64)
    p = np.abs((i * (i - n // 2) * (i - n)).astype(np.float64))
    x = _rows(3, 65792, 3)
    found = 0
    for sp in (lo, hi):
        i0 = sp // LANE * LANE
        assert i0 < sp < i0 + LANE - 1  # the stationary point is inside the lane's span
        peak, ends = p[i0:i0 + LANE].max(), max(p[i0], p[i0 + LANE - 1])
        assert peak > ends
        jf = 40.5 / (0.5 * (peak + ends))
        for f in (jf, -jf):
            lane = ref.jerk_shift(n, f)[i0:i0 + LANE]
            found += int(lane[0] == lane[-1] and len(set(lane.tolist())) == 2)
        _check(x, n, n, [jf, -jf, 40.0 * S3 / float(n) ** 3], 65792)
    assert found == 4


def test_kernel_many_rows_and_factors():
    n, nrow = 4101, 4138
    x = _rows(7, 4352, 23)
    _check(x, nrow, n, [k * 1.7 * S3 / float(n) ** 3 for k in range(-6, 7)], 4352)


def test_kernel_refusals():
    import torch

    from peasoup_amd import ops

    d = torch.zeros((2, 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.jerk_resample(d, 256, (), 0.0, factors=[float("inf")])
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.jerk_resample(d, 256, (), 0.0, factors=[float("nan")])
    with pytest.raises(ValueError):
        ops.jerk_resample(d, 300, (), 0.0, factors=[0.0])
    with pytest.raises(RuntimeError, match="overlap"):
        C.jerk_resample_raw(d.data_ptr(), 256, 2, 256, 256, np.zeros(1), torch.zeros(1, dtype=torch.float64, device="cuda").data_ptr(),
                            d.data_ptr() + 16, 256, 0)
    with pytest.raises(RuntimeError, match="jerk factors"):
        ops.jerk_resample(d, 256, (), 0.0, factors=np.zeros(4097))


# --------------------------------------------------------- a grid of {0} ----
def _jerk_args(path, extra):
    ok, _, args = C.parse_jerk_cmdline(["jerksearch", "-i", path] + [str(e) for e in extra])
    assert ok
    return args


def _bits(v):
    return np.float32(v).view(np.uint32)


def test_grid_of_zero_equals_the_plain_search(tmp_path):
    """2^16 samples, 64 channels, 2-bit, 4 DMs, +-acc with a few trials: run_jerk_search at the jerk grid {0}
    returns exactly the candidates of the existing single-device search, bit patterns and order."""
    from peasoup_amd.models.jerk import run_jerk_search

    path = str(tmp_path / "plain.fil")
    hdr = synthetic.make_header(nchans=64, nbits=2, tsamp=320e-6)
    synthetic.write(path, 1 << 16, hdr, [PulsarSpec(period=0.0123, dm=12.0, duty=0.06, amplitude=0.6, accel=4000.0)],
                    seed=5)
    opts = ["--dm_start", 0, "--dm_end", 20, "--dm_tol", 1.5, "--acc_start", -15000, "--acc_end", 15000, "-n", 3, "-m", 7]
    ok, _, pargs = C.parse_cmdline(["peasoup", "-i", path, "-o", str(tmp_path / "plain"), "-t", "1"] + [str(o) for o in opts])
    assert ok
    plain = C.run_pipeline_native(pargs)
    assert len(plain["dm_list"]) == 4
    want = plain["candidates"]
    assert len(want) >= 3
    args = _jerk_args(path, opts + ["-o", str(tmp_path / "jerk.out")])
    res = run_jerk_search(args)
    assert [len(j) for j in res.setup.jerks] == [1] * 4 and all(j[0] == 0.0 for j in res.setup.jerks)
    assert 2 < len(res.setup.accel_plan.generate(0.0)) < 40
    got = res.candidates
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.jerk == 0.0
        assert (g.cand.dm_idx, g.cand.nh) == (w.dm_idx, w.nh)
        for f in ("dm", "acc", "snr", "freq"):
            assert _bits(getattr(g.cand, f)) == _bits(getattr(w, f)), f
        assert _bits(1.0 / g.cand.freq) == _bits(1.0 / w.freq)
        assert g.cand.count_assoc() == w.count_assoc()


# ---------------------------------------------------------------- recovery ----
NS3 = 1 << 17
TS3 = 320e-6
P3 = 0.0101
AMP3 = 0.1
SEED3 = 1


def _hdr3():
    return synthetic.make_header(nchans=64, nbits=8, tsamp=TS3)


@functools.lru_cache(maxsize=None)
def _recovery(tmp):
    """The two files of the recovery test and J (float32, exact in the grid J / 4 ... 5 J / 4)."""
    hdr = dict(_hdr3())
    hdr["nsamples"] = NS3
    plain = os.path.join(tmp, "plain.fil")
    write_filterbank(plain, hdr, synthetic.generate(NS3, hdr, [PulsarSpec(period=P3, dm=20.0, duty=0.05,
                                                                          amplitude=AMP3)], seed=SEED3))
    # (the default transform is the power of two below the file's 2^17 samples: ask for all of them)
    base = ["--dm_start", 20, "--dm_end", 20, "--fft_size", NS3]
    n = C.jerk_setup(_jerk_args(plain, base)).span
    assert NS3 - 64 < n < NS3  # the dedispersed row, padded to the transform
    # |jf| n^3 / (12 sqrt 3) = 20 samples
    J = float(np.float32(20.0 * S3 / float(n) ** 3 * 6 * C_LIGHT / float(np.float32(TS3)) ** 2))
    jerked = os.path.join(tmp, "jerked.fil")
    write_filterbank(jerked, hdr, synthetic.generate(NS3, hdr, [PulsarSpec(period=P3, dm=20.0, duty=0.05,
                                                                           amplitude=AMP3, jerk=J)], seed=SEED3))
    T = n * float(np.float32(TS3))
    # the matching acceleration is the one at mid-span, J T / 2: the range must hold it
    acc = base + ["--acc_start", 0, "--acc_end", repr(float(np.float32(0.6 * J * T)))]
    grid = ["--jerk_start", 0, "--jerk_end", repr(float(np.float32(1.25 * J))), "--jerk_step",
            repr(float(np.float32(J / 4)))]
    return plain, jerked, J, n, acc, grid


@pytest.fixture(scope="module")
def recovery(tmp_path_factory):
    return _recovery(str(tmp_path_factory.mktemp("jerk_recovery")))


def test_recovery_of_an_injected_jerk(recovery, tmp_path):
    """A 42 s series made jerk-limited by J = 3.2e3 m/s^3 (20 samples of cubic shift).  (a) the same pulsar without
    jerk through the grid {0}: the ceiling; (b) the jerked data through {0}: the floor; (c) the jerked data through
    the grid 0, J/4 ... 5J/4.  The top candidate of (c) is at the grid point J, above the midpoint of (a) and (b),
    at the injected period.

    The period: the engine reports, as for any accelerated pulsar, the frequency its resample leaves, which is the
    t-coefficient of the residual phase times 1 - acc T_fft / (2c) (the shift i (i - N) of SearchEngine is zero at
    both ends, N = fft_size).  jerksearch corrects the jerk's factor 1 + J T^2 / (12c) only; the acceleration's
    factor is the plain search's convention and stays.  So the corrected period is compared with the injected one
    divided by 1 - acc T_fft / (2c) at the candidate's acc, within freq_tol (the distillers' tolerance, 1e-4)."""
    from peasoup_amd.models.jerk import run_jerk_search

    plain, jerked, J, n, acc, grid = recovery
    out = ["-o", str(tmp_path / "o.txt")]
    a = run_jerk_search(_jerk_args(plain, acc + out), write=False)
    b = run_jerk_search(_jerk_args(jerked, acc + out), write=False)
    c = run_jerk_search(_jerk_args(jerked, acc + grid + out), write=False)
    assert np.float32(J) in np.asarray(c.setup.jerks[0], dtype=np.float32)
    sa, sb, top = a.candidates[0].cand.snr, (b.candidates[0].cand.snr if b.candidates else 0.0), c.candidates[0]
    print(f"S/N (a) {sa:.3f} (b) {sb:.3f} (c) {top.cand.snr:.3f} at jerk {top.jerk:.6g} acc {top.cand.acc:.6g}")
    assert abs(1.0 / a.candidates[0].cand.freq / P3 - 1) < 1e-4
    assert _bits(top.jerk) == _bits(J)
    assert top.cand.snr > 0.5 * (sa + sb)
    T = n * float(np.float32(TS3))
    assert abs(top.cand.acc / (J * T / 2) - 1) < 0.05
    period = C.jerk_freq_factor(top.jerk, n, TS3) / top.cand.freq
    want = P3 / (1.0 - top.cand.acc * (NS3 * float(np.float32(TS3))) / (2 * C_LIGHT))
    print(f"corrected period {period:.9g}, expected {want:.9g}, injected {P3}")
    assert abs(period / want - 1) < 1e-4


# ------------------------------------------------------- the two drivers ----
def _cand_lines(path):
    with open(path) as f:
        return [ln for ln in f if not ln.startswith("#")]


def test_native_and_python_drivers_write_the_same_lines(recovery, tmp_path):
    plain, jerked, J, n, acc, grid = recovery
    opts = [str(o) for o in acc + grid + ["--npdmp", 3, "--limit", 50]]
    o1, o2 = str(tmp_path / "native.out"), str(tmp_path / "module.out")
    r = subprocess.run([os.path.join(REPO, "bin", "jerksearch"), "-i", jerked, "-o", o1] + opts, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "jerk", "-i", jerked, "-o", o2] + opts,
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    l1, l2 = _cand_lines(o1), _cand_lines(o2)
    assert len(l1) >= 1 and l1 == l2
    first = l1[0].split()
    assert len(first) == 9 and _bits(float(first[3])) == _bits(J)  # the jerk column holds the grid point
    assert any(float(ln.split()[7]) != 0 for ln in l1)               # --npdmp folded the re-made DM-jerk rows
    with open(o1) as f:
        head = [ln for ln in f if ln.startswith("#")]
    assert any("jerk_step" in ln for ln in head) and any("mid-span" in ln for ln in head)
    assert head[-1].split()[1:] == "period_s dm acc jerk freq nh snr folded_snr dm_idx".split()
    assert not os.path.exists(o1 + ".tmp")


# ---------------------------------------------------------------- refusals ----
def _refused(tmp_path, fil, extra, what):
    out = str(tmp_path / "refused.out")
    r = subprocess.run([os.path.join(REPO, "bin", "jerksearch"), "-i", fil, "-o", out] + [str(e) for e in extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert what in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_every_refusal_reaches_the_user_by_name(recovery, tmp_path):
    plain = recovery[0]
    dm = ["--dm_start", 20, "--dm_end", 20]
    _refused(tmp_path, plain, dm + ["--jerk_start", 2, "--jerk_end", 1], "jerk_start > jerk_end")
    _refused(tmp_path, plain, dm + ["--jerk_end", "inf"], "non-finite")
    _refused(tmp_path, plain, dm + ["--jerk_start", "nan"], "non-finite")
    _refused(tmp_path, plain, dm + ["--jerk_end", 1, "--jerk_step", 1e-5], "more than 4096 jerk trials")
    _refused(tmp_path, plain, dm + ["--jerk_start", 3e7, "--jerk_end", 3e7], "0.9 samples per sample")
    _refused(tmp_path, plain, dm + ["-t", 2], "one device")
    # n > 2^26: a sparse 1-bit file of 2^26 + 4096 samples, refused from its header before any data is read
    big = str(tmp_path / "big.fil")
    hdr = synthetic.make_header(nchans=8, nbits=1, tsamp=64e-6)
    hdr["nsamples"] = (1 << 26) + 4096
    write_filterbank(big, hdr, np.zeros((0, 8), dtype=np.uint8))
    with open(big, "r+b") as f:
        f.truncate(os.path.getsize(big) + hdr["nsamples"])
    _refused(tmp_path, big, ["--dm_start", 0, "--dm_end", 0, "--fft_size", 1 << 27, "--jerk_end", 0.001],
             "longer than 2^26")
