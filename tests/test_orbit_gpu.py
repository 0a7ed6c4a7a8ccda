"""orbsearch on the GPU: the kernel's output must EQUAL the NumPy oracle's
(utils.reference.orbit_resample) at the smallest shapes that reach each path;
the one-template identity bank must return the plain search's candidates bit
for bit; an injected orbit must be recovered at its grid point; the binary and
the module write the same candidate lines; every refusal reaches the user by
name."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import orbit_cases as oc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import write_filterbank
from peasoup_amd.utils.synthetic import PulsarSpec

pytestmark = pytest.mark.gpu

LANE = C.ORBIT_LANE
GUARD = 64
TS = oc.TS


def _run(x, nrow, n, tpl, out_stride, offset=0, in_offset=0):
    """The op on host rows x [nrows, row_stride]: out [nrows, K, nrow].  The output is guarded by GUARD bytes on both
    sides and between rows (out_stride > nrow), and every guard byte must come back unchanged.  ``offset`` shifts the
    first output byte off its 16-byte alignment, ``in_offset`` the first input byte off its 4-byte alignment."""
    import torch

    from peasoup_amd import ops

    nrows, K = x.shape[0], len(tpl)
    d = torch.from_numpy(x).cuda()
    if in_offset:
        raw = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
        d = raw[in_offset:in_offset + x.size].view(x.shape).copy_(d)
        assert d.data_ptr() % 4 == in_offset % 4 != 0
    total = nrows * K * out_stride
    buf = torch.full((GUARD + offset + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + offset:GUARD + offset + total].view(nrows, K, out_stride)
    ops.orbit_resample(d, n, (), 0.0, nrow=nrow, out=out, quant=tpl)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + offset] == 0xA5) and np.all(h[GUARD + offset + total:] == 0xA5), "wrote outside the output"
    y = h[GUARD + offset:GUARD + offset + total].reshape(nrows, K, out_stride)
    assert np.all(y[:, :, nrow:] == 0xA5), "wrote past the end of a row"
    return y[:, :, :nrow]


def _check(x, nrow, n, tpl, out_stride, offset=0, in_offset=0):
    got = _run(x, nrow, n, tpl, out_stride, offset, in_offset)
    oc.check_rows(got, x, nrow, n, tpl)
    return got


# ------------------------------------------------------------------ kernel ----
@pytest.mark.parametrize("n,pad", oc.SHAPES)
def test_kernel_equals_oracle(n, pad):
    """3 rows; K of 1, 5 and 13; amplitudes of 0, 0.4, 3, 40 and 1000 samples at orbits of 64 samples, n / 3, n and
    10 n from the phases 0, 0.25 and 0.37."""
    nrow = n + pad
    stride = (nrow + 255) // 256 * 256
    x = oc.rows(3, stride, n + pad)
    tpl = oc.templates(n)
    for grp in oc.groups(tpl):
        _check(x, nrow, n, grp, stride)
    ident = _run(x, nrow, n, tpl[:12], stride)   # a1 = 0 at every orbit and phase
    for k in range(12):
        np.testing.assert_array_equal(ident[:, k], x[:, :nrow])


@pytest.mark.parametrize("n,pad", [(17, 0), (4101, 37), (65539, 0)])
def test_kernel_strides_that_are_no_multiple_of_16(n, pad):
    """Rows that start off a 16-byte (and 4-byte) boundary: byte stores, and source windows of every alignment."""
    nrow = n + pad
    tpl = oc.templates(n)[25:60:7]             # 3, 40 and 1000 samples over every orbit and phase
    assert len(tpl) == 5 and all(q[2] > 0 for q in tpl)
    x = oc.rows(3, nrow + 3, 5 * n)            # row_stride = nrow + 3
    _check(x, nrow, n, tpl, nrow + 5)          # out_stride = nrow + 5
    _check(x, nrow, n, tpl, (nrow + 255) // 256 * 256, offset=7)  # aligned stride, base off by 7
    # an input base that is not 4-byte aligned: the kernel reads by bytes throughout
    for off in (1, 2, 3):
        _check(x, nrow, n, tpl, (nrow + 255) // 256 * 256, in_offset=off)


def test_kernel_wide_load_is_not_taken_across_a_turning_point():
    """A lane span with a turning point of the sine strictly inside, equal shifts at its ends and another inside
    (found with the oracle): the wide load would copy 16 contiguous bytes there."""
    n = 65539
    q, i0 = oc.turning_case(n)
    s = ref.orbit_shift(n, q)[i0:i0 + LANE]
    assert i0 % LANE == 0 and s[0] == s[-1] and len(set(s.tolist())) == 2
    th = [(q[1] + i * q[0]) % (1 << 64) for i in (i0, i0 + LANE - 1)]
    assert ((th[0] + (1 << 62)) % (1 << 64)) >> 63 != ((th[1] + (1 << 62)) % (1 << 64)) >> 63
    assert all(t not in (1 << 62, 3 << 62) for t in th)          # strictly inside
    x = oc.rows(3, 65792, 3)
    got = _check(x, n, n, [q, oc.quant(1000.3, 0.0, 0.1)], 65792)
    src = np.arange(i0, i0 + LANE) + s
    np.testing.assert_array_equal(got[1, 0, i0:i0 + LANE], x[1, src])
    assert np.any(src != src[0] + np.arange(LANE))               # the source bytes are not contiguous


def test_kernel_both_clamps_and_exact_halves():
    n = 4096
    x = oc.rows(3, n, 11)
    _check(x, n, n, [oc.clamp_case(n)], n)
    q, hits = oc.exact_half_case(8192)
    x = oc.rows(3, 8192 + 37, 12)
    got = _check(x, 8192 + 37, 8192, [q], 8192 + 37)
    s = ref.orbit_shift(8192, q)
    for h in hits:
        assert got[0, 0, h] == x[0, h + s[h]]


def test_kernel_many_rows_and_templates():
    n, nrow = 4101, 4138
    x = oc.rows(7, 4352, 23)
    _check(x, nrow, n, [oc.quant(700.0 + 311.0 * k, 1.7 * k, 0.083 * k) for k in range(13)], 4352)
    # a row longer than one workgroup's tiles: the second workgroup starts mid-row
    n = C.ORBIT_TILE * C.ORBIT_TILES_PER_GROUP + 4101
    x = oc.rows(2, n + 11, 29)
    _check(x, n + 11, n, [oc.quant(n / 3.0, 40.0, 0.37), oc.quant(5000.0, 300.0, 0.25)], n + 11 + 5)


def test_kernel_refusals():
    import torch

    from peasoup_amd import ops

    d = torch.zeros((2, 256), dtype=torch.uint8, device="cuda")
    q = oc.quant(100.0, 3.0, 0.0)
    dq = torch.tensor([list(q)], dtype=torch.int64, device="cuda")
    tab = torch.from_numpy(ref.orbit_sine_table().copy()).cuda()
    out = torch.zeros((2, 1, 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):
        C.orbit_resample_raw(d.data_ptr(), 256, 2, 256, 256, [q], dq.data_ptr(), tab.data_ptr(), d.data_ptr() + 16, 256, 0)
    with pytest.raises(RuntimeError, match="span must be in 1..nrow"):           # n > nrow
        C.orbit_resample_raw(d.data_ptr(), 256, 2, 256, 300, [q], dq.data_ptr(), tab.data_ptr(), out.data_ptr(), 256, 0)
    with pytest.raises(ValueError):
        ops.orbit_resample(d, 300, (), 0.0, quant=[q])
    with pytest.raises(RuntimeError, match="templates per launch"):              # K > 4096
        ops.orbit_resample(d, 256, (), 0.0, quant=[q] * 4097)
    with pytest.raises(RuntimeError, match="Aq >= 2\\^30"):
        ops.orbit_resample(d, 256, (), 0.0, quant=[(q[0], q[1], 1 << 30)])
    with pytest.raises(RuntimeError, match="pb < 64 tsamp"):
        ops.orbit_resample(d, 256, [(32 * TS, 0.0, 0.0)], TS)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0


# ------------------------------------------------------ the identity bank ----
def _orbit_args(path, extra):
    ok, _, args = C.parse_orbit_cmdline(["orbsearch", "-i", path] + [str(e) for e in extra])
    assert ok
    return args


def _bits(v):
    return np.float32(v).view(np.uint32)


def _bankfile(tmp, text, name="bank.txt"):
    p = os.path.join(str(tmp), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_identity_bank_equals_the_plain_search(tmp_path):
    """2^16 samples, 64 channels, 2-bit, 4 DMs, +-acc with a few trials: run_orbit_search with the one-template bank
    pb=100 a1=0 ph=0 returns exactly the candidates of the existing single-device search, bit patterns and order."""
    from peasoup_amd.models.orbit import run_orbit_search

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
    args = _orbit_args(path, opts + ["-o", str(tmp_path / "orb.out"), "--bankfile", _bankfile(tmp_path, "100 0 0\n")])
    res = run_orbit_search(args)
    assert res.setup.bank == [(100.0, 0.0, 0.0)] and res.template_trials == 4
    assert 2 < len(res.setup.accel_plan.generate(0.0)) < 40
    got = res.candidates
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.tmpl == 0
        assert (g.cand.dm_idx, g.cand.nh) == (w.dm_idx, w.nh)
        for f in ("dm", "acc", "snr", "freq"):
            assert _bits(getattr(g.cand, f)) == _bits(getattr(w, f)), f
        assert _bits(1.0 / g.cand.freq) == _bits(1.0 / w.freq)
        assert g.cand.count_assoc() == w.count_assoc()


# ---------------------------------------------------------------- recovery ----
NS3 = 1 << 17
P3 = 0.0101
AMP3 = 0.1
SEED3 = 1
MIN_SNR = 9.0   # the default -m: what a run without a candidate stayed below
GRID3 = (40.0, 90.0, 3, 0.0, 0.0144, 4, 4)      # pb 40, 60, 90 s; a1 0 ... 45 samples; 4 phases
TRUE3 = 16 + 2 * 4 + 3                          # pb = 60 s, a1 = 0.0096 ls = 30 samples, phase 0.75


@functools.lru_cache(maxsize=None)
def _recovery(tmp):
    """The two files of the recovery test and the options of its three runs."""
    hdr = dict(synthetic.make_header(nchans=64, nbits=8, tsamp=320e-6))
    hdr["nsamples"] = NS3
    truth = ref.orbit_grid(*GRID3)[TRUE3]
    assert truth[0] == 60.0 and truth[2] == 0.75 and abs(truth[1] / TS - 30.0) < 0.01
    spec = dict(period=P3, dm=20.0, duty=0.05, amplitude=AMP3)
    plain = os.path.join(tmp, "plain.fil")
    write_filterbank(plain, hdr, synthetic.generate(NS3, hdr, [PulsarSpec(**spec)], seed=SEED3))
    orbital = os.path.join(tmp, "orbital.fil")
    write_filterbank(orbital, hdr, synthetic.generate(NS3, hdr, [PulsarSpec(orbit=truth, **spec)], seed=SEED3))
    # (the default transform is the power of two below the file's 2^17 samples: ask for all of them); acc 0 only
    base = ["--dm_start", 20, "--dm_end", 20, "--fft_size", NS3, "--acc_start", 0, "--acc_end", 0]
    ident = ["--bankfile", _bankfile(tmp, "100 0 0\n", "identity.txt")]
    grid = ["--pb_start", GRID3[0], "--pb_end", GRID3[1], "--npb", GRID3[2], "--a1_start", GRID3[3], "--a1_end",
            repr(GRID3[4]), "--na1", GRID3[5], "--nphase", GRID3[6]]
    return plain, orbital, truth, base, ident, grid


@pytest.fixture(scope="module")
def recovery(tmp_path_factory):
    return _recovery(str(tmp_path_factory.mktemp("orbit_recovery")))


def test_recovery_of_an_injected_orbit(recovery, tmp_path):
    """A 42 s series of a 10.1 ms pulsar on a 60 s orbit of 30 samples amplitude (0.7 of an orbit: no Taylor term
    helps).  (a) the same pulsar without an orbit through the identity bank: the ceiling; (b) the orbital data
    through the identity bank: the floor (the -m threshold when nothing is found); (c) the orbital data through the
    3 x 4 x 4 grid that holds the truth.  The top candidate of (c) is at the true grid point, above the midpoint of
    (a) and (b), at the injected period within the distillers' freq_tol."""
    from peasoup_amd.models.orbit import run_orbit_search

    plain, orbital, truth, base, ident, grid = recovery
    out = ["-o", str(tmp_path / "o.txt")]
    a = run_orbit_search(_orbit_args(plain, base + ident + out), write=False)
    b = run_orbit_search(_orbit_args(orbital, base + ident + out), write=False)
    c = run_orbit_search(_orbit_args(orbital, base + grid + out), write=False)
    assert c.setup.bank[TRUE3] == truth and len(c.setup.bank) == 48 and c.template_trials == 48
    assert len(c.setup.accel_plan.generate(20.0)) == 1
    sa, sb, top = a.candidates[0].cand.snr, (b.candidates[0].cand.snr if b.candidates else MIN_SNR), c.candidates[0]
    print(f"S/N (a) {sa:.3f} (b) {sb:.3f}{'' if b.candidates else ' (no candidate: the threshold)'} "
          f"(c) {top.cand.snr:.3f} at template {top.tmpl} {c.setup.bank[top.tmpl]}, period {1.0 / top.cand.freq:.9g}")
    assert abs(1.0 / a.candidates[0].cand.freq / P3 - 1) < 1e-4
    assert top.tmpl == TRUE3
    assert top.cand.snr > 0.5 * (sa + sb)
    assert abs(1.0 / top.cand.freq / P3 - 1) < 1e-4


# ------------------------------------------------------- the two drivers ----
def _cand_lines(path):
    with open(path) as f:
        return [ln for ln in f if not ln.startswith("#")]


def test_native_and_python_drivers_write_the_same_lines(recovery, tmp_path):
    plain, orbital, truth, base, ident, grid = recovery
    opts = [str(o) for o in base + grid + ["--npdmp", 3, "--limit", 50]]
    o1, o2 = str(tmp_path / "native.out"), str(tmp_path / "module.out")
    r = subprocess.run([os.path.join(REPO, "bin", "orbsearch"), "-i", orbital, "-o", o1] + opts, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "orb", "-i", orbital, "-o", o2] + opts,
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    l1, l2 = _cand_lines(o1), _cand_lines(o2)
    assert len(l1) >= 1 and l1 == l2
    first = l1[0].split()
    assert len(first) == 11 and tuple(float(v) for v in first[3:6]) == truth   # the template columns hold the grid point
    assert any(float(ln.split()[9]) != 0 for ln in l1)                          # --npdmp folded the re-made rows
    with open(o1) as f:
        head = [ln for ln in f if ln.startswith("#")]
    assert any("pb_start 40 pb_end 90 npb 3" in ln and "nphase 4" in ln for ln in head)
    assert any(ln.startswith("# templates 48 ") for ln in head) and any("intrinsic" in ln for ln in head)
    assert any("acc_start 0 acc_end 0" in ln for ln in head) and any("bankfile -" in ln for ln in head)
    assert head[-1].split()[1:] == "period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx".split()
    assert not os.path.exists(o1 + ".tmp")


# ---------------------------------------------------------------- refusals ----
def _refused(tmp_path, fil, extra, what):
    out = str(tmp_path / "refused.out")
    r = subprocess.run([os.path.join(REPO, "bin", "orbsearch"), "-i", fil, "-o", out] + [str(e) for e in extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert what in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_every_refusal_reaches_the_user_by_name(recovery, tmp_path):
    plain, ident = recovery[0], recovery[4]
    dm = ["--dm_start", 20, "--dm_end", 20]
    for extra, what in oc.refusal_cases(tmp_path):
        _refused(tmp_path, plain, dm + extra, what)
    _refused(tmp_path, plain, dm + ident + ["-t", 2], "one device")
    _refused(tmp_path, oc.big_file(tmp_path), ["--dm_start", 0, "--dm_end", 0, "--fft_size", 1 << 27] + ident,
             "longer than 2^26")
