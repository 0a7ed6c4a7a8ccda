"""Templates and oracle-found cases shared by test_orbit.py (host transcription)
and test_orbit_gpu.py (kernel): the same shapes reach the same paths."""
import os

import numpy as np

from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import write_filterbank

TS = float(np.float32(320e-6))
LANE = 16
SHAPES = [(n, pad) for n in (1, 15, 16, 17, 4101, 65539) for pad in (0, 37)]


def rows(nrows, row_stride, seed):
    return np.random.default_rng(seed).integers(0, 256, (nrows, row_stride), dtype=np.uint8)


def quant(pb_samples, amp_samples, ph):
    return ref.orbit_quantise(pb_samples * TS, amp_samples * TS, ph, TS)


def templates(n):
    """Every amplitude (0, 0.4 = identity, 3, 40, 1000 samples) at every orbital period (64 samples, n / 3, n, 10 n;
    none below the 64 samples the quantisation admits) and every phase (0; 0.25, starting on a turning point; 0.37):
    60 quantised templates."""
    out = []
    for amp in (0.0, 0.4, 3.0, 40.0, 1000.0):
        for pb in (64.0, max(64.0, n / 3.0), max(64.0, float(n)), max(64.0, 10.0 * n)):
            for ph in (0.0, 0.25, 0.37):
                out.append(quant(pb, amp, ph))
    return out


def groups(tpl):
    """K of 1, 5 and 13 (and the rest): every template is used once."""
    out, k = [], 0
    for size in (1, 5, 13, 13, 13, len(tpl)):
        if k < len(tpl):
            out.append(tpl[k:k + size])
            k += size
    return out


def check_rows(got, x, nrow, n, tpl):
    """got [nrows, K, nrow] against the oracle, byte for byte."""
    i = np.arange(n, dtype=np.int64)
    for k, q in enumerate(tpl):
        src = np.clip(i + ref.orbit_shift(n, q), 0, n - 1)
        for r in range(x.shape[0]):
            want = x[r, :nrow].copy()
            want[:n] = x[r, src]
            np.testing.assert_array_equal(got[r, k], want, err_msg=f"row {r} template {q}")
    np.testing.assert_array_equal(ref.orbit_resample(x[0, :nrow], n, tpl[0]), got[0, 0])


def turning_case(n=65539):
    """A template and a lane start i0 whose 16-sample span has a turning point of the sine strictly inside, equal
    shifts at its two ends and another shift inside: a wide load taken there would show.  Found with the oracle."""
    i = np.arange(n, dtype=np.uint64)
    for amp in np.arange(100.0, 140.0, 0.37):
        q = quant(1000.3, float(amp), 0.1)
        s = ref.orbit_shift(n, q)
        with np.errstate(over="ignore"):
            th = np.uint64(q[1]) + i * np.uint64(q[0])
            top = (th + np.uint64(1 << 62)) >> np.uint64(63)
        on_point = (th == np.uint64(1 << 62)) | (th == np.uint64(3 << 62))
        for i0 in range(0, n - LANE, LANE):
            a, b = i0, i0 + LANE - 1
            if top[a] != top[b] and not on_point[a] and not on_point[b] and s[a] == s[b] \
                    and len(set(s[a:b + 1].tolist())) == 2:
                return q, i0
    raise AssertionError("no lane span with a turning point inside and equal end shifts")


def clamp_case(n=4096):
    """Most indices clamp, at both ends: an amplitude of 10 n over an orbit of n samples."""
    q = quant(float(n), 10.0 * n, 0.0)
    j = np.arange(n, dtype=np.int64) + ref.orbit_shift(n, q)
    assert np.mean(j > n - 1) > 0.4 and np.mean(j < 0) > 0.4
    return q


def exact_half_case(n=8192):
    """A template at which Aq (S - S(F)) + 2^37 is an exact multiple of 2^38 inside the row.  An orbit of 4096 samples
    from phase 0 puts every sample on a table entry, so S(th_1024) = T[1024] = 2^30 exactly; Aq = 81 * 2^7 (40.5
    samples) then gives 81 * 2^37 + 2^37 at i = 1024 (+ 4096 k) and -81 * 2^37 + 2^37 at i = 3072.  The oracle confirms
    it and returns the indices."""
    q = quant(4096.0, 40.5, 0.0)
    assert q == (1 << 52, 0, 81 << 7)
    with np.errstate(over="ignore"):
        th = np.uint64(q[1]) + np.arange(n, dtype=np.uint64) * np.uint64(q[0])
    v = np.int64(q[2]) * (ref.orbit_sine(th) - int(ref.orbit_sine(np.array([q[1]], dtype=np.uint64))[0])) + (1 << 37)
    hits = np.nonzero((v % (1 << 38) == 0) & (v != 0))[0]
    s = ref.orbit_shift(n, q)
    assert 1024 in hits and 3072 in hits and s[1024] == 41 and s[3072] == -40
    assert all(0 <= h + s[h] < n for h in hits)  # not hidden by a clamp
    return q, hits


def bank_file(tmp_path, text, name="bank.txt"):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text)
    return p


def refusal_cases(tmp_path):
    """(extra options, the name the refusal carries), shared with the GPU test of the binary."""
    b = lambda text, name: ["--bankfile", bank_file(tmp_path, text, name)]  # noqa: E731
    return [
        (b("100 0 nan\n", "nan.txt"), "non-finite"),
        (b("inf 0 0\n", "inf.txt"), "non-finite"),
        (["--pb_start", "nan", "--pb_end", 100, "--npb", 2, "--na1", 1, "--nphase", 1], "non-finite"),
        (b("100 0 0\n0.01 0 0\n", "short.txt"), "pb < 64 tsamp"),
        (b("100 -0.001 0\n", "neg.txt"), "a1 < 0"),
        (b("1e9 2000 0\n", "aq.txt"), "Aq >= 2^30"),
        (b("100 20 0\n", "fast.txt"), "0.9 samples per sample"),
        (b("# no template\n\n", "empty.txt"), "empty bank"),
        (["--pb_start", 100, "--pb_end", 200, "--npb", 1025, "--a1_end", 1, "--na1", 1024, "--nphase", 1],
         "more than 2^20 templates"),
        (b("100 0 0\n100 0\n", "bad.txt"), "bank line 2 is malformed"),
        ([], "exactly one source"),
        (b("100 0 0\n", "both.txt") + ["--npb", 1, "--na1", 1, "--nphase", 1, "--pb_start", 100], "exactly one source"),
        (["--bankfile", str(tmp_path / "missing.txt")], "cannot open the bank file"),
        (["--pb_start", 100, "--pb_end", 200, "--npb", 2, "--na1", 0, "--nphase", 1], "at least 1"),
    ]


def big_file(tmp_path):
    """n > 2^26 from the header alone: a sparse 1-bit file whose data block is never read."""
    big = str(tmp_path / "big.fil")
    hdr = synthetic.make_header(nchans=8, nbits=1, tsamp=64e-6)
    hdr["nsamples"] = (1 << 26) + 4096
    write_filterbank(big, hdr, np.zeros((0, 8), dtype=np.uint8))
    with open(big, "r+b") as f:
        f.truncate(os.path.getsize(big) + hdr["nsamples"])
    return big
