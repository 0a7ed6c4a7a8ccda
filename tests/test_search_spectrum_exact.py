"""The search spectrum of the fused FFT passes against a float64 oracle at unit scale.

The kernels under test are the fused resample + pass A (fft4step.hip
fft4_colpass_onex_kernel and its Stockham sibling fft4_colpass_kernel) and the
fused spectrum pass (fft4_rowpass_spectrum_kernel), at every four-step
geometry from 2^15 (128 x 128) to 2^25 (4096 x 4096).  The oracle
(utils/reference.py search_spectrum) is the definition in float64: exact-index
resampling, numpy's real FFT, the interbinned amplitude, (amp - mean) / sigma.

Inputs are seeded integers in [-8, 8] (exact in float32; a gather that reads
a neighbouring sample changes the value with probability 16/17), optionally
plus a sinusoid of amplitude 50.  The normalisation is always at unit scale:
mean = 0.8 rms|X|, sigma = 0.4 rms|X| (rms|X| of the acc = 0 spectrum, from
Parseval's identity), so P is O(1) with both signs and the screening bytes
take many values (asserted: at least 32 per row of Q on noise input).

Errors are absolute errors of P per bin, in units of rms|X| / sigma (that is,
the error of the amplitude relative to rms|X|).

Measured error (MI355X, the kernels as of this module's first commit, noise
input, worst trial; `fused` = fft4_spectrum_pass, `unfused` =
fft4_resample_interbin):

    log2 n   fused max   fused rms   unfused max  unfused rms
      15     9.91e-07    1.93e-07    1.12e-06     1.78e-07
      16     1.09e-06    2.03e-07    9.66e-07     1.84e-07
      17     1.09e-06    2.15e-07    1.09e-06     1.95e-07
      18     1.68e-06    2.33e-07    1.44e-06     2.10e-07
      19     1.77e-06    2.39e-07    1.53e-06     2.17e-07
      20     1.70e-06    2.26e-07    1.61e-06     2.06e-07
      21     1.74e-06    2.26e-07    1.74e-06     2.06e-07
      22     1.80e-06    2.12e-07    1.49e-06     1.98e-07
      23     1.40e-06    2.00e-07    1.22e-06     1.76e-07
      24     1.30e-06    2.09e-07    1.25e-06     1.85e-07
      25     1.64e-06    2.12e-07    1.67e-06     1.99e-07

(about 10 x numpy's complex64 FFT; a P of size 2 stored in float32 is itself
on a grid of 1e-7 of rms|X| / sigma.)  No length comes near the caps.

tol = 4 x the measured value of the worse path per log2 n (TOL below), under
the caps 2e-5 (max) and 2e-6 (rms).

Bright line (b): a float32 P cannot be closer to its float64 value than half
an ulp, and at the line bins |P| is ~ sqrt(M) / 0.4 (all the power in one or
two bins), whose float32 grid alone is 6e-5 of rms|X| / sigma at 2^21 -- above
the 2e-5 cap for any float32 kernel.  Bins with |P| > 8 (there are none on
noise input) therefore get an allowance of 2^-22 (|P| - 8) on top of tol_max:
four float32 half-ulps of the stored value, for the stored P, the division,
the square root and the amplitude's own relative rounding.  Bin k is formed
from Z_k and Z_{M-k} of the packed half-length transform and from X_{k-1}, so
the same allowance of bins k - 1, M - k and M - k + 1 is added to bin k's: a
float32 Z_{M-k} holding the line carries the line's rounding into bin k
(measured: 7.9e-6 at bin M - 1 for a line at 1.5, 4e-8 of the line).  And a
float32 butterfly that adds the line to a noise value rounds at the line's
ulp wherever that butterfly's outputs go, so every bin also gets the
allowance of the largest bin (measured, both paths alike: up to 4.4e-5 at
2^21 in bins such as 7 M / 8 + 1, one float32 ulp of the line; with tol_max
alone every case of this test fails for that reason).  The rms bound is
tol_rms unchanged, and an index mistake near the line is an error of the
line's own size, 10^6 times the allowance.

Exact gather (c): the inverse float64 FFT of fft4_resample_spectrum's Z,
rounded to integers, must equal the resampled series sample for sample.  The
literal accelerations in ACCS were chosen on the CPU (float32 acc, tsamp =
float32(64e-6), as accel_factor sees them):
  * "safe": no sample's read position is within 1e-6 of a rounding tie;
  * "ulp": no sample within max(2e-8, ten ulps of the position in double).
    For any acceleration whose shift exceeds one sample about 2e-6 n samples
    lie within 1e-6 of a tie (every tie crossing at slope s has one sample
    within s / 2), so at 2^21 and above -- and for the fixed +-500 from 2^20
    -- the 1e-6 margin does not exist; ten ulps still make numpy's and the
    device's double arithmetic round alike, so a difference is an index bug;
  * "tie": the minimum distance from a tie is in [2e-8, 8e-8], inside the
    span path's 1e-7 guard.  Below 2^20 the shift at +-500 m/s^2 stays under
    half a sample, so these (and the vertex-plateau and |af| n = 0.3 cases)
    are larger, unphysical accelerations; the kernels take any af.
test_literal_accelerations_are_where_stated checks all of this without a GPU.

The CPU tests also build six defective oracles (a sample off by one, no
interbin, interbin factor 0.45, two bins swapped, a wrapped bin 0, one
four-step column's twiddles off by a phase of 1e-5).  The first five exceed
the tolerances at 2^15 and 2^20 by orders of magnitude (asserted).  The sixth
does NOT, at either length: one column of N1 perturbed by 1e-5 moves the
spectrum by max 2.98e-6 / rms 6.2e-7 at 2^15 (tolerance 4.5e-6 / 7.7e-7) and
max 8.3e-7 / rms 2.2e-7 at 2^20 (6.8e-6 / 9.1e-7) -- at 2^20 no more than the
kernels' own measured rounding, most of which is the float32 grid of the
stored P.  A twiddle error of that size in a single column is below what a
comparison of float32 P can resolve; the tolerances are not widened or
narrowed for it, and its test only prints the figures.
"""
import functools

import numpy as np
import pytest

from peasoup_amd.utils import reference as ref

dev = "cuda"
TSAMP = 64e-6
LOG2NS = list(range(15, 26))

# tol_max, tol_rms per log2 n, in units of rms|X| / sigma
TOL_CAP = (2e-5, 2e-6)
MEASURED = {15: (1.123e-6, 1.927e-7), 16: (1.091e-6, 2.030e-7), 17: (1.093e-6, 2.150e-7), 18: (1.681e-6, 2.330e-7),
            19: (1.767e-6, 2.390e-7), 20: (1.703e-6, 2.263e-7), 21: (1.737e-6, 2.255e-7), 22: (1.796e-6, 2.118e-7),
            23: (1.402e-6, 1.997e-7), 24: (1.303e-6, 2.088e-7), 25: (1.666e-6, 2.117e-7)}  # the worse path
TOL = {lg: (min(4 * m, TOL_CAP[0]), min(4 * r, TOL_CAP[1])) for lg, (m, r) in MEASURED.items()}

FFT4_FLAG_SETS = [None, 0, 1, 259, 1299, 3331, 7427, 15619, 81155, 212227]  # test_kernels_gpu.py: the kernel-shape chain

_S = [470.0, 407.3333435058594, 344.6666564941406, 282.0, 219.3333282470703, 156.6666717529297, 94.0,
      31.33333396911621]
_SPREAD = [-a for a in _S] + _S[::-1]
# log2n -> accelerations by class (see the module docstring); vertex-plateau values come after the spread ones,
# the |af| n = 0.3 one last
ACCS = {
    15: dict(safe=[0.0, 500.0, -500.0] + _SPREAD + [17448.47265625, 85771312.0], ulp=[],
             tie=[52350.65234375, -87251.1015625]),
    16: dict(safe=[0.0, 500.0, -500.0] + _SPREAD + [4362.1181640625, 42885656.0], ulp=[],
             tie=[13087.6630859375, -21812.775390625]),
    17: dict(safe=[0.0, 500.0, -500.0] + _SPREAD + [1090.529541015625, 21442828.0], ulp=[],
             tie=[3271.915771484375, -5453.19580078125]),
    18: dict(safe=[0.0, 500.0, -500.0, -470.0, -407.3333740234375, -344.6666564941406, -269.0, -219.3333282470703,
                   -156.6666717529297, -94.0, -31.33333396911621, 31.33333396911621, 94.0, 156.6666717529297,
                   219.3333282470703, 295.0008544921875, 344.6666564941406, 407.3333740234375, 470.0,
                   272.63238525390625, 10721414.0],
             ulp=[], tie=[817.9789428710938, -1363.301025390625]),
    19: dict(safe=[0.0, -470.0, -407.3333435058594, -344.6686706542969, -282.0, -219.3333740234375,
                   -156.6666717529297, -94.00028991699219, -31.33333396911621, 31.33333396911621,
                   94.00028991699219, 156.6666717529297, 219.3333740234375, 282.0, 344.6686706542969,
                   407.3333435058594, 470.0, 68.15809631347656, 340.81817626953125, 5360708.0],
             ulp=[500.0, -500.0], tie=[204.49473571777344, -340.8265380859375]),
    20: dict(safe=[0.0, -470.0, -407.3334045410156, -344.6667175292969, -282.0, -219.3333282470703,
                   -156.66668701171875, -94.00017547607422, -31.333417892456055, 31.333417892456055,
                   94.00017547607422, 156.66668701171875, 219.3333282470703, 282.0, 344.6667175292969,
                   407.3334045410156, 470.0, 17.03952407836914, 255.61671447753906, 2680353.5],
             ulp=[500.0, -500.0], tie=[113.00027465820312, -331.0]),
    21: dict(safe=[0.0, 4.259881019592285, 251.35769653320312], ulp=[500.0, -500.0] + _SPREAD + [1340176.75],
             tie=[113.00004577636719, -331.00018310546875]),
    22: dict(safe=[0.0, 1.0649702548980713], ulp=[500.0, -500.0] + _SPREAD + [250.29293823242188, 670088.375],
             tie=[113.00003051757812, -331.0]),
    23: dict(safe=[0.0, 0.2662425637245178],
             ulp=[500.0, -500.0] + [a if abs(a) != 219.3333282470703 else float(np.sign(a)) * 219.33334350585938
                                    for a in _SPREAD] + [250.02674865722656, 335044.1875],
             tie=[113.00001525878906, -331.0000915527344]),
    24: dict(safe=[], ulp=[-437.0, 167522.09375], tie=[]),
    25: dict(safe=[], ulp=[-437.0000305175781, 83761.0703125], tie=[]),
}


def _accs(log2n):
    a = ACCS[log2n]
    return a["safe"] + a["ulp"] + a["tie"]


def _ulp_floor(log2n):
    return max(2e-8, 10.0 * 2.0 ** (log2n - 1 - 52))


def _tie_distance(acc, n, chunk=1 << 22):
    """min over samples of | frac(read position) - 0.5 |, in double as resample_ii evaluates it"""
    af = ref.accel_factor(acc, TSAMP)
    best = 1.0
    for s in range(0, n, chunk):
        i = np.arange(s, min(n, s + chunk), dtype=np.float64)
        pos = i + i * af * (i - n)
        best = min(best, float(np.abs(pos - np.floor(pos) - 0.5).min()))
    return best


# ------------------------------------------------------------------ inputs --
@functools.lru_cache(maxsize=2)
def _noise(log2n):
    # The first seed whose X_0 = sum x and X_M = sum (-1)^i x_i have opposite signs, |X_M| > |X_0| > 0.3 rms|X|:
    # only then does bin 0 change when X_{-1} is taken as X_M (0.5 |X_0 - X_M|^2 > 2 |X_0|^2), so that
    # mistake in a kernel is visible in bin 0 of every test below.
    for seed in range(7000 + log2n, 13000, 100):
        x = np.random.default_rng(seed).integers(-8, 9, size=1 << log2n).astype(np.float32)
        x0, xm = float(x.sum(dtype=np.float64)), float(x[0::2].sum(dtype=np.float64) - x[1::2].sum(dtype=np.float64))
        if x0 * xm < 0 and abs(xm) > abs(x0) > 0.3 * np.sqrt(24.0 * len(x)):
            break
    else:
        raise AssertionError("no seed")
    x.setflags(write=False)
    return x


def _with_line(log2n, fbin):
    """noise plus 50 sin(2 pi fbin i / n), fbin in (fractional) bins of the n-point spectrum"""
    n = 1 << log2n
    i = np.arange(n, dtype=np.float64)
    return (_noise(log2n).astype(np.float64) + 50.0 * np.sin(2.0 * np.pi * (fbin / n) * i)).astype(np.float32)


def _rms_spectrum(x):
    """rms over the n/2 + 1 bins of |rfft(x)|, by Parseval: sum_{k <= M} |X_k|^2 =
    (n sum x^2 + X_0^2 + X_M^2) / 2 with X_0 = sum x, X_M = sum (-1)^i x_i."""
    x = x.astype(np.float64)
    n = len(x)
    x0, xm = x.sum(), x[0::2].sum() - x[1::2].sum()
    return float(np.sqrt(0.5 * (n * np.dot(x, x) + x0 * x0 + xm * xm) / (n // 2 + 1)))


def _unit_scale(x):
    """(stats row, nscale, mean, sigma, rms|X|): mean = 0.8 rms|X| and sigma = 0.4 rms|X| as the kernels form
    them in float32 (stats[0] * nscale, stats[2] * nscale; nscale = n is a power of two, so both are exact)."""
    n = len(x)
    rms = _rms_spectrum(x)
    m, s = np.float32(0.8 * rms / n), np.float32(0.4 * rms / n)
    return [float(m), 0.0, float(s), 0.0], float(n), float(m) * n, float(s) * n, rms


def _spectrum_accs(log2n):
    if log2n == 17:
        return [-500.0, -37.5, 0.0, 3.0, 499.0, 250.0, -250.0, 120.0, -7.0]  # K = 9: one trial into the next 8
    if log2n <= 21:
        return [-500.0, -37.5, 0.0, 3.0, 499.0]
    return [-500.0, 0.0, 499.0] if log2n <= 23 else [-37.5]


@functools.lru_cache(maxsize=1)
def _noise_oracle(log2n):
    x = _noise(log2n)
    st, nscale, mean, sigma, rms = _unit_scale(x)
    P = np.stack([ref.search_spectrum(x, a, TSAMP, mean, sigma) for a in _spectrum_accs(log2n)])
    P.setflags(write=False)
    return P


def _named_bins(n1, n2):
    M = n1 * n2
    return {"0": 0, "1": 1, "n2/2": n2 // 2, "n2/2+1": n2 // 2 + 1, "n2-1": n2 - 1, "n2": n2, "M/2": M // 2,
            "M-1": M - 1, "M": M}


def _errors(P, Pref, sigma, rms):
    """(err per bin [K, M + 1], worst trial's max, worst trial's rms) in units of rms|X| / sigma"""
    err = np.abs(P.astype(np.float64) - Pref) * (sigma / rms)
    return err, float(err.max()), float(np.sqrt((err ** 2).mean(axis=1)).max())


def _run_path(path, x, accs, st, nscale):
    """(P natural order [K, M + 1] float32, Q bytes of bins 0..M or None, geometry)"""
    import torch

    import peasoup_amd._C as C
    from peasoup_amd import ops

    xd = torch.from_numpy(np.array(x)).to(dev)
    std = torch.tensor(st, dtype=torch.float32, device=dev)
    if path == "fused":
        Pb, Q, g = ops.fft4_spectrum_pass(xd, accs, TSAMP, std, nscale)
        sh = C.kernels.spec_q_shift
        M = g.n1 * g.n2
        return ops.spec_unblock(Pb, g).cpu().numpy(), Q.cpu().numpy()[:, sh:sh + M + 1], g
    g = C.kernels.fft4_geometry(len(x) // 2)
    return ops.fft4_resample_interbin(xd, accs, TSAMP, std, nscale).cpu().numpy(), None, g


def measure_noise(log2n, path):
    """The figures of test_spectrum_against_oracle without its assertions."""
    x = _noise(log2n)
    st, nscale, mean, sigma, rms = _unit_scale(x)
    P, Q, g = _run_path(path, x, _spectrum_accs(log2n), st, nscale)
    err, emax, erms = _errors(P, _noise_oracle(log2n), sigma, rms)
    return P, Q, g, err, emax, erms


# --------------------------------------------------------------- GPU tests --
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "unfused"])
@pytest.mark.parametrize("log2n", LOG2NS)
def test_spectrum_against_oracle(log2n, path):
    """(a) every geometry, both paths, per bin against the float64 definition."""
    P, Q, g, err, emax, erms = measure_noise(log2n, path)
    M = g.n1 * g.n2
    assert g.ok and P.shape == (len(_spectrum_accs(log2n)), M + 1)
    tol_max, tol_rms = TOL[log2n]
    named = {k: float(err[:, b].max()) for k, b in _named_bins(g.n1, g.n2).items()}
    print(f"log2n={log2n} {path}: max {emax:.3e} rms {erms:.3e} (tol {tol_max:.1e} / {tol_rms:.1e}) named {named}")
    for name, e in named.items():
        assert e < tol_max, f"bin {name}: error {e:.3e} of rms|X|/sigma"
    assert emax < tol_max, (int(np.argmax(err.max(axis=0))), emax)
    assert erms < tol_rms, erms
    if Q is not None:
        for row in Q:
            assert len(np.unique(row)) >= 32, "the screening bytes take too few values to show a misplaced one"
        assert np.array_equal(Q, ref.q8(P))


LINE_CASES = [(lg, k, half) for lg in (17, 21) for k in ("1", "n2/2", "n2-1", "M/2", "M-2") for half in (0.5, 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,kname,half", LINE_CASES)
def test_bright_line_against_oracle(log2n, kname, half):
    """(b) a line of amplitude 50 at bin k (+ 0.5: the interbin branch), both paths, acc 0 and 120."""
    import peasoup_amd._C as C

    g = C.kernels.fft4_geometry((1 << log2n) // 2)
    M = g.n1 * g.n2
    k = {"1": 1, "n2/2": g.n2 // 2, "n2-1": g.n2 - 1, "M/2": M // 2, "M-2": M - 2}[kname]
    x = _with_line(log2n, k + half)
    st, nscale, mean, sigma, rms = _unit_scale(x)
    accs = [0.0, 120.0]
    Pref = np.stack([ref.search_spectrum(x, a, TSAMP, mean, sigma) for a in accs])
    tol_max, tol_rms = TOL[log2n]
    # float32 grid of the few line-dominated bins (module docstring)
    big = np.maximum(np.abs(Pref) - 8.0, 0.0)
    prev = np.concatenate([np.zeros((len(accs), 1)), big[:, :-1]], axis=1)  # X_{k-1} enters bin k's interbin term
    nxt = np.concatenate([big[:, 1:], np.zeros((len(accs), 1))], axis=1)  # (so that the mirror of k - 1 is covered)
    own = big + prev + nxt
    # [:, ::-1]: the mirror bins M - k; big.max: the line's rounding in a butterfly lands in any bin
    bound = tol_max + 2.0 ** -22 * (own + own[:, ::-1] + big.max(axis=1, keepdims=True)) * (sigma / rms)
    around = np.arange(max(k - 3, 0), min(k + 5, M + 1))
    for path in ("fused", "unfused"):
        P, Q, _ = _run_path(path, x, accs, st, nscale)
        err, emax, erms = _errors(P, Pref, sigma, rms)
        print(f"log2n={log2n} k={kname}+{half} {path}: max {emax:.3e} rms {erms:.3e} "
              f"around the line {err[:, around].max(axis=0)} bound {bound[:, around].max(axis=0)}")
        for b in around:
            assert (err[:, b] < bound[:, b]).all(), f"{path}: bin {b} (line at {k + half}): {err[:, b]}"
        worst = int(np.argmax((err / bound).max(axis=0)))
        assert (err < bound).all(), f"{path}: bin {worst}: {err[:, worst]} bound {bound[:, worst]}"
        assert erms < tol_rms, (path, erms)
        if Q is not None:
            assert np.array_equal(Q, ref.q8(P))


@functools.lru_cache(maxsize=1)
def _resampled(log2n):
    """resample_ii of the noise at every acceleration of ACCS[log2n], as int8 [K, n]"""
    x = _noise(log2n)
    R = np.stack([ref.resample_ii(x, ref.accel_factor(a, TSAMP)).astype(np.int8) for a in _accs(log2n)])
    R.setflags(write=False)
    return R


GATHER_CASES = [(lg, f) for lg in LOG2NS for f in (FFT4_FLAG_SETS if lg in (15, 16, 18, 21, 23) else [None])]


@pytest.fixture
def fft4_flags(request):
    import peasoup_amd._C as C

    old = C.kernels.fft4_flags()
    try:
        if request.param is not None:
            C.kernels.fft4_set_flags(request.param)
        yield request.param
    finally:
        C.kernels.fft4_set_flags(old)


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,fft4_flags", GATHER_CASES, indirect=["fft4_flags"])
def test_gather_is_exact_through_the_inverse_transform(log2n, fft4_flags):
    """(c) every sample pass A gathers, recovered from the fused FFT's spectrum, is resample_ii's."""
    import scipy.fft
    import torch

    from peasoup_amd import ops

    x = _noise(log2n)
    n = len(x)
    accs = _accs(log2n)
    R = _resampled(log2n)
    Z = ops.fft4_resample_spectrum(torch.from_numpy(np.array(x)).to(dev), accs, TSAMP).cpu().numpy()
    assert Z.shape == (len(accs), n // 2)
    for k0 in range(0, len(accs), 8):
        z = scipy.fft.ifft(Z[k0:k0 + 8].astype(np.complex128), axis=-1, workers=8)
        r = np.empty((z.shape[0], n), dtype=np.float64)
        r[:, 0::2], r[:, 1::2] = z.real, z.imag
        q = np.rint(r)
        assert np.abs(r - q).max() < 0.05, "the inverse transform is too far from integers to round"
        for j in range(z.shape[0]):
            if not np.array_equal(q[j], R[k0 + j]):
                bad = np.flatnonzero(q[j] != R[k0 + j])
                i0 = int(bad[0])
                pytest.fail(f"acc {accs[k0 + j]!r}: {bad.size} samples differ, first at {i0} "
                            f"({i0 - n // 2:+d} from n/2): got {q[j][i0]:.0f}, resample_ii gives {R[k0 + j][i0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("log2n", [16, 18, 22])
def test_pair_y_and_pruned_variants_at_unit_scale(log2n):
    """(d) the tiled-Y hand-over and the pruned pass give the default pass's bits where they write."""
    import torch

    import peasoup_amd._C as C
    from peasoup_amd import ops

    x = _noise(log2n)
    st, nscale, mean, sigma, rms = _unit_scale(x)
    accs = _spectrum_accs(log2n)
    xd = torch.from_numpy(np.array(x)).to(dev)
    std = torch.tensor(st, dtype=torch.float32, device=dev)
    Pb, Q, g = ops.fft4_spectrum_pass(xd, accs, TSAMP, std, nscale)
    M = g.n1 * g.n2
    sh = C.kernels.spec_q_shift
    Qn = Q.cpu().numpy()
    assert min(len(np.unique(row[sh:sh + M + 1])) for row in Qn) >= 32
    assert g.ypair, "the default pass A hands over row-pair Y at every length"
    Pt, Qt, gt = ops.fft4_spectrum_pass(xd, accs, TSAMP, std, nscale, pair_y=False)
    assert not gt.ypair
    assert torch.equal(Pt, Pb) and torch.equal(Qt, Q)
    nb = int(0.14 * M) + 3
    Ps, Qs, _ = ops.fft4_spectrum_pass(xd, accs, TSAMP, std, nscale, nbins=nb)
    Pn, Pns, Qsn = ops.spec_unblock(Pb, g).cpu().numpy(), ops.spec_unblock(Ps, g).cpu().numpy(), Qs.cpu().numpy()
    assert np.array_equal(Pns[:, :nb], Pn[:, :nb])
    assert np.array_equal(Qsn[:, sh:sh + nb], Qn[:, sh:sh + nb])
    hi_ = (nb + 3) // 4 * 4 + 4
    assert not Pns[:, hi_:M].any() and not Qsn[:, sh + hi_:sh + M].any()


# --------------------------------------------------------------- CPU tests --
def _defective(name, x, n1, n2, mean, sigma):
    """The oracle's P (acc = 0) with one defect a kernel rewrite could introduce."""
    n, M = len(x), len(x) // 2
    r = x.astype(np.float64)
    if name == "sample off by one":
        i = 3 * n // 8 + 5
        r = r.copy()
        r[i] = x[i + 1] if x[i + 1] != x[i] else x[i] + 1.0
    if name == "column twiddles off by 1e-5":
        # column c of the N2 x N1 array of z = r[0::2] + i r[1::2], times exp(1e-5 i) before the row transforms
        z = r[0::2] + 1j * r[1::2]
        z[n1 // 3::n1] *= np.exp(1e-5j)
        Z = np.fft.fft(z)
        k = np.arange(M + 1)
        za, zb = Z[k % M], np.conj(Z[(M - k) % M])
        X = 0.5 * (za + zb) - 0.5j * np.exp(-1j * np.pi * k / M) * (za - zb)
    else:
        X = np.fft.rfft(r)
    amp = ref.interbin64(X)
    if name == "no interbin":
        amp = np.abs(X)
    if name == "interbin factor 0.45":
        d = X - np.concatenate([[0j], X[:-1]])
        amp = np.sqrt(np.maximum(np.abs(X) ** 2, 0.45 * np.abs(d) ** 2))
    if name == "bin 0 wraps to X_M":
        amp[0] = np.sqrt(max(abs(X[0]) ** 2, 0.5 * abs(X[0] - X[M]) ** 2))
    if name == "bins n2-1 and n2 swapped":
        amp[[n2 - 1, n2]] = amp[[n2, n2 - 1]]
    return (amp - mean) / sigma


DEFECTS = ["sample off by one", "no interbin", "interbin factor 0.45", "bins n2-1 and n2 swapped",
           "bin 0 wraps to X_M", "column twiddles off by 1e-5"]


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("log2n", [15, 20])
def test_tolerances_reject_defective_oracles(log2n, defect):
    x = _noise(log2n)
    lg = log2n - 1
    n2, n1 = 1 << (lg // 2), 1 << (lg - lg // 2)  # kernels.hpp fft4_geometry
    st, nscale, mean, sigma, rms = _unit_scale(x)
    Pref = ref.search_spectrum(x, 0.0, TSAMP, mean, sigma)
    if defect == "column twiddles off by 1e-5":  # the emulation's own r2c step reproduces the oracle
        assert np.abs(_defective("", x, n1, n2, mean, sigma) - Pref).max() < 1e-9
    err, emax, erms = _errors(_defective(defect, x, n1, n2, mean, sigma)[None], Pref[None], sigma, rms)
    tol_max, tol_rms = TOL[log2n]
    print(f"log2n={log2n} {defect}: max {emax:.3e} rms {erms:.3e} (tol {tol_max:.1e} / {tol_rms:.1e})")
    if defect == "column twiddles off by 1e-5":  # below the resolution of a float32 P (module docstring)
        assert emax > 0
        return
    assert emax > tol_max or erms > tol_rms


def test_oracle_pieces_agree():
    """search_spectrum's bins, the packed half spectrum, Parseval's rms and the byte range at unit scale."""
    x = _noise(15)
    n, M = len(x), len(x) // 2
    st, nscale, mean, sigma, rms = _unit_scale(x)
    X = np.fft.rfft(x.astype(np.float64))
    assert abs(rms - np.sqrt(np.mean(np.abs(X) ** 2))) < 1e-9 * rms
    assert abs(mean - 0.8 * rms) < 1e-6 * rms and abs(sigma - 0.4 * rms) < 1e-6 * rms
    P = ref.search_spectrum(x, 0.0, TSAMP, mean, sigma)
    assert P.shape == (M + 1,) and P.dtype == np.float64
    assert np.allclose(ref.interbin64(X), ref.interbin(X), rtol=1e-5)
    Z = ref.half_spectrum(x)
    k = np.arange(1, M)
    Xk = 0.5 * (Z[k] + np.conj(Z[M - k])) - 0.5j * np.exp(-1j * np.pi * k / M) * (Z[k] - np.conj(Z[M - k]))
    assert np.abs(Xk - X[1:M]).max() < 1e-9 * rms
    assert P.min() < -1.0 and P.max() > 4.0 and len(np.unique(ref.q8(P.astype(np.float32)))) >= 32


def test_float32_spectrum_inverts_to_the_integers():
    """The rounding argument of the gather test: a complex64 FFT of the integer noise, inverted in float64,
    is within 0.05 of the integers it came from."""
    import scipy.fft

    x = _noise(20)
    Z = scipy.fft.fft((x[0::2] + 1j * x[1::2]).astype(np.complex64))
    assert Z.dtype == np.complex64
    z = np.fft.ifft(Z.astype(np.complex128))
    r = np.empty(len(x))
    r[0::2], r[1::2] = z.real, z.imag
    assert np.abs(r - np.rint(r)).max() < 0.05
    assert np.array_equal(np.rint(r), x)


@pytest.mark.parametrize("log2n", LOG2NS)
def test_literal_accelerations_are_where_stated(log2n):
    n = 1 << log2n
    a = ACCS[log2n]
    assert len(set(_accs(log2n))) == len(_accs(log2n))
    for acc in _accs(log2n):
        assert float(np.float32(acc)) == acc, acc
    for acc in a["safe"]:
        assert _tie_distance(acc, n) >= 1e-6, acc
    for acc in a["ulp"]:
        assert _tie_distance(acc, n) >= _ulp_floor(log2n), acc
    for acc in a["tie"]:
        assert 2e-8 <= _tie_distance(acc, n) <= 8e-8, acc
    if log2n <= 23:
        assert len(a["tie"]) == 2 and {0.0, 500.0, -500.0} <= set(_accs(log2n))
        # vertex plateau: the shift at n / 2 within 1e-4 of a tie; |af| n = 0.3
        sv = [abs(ref.accel_factor(acc, TSAMP)) * n * n / 4 for acc in _accs(log2n)]
        assert any(abs(s - 0.5) < 1e-4 for s in sv)
        half_largest = ref.accel_factor(500.0, TSAMP) * n * n / 8  # half the shift at 500 m/s^2
        assert half_largest < 1 or any(abs(s - np.floor(s) - 0.5) < 1e-4 and abs(s - half_largest) < 2
                                       for s in sv)
    assert any(abs(abs(ref.accel_factor(acc, TSAMP)) * n - 0.3) < 1e-3 for acc in _accs(log2n))
