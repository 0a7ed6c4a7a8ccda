"""The candidate folding stage (fold.hip fold_accumulate / fold_reduce /
fold_optimise, FoldEngine and fold_calculate_sn in engine.cpp) against exact
and float64 NumPy oracles: acceleration, batches of series, chunk geometry,
every optimiser output, the host S/N over its whole argument grid.

GPU tests carry the ``gpu`` marker one by one; the oracle self-checks and the
input conditions the GPU tests rely on are unmarked and run anywhere."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from peasoup_amd.utils import reference as ref

gpu = pytest.mark.gpu
dev = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def to_dev(a):
    """A device copy (the shared inputs are read-only arrays)."""
    return torch.tensor(a, device=dev)


# =========================================================== a. raw fold ====
LENGTHS = [1024, 1040, 20000, 70001, 1 << 17]
JOB_DTYPE = [("tsamp_by_period", "<f8"), ("af", "<f8"), ("series", "<u8")]  # kern::FoldJob
ACCELS = [(a, ts) for ts in (64e-6, 320e-6) for a in (5.0, -5.0, 500.0, -500.0)]


def raw_periods(n, nints):
    """Periods in samples: 2.5 and 777.3, each moved by an irrational ~1e-4
    (at the decimal values themselves every 5th / 7773rd sample is an inexact
    product that lands on a bin edge), exactly 64 (a dyadic tsamp/period:
    every product is exact), one longer than a subint (empty bins), one longer
    than the series (every sample in bin 0)."""
    nps = n // nints
    return [2.5 + 1e-4 * math.sqrt(2), 64.0, 777.3 + 1e-4 * math.sqrt(3), (1.37 + 1e-4 * math.sqrt(5)) * nps,
            (3.1 + 1e-4 * math.sqrt(7)) * n]


def tie_margin(n, af):
    """Smallest distance of a source position from a .5 rounding tie."""
    pos = ref.fold_indices(n, 1.0, af)[4]
    return np.abs(pos - np.floor(pos) - 0.5).min()


@functools.lru_cache(maxsize=None)
def clamp_af(n):
    """The synthetic factor c / n, c = 2: the source position c j^2/n - (c - 1) j
    is negative for j < n/2 (clamp at 0), its mirror (af < 0) exceeds n - 1
    for n/2 < j < n.  Where 2 j^2/n hits exact .5 ties (n = 1024: j = 16,
    48, ...) c is the first of a fixed list without a tie within 1e-6."""
    for c in (2.0, 2.001, 2.003, 2.007):
        if min(tie_margin(n, c / n), tie_margin(n, -c / n)) > 1e-6:
            return c / n
    raise AssertionError(n)


def raw_afs(n):
    return [0.0] + [ref.accel_factor(a, ts) for a, ts in ACCELS] + [clamp_af(n), -clamp_af(n)]


def raw_jobs(n, nints=16):
    """One job per (period, af), each on a series of its own."""
    pa = [(1.0 / p, af) for p in raw_periods(n, nints) for af in raw_afs(n)]
    return np.array([(tbp, af, k) for k, (tbp, af) in enumerate(pa)], dtype=JOB_DTYPE)


def int_series(seed, n):
    """Small integers: every partial sum of at most 2^17 of them is below 2^24,
    so float32 sums are exact in any order."""
    return np.random.default_rng(seed).integers(-8, 9, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def raw_case(n, nbins=64, nints=16):
    """(jobs, series [njobs, n], oracle sums [njobs, nints, nbins], counts)."""
    jobs = raw_jobs(n, nints)
    series = np.stack([int_series(1000 * n + k, n) for k in range(len(jobs))])
    sums, cnts = zip(*(ref.fold_sums(series[k], j["tsamp_by_period"], j["af"], nbins, nints)
                       for k, j in enumerate(jobs)))
    for a in (jobs, series):
        a.setflags(write=False)
    return jobs, series, np.stack(sums), np.stack(cnts)


def exact_product(tbp, j):
    """True where j * tbp is computed without rounding (j == 0, or tbp a
    dyadic m / 2^k with m * j below 2^53): such a phase is the same number
    on both sides even on a bin edge."""
    m, e = math.frexp(tbp)
    m = m * (1 << 53)
    while m and m % 2 == 0:
        m /= 2
    return (j == 0) | (j * m < 2.0 ** 53)


@pytest.mark.parametrize("nbins,nints", [(64, 16), (50, 8), (1, 16)])
@pytest.mark.parametrize("n", LENGTHS)
def test_raw_fold_inputs_are_unambiguous(n, nbins, nints):
    """Input condition of the exact tests, by the oracle alone: no source
    position within 1e-6 of a .5 tie, no phase within 1e-9 of a bin edge
    unless its product is exact; the clamp_af jobs clamp > 1% of their samples."""
    for job in raw_jobs(n, nints):
        tbp, af = float(job["tsamp_by_period"]), float(job["af"])
        s, b, src, ph, pos = ref.fold_indices(n, tbp, af, nbins, nints)
        frac = pos - np.floor(pos)
        assert np.abs(frac - 0.5).min() > 1e-6, (n, tbp, af)
        y = ph * nbins
        d = np.minimum(y - np.floor(y), np.ceil(y) - y)
        near = d <= 1e-9 * nbins
        j = np.arange(len(ph), dtype=np.float64)
        assert not (near & ~exact_product(tbp, j)).any(), (n, tbp, af)
        assert b.min() >= 0 and b.max() < nbins
        if abs(af) == clamp_af(n):
            clamped = (np.rint(pos) < 0) if af > 0 else (np.rint(pos) > n - 1)
            assert clamped.mean() > 0.01, (n, af, clamped.mean())
            assert (src[clamped] == (0 if af > 0 else n - 1)).all()


def test_fold_sums_definition():
    """fold_sums against a literal loop on a short series."""
    n, nbins, nints = 1040, 7, 4
    x = int_series(3, n)
    tbp, af = 1.0 / 11.3, 3e-4
    sums, cnts = ref.fold_sums(x, tbp, af, nbins, nints)
    es, ec = np.zeros((nints, nbins)), np.zeros((nints, nbins), np.int64)
    nps, h = n // nints, n / 2.0
    for j in range(nps * nints):
        b = int(math.floor(math.modf(j * tbp)[0] * nbins))
        src = min(max(int(np.rint(j + af * ((j - h) ** 2 - h * h))), 0), n - 1)
        es[j // nps, b] += x[src]
        ec[j // nps, b] += 1
    assert (sums == es).all() and (cnts == ec).all() and ec.sum() == nps * nints


def check_raw(out, sums, cnts):
    psum, pcount, fold = (t.cpu().numpy() for t in out)
    assert (pcount.sum(axis=2, dtype=np.int64) == cnts).all()
    assert (psum.astype(np.float64).sum(axis=2) == sums).all()
    assert (fold == sums.astype(np.float32) / (cnts + 1).astype(np.float32)).all()
    return fold


@gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_raw_fold_exact(n):
    """Every (period, af) job at FoldEngine's chunk: counts, sums and the
    reduced fold equal the oracle with == (integer data, exact float32 sums)."""
    from peasoup_amd import ops

    jobs, series, sums, cnts = raw_case(n)
    out = ops.fold_raw(to_dev(series), jobs)
    nps = n // 16
    assert out[0].shape == (len(jobs), 16, -(-nps // min(4096, nps)), 64)
    fold = check_raw(out, sums, cnts)
    assert (fold[cnts == 0] == 0).all() and (cnts == 0).any()  # empty bins: 0 / 1


@gpu
def test_raw_fold_chunk_geometry():
    """n = 70001 (nps 4375): chunks below 256 threads, not a multiple of 256,
    with a short last chunk; all give the oracle's, hence the same, fold."""
    from peasoup_amd import ops

    n = 70001
    jobs, series, sums, cnts = raw_case(n)
    d = to_dev(series)
    folds = []
    for chunk in (64, 100, 1000, 4096):
        out = ops.fold_raw(d, jobs, chunk=chunk)
        assert out[0].shape[2] == -(-4375 // chunk)
        folds.append(check_raw(out, sums, cnts))
    for f in folds[1:]:
        assert (f == folds[0]).all()


@gpu
@pytest.mark.parametrize("nbins,nints", [(50, 8), (1, 16)])
@pytest.mark.parametrize("n", [1040, 70001])
def test_raw_fold_other_geometry(n, nbins, nints):
    from peasoup_amd import ops

    jobs, series, sums, cnts = raw_case(n, nbins, nints)
    check_raw(ops.fold_raw(to_dev(series), jobs, nbins=nbins, nints=nints), sums, cnts)


@gpu
def test_raw_fold_rejects_65_bins(C):
    from peasoup_amd import ops

    assert C.kernels.fold_job_size == np.dtype(JOB_DTYPE).itemsize == 24
    assert np.dtype(ops.core.FOLD_JOB_DTYPE) == np.dtype(JOB_DTYPE)
    x = torch.zeros((1, 2048), dtype=torch.float32, device=dev)
    with pytest.raises((RuntimeError, ValueError)):
        ops.fold_raw(x, [(0.01, 0.0, 0)], nbins=65)
    with pytest.raises(ValueError):
        ops.fold_raw(x, [(0.01, 0.0, 1)])  # series past the batch


@gpu
def test_raw_fold_jobs_index_series():
    """One launch of 6 jobs over 3 series (jobs 1 and 3 identical): every job
    equals its own oracle."""
    from peasoup_amd import ops

    n = 20000
    series = np.stack([int_series(77 + k, n) for k in range(3)])
    af = ref.accel_factor(500.0, 320e-6)
    spec = [(1 / 777.3, af, 0), (1 / 64.0, -af, 2), (1 / 2.5003, 0.0, 1), (1 / 64.0, -af, 2), (1 / 64.0, -af, 0),
            (1 / 777.3, af, 2)]
    jobs = np.array(spec, dtype=JOB_DTYPE)
    sums, cnts = zip(*(ref.fold_sums(series[s], t, a) for t, a, s in spec))
    out = ops.fold_raw(to_dev(series), jobs)
    fold = check_raw(out, np.stack(sums), np.stack(cnts))
    assert (fold[1] == fold[3]).all() and (out[0][1] == out[0][3]).all()
    assert not (fold[1] == fold[4]).all() and not (fold[0] == fold[5]).all()


# ========================================================= b. float data ====
@functools.lru_cache(maxsize=None)
def float_case():
    n, tsamp, period, acc = 1 << 17, 320e-6, 0.0137, 500.0
    rng = np.random.default_rng(21)
    t = np.arange(n) * tsamp
    ph = ((t - acc * t * t / (2 * ref.C_LIGHT)) / period) % 1.0
    x = (rng.standard_normal(n) + 4.0 * np.exp(-0.5 * ((ph - 0.4) / 0.03) ** 2)).astype(np.float32)
    x.setflags(write=False)
    return x, tsamp / period, ref.accel_factor(acc, tsamp)


@gpu
def test_raw_fold_float_data_within_summation_bound():
    """fold = fl(fl(sum) / (count + 1)): a float32 sum of `count` terms in any
    order is within (count - 1) u sum|x| of the exact one (u = 2^-24, first
    order), its rounding when the partial sums are combined and the division
    add two more relative roundings of a value <= sum|x| / (count + 1):
    |fold - exact| <= (count + 2) u sum|x| / (count + 1)  (>= the above)."""
    from peasoup_amd import ops

    x, tbp, af = float_case()
    assert abs(af) * (len(x) / 2.0) ** 2 > 1.0  # the resampler moves samples by more than one
    sums, cnts = ref.fold_sums(x, tbp, af)
    sabs, _ = ref.fold_sums(np.abs(x), tbp, af)
    psum, pcount, fold = (t.cpu().numpy() for t in ops.fold_raw(to_dev(x[None]), [(tbp, af, 0)]))
    assert (pcount.sum(axis=2)[0] == cnts).all()
    bound = (cnts + 2) * 2.0 ** -24 * sabs / (cnts + 1)
    err = np.abs(fold[0].astype(np.float64) - sums / (cnts + 1))
    print("float fold: max err / bound = %.3f" % (err / bound).max())
    assert (err <= bound).all(), (err / bound).max()


# ====================================================== c. fold_optimise ====
# The float32 (complex64) oracle's magnitude cube deviates from the complex128
# one by at most 2.70e-7 * max(cube) over the sweep below (measured on the CPU,
# NumPy 2.2 pocketfft; test_optimise_eps_is_measured recomputes it).  The
# kernel's radix-8 register FFTs and 63-term sliding sums order the arithmetic
# differently from NumPy's FFT, so it is allowed 8x that: EPS = 2.24e-6.
EPS_MEASURED = 2.8e-7
EPS = 8 * EPS_MEASURED


def _pulse_fold(rng, width, drift, c0=20.0, amp=6.0):
    f = rng.standard_normal((16, 64)).astype(np.float32)
    for i in range(16):
        b0 = int(math.floor(c0 + drift * i / 16.0))
        f[i, (b0 + np.arange(width)) % 64] += amp
    return f


@functools.lru_cache(maxsize=None)
def optimise_sweep():
    """(folds [nf, 16, 64], kinds): drifting pulses, noise, wrap-around,
    two-peaked profiles and the folds of the former
    test_kernels_gpu.test_fold_optimise_matches_fft_reference."""
    rng = np.random.default_rng(2024)
    folds, kinds = [], []
    for width in (1, 4, 20):
        for drift in (0, 7, -13, 31, -31):
            folds.append(_pulse_fold(rng, width, drift))
            kinds.append("pulse")
    for _ in range(14):
        folds.append(rng.standard_normal((16, 64)).astype(np.float32))
        kinds.append("noise")
    for c0, width in ((0.0, 1), (63.0, 1), (0.0, 4), (63.0, 4)):  # the last two wrap round the edge
        folds.append(_pulse_fold(rng, width, 0, c0=c0))
        kinds.append("edge")
    for sep in (9, 32):
        f = _pulse_fold(rng, 3, 0, c0=10.0)
        f[:, (10 + sep + np.arange(3)) % 64] += 5.0
        folds.append(f)
        kinds.append("double")
    old = np.random.default_rng(9).standard_normal((6, 16, 64)).astype(np.float32)
    for f in range(3):
        for i in range(16):
            old[f, i, (20 + (i * (f + 1)) // 4) % 64] += 8.0
    folds.extend(old)
    kinds.extend(["pulse"] * 3 + ["noise"] * 3)
    folds = np.stack(folds)
    folds.setflags(write=False)
    return folds, tuple(kinds)


@functools.lru_cache(maxsize=None)
def optimise_oracle(k):
    """(t, s, j, max, runner-up, mag) of sweep fold k in complex128."""
    t, s, j, _, _, mag = ref.fold_optimise64(optimise_sweep()[0][k])
    flat = mag.ravel()
    am = (t * 64 + s) * 64 + j
    second = max(flat[:am].max(initial=0.0), flat[am + 1:].max(initial=0.0))
    return t, s, j, flat[am], second, mag


def unambiguous(k):
    t, s, j, top, second, _ = optimise_oracle(k)
    return second < (1 - 2 * EPS) * top


def test_optimise_eps_is_measured():
    """EPS_MEASURED is the sweep's largest |cube32 - cube64| / max(cube64),
    rounded up (and not more than twice it, should the FFT library change)."""
    folds, _ = optimise_sweep()
    worst = 0.0
    for k in range(len(folds)):
        mag = optimise_oracle(k)[5]
        worst = max(worst, np.abs(ref.fold_optimise_cube(folds[k]).astype(np.float64) - mag).max() / mag.max())
    print("measured complex64 cube deviation: %.3e" % worst)
    assert worst <= EPS_MEASURED <= 2 * worst


def test_optimise_sweep_is_mostly_unambiguous():
    folds, kinds = optimise_sweep()
    assert len(folds) >= 40 and kinds.count("noise") >= 12
    un = [unambiguous(k) for k in range(len(folds))]
    noise = [u for u, kd in zip(un, kinds) if kd == "noise"]
    assert sum(un) >= 30 and 2 * sum(noise) >= len(noise), (sum(un), sum(noise))


def test_optimise_oracles_agree_on_pulses():
    """fold_optimise64 and fold_optimise pick the same cell on the pulse folds,
    and their outputs agree."""
    folds, kinds = optimise_sweep()
    for k, kd in enumerate(kinds):
        if kd == "noise":
            continue
        t, s, j, of, op = ref.fold_optimise(folds[k])
        t64, s64, j64, of64, op64, _ = ref.fold_optimise64(folds[k])
        assert (t, s, j) == (t64, s64, j64), k
        assert np.allclose(of, of64, rtol=0, atol=1e-4 * np.abs(of64).max())
        assert np.allclose(op, op64, rtol=0, atol=1e-4 * np.abs(op64).max())


def run_optimise(folds):
    from peasoup_amd import ops

    out = ops.fold_optimise(to_dev(folds), return_val=True)
    return tuple(t.cpu().numpy() for t in out)


def check_optimise(fold, k, oi, of, op, ov):
    """One kernel result against the complex128 oracle of sweep fold k."""
    t, s, j, top, second, mag = optimise_oracle(k)
    kt, ks, kj = (int(v) for v in oi)
    assert 0 <= kt < 63 and 0 <= ks < 64 and 0 <= kj < 64, (k, kt, ks, kj)
    assert mag[kt, ks, kj] >= (1 - EPS) * top, (k, (kt, ks, kj), (t, s, j), mag[kt, ks, kj] / top)
    assert abs(float(ov) - top) <= EPS * top, (k, float(ov), top)
    if unambiguous(k):
        assert (kt, ks, kj) == (t, s, j), k
    # outputs at the kernel's own shift.  Like the cube they are 64-point
    # inverse DFTs, so they get the cube's allowance: EPS times the largest
    # magnitude of the oracle output compared (EPS was measured against
    # max(cube), an output too).  Scaling by the largest spectrum value
    # max|fft(fold)| instead cannot be met in float32: a one-bin pulse has a
    # flat spectrum and outputs of 64 max|fft(fold)|, which puts EPS max|fft|
    # below one ulp of them (measured on the MI355X: fold 36 of the sweep
    # errs by 4.8e-6 max|fft(fold)|, which is 1.6e-7 max|opt_fold|; the worst
    # over the sweep are 2.0e-7 max|opt_fold| and 1.8e-7 max|opt_prof|).
    _, _, _, of64, op64, _ = ref.fold_optimise64(fold, shift=ks)
    ef, ep = np.abs(of - of64).max() / np.abs(of64).max(), np.abs(op - op64).max() / np.abs(op64).max()
    WORST["fold"], WORST["prof"] = max(WORST["fold"], ef), max(WORST["prof"], ep)
    WORST["cell"] = max(WORST["cell"], 1 - mag[kt, ks, kj] / top)
    WORST["val"] = max(WORST["val"], abs(float(ov) - top) / top)
    WORST["fold_vs_spectrum"] = max(WORST["fold_vs_spectrum"],
                                    np.abs(of - of64).max() / np.abs(np.fft.fft(fold.astype(np.float64), axis=1)).max())
    assert ef <= EPS, (k, ef)
    assert ep <= EPS, (k, ep)


WORST = dict(fold=0.0, prof=0.0, cell=0.0, val=0.0, fold_vs_spectrum=0.0)  # largest figures seen, printed per test


@gpu
@pytest.mark.parametrize("nfold", [1, 7, 300])
def test_fold_optimise_every_fold(nfold):
    """Every fold of the sweep, pulse or noise: the kernel's cell is a maximum
    of the complex128 cube within EPS, equal to the oracle's where that is
    unambiguous, and opt_fold / opt_prof match the oracle at the kernel's shift."""
    folds, _ = optimise_sweep()
    idx = (np.arange(nfold) * 5 + (3 if nfold < len(folds) else 0)) % len(folds)
    oi, of, op, ov = run_optimise(folds[idx])
    assert oi.shape == (nfold, 3) and ov.shape == (nfold,)
    seen = {}
    for r, k in enumerate(idx):
        if k in seen:  # a repeated fold repeats its result bit for bit
            q = seen[k]
            assert (oi[r] == oi[q]).all() and ov[r] == ov[q] and (of[r] == of[q]).all() and (op[r] == op[q]).all()
            continue
        seen[k] = r
        check_optimise(folds[k], k, oi[r], of[r], op[r], ov[r])
    print("fold_optimise worst figures so far (EPS = %.3g): %s" % (EPS, {k: "%.3g" % v for k, v in WORST.items()}))
    if nfold == 300:
        assert len(seen) == len(folds)


@gpu
def test_fold_optimise_exact_ties():
    """All-zero fold: every cell ties at 0, the first is (0, 0, 0).  A fold
    with only subint 0 nonzero: the 64 drifts are bit-identical, so s = 0."""
    folds = np.zeros((4, 16, 64), np.float32)
    deltas = {1: (17, 3.0), 2: (0, 1.0), 3: (63, 2.5)}
    for r, (j0, a) in deltas.items():
        folds[r, 0, j0] = a
    oi, of, op, ov = run_optimise(folds)
    assert tuple(oi[0]) == (0, 0, 0) and ov[0] == 0
    assert np.isfinite(of[0]).all() and np.isfinite(op[0]).all() and (of[0] == 0).all() and (op[0] == 0).all()
    for r, (j0, a) in deltas.items():
        t, _, j, _, _, mag = ref.fold_optimise64(folds[r])
        assert (t, j) == (0, j0)
        assert np.ptp(mag[0, :, j0]) <= 1e-12 * mag.max()  # the oracle's drifts tie (to float64 rounding)
        assert tuple(oi[r]) == (t, 0, j), (r, tuple(oi[r]))
        assert ov[r] == pytest.approx(63 * a, rel=1e-5)
        assert np.abs(of[r] - 64 * folds[r]).max() <= 1e-4 * a
        assert np.abs(op[r] - 64 * folds[r, 0]).max() <= 1e-4 * a


# ========================================================= d. FoldEngine ====
def f32_tobs(n, tsamp):
    return float(np.float32(n * float(np.float32(tsamp))))


def opt_period_of(p, s, n, tsamp):
    return float(np.float32(p * ((((32.0 - s) * p) / (64 * f32_tobs(n, tsamp))) + 1)))  # 64 * tobs is exact in float32


def oracle_chain(x, period, acc, tsamp):
    """fold_series(af) -> fold_optimise -> calculate_sn, plus the complex128
    optimiser's margin (rule c) on the same fold."""
    tsf = float(np.float32(tsamp))  # the folder's tsamp is float32
    fold = ref.fold_series(x, period, tsf, af=ref.accel_factor(acc, tsamp))
    t, s, j, ofold, oprof = ref.fold_optimise(fold)
    sn = max(ref.calculate_sn(oprof, j - t // 2, t))
    t64, s64, j64, _, _, mag = ref.fold_optimise64(fold)
    flat = np.sort(mag.ravel())
    clear = flat[-2] < (1 - 2 * EPS) * flat[-1] and (t, s, j) == (t64, s64, j64)
    return dict(t=t, s=s, j=j, fold=ofold, snr=sn, clear=clear)


@functools.lru_cache(maxsize=None)
def accel_pulsar():
    """The accelerated pulsar of test_results_independent_of_accel_batching
    (64 us, P = 2 ms, a = 310, 4 % duty), as a zero-mean float series.  The
    v1 resampler at a = 310 turns its phase (t - a t^2 / 2c) / P into the
    linear j tsamp (1 - af n) / P, so the three jobs fold at the period the
    search reports for it, P / (1 - af n); at P itself the straightened pulse
    drifts by 1.17 turns and the fold at a = 310 is the worst of the three."""
    rng = np.random.default_rng(33)
    n, tsamp, period, a_true = 1 << 20, 64e-6, 0.002, 310.0
    t = np.arange(n) * tsamp
    ph = ((t - a_true * t * t / (2 * 299792458.0)) / period) % 1.0
    x = (rng.normal(0, 6, n) + 2.0 * (np.minimum(ph, 1 - ph) < 0.04)).astype(np.float32)
    x.setflags(write=False)
    p_fold = period / (1 - ref.accel_factor(a_true, tsamp) * n)
    jobs = [(p_fold, 310.0), (p_fold, 0.0), (p_fold, -310.0)]
    return x, tsamp, jobs, [oracle_chain(x, p, a, tsamp) for p, a in jobs]


def test_accel_pulsar_oracle_is_clear():
    """The a = 310 fold has an unambiguous optimum (so the exact comparisons
    of test_fold_engine_accelerated_pulsar apply) and the highest S/N."""
    _, _, _, exp = accel_pulsar()
    assert exp[0]["clear"]
    assert exp[0]["snr"] > 1.5 * max(exp[1]["snr"], exp[2]["snr"])


@gpu
def test_fold_engine_accelerated_pulsar():
    from peasoup_amd import ops

    x, tsamp, jobs, exp = accel_pulsar()
    res = ops.fold_series(to_dev(x), [p for p, _ in jobs], [a for _, a in jobs], tsamp)
    assert len(res) == 3
    for r, e, (p, a) in zip(res, exp, jobs):
        print("acc %6.1f: S/N %.3f (oracle %.3f), width %d bin %d" % (a, r.folded_snr, e["snr"], r.opt_width, r.opt_bin))
        assert r.folded_snr == pytest.approx(e["snr"], rel=1e-2)
        if e["clear"]:
            assert r.opt_width == e["t"] + 1 and r.opt_bin == e["j"] - e["t"] // 2
            assert r.opt_period == opt_period_of(p, e["s"], len(x), tsamp)
            assert np.allclose(np.array(r.fold).reshape(16, 64), e["fold"], rtol=2e-3, atol=2e-2)
    assert res[0].folded_snr > res[1].folded_snr and res[0].folded_snr > res[2].folded_snr


@functools.lru_cache(maxsize=None)
def drifting_pulsar():
    """A pulsar folded at a period that drifts it by 5.4 bins over the series."""
    n, tsamp, p_true = 1 << 18, 64e-6, 0.002
    p_fold = p_true * (1 + 5.4 * p_true / (64 * n * tsamp))
    t = np.arange(n) * tsamp
    ph = (t / p_true) % 1.0
    x = (np.random.default_rng(8).normal(0, 1, n) + 1.0 * (np.minimum(ph, 1 - ph) < 0.03)).astype(np.float32)
    x.setflags(write=False)
    return x, tsamp, p_true, p_fold, oracle_chain(x, p_fold, 0.0, tsamp)


def test_drifting_pulsar_oracle_is_clear():
    x, tsamp, p_true, p_fold, e = drifting_pulsar()
    assert e["clear"] and e["s"] != 32
    assert abs(opt_period_of(p_fold, e["s"], len(x), tsamp) - p_true) < 0.5 * abs(p_fold - p_true)


@gpu
def test_fold_engine_recovers_period_from_drift():
    from peasoup_amd import ops

    x, tsamp, p_true, p_fold, e = drifting_pulsar()
    r = ops.fold_series(to_dev(x), [p_fold], [0.0], tsamp)[0]
    hits = [k for k in range(64) if opt_period_of(p_fold, k, len(x), tsamp) == r.opt_period]
    assert len(hits) == 1, hits
    s = hits[0]
    print("drift: shift %d (oracle %d), opt_period %.9g, true %.9g, folded at %.9g" % (s, e["s"], r.opt_period, p_true, p_fold))
    assert s != 32 and s == e["s"]
    assert r.opt_period == opt_period_of(p_fold, s, len(x), tsamp)
    assert abs(r.opt_period - p_true) < abs(p_fold - p_true)
    assert r.opt_width == e["t"] + 1 and r.opt_bin == e["j"] - e["t"] // 2
    assert r.folded_snr == pytest.approx(e["snr"], rel=1e-2)
    assert np.allclose(np.array(r.fold).reshape(16, 64), e["fold"], rtol=2e-3, atol=2e-2)


def result_key(r):
    """Every field of a FoldResult, floats as bit patterns."""
    return (np.float32(r.folded_snr).tobytes(), np.float32(r.opt_period).tobytes(), r.opt_width, r.opt_bin,
            np.asarray(r.fold, np.float32).tobytes(), np.asarray(r.prof, np.float32).tobytes())


@gpu
def test_fold_engine_batched_trials_equal_single(C):
    """fold_trials / fold_rows over max_batch + 6 trials with ragged candidate
    lists (empty first and last) equal fold_trial on each row alone, bit for
    bit and in order."""
    n, nsamps, stride, tsamp = 4096, 4000, 4096, 64e-6
    s = torch.cuda.current_stream().cuda_stream
    fe = C.FoldEngine(n, tsamp, s)
    ntr = fe.max_batch + 6
    assert ntr > fe.max_batch >= 1
    rng = np.random.default_rng(41)
    t = np.arange(nsamps) * tsamp
    rows = np.zeros((ntr, stride), np.uint8)
    periods, accs = [], []
    for b in range(ntr):
        p0 = 0.003 * (1 + 0.05 * (b % 11))
        rows[b, :nsamps] = np.clip(np.rint(rng.normal(120, 9, nsamps) + 30 * (((t / p0) % 1.0) < 0.06)), 0, 255)
        rows[b, nsamps:] = 255  # past the trial: never read as data
        k = 0 if b in (0, ntr - 1) else (0, 1, 5)[b % 3]
        periods.append([float(p0 * (1 + 0.002 * i)) for i in range(k)])
        accs.append([float(a) for a in rng.uniform(-300, 300, k)])
    assert {len(p) for p in periods} == {0, 1, 5}
    d = torch.from_numpy(rows).to(dev)
    single = [C.FoldEngine(n, tsamp, s).fold_trial(d.data_ptr() + b * stride, nsamps, periods[b], accs[b]) if periods[b]
              else [] for b in range(ntr)]
    # one engine whitens row by row: its results do not depend on the engine
    again = fe.fold_trial(d.data_ptr() + 4 * stride, nsamps, periods[4], accs[4])
    assert [result_key(r) for r in again] == [result_key(r) for r in single[4]]
    want = [[result_key(r) for r in rs] for rs in single]
    assert sum(len(w) for w in want) == sum(len(p) for p in periods) > ntr
    assert len({w[0][0] for w in want if w}) > ntr // 4  # the rows differ

    batched = fe.fold_trials(d.data_ptr(), stride, nsamps, periods, accs)
    assert [[result_key(r) for r in rs] for rs in batched] == want

    # scattered, 16-byte aligned rows: a pool in another order, each row 16 * (b % 3) bytes into its slot
    pool = torch.full((ntr, stride + 256), 7, dtype=torch.uint8, device=dev)
    perm = np.random.default_rng(5).permutation(ntr)
    ptrs = []
    for b in range(ntr):
        off = 16 * (b % 3)
        pool[int(perm[b]), off:off + stride] = d[b]
        ptrs.append(pool.data_ptr() + int(perm[b]) * (stride + 256) + off)
    assert all(p % 16 == 0 for p in ptrs)
    torch.cuda.synchronize()
    by_rows = fe.fold_rows(ptrs, nsamps, periods, accs)
    assert [[result_key(r) for r in rs] for rs in by_rows] == want

    empty = [[] for _ in range(ntr)]
    assert fe.fold_trials(d.data_ptr(), stride, nsamps, empty, empty) == empty
    assert fe.fold_rows(ptrs, nsamps, empty, empty) == empty
    torch.cuda.synchronize()


# ============================================================ e. host S/N ===
def sn_profiles():
    rng = np.random.default_rng(6)
    a = rng.standard_normal(64).astype(np.float32)
    a[40:44] += 10
    b = (rng.standard_normal(64) * 0.2 + 3.0).astype(np.float32)
    b[:2] += 4
    b[-3:] += 4  # a pulse across the wrap
    c = np.zeros(64, np.float32)
    c[10] = 1.0  # zero off-pulse variance once the on-pulse window covers bin 10
    return a, b, c


def same_number(x, y, rel):
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) and math.isnan(y)
    if math.isinf(x) or math.isinf(y):
        return x == y
    return x == pytest.approx(y, rel=rel)


def test_calculate_sn_full_grid(C):
    """fold_calculate_sn against the oracle for every bin in -31..63 (the
    engine passes bin - template / 2) and width in 0..63 (opt_template)."""
    nans = infs = 0
    for prof in sn_profiles():
        for b in range(-31, 64):
            for w in range(0, 64):
                got = C.fold_calculate_sn(prof.tolist(), b, w)
                want = ref.calculate_sn(prof, b, w)
                for g, e in zip(got, want):
                    assert same_number(g, e, 1e-5), (b, w, got, want)
                    nans += math.isnan(e)
                    infs += math.isinf(e)
    assert nans > 0  # the empty off-pulse set of wide templates is covered


# ================================================= f. oracle self-checks ====
def _parent_fold_series(x, period, tsamp, nbins=64, nints=16):
    """ref.fold_series as it stood before it grew ``af`` (kept to pin its output)."""
    n = len(x)
    nps = n // nints
    out = np.zeros((nints, nbins), np.float64)
    cnt = np.ones((nints, nbins), np.int64)
    j = np.arange(nps * nints, dtype=np.float64)
    ph = np.modf(j * (tsamp / period))[0]
    b = np.floor(ph * nbins).astype(np.int64)
    s = (np.arange(nps * nints) // nps)
    np.add.at(out, (s, b), x[: nps * nints].astype(np.float64))
    np.add.at(cnt, (s, b), 1)
    return (out / cnt).astype(np.float32)


def test_fold_series_af0_is_unchanged():
    """fold_series(af = 0) bit for bit: against the former implementation and
    against its recorded output (tests/golden/fold_series_af0.npy)."""
    n = 50003
    x = ((np.arange(n, dtype=np.int64) * 2654435761 % 1000003) / 37.0 - 13000.0).astype(np.float32)
    tsamp, period = float(np.float32(0.00032)), 0.2513
    got = ref.fold_series(x, period, tsamp)
    assert got.dtype == np.float32 and got.shape == (16, 64)
    assert got.tobytes() == _parent_fold_series(x, period, tsamp).tobytes()
    assert got.tobytes() == ref.fold_series(x, period, tsamp, af=0.0).tobytes()
    assert got.tobytes() == np.load(os.path.join(GOLDEN, "fold_series_af0.npy")).tobytes()
    rng_x = np.random.default_rng(1).standard_normal(1 << 16).astype(np.float32)
    assert ref.fold_series(rng_x, 0.0071, 64e-6).tobytes() == _parent_fold_series(rng_x, 0.0071, 64e-6).tobytes()


def test_fold_series_accelerated_differs_and_matches_resampler():
    """fold_series(af) is fold_series of the v1-resampled series."""
    x = np.random.default_rng(2).standard_normal(1 << 15).astype(np.float32)
    af = 3e-9
    got = ref.fold_series(x, 0.0071, 64e-6, af=af)
    assert got.tobytes() == ref.fold_series(ref.resample_v1(x, af), 0.0071, 64e-6).tobytes()
    assert got.tobytes() != ref.fold_series(x, 0.0071, 64e-6).tobytes()
