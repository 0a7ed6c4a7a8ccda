"""NumPy reference implementations (float32 semantics) of every device stage.

Each function mirrors the reference CUDA code it replaces (cited per
function) and is the oracle for the HIP-kernel numerics tests.  The whole
chain also forms a CPU reference search (``search_trial``) used to validate
the algorithm on tutorial.fil without a GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

C_LIGHT = 299792458.0
LEVEL_SCALE = [1.0, 1.0 / math.sqrt(2.0), 0.5, 1.0 / math.sqrt(8.0), 0.25, 1.0 / math.sqrt(32.0)]


# ------------------------------------------------------------ dedispersion --
def delay_table(nchans: int, tsamp: float, fch1: float, foff: float) -> np.ndarray:
    f0, df, dt = np.float32(fch1), np.float32(foff), np.float32(tsamp)
    c = np.arange(nchans, dtype=np.float32)
    a = np.float32(1.0) / (f0 + c * df)
    b = np.float32(1.0) / f0
    return (4.15e3 / float(dt) * (a * a - b * b).astype(np.float64)).astype(np.float32)


def dm_offsets(dms: Sequence[float], delays: np.ndarray) -> np.ndarray:
    d = np.asarray(dms, dtype=np.float32)[:, None] * delays[None, :]
    return (d + np.float32(0.5)).astype(np.int32)


def dedisperse(values: np.ndarray, offsets: np.ndarray, nbits: int, killmask=None,
               out_nsamps: int = None) -> np.ndarray:
    """values [nsamps, nchans] (raw) -> uint8 [ndm, out_nsamps] (dedisp 8-bit scaling)."""
    nsamps, nchans = values.shape
    kill = np.ones(nchans, bool) if killmask is None else np.asarray(killmask) != 0
    if out_nsamps is None:
        out_nsamps = nsamps - int(offsets.max())
    scale = np.float32(192.0 / (((1 << nbits) - 1) * nchans))
    x = values.T.astype(np.int64)
    out = np.empty((offsets.shape[0], out_nsamps), dtype=np.uint8)
    for d in range(offsets.shape[0]):
        s = np.zeros(out_nsamps, dtype=np.int64)
        for c in np.nonzero(kill)[0]:
            o = int(offsets[d, c])
            s += x[c, o:o + out_nsamps]
        v = np.clip(s.astype(np.float32) * scale, 0, 255)
        out[d] = v.astype(np.uint8)
    return out


# --------------------------------------------------------------- spectra ----
def convert_pad(trial_u8: np.ndarray, n: int) -> np.ndarray:
    nvalid = min(len(trial_u8), n)
    out = np.empty(n, dtype=np.float32)
    out[:nvalid] = trial_u8[:nvalid]
    if n > nvalid:
        out[nvalid:] = np.float32(float(trial_u8[:nvalid].astype(np.int64).sum()) / nvalid)
    return out


def amplitude(X: np.ndarray) -> np.ndarray:
    return np.abs(X.astype(np.complex64)).astype(np.float32)


def interbin(X: np.ndarray) -> np.ndarray:
    X = X.astype(np.complex64)
    prev = np.concatenate([[0j], X[:-1]]).astype(np.complex64)
    a = (X.real * X.real + X.imag * X.imag).astype(np.float32)
    d = (X - prev)
    b = (0.5 * (d.real * d.real + d.imag * d.imag).astype(np.float64)).astype(np.float32)
    return np.sqrt(np.maximum(a, b)).astype(np.float32)


def interbin64(X: np.ndarray) -> np.ndarray:
    """``interbin`` from its definition in float64 (no rounding to complex64):
    sqrt(max(|X_k|^2, 0.5 |X_k - X_{k-1}|^2)) with X_{-1} = 0."""
    X = np.asarray(X, dtype=np.complex128)
    prev = np.concatenate([[0j], X[:-1]])
    d = X - prev
    a = X.real * X.real + X.imag * X.imag
    b = 0.5 * (d.real * d.real + d.imag * d.imag)
    return np.sqrt(np.maximum(a, b))


def q8(P: np.ndarray) -> np.ndarray:
    """device_common.hpp dev::q8, the harmonic sum's screening byte of a
    float32 P: v = rint(4p) + 128; bytes 0..253 = v - 1, 254 = v >= 255 or
    NaN, 255 = v <= 0."""
    with np.errstate(invalid="ignore"):
        v = np.rint(P.astype(np.float32) * np.float32(4.0)) + np.float32(128.0)
        q = np.where(np.isnan(v) | (v >= 255), 254, np.where(v <= 0, 255, v - 1))
    return q.astype(np.uint8)


def median_scrunch5(x: np.ndarray) -> np.ndarray:
    n = len(x)
    if n < 5:
        if n == 1:
            return x[:1].copy()
        if n == 2:
            return np.array([np.float32(0.5) * (x[0] + x[1])], np.float32)
        if n == 3:
            return np.array([np.median(x)], np.float32)
        s = np.sort(x)
        return np.array([np.float32(0.5) * (s[1] + s[2])], np.float32)
    m = n // 5
    return np.median(x[: 5 * m].reshape(m, 5), axis=1).astype(np.float32)


def linear_stretch(x: np.ndarray, out_count: int) -> np.ndarray:
    in_count = len(x)
    step = np.float32(in_count - 1) / np.float32(out_count - 1)
    xi = np.arange(out_count, dtype=np.uint32).astype(np.float32) * step
    j = np.minimum(xi.astype(np.uint32), in_count - 1)
    frac = (xi - j.astype(np.float32)).astype(np.float32)
    a = x[j]
    nxt = x[np.minimum(j + 1, in_count - 1)]
    use = (frac > np.float32(1e-5)) & (j + 1 < in_count)
    return np.where(use, a + frac * (nxt - a), a).astype(np.float32)


def running_median(amp: np.ndarray, bin_width: float, b5: float = 0.05, b25: float = 0.5) -> np.ndarray:
    """Dereddener::calculate_median (dereddener.hpp:44-62)."""
    nb = len(amp)
    m5 = median_scrunch5(amp)
    m25 = median_scrunch5(m5)
    m125 = median_scrunch5(m25)
    pos5 = int(np.float32(b5) / np.float32(bin_width))
    pos25 = int(np.float32(b25) / np.float32(bin_width))
    s5, s25, s125 = linear_stretch(m5, nb), linear_stretch(m25, nb), linear_stretch(m125, nb)
    k = np.arange(nb)
    return np.where(k >= pos25, s125, np.where(k >= pos5, s25, s5)).astype(np.float32)


def deredden(X: np.ndarray, median: np.ndarray, zapmask: np.ndarray = None) -> np.ndarray:
    out = (X / median.astype(np.complex64)).astype(np.complex64)
    out[:5] = 0
    if zapmask is not None:
        out[zapmask] = 1 + 0j
    return out


def zap_mask(freqs, widths, bin_width: float, nbins: int) -> np.ndarray:
    m = np.zeros(nbins, bool)
    for f, w in zip(freqs, widths):
        lo = int(math.floor((np.float32(f) - np.float32(w)) / np.float32(bin_width)))
        hi = int(math.ceil((np.float32(f) + np.float32(w)) / np.float32(bin_width)))
        lo = max(lo, 0)
        if lo >= nbins:
            continue
        hi = min(hi, nbins - 1)
        m[lo:hi] = True
    return m


def stats(P: np.ndarray) -> Tuple[float, float, float]:
    s = float(P.astype(np.float64).sum())
    s2 = float((P.astype(np.float64) ** 2).sum())
    n = np.float32(len(P))
    mean = np.float32(s) / n
    rms = np.sqrt(np.float32(s2) / n)
    std = np.sqrt(max(rms * rms - mean * mean, np.float32(0)))
    return float(mean), float(rms), float(std)


def whiten(trial_u8: np.ndarray, n: int, tsamp: float, zapmask=None, with_stats=True):
    """Worker::start per-DM whitening (pipeline_multi.cu:156-204)."""
    x = convert_pad(trial_u8, n)
    X = np.fft.rfft(x.astype(np.float64)).astype(np.complex64)
    bw = np.float32(1.0 / np.float32(np.float32(n) * np.float32(tsamp)))
    med = running_median(amplitude(X), float(bw))
    X = deredden(X, med, zapmask)
    st = stats(interbin(X)) if with_stats else None
    series = (np.fft.irfft(X.astype(np.complex128), n) * n).astype(np.float32)
    return series, st


# The whitener from its definition in float64.  The values are float64; the
# integer decisions of the algorithm (the region switches, the zap ranges, the
# stretch's node index and its interpolation guard) are taken in float32,
# exactly as ``running_median`` / ``linear_stretch`` / ``zap_mask`` and the
# kernels take them.
def whiten_positions(n: int, tsamp: float, b5: float = 0.05, b25: float = 0.5):
    """(bin_width as float32, pos5, pos25): the bins at which the running
    median switches from the medians of 5 to those of 25 and of 125."""
    bw = np.float32(1.0 / np.float32(np.float32(n) * np.float32(tsamp)))
    return bw, int(np.float32(b5) / bw), int(np.float32(b25) / bw)


def stretch_nodes(in_count: int, out_count: int):
    """``linear_stretch``'s decisions per output bin: (j, frac, interpolate),
    j the left node (int64), frac the float32 weight of node j + 1 (as
    float64), interpolate = frac > 1e-5f and j + 1 < in_count."""
    step = np.float32(in_count - 1) / np.float32(out_count - 1)
    xi = np.arange(out_count, dtype=np.uint32).astype(np.float32) * step
    j = np.minimum(xi.astype(np.uint32), in_count - 1).astype(np.int64)
    frac = (xi - j.astype(np.float32)).astype(np.float32)
    use = (frac > np.float32(1e-5)) & (j + 1 < in_count)
    return j, frac.astype(np.float64), use


def linear_stretch64(x: np.ndarray, out_count: int, nodes=None) -> np.ndarray:
    """``linear_stretch`` with float64 values (nodes: ``stretch_nodes``'s
    tuple, default the stretch's own)."""
    x = np.asarray(x, dtype=np.float64)
    j, frac, use = stretch_nodes(len(x), out_count) if nodes is None else nodes
    a = x[j]
    nxt = x[np.minimum(j + 1, len(x) - 1)]
    return np.where(use, a + frac * (nxt - a), a)


def median_scrunch5_64(x: np.ndarray) -> np.ndarray:
    """``median_scrunch5`` in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n < 5:
        if n == 1:
            return x[:1].copy()
        if n == 2:
            return np.array([0.5 * (x[0] + x[1])])
        if n == 3:
            return np.array([np.median(x)])
        s = np.sort(x)
        return np.array([0.5 * (s[1] + s[2])])
    m = n // 5
    return np.median(x[: 5 * m].reshape(m, 5), axis=1)


def running_median64(amp: np.ndarray, pos5: int, pos25: int) -> np.ndarray:
    """``running_median`` in float64 with the switches given as bins: bin k
    takes the stretched medians of 125 if k >= pos25, else of 25 if
    k >= pos5, else of 5."""
    nb = len(amp)
    m5 = median_scrunch5_64(amp)
    m25 = median_scrunch5_64(m5)
    m125 = median_scrunch5_64(m25)
    k = np.arange(nb)
    return np.where(k >= pos25, linear_stretch64(m125, nb),
                    np.where(k >= pos5, linear_stretch64(m25, nb), linear_stretch64(m5, nb)))


def convert_pad64(trial_u8: np.ndarray, n: int) -> np.ndarray:
    """``convert_pad`` as float64: the pad is the kernels' own value, the
    float32 rounding of double(sum) / nvalid."""
    return convert_pad(trial_u8, n).astype(np.float64)


def stats64(P: np.ndarray) -> Tuple[float, float, float]:
    P = np.asarray(P, dtype=np.float64)
    mean = float(P.mean())
    rms = float(np.sqrt((P * P).mean()))
    return mean, rms, float(np.sqrt(max(rms * rms - mean * mean, 0.0)))


def whiten64(trial_u8: np.ndarray, n: int, tsamp: float, zap_freqs=(), zap_widths=(), b5: float = 0.05,
             b25: float = 0.5):
    """The whitener's dereddened half spectrum from its definition, float64:
    the first min(nsamps, n) samples mean-padded to n -> real FFT -> divided
    by the running median of |X| -> bins 0..4 zeroed -> zapped bins 1 + 0i
    (zap wins over the zeroing).  Returns (D complex128 [n/2 + 1],
    (mean, rms, std) of interbin64(D), pos5, pos25).  The whitened series is
    irfft(D) * n."""
    X = np.fft.rfft(convert_pad64(trial_u8, n))
    nb = len(X)
    bw, pos5, pos25 = whiten_positions(n, tsamp, b5, b25)
    D = X / running_median64(np.abs(X), pos5, pos25)
    D[:5] = 0
    if len(zap_freqs):
        D[zap_mask(zap_freqs, zap_widths, float(bw), nb)] = 1 + 0j
    return D, stats64(interbin64(D)), pos5, pos25


# ---------------------------------------------------------- acceleration ---
def accel_factor(acc: float, tsamp: float) -> float:
    return (float(np.float32(acc)) * float(np.float32(tsamp))) / (2 * C_LIGHT)


def resample_ii(x: np.ndarray, af: float) -> np.ndarray:
    n = len(x)
    i = np.arange(n, dtype=np.float64)
    j = np.rint(i + i * af * (i - n))
    j = np.clip(j, 0, n - 1).astype(np.int64)
    return x[j]


def half_spectrum(r: np.ndarray) -> np.ndarray:
    """The Z that ``ops.fft4_resample_spectrum`` defines, in complex128: the
    n/2-point FFT of the packed series z[m] = r[2m] + i r[2m+1]."""
    r = np.asarray(r, dtype=np.float64)
    return np.fft.fft(r[0::2] + 1j * r[1::2])


def search_spectrum(x: np.ndarray, acc: float, tsamp: float, mean: float, sigma: float) -> np.ndarray:
    """One acceleration trial's normalised search spectrum from its
    definition, float64 throughout: resampleII -> real FFT -> interbinned
    amplitude -> (amp - mean) / sigma.  Returns all n/2 + 1 bins."""
    r = resample_ii(x, accel_factor(acc, tsamp))
    X = np.fft.rfft(r.astype(np.float64))
    return (interbin64(X) - float(mean)) / float(sigma)


def resample_v1(x: np.ndarray, af: float) -> np.ndarray:
    n = len(x)
    h = n / 2.0
    i = np.arange(n, dtype=np.float64)
    j = np.clip(np.rint(i + af * ((i - h) ** 2 - h * h)), 0, n - 1).astype(np.int64)
    return x[j]


def harmonic_sums(P: np.ndarray, nlevels: int) -> List[np.ndarray]:
    """harmonic_sum_kernel (kernels.cu:33-99) -> [level1..levelH] arrays."""
    n = len(P)
    i = np.arange(n, dtype=np.int64)
    val = P.astype(np.float32).copy()
    out = []
    orders = {1: [1], 2: [3, 1], 3: [1, 3, 5, 7], 4: list(range(1, 16, 2)), 5: list(range(1, 32, 2))}
    for h in range(1, nlevels + 1):
        for m in orders[h]:
            val = (val + P[(i * m + (1 << (h - 1))) >> h]).astype(np.float32)
        out.append((val.astype(np.float64) * LEVEL_SCALE[h]).astype(np.float32))
    return out


def peak_bounds(nbins: int, bin_width: float, nh: int, min_freq: float, max_freq: float):
    nyquist = np.float32(bin_width) * np.float32(nbins)
    orig = int(2.0 * (nbins - 1.0))
    p2 = 2.0 ** nh
    max_bin = int(float(np.float32(max_freq) / np.float32(bin_width)) * p2)
    start = int(float(np.float32(orig) * (np.float32(min_freq) / nyquist)) * p2)
    factor = 1.0 / nbins * float(nyquist) / 2.0 ** nh
    return max(start, 0), min(nbins, max_bin), factor


def unique_peaks(idxs: np.ndarray, snrs: np.ndarray, min_gap: int = 30):
    out = []
    ii, n = 0, len(idxs)
    while ii < n:
        cpeak, cidx, last = snrs[ii], idxs[ii], idxs[ii]
        ii += 1
        while ii < n and idxs[ii] - last < min_gap:
            if snrs[ii] > cpeak:
                cpeak, cidx, last = snrs[ii], idxs[ii], idxs[ii]
            ii += 1
        out.append((int(cidx), float(cpeak)))
    return out


# -------------------------------------------- the search of one DM trial ----
# Float64 oracle of SearchEngine::search_trial, written from the definition of
# the search: whiten64 -> search_spectrum per acceleration -> harmonic sums ->
# crossings inside peak_bounds -> unique_peaks -> candidates -> the per-trial
# harmonic distiller -> the per-DM acceleration distiller.  The values are
# float64; the integer and float32 decisions (tobs, bin_width, the search
# ranges, the threshold, the candidate frequency, the distillers' tolerances)
# are taken in float32 where the engine takes them.
class Cand:
    """A candidate of the Python distillers (the fields of psoup::Candidate)."""

    def __init__(self, dm, dm_idx, acc, nh, snr, freq):
        self.dm, self.dm_idx, self.acc, self.nh, self.snr, self.freq = dm, dm_idx, acc, nh, snr, freq
        self.assoc = []


def f32(x):
    return float(np.float32(x))


def py_distill(cands, cond):
    """BaseDistiller::distill (distiller.hpp): sort by descending S/N, then
    every still-unique candidate in turn marks the later ones related to it."""
    cands = sorted(cands, key=lambda c: -c.snr)
    uniq = [True] * len(cands)
    start = 0
    while True:
        idx = -1
        for ii in range(start, len(cands)):
            if uniq[ii]:
                start, idx = ii + 1, ii
                break
        if idx < 0:
            break
        cond(cands, idx, uniq)
    return [c for c, u in zip(cands, uniq) if u]


def harm_related(f0, freqs, nhs, tol, max_harm, frac):
    """HarmonicDistiller::condition: per later candidate (freqs, nhs) the
    number of (jj, kk), jj = 1..max_harm, kk = 1..(2^nh if frac else 1), with
    1 - tol < kk f / (jj f0) < 1 + tol (the ratio in double; tol a float32 and
    the bounds formed in float32, `double upper_tol = 1 + tolerance` with a
    float tolerance, distiller.hpp:74-75 -- 1 - 1e-4f is 0.99989998, not the
    0.9999000000025 of double arithmetic, and a ratio can fall between)."""
    f = np.asarray(freqs, dtype=np.float64)
    maxd = np.array([2.0 ** h if frac else 1.0 for h in nhs], dtype=np.float64)
    if not len(f):
        return np.zeros(0, dtype=np.int64)
    jj = np.arange(1, int(max_harm) + 1, dtype=np.float64)
    kk = np.arange(1, int(maxd.max()) + 1, dtype=np.float64)
    r = (kk[None, None, :] * f[:, None, None]) / (jj[None, :, None] * f0)
    lower, upper = float(np.float32(1) - np.float32(tol)), float(np.float32(1) + np.float32(tol))
    hit = (r > lower) & (r < upper) & (kk[None, None, :] <= maxd[:, None, None])
    return hit.sum(axis=(1, 2))


def harm_cond(tol, max_harm, keep, frac):
    def cond(c, idx, uniq):
        rest = c[idx + 1:]
        n = harm_related(c[idx].freq, [x.freq for x in rest], [x.nh for x in rest], tol, max_harm, frac)
        for ii in np.nonzero(n)[0]:
            if keep:  # once per matching (jj, kk)
                c[idx].assoc.extend([rest[ii]] * int(n[ii]))
            uniq[idx + 1 + ii] = False
    return cond


def acc_related(f0, a0, f, a, tobs, tol):
    """AccelerationDistiller::condition: is (f, a) inside the window that the
    fundamental (f0, a0) sweeps to at acceleration a, widened by f0 tol."""
    edge = f0 * f32(tol)
    af = f32(f0 + (a0 - a) * f0 * (f32(tobs) / C_LIGHT))
    return (f0 - edge < f < af + edge) if af > f0 else (af - edge < f < f0 + edge)


def acc_cond(tobs, tol, keep):
    def cond(c, idx, uniq):
        f0, a0 = c[idx].freq, c[idx].acc
        for ii in range(idx + 1, len(c)):
            if acc_related(f0, a0, c[ii].freq, c[ii].acc, tobs, tol):
                if keep:
                    c[idx].assoc.append(c[ii])
                uniq[ii] = False
    return cond


def harmonic_levels64(P: np.ndarray, nlevels: int, scales=None, rounding: bool = True) -> List[np.ndarray]:
    """Levels 0..nlevels of the incoherent harmonic sum in float64, every bin:
    level h at bin i is 2^(-h/2) sum_{m = 1..2^h} P[(i m + 2^(h-1)) >> h]
    (the nearest bin to i m / 2^h, ties up).  scales: the factor per level
    (default LEVEL_SCALE); rounding False drops the 2^(h-1)."""
    P = np.asarray(P, dtype=np.float64)
    scales = LEVEL_SCALE if scales is None else scales
    i = np.arange(len(P), dtype=np.int64)
    out = [P * scales[0]]
    for h in range(1, nlevels + 1):
        r = (1 << (h - 1)) if rounding else 0
        val = np.zeros(len(P))
        for m in range(1, (1 << h) + 1):
            val += P[(i * m + r) >> h]
        out.append(val * scales[h])
    return out


def search_setup(params) -> Dict:
    """What SearchEngine's constructor derives from its SearchParams: n, nb,
    tobs and bin_width (float32, formed as the constructor forms them),
    nlevels and per level the (start, end, factor) of the search range, end
    not below start."""
    n = int(params.fft_size)
    nb = n // 2 + 1
    tobs = np.float32(np.float32(n) * np.float32(params.tsamp))
    bw = np.float32(1.0 / float(tobs))
    nlev = min(max(int(params.nharmonics), 0), 5)
    bounds = []
    for h in range(nlev + 1):
        s, e, fac = peak_bounds(nb, float(bw), h, params.min_freq, params.max_freq)
        bounds.append((s, max(s, e), fac))
    return dict(n=n, nb=nb, tobs=float(tobs), bin_width=float(bw), nlevels=nlev, bounds=bounds)


def search_levels64(trial_u8: np.ndarray, nsamps: int, params, accs, floor: float, bounds=None, stats=None,
                    search_accs=None, scales=None, rounding: bool = True) -> Dict:
    """The dense part of the oracle: per acceleration trial and level, the
    bins (ascending) inside the level's search range whose float64 value
    exceeds ``floor``, and those values.

    The whitened series is n irfft(D) of whiten64's D, the normalisation its
    interbin (mean, std) times n: the engine's series is the unnormalised
    inverse transform, and SpecOut::nscale = n scales the unit-scale stats to
    it.  The keyword arguments exist for defective oracles: bounds replaces
    search_setup's, stats = (mean, std) the trial's own, search_accs the
    accelerations the spectra are formed at (the candidates keep accs)."""
    su = search_setup(params)
    n = su["n"]
    if bounds is not None:
        su["bounds"] = list(bounds)
    tsamp = f32(params.tsamp)
    D, st, _, _ = whiten64(np.asarray(trial_u8)[:nsamps], n, tsamp, list(params.zap_freqs), list(params.zap_widths),
                           params.boundary_5_freq, params.boundary_25_freq)
    x = np.fft.irfft(D, n) * n
    mean, std = (st[0], st[2]) if stats is None else stats
    trials = []
    for a in (accs if search_accs is None else search_accs):
        P = search_spectrum(x, a, tsamp, mean * n, std * n)
        rows = []
        for h, L in enumerate(harmonic_levels64(P, su["nlevels"], scales, rounding)):
            s, e, _ = su["bounds"][h]
            idx = np.nonzero(L[s:e] > floor)[0] + s
            rows.append((idx, L[idx]))
        trials.append(rows)
    su.update(accs=[f32(a) for a in accs], floor=float(floor), trials=trials, stats=(mean, st[1], std))
    return su


def cluster_peaks64(idx: np.ndarray, val: np.ndarray, min_gap: int):
    """unique_peaks with the evidence a test of it needs: per cluster (peak
    bin, peak value, largest other value or -inf, number of crossings)."""
    out = []
    ii, n = 0, len(idx)
    while ii < n:
        first = ii
        cpeak, cidx, last = val[ii], idx[ii], idx[ii]
        ii += 1
        while ii < n and idx[ii] - last < min_gap:
            if val[ii] > cpeak:
                cpeak, cidx, last = val[ii], idx[ii], idx[ii]
            ii += 1
        rest = np.sort(val[first:ii])[:-1]
        out.append((int(cidx), float(cpeak), float(rest[-1]) if len(rest) else -np.inf, ii - first))
    return out


def search_candidates64(levels: Dict, params, min_snr: float, dm: float, dm_idx: int, raw: bool = False,
                        min_gap: Optional[int] = None) -> Dict:
    """The decisions of the oracle on search_levels64's values: crossings
    strictly above float32(min_snr) (not below levels['floor']), clusters,
    candidates (dm, dm_idx, acc, nh, snr, float32(bin factor)), the per-trial
    harmonic distiller (freq_tol, max_harm, fractional, nothing kept) and,
    unless raw, the per-DM acceleration distiller (tobs, freq_tol, related
    ones kept).  Returns dict(cands, per_trial = the harmonic-distilled list
    of every trial, harm_in = the lists before it, clusters[trial][level] =
    cluster_peaks64's tuples)."""
    thresh = f32(min_snr)
    assert thresh >= levels["floor"], "the levels were not kept down to this threshold"
    gap = int(params.min_gap) if min_gap is None else int(min_gap)
    harm = harm_cond(params.freq_tol, f32(params.max_harm), False, True)
    clusters, harm_in, per_trial = [], [], []
    for acc, rows in zip(levels["accs"], levels["trials"]):
        cl, trial = [], []
        for h, (idx, val) in enumerate(rows):
            keep = val > thresh
            cl.append(cluster_peaks64(idx[keep], val[keep], gap))
            fac = levels["bounds"][h][2]
            trial += [Cand(f32(dm), int(dm_idx), acc, h, snr, f32(pi * fac)) for pi, snr, _, _ in cl[-1]]
        clusters.append(cl)
        harm_in.append(trial)
        per_trial.append(py_distill(trial, harm))
    cands = [c for t in per_trial for c in t]
    if not raw:
        cands = py_distill(cands, acc_cond(levels["tobs"], params.freq_tol, True))
    return dict(cands=cands, per_trial=per_trial, harm_in=harm_in, clusters=clusters, min_snr=thresh)


def search_trial64(trial_u8: np.ndarray, nsamps: int, params, accs, dm: float, dm_idx: int, raw: bool = False,
                   **variant) -> Dict:
    """SearchEngine::search_trial from its definition (search_levels64 at
    floor = min_snr, then search_candidates64)."""
    levels = search_levels64(trial_u8, nsamps, params, accs, f32(params.min_snr), **variant)
    return search_candidates64(levels, params, params.min_snr, dm, dm_idx, raw)


# ---------------------------------------------------------------- folding --
def fold_indices(n: int, tsamp_by_period: float, af: float, nbins: int = 64, nints: int = 16):
    """Per folded sample j < (n // nints) * nints: (subint, phase bin, source
    index, phase in [0, 1), unrounded source position), all from float64.
    The source is the v1 resampler's (resample_v1), clamped to [0, n - 1]."""
    nps = n // nints
    j = np.arange(nps * nints, dtype=np.float64)
    ph = np.modf(j * tsamp_by_period)[0]
    b = np.floor(ph * nbins).astype(np.int64)
    s = np.arange(nps * nints) // nps
    h = n / 2.0
    pos = j + af * ((j - h) ** 2 - h * h)
    src = np.clip(np.rint(pos), 0, n - 1).astype(np.int64)
    return s, b, src, ph, pos


def fold_sums(x: np.ndarray, tsamp_by_period: float, af: float, nbins: int = 64, nints: int = 16):
    """The raw fold of one job (fold.hip fold_accumulate): sums float64
    [nints, nbins] and counts int64 [nints, nbins] (from 0) of the resampled
    series x[src(j)] over the samples j of each subint and phase bin."""
    s, b, src, _, _ = fold_indices(len(x), tsamp_by_period, af, nbins, nints)
    out = np.zeros((nints, nbins), np.float64)
    cnt = np.zeros((nints, nbins), np.int64)
    np.add.at(out, (s, b), x[src].astype(np.float64))
    np.add.at(cnt, (s, b), 1)
    return out, cnt


def fold_series(x: np.ndarray, period: float, tsamp: float, nbins: int = 64, nints: int = 16,
                af: float = 0.0) -> np.ndarray:
    """fold_time_series_kernel (kernels.cu:597-633): counts start at 1.  af
    (accel_factor) folds the v1-resampled series, as the fused fold kernel."""
    out, cnt = fold_sums(x, tsamp / period, af, nbins, nints)
    return (out / (cnt + 1)).astype(np.float32)


def shift_table(nbins: int = 64, nints: int = 16) -> np.ndarray:
    two_pi = np.float32(2 * 3.14159265359)
    s = np.arange(nbins)[:, None, None]
    i = np.arange(nints)[None, :, None].astype(np.float32)
    b = np.arange(nbins)[None, None, :]
    shift = (i / np.float32(nints)) * (s - nbins // 2).astype(np.float32)
    ramp = (b.astype(np.float32) * two_pi / np.float32(nbins)).astype(np.float32)
    ramp = np.where(b > nbins // 2, ramp - two_pi, ramp).astype(np.float32)
    ph = (-1.0 * ramp * shift).astype(np.float32)
    return np.exp(1j * ph.astype(np.float64)).astype(np.complex64)


def fold_optimise(fold: np.ndarray, nbins: int = 64, nints: int = 16):
    """FoldOptimiser::optimise (folder.hpp:235-334) with numpy FFTs:
    returns (opt_template, opt_shift, opt_bin_raw, opt_fold, opt_prof)."""
    F = np.fft.fft(fold.astype(np.complex64), axis=1)
    sh = shift_table(nbins, nints)
    post = F[None, :, :] * sh                      # [shift][int][bin]
    prof = post.sum(axis=1)                        # [shift][bin]
    ntmpl = nbins - 1
    box = (np.arange(nbins)[None, :] <= np.arange(ntmpl)[:, None]).astype(np.complex64)
    T = np.fft.fft(box, axis=1)                    # [template][bin]
    arr = prof[None, :, :] * T[:, None, :] / np.sqrt(np.arange(1, ntmpl + 1, dtype=np.float32))[:, None, None]
    arr[:, :, 0] = 0
    inv = np.fft.ifft(arr, axis=2) * nbins         # unnormalised inverse
    mag = np.abs(inv).astype(np.float32)
    am = int(np.argmax(mag))
    t = am // (nbins * nbins)
    s = (am // nbins) % nbins
    j = am % nbins
    opt_fold = (np.fft.ifft(post[s], axis=1) * nbins).real.astype(np.float32)
    opt_prof = (np.fft.ifft(prof[s]) * nbins).real.astype(np.float32)
    return t, s, j, opt_fold, opt_prof


def fold_optimise_cube(fold: np.ndarray, nbins: int = 64, nints: int = 16) -> np.ndarray:
    """The float32 magnitude cube [template][shift][bin] whose argmax
    fold_optimise returns (its complex64 arithmetic, before the cast)."""
    F = np.fft.fft(fold.astype(np.complex64), axis=1)
    prof = (F[None, :, :] * shift_table(nbins, nints)).sum(axis=1)
    ntmpl = nbins - 1
    box = (np.arange(nbins)[None, :] <= np.arange(ntmpl)[:, None]).astype(np.complex64)
    T = np.fft.fft(box, axis=1)
    arr = prof[None, :, :] * T[:, None, :] / np.sqrt(np.arange(1, ntmpl + 1, dtype=np.float32))[:, None, None]
    arr[:, :, 0] = 0
    return np.abs(np.fft.ifft(arr, axis=2) * nbins)


def fold_optimise64(fold: np.ndarray, nbins: int = 64, nints: int = 16, shift: Optional[int] = None):
    """fold_optimise in complex128: the shift phases stay the float32 values
    of shift_table (they define the operation), everything after them is
    float64.  Returns (opt_template, opt_shift, opt_bin_raw, opt_fold float64,
    opt_prof float64, mag float64 [nbins - 1, nbins, nbins]); opt_fold and
    opt_prof are evaluated at ``shift`` when given, else at opt_shift."""
    F = np.fft.fft(fold.astype(np.float64), axis=1)
    two_pi = np.float32(2 * 3.14159265359)
    sv = np.arange(nbins)[:, None, None]
    iv = np.arange(nints)[None, :, None].astype(np.float32)
    bv = np.arange(nbins)[None, None, :]
    sf = (iv / np.float32(nints)) * (sv - nbins // 2).astype(np.float32)
    ramp = (bv.astype(np.float32) * two_pi / np.float32(nbins)).astype(np.float32)
    ramp = np.where(bv > nbins // 2, ramp - two_pi, ramp).astype(np.float32)
    sh = np.exp(1j * (-1.0 * ramp * sf).astype(np.float32).astype(np.float64))
    post = F[None, :, :] * sh                      # [shift][int][bin]
    prof = post.sum(axis=1)                        # [shift][bin]
    ntmpl = nbins - 1
    box = (np.arange(nbins)[None, :] <= np.arange(ntmpl)[:, None]).astype(np.float64)
    T = np.fft.fft(box, axis=1)                    # [template][bin]
    arr = prof[None, :, :] * T[:, None, :] / np.sqrt(np.arange(1, ntmpl + 1, dtype=np.float64))[:, None, None]
    arr[:, :, 0] = 0
    mag = np.abs(np.fft.ifft(arr, axis=2) * nbins)
    am = int(np.argmax(mag))
    t = am // (nbins * nbins)
    s = (am // nbins) % nbins
    j = am % nbins
    at = s if shift is None else int(shift)
    opt_fold = (np.fft.ifft(post[at], axis=1) * nbins).real
    opt_prof = (np.fft.ifft(prof[at]) * nbins).real
    return t, s, j, opt_fold, opt_prof, mag


def calculate_sn(prof: np.ndarray, bin: int, width: int) -> Tuple[float, float]:
    nbins = len(prof)
    edge = int(width * 0.3 + 0.5)
    wb2 = int(width / 2.0 + 0.5)
    rprof = np.array([prof[(bin - nbins // 2 + ii) % nbins] for ii in range(nbins)], np.float32)
    b = nbins // 2 - 1
    up, lo = b + (wb2 + edge), b - (wb2 + edge)
    on = np.array([rprof[i] for i in range(nbins) if lo <= i <= up], np.float32)
    off = np.array([rprof[i] for i in range(nbins) if not (lo <= i <= up)], np.float32)
    # an empty off-pulse set (wide templates) has mean NaN, as the native code
    on_mean = np.float32(on.astype(np.float64).sum() / len(on))
    off_mean = np.float32(off.astype(np.float64).sum() / len(off)) if len(off) else np.float32(np.nan)
    acc = np.float32(0)
    for v in off:
        acc = np.float32(float(acc) + (float(v) - float(off_mean)) ** 2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        off_std = np.sqrt(acc / np.float32(len(off)))
        sn1 = np.float32(np.float64(on_mean - off_mean) * math.sqrt(width) / np.float64(off_std))
        r = ((rprof - off_mean) / off_std).astype(np.float32)
        # width 0 divides by zero: +-inf or NaN by the sign of the sum
        sn2 = np.float32(np.float64(r.astype(np.float64).sum()) / np.float64(math.sqrt(width)))
    if sn1 > 99999:
        sn1 = np.float32(0)
    if sn2 > 99999:
        sn2 = np.float32(0)
    return float(sn1), float(sn2)


def coincidence_mask(arrays: Sequence[np.ndarray], thresh: float, beam_thresh: int) -> np.ndarray:
    cnt = np.zeros(len(arrays[0]), np.int64)
    for a in arrays:
        cnt += (a > np.float32(thresh))
    return (cnt < beam_thresh).astype(np.float32)


# ----------------------------------------------------------------- FFA ------
def ffa_transform(X: np.ndarray) -> np.ndarray:
    """Radix-2 FFA (Staelin) of an [m, P] fold matrix, m a power of two:
    out[s] = H[s//2] + roll(T[s//2], -((s+1)//2)) over the two transformed
    halves; row s is the fold at period P + s/(m-1) bins (ffa.hip convention).
    Evaluated in float64 (the oracle)."""
    X = np.asarray(X, dtype=np.float64)
    m = X.shape[0]
    if m == 1:
        return X.copy()
    h = m // 2
    H, T = ffa_transform(X[:h]), ffa_transform(X[h:])
    out = np.empty_like(X)
    for s in range(m):
        j = s // 2
        out[s] = H[j] + np.roll(T[j], -((s + 1) // 2))
    return out


def ffa_fold_matrix(ds: np.ndarray, P: int) -> np.ndarray:
    """[m2, P]: floor(len/P) rows of the series, zero rows up to a power of two."""
    m = len(ds) // P
    m2 = 1 << int(np.ceil(np.log2(max(1, m))))
    X = np.zeros((m2, P), dtype=np.float64)
    X[:m] = np.asarray(ds[: m * P], dtype=np.float64).reshape(m, P)
    return X


def boxcar_best_snr(profile: np.ndarray, widths, var: float) -> float:
    """Max over widths and circular phases of boxcar_sum / sqrt(w var)."""
    p = np.asarray(profile, dtype=np.float64)
    P = len(p)
    ext = np.concatenate([p, p])
    c = np.concatenate([[0.0], np.cumsum(ext)])
    best = -np.inf
    for w in widths:
        if w >= P:
            break
        s = (c[w: w + P] - c[:P]).max()
        best = max(best, s / np.sqrt(w * var))
    return best


def ffa_downsample(x: np.ndarray, f: float) -> np.ndarray:
    """Piecewise-constant integration over [j f, (j+1) f)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    nout = int(np.floor(n / f))
    c = np.concatenate([[0.0], np.cumsum(x)])

    def integ(t):
        i = np.minimum(np.floor(t).astype(np.int64), n)
        frac = t - i
        return c[i] + np.where(i < n, x[np.minimum(i, n - 1)] * frac, 0.0)

    j = np.arange(nout + 1, dtype=np.float64) * f
    I = integ(j)
    return I[1:] - I[:-1]


# Exact FFA oracles.  The FFA only adds: on integer-valued input every float32
# partial sum of the kernels is an exact integer (below 2^24), so planes and
# boxcar sums must equal these int64 results bit for bit.
def ffa_transform_exact(X: np.ndarray) -> np.ndarray:
    """ffa_transform on an integer [m2, P] matrix in int64, stage by stage:
    stage st merges transformed blocks of q = 2^st rows into blocks of 2q with
    one row gather and one add (fast at m2 = 2^17)."""
    X = np.asarray(X)
    assert X.ndim == 2 and np.issubdtype(X.dtype, np.integer), "integer [m2, P] matrix"
    m2, P = X.shape
    assert m2 >= 1 and m2 & (m2 - 1) == 0, "rows must be a power of two"
    cur = X.astype(np.int64)
    r = np.arange(m2)
    cols = np.arange(P)
    q = 1
    while q < m2:
        s = r & (2 * q - 1)  # row within its output block
        h = (r - s) + (s >> 1)  # head-half source row; the tail-half one is q further
        sh = ((s + 1) >> 1) % P
        idx = (cols[None, :] + sh[:, None]) % P
        cur = cur[h] + np.take_along_axis(cur[h + q], idx, axis=1)
        q *= 2
    return cur


def ffa_fold_matrix_exact(ds: np.ndarray, P: int) -> np.ndarray:
    """ffa_fold_matrix of an integer series, in int64."""
    ds = np.asarray(ds)
    m = len(ds) // P
    m2 = 1
    while m2 < m:
        m2 *= 2
    X = np.zeros((m2, P), dtype=np.int64)
    X[:m] = ds[: m * P].astype(np.int64).reshape(m, P)
    return X


def ffa_boxcar_snr(planes: np.ndarray, widths, var: float) -> Tuple[List[int], np.ndarray]:
    """(used widths, snr[len(used), m2]) in float64 of the [m2, P] profiles:
    snr = max over circular phases of the boxcar sum / sqrt(w var), for every
    ladder width that passes the w < P cut.  Exact sums on integer planes."""
    p = np.asarray(planes)
    if not np.issubdtype(p.dtype, np.integer):
        p = p.astype(np.float64)
    P = p.shape[1]
    c = np.concatenate([np.zeros((p.shape[0], 1), dtype=p.dtype), np.cumsum(np.concatenate([p, p], axis=1), axis=1)],
                       axis=1)
    used = [int(w) for w in widths if w < P]
    snr = np.empty((len(used), p.shape[0]), dtype=np.float64)
    for k, w in enumerate(used):
        snr[k] = (c[:, w: w + P] - c[:, :P]).max(axis=1) / np.sqrt(np.float64(w) * np.float64(var))
    return used, snr


def ffa_search_oracle(u8: np.ndarray, params, min_snr: Optional[float] = None, dense: Optional[List[Dict]] = None):
    """Oracle of FfaEngine.search for inputs on which the engine is exact.

    Octaves, chunks and periods come from _C.ffa_plan(params, n); detrend
    (sp_trend over the engine's window), mean / standard deviation and the
    per-profile S/N are float64, the normalised series, the downsampled series
    and the planes int64.  Raises ValueError unless the normalised series is
    integer-valued and every octave factor an integer.

    Returns (dense, raw, candidates).  dense: one dict per (octave, chunk,
    period index) with P, m, m2, factor, the used widths and snr[width, drift];
    pass it back in to threshold again without recomputing.  raw (None when
    min_snr is None): the records with best S/N > float32(min_snr) in (octave,
    chunk, period index, drift) order, as dicts with period
    (P + drift / (m2 - 1)) * factor * tsamp, the float64 snr, the narrowest
    best width, nbins, octave and the per-width snr.  candidates:
    _C.ffa_cluster of raw (S/N rounded to float32)."""
    from peasoup_amd import _C as C

    u8 = np.asarray(u8, dtype=np.uint8)
    n = len(u8)
    if dense is None:
        window = int(math.ceil((params.detrend_s if params.detrend_s > 0 else 3.0 * params.p_end) / params.tsamp))
        window = min(max(window, 64), n)
        x = u8.astype(np.float64) - sp_trend(u8, window)
        mean = x.mean()
        std = math.sqrt(max((x * x).mean() - mean * mean, 0.0))
        xn = (x - mean) / std
        if not np.array_equal(xn, np.rint(xn)):
            raise ValueError("ffa_search_oracle: the normalised series is not integer-valued")
        xi = np.rint(xn).astype(np.int64)
        dense = []
        for o, oc in enumerate(C.ffa_plan(params, n)):
            f = int(oc["factor"])
            if f != oc["factor"]:
                raise ValueError("ffa_search_oracle: octave factor %r is not an integer" % oc["factor"])
            nds = int(oc["nds"])
            ds = xi[: nds * f].reshape(nds, f).sum(axis=1)
            for ci, ch in enumerate(oc["chunks"]):
                for pi, (P, m, m2, lg, off) in enumerate(ch["periods"]):
                    plane = ffa_transform_exact(ffa_fold_matrix_exact(ds, P))
                    assert plane.shape == (m2, P) and m == nds // P
                    used, snr = ffa_boxcar_snr(plane, C.ffa_widths(C.ffa_base_bins(params)), float(m) * float(f))
                    dense.append(dict(octave=o, chunk=ci, period_idx=pi, P=P, m=m, m2=m2, factor=float(f),
                                      widths=used, snr=snr))
    if min_snr is None:
        return dense, None, None
    thresh = float(np.float32(min_snr))
    raw = []
    for d in dense:
        best = d["snr"].max(axis=0)
        arg = d["snr"].argmax(axis=0)  # first maximum: the narrowest width
        for s in np.nonzero(best > thresh)[0]:
            pbins = d["P"] + float(s) / (d["m2"] - 1) if d["m2"] > 1 else float(d["P"])
            raw.append(dict(period=pbins * (d["factor"] * params.tsamp), snr=float(best[s]),
                            width=d["widths"][int(arg[s])], nbins=d["P"], octave=d["octave"], drift=int(s),
                            widths=d["widths"], snr_by_width=d["snr"][:, s]))
    cands = []
    for r in raw:
        c = C.FfaCandidate()
        c.period, c.snr, c.width, c.nbins, c.octave = r["period"], r["snr"], r["width"], r["nbins"], r["octave"]
        cands.append(c)
    tobs = n * params.tsamp
    return dense, raw, C.ffa_cluster(cands, params.cluster_tol / tobs)


# ------------------------------------------------------- single pulses ------
# Float64 oracle of the single-pulse search, written from its definition
# (csrc/include/psoup/singlepulse.hpp), not from the kernel.
def sp_widths(n: int, wmax: int) -> List[int]:
    """Powers of two up to min(wmax, n // 2)."""
    out, w = [], 1
    while w <= min(int(wmax), int(n) // 2):
        out.append(w)
        w *= 2
    return out


def sp_trend(u8: np.ndarray, baseline: int) -> np.ndarray:
    """Block means over `baseline` samples (exact integer sums), linear
    between block centres, flat before the first and after the last."""
    u = np.asarray(u8)
    n = len(u)
    nblk = (n + baseline - 1) // baseline
    means = np.array([u[b * baseline:(b + 1) * baseline].astype(np.int64).sum() /
                      float(len(u[b * baseline:(b + 1) * baseline])) for b in range(nblk)], dtype=np.float64)
    if nblk == 1:
        return np.full(n, means[0])
    pos = (np.arange(n, dtype=np.float64) - 0.5 * baseline) / baseline  # in block-centre units
    return np.interp(pos, np.arange(nblk, dtype=np.float64), means)  # clamps outside [0, nblk - 1]


def sp_boxcar_snr(u8: np.ndarray, baseline: int, widths) -> List[np.ndarray]:
    """snr_k[i] = sum(x[i:i + w_k]) / (sigma sqrt(w_k)) for 0 <= i <= n - w_k,
    x = u8 - trend, sigma = sqrt(mean(x^2)); all zeros when sigma == 0."""
    x = np.asarray(u8, dtype=np.float64) - sp_trend(u8, baseline)
    n = len(x)
    sigma = math.sqrt(float(np.mean(x * x)))
    c = np.concatenate([[0.0], np.cumsum(x)])
    out = []
    for w in widths:
        s = c[w:n + 1] - c[:n + 1 - w]
        out.append(s / (sigma * math.sqrt(w)) if sigma > 0 else np.zeros_like(s))
    return out


def sp_block_maxima(snr: Sequence[np.ndarray], block: int = 64):
    """Per width: (maxima, argmax) over the aligned blocks of `block` start
    samples that hold at least one start (the last may be partial); the
    lowest index on a tie."""
    out = []
    for s in snr:
        nb = (len(s) + block - 1) // block
        mx = np.empty(nb, dtype=np.float64)
        am = np.empty(nb, dtype=np.int64)
        for b in range(nb):
            seg = s[b * block:(b + 1) * block]
            j = int(np.argmax(seg))  # first occurrence
            mx[b], am[b] = seg[j], b * block + j
        out.append((mx, am))
    return out


SP_EPS32 = 2.0 ** -23  # float32 machine epsilon: twice the unit roundoff of one rounded operation


def sp_block_means(u8: np.ndarray, baseline: int) -> Tuple[np.ndarray, np.ndarray]:
    """(exact int64 sum, sample count) of every trend block."""
    u = np.asarray(u8).astype(np.int64)
    n = len(u)
    nblk = (n + baseline - 1) // baseline
    sums = np.array([u[b * baseline:(b + 1) * baseline].sum() for b in range(nblk)], dtype=np.int64)
    counts = np.array([min(n, (b + 1) * baseline) - b * baseline for b in range(nblk)], dtype=np.int64)
    return sums, counts


def sp_sigma(u8: np.ndarray, baseline: int) -> float:
    """sqrt(mean((u8 - trend)^2)) over all n samples, as in sp_boxcar_snr."""
    x = np.asarray(u8, dtype=np.float64) - sp_trend(u8, baseline)
    return math.sqrt(float(np.mean(x * x)))


def _sp_trend_error(u8: np.ndarray, baseline: int) -> np.ndarray:
    """Per sample: bound on |float32 kernel trend - sp_trend| (see sp_error_bound)."""
    u = np.asarray(u8)
    n = len(u)
    sums, counts = sp_block_means(u, baseline)
    M = sums / counts.astype(np.float64)
    t = sp_trend(u, baseline)
    nblk = len(M)
    if nblk == 1:
        return SP_EPS32 * np.abs(t)  # means[0] is returned as it is: one rounding
    pos = (np.arange(n, dtype=np.float64) - 0.5 * baseline) / baseline
    b = np.clip(np.floor(pos).astype(np.int64), 0, nblk - 2)
    m_abs = np.maximum(np.abs(M[b]), np.abs(M[b + 1]))
    d = np.abs(M[b + 1] - M[b])
    # At an exact block centre the kernel's double pos may fall a rounding
    # below the integer: it then interpolates in the block before, fr ~ 1.
    dl = np.abs(np.diff(M))
    dmax = np.maximum(np.concatenate([[0.0], dl]), np.concatenate([dl, [0.0]]))  # per centre: both neighbours
    j = np.rint(pos)
    centre = (np.abs(pos - j) < 1e-6) & (j >= 0) & (j <= nblk - 1)
    jj = np.clip(j.astype(np.int64), 0, nblk - 1)
    d = np.where(centre, dmax[jj], d)
    m_abs = np.where(centre, np.maximum(m_abs, np.abs(M[np.clip(jj - 1, 0, nblk - 1)])), m_abs)
    e = SP_EPS32 * (m_abs + 3.0 * d + np.abs(t))
    flat = ((pos <= 0) | (pos >= nblk - 1)) & ~centre
    return np.where(flat, SP_EPS32 * np.abs(t), e)


def sp_sigma_rel_bound(u8: np.ndarray, baseline: int) -> float:
    """Bound on |kernel sigma - oracle sigma| / sigma.  The kernel's sigma is
    the root mean square (in double) of x^ = fl32(u - t^); with x^ = x + d,
    |d_i| <= e_t[i] + eps32 |x_i| (trend error, one subtraction), the
    triangle inequality on the 2-norm gives |sigma^ - sigma| <= rms(e_t) +
    eps32 sigma.  The double accumulation, division and root add a few 2^-53
    n, covered by 1e-12.  Zero for a constant row (both sigmas are 0)."""
    sigma = sp_sigma(u8, baseline)
    if sigma == 0:
        return 0.0
    e_t = _sp_trend_error(u8, baseline)
    return math.sqrt(float(np.mean(e_t * e_t))) / sigma + SP_EPS32 + 1e-12


def sp_error_bound(u8: np.ndarray, baseline: int, widths) -> List[np.ndarray]:
    """Per width w = 2^k: float64 array over the starts 0..n - w, a worst-case
    bound on |kernel S/N - sp_boxcar_snr|, from the kernel's arithmetic and
    oracle quantities only.  Every rounded float32 operation is charged eps32 =
    2^-23 (relative), twice its unit roundoff: the factor of two pays for all
    second-order terms, for the double arithmetic of pos and for the contraction
    of a multiply-add, which only removes a rounding.

    Trend t^ = fl(m0 + fl(fr fl(m1 - m0))), M the exact means, d = |M1 - M0|:
      means rounded to float32         max(|M0|, |M1|) eps32
      fr = fl32(pos - b), |dfr| eps32  d eps32
      the difference, the product      2 d eps32
      the sum                          |t| eps32
    so e_t = eps32 (max|M| + 3 d + |t|) <= 5 * 255 eps32; where the trend is
    flat (before the first centre, past the last, one block) a mean is returned
    as it is and e_t = eps32 |t|.
    Staged y^ = fl(fl(u - t^) fl32(1 / sigma^)): the subtraction, the rounding
    of 1 / sigma^ and the product cost 3 eps32 |y|, sigma^ itself r' |y| with
    r' = r / (1 - r), r = sp_sigma_rel_bound:  e_y = e_t / sigma + (3 eps32 + r') |y|.
    A dyadic sum of 2^k terms passes every term through k additions:
    k eps32 sum|y^|; the scale (a float32 constant, one product) 2 eps32.  With
    sum|y^| <= sum(|y| + e_y):

      bound_w[i] = ((1 + (k + 2) eps32) sum e_y + (k + 2) eps32 sum|y|) / sqrt(w)
                <= eps32 (c1 255 sqrt(w) / sigma + (k + c2) sum|y| / sqrt(w)),
      c1 = 5 (1 + 15 eps32), c2 = 5 + r' / eps32,

    the sums over the window [i, i + w).  All zeros for a constant row: the
    kernel's means, residuals and sigma are then exactly 0 and so is its S/N."""
    u = np.asarray(u8)
    n = len(u)
    x = u.astype(np.float64) - sp_trend(u, baseline)
    sigma = math.sqrt(float(np.mean(x * x)))
    if sigma == 0:
        return [np.zeros(n + 1 - w) for w in widths]
    r = sp_sigma_rel_bound(u, baseline)
    r = r / (1.0 - r)
    y = np.abs(x) / sigma
    e_y = _sp_trend_error(u, baseline) / sigma + (3.0 * SP_EPS32 + r) * y
    cy = np.concatenate([[0.0], np.cumsum(y)])
    ce = np.concatenate([[0.0], np.cumsum(e_y)])
    out = []
    for w in widths:
        k = int(w).bit_length() - 1
        assert 1 << k == w
        sy = cy[w:n + 1] - cy[:n + 1 - w]
        se = ce[w:n + 1] - ce[:n + 1 - w]
        out.append(((1.0 + (k + 2) * SP_EPS32) * se + (k + 2) * SP_EPS32 * sy) / math.sqrt(w))
    return out


def sp_scale32(k: int) -> np.float32:
    """The search's float32 scale 2^(-k / 2) of level k: exact for even k, the
    rounded 1 / sqrt(2) over a power of two for odd k."""
    if k & 1:
        return np.float32(np.float32(0.70710678118654752) / np.float32(1 << (k >> 1)))
    return np.float32(1.0 / (1 << (k >> 1)))


def sp_boxcar_snr_exact(u8: np.ndarray, widths) -> Dict:
    """Integer-exact single-pulse S/N for a row whose trend is one block (the
    baseline is the row) with an integer mean and whose sigma is a power of
    two.  Then x = u - mean are integers, x / sigma and every window sum of
    them are exact in float32 (|sum| sigma < 2^24) in any order, and the only
    rounding is the product with the float32 scale of the level.  Returns
    sums (int64 per width), sigma, snr (float64 sums / (sigma sqrt(w))) and
    snr32: the float32 the search must return, fl32(sum / sigma * scale32(k)),
    the product exact in float64."""
    u = np.asarray(u8).astype(np.int64)
    n = len(u)
    tot = int(u.sum())
    assert tot % n == 0, "sp_boxcar_snr_exact: the mean must be an integer"
    x = u - tot // n
    sumsq = int((x * x).sum())
    sigma = math.sqrt(sumsq / n)
    assert sigma > 0 and math.frexp(sigma)[0] == 0.5 and sigma * sigma * n == sumsq, \
        "sp_boxcar_snr_exact: sigma must be a power of two"
    c = np.concatenate([[0], np.cumsum(x)])
    sums, snr, snr32 = [], [], []
    for w in widths:
        k = int(w).bit_length() - 1
        s = c[w:n + 1] - c[:n + 1 - w]
        assert np.abs(s).max() * max(sigma, 1.0) < 2 ** 24
        sums.append(s)
        snr.append(s / (sigma * math.sqrt(w)))
        snr32.append(((s / sigma) * float(sp_scale32(k))).astype(np.float32))
    return dict(sums=sums, sigma=sigma, snr=snr, snr32=snr32)


def sp_search_f32(u8: np.ndarray, baseline: int, kmax: int, tile: int = 8192, halo_max: int = 4096,
                  block: int = 64) -> Tuple[np.ndarray, np.ndarray]:
    """Float32 NumPy emulation of the search in its own order, per tile of
    `tile` starts with a window of tile + 2^kmax samples: float32 means and
    trend, sigma from float32 residuals summed in double, staging (samples past
    n are zero), widths 1..8 from twelve staged samples per group of four,
    then B_2w[i] = B_w[i] + B_w[i + w] with the window's guards (a group whose
    partner lies past the window keeps its value, and its stale copy in the
    window).  Unstaged window memory is NaN, so a result that depended on it
    would show.  Returns (best float32, arg uint32) [kmax + 1, ceil(n / 64)]
    as the search's dense outputs: the lowest index on a tie, 0 and 0xffffffff
    where a block holds no valid start."""
    f32 = np.float32
    u = np.asarray(u8)
    n = len(u)
    sums, counts = sp_block_means(u, baseline)
    means = (sums / counts.astype(np.float64)).astype(f32)
    nblk = len(means)
    if nblk == 1:
        trend = np.full(n, means[0], dtype=f32)
    else:
        pos = (np.arange(n, dtype=np.float64) - 0.5 * baseline) * (1.0 / baseline)
        b = np.clip(pos.astype(np.int64), 0, nblk - 2)
        fr = (pos - b).astype(f32)
        m0 = means[b]
        trend = (m0 + (fr * (means[b + 1] - m0)).astype(f32)).astype(f32)
        trend = np.where(pos <= 0.0, means[0], trend)
        trend = np.where(pos >= nblk - 1, means[nblk - 1], trend).astype(f32)
    x = (u.astype(f32) - trend).astype(f32)
    sigma = math.sqrt(float((x.astype(np.float64) ** 2).sum()) / n)
    inv_sigma = f32(1.0 / sigma) if sigma > 0 else f32(0)
    y = (x * inv_sigma).astype(f32)

    H = 1 << kmax
    L = tile + H
    ngroups = (tile + halo_max) // 4
    own = tile // 4
    gi = 4 * np.arange(ngroups)
    four = np.arange(4)
    nb64 = (n + block - 1) // block
    best = np.zeros((kmax + 1, nb64), dtype=f32)
    arg = np.full((kmax + 1, nb64), 0xFFFFFFFF, dtype=np.uint32)

    def emit(k, t0, sums_own):
        w = 1 << k
        vals = (sums_own.reshape(-1) * sp_scale32(k)).astype(f32)  # starts t0 .. t0 + tile - 1
        start = t0 + np.arange(tile)
        valid = start + w <= n
        masked = np.where(valid, vals, -np.inf).reshape(-1, block)
        nanrow = (np.isnan(vals) & valid).reshape(-1, block).any(axis=1)
        j = np.argmax(np.where(np.isnan(masked), -np.inf, masked), axis=1)  # first occurrence
        for r in range(tile // block):
            blk = t0 // block + r
            if blk >= nb64 or not valid[r * block:(r + 1) * block].any():
                continue
            best[k, blk] = np.nan if nanrow[r] else masked[r, j[r]]
            arg[k, blk] = t0 + r * block + j[r]

    for t0 in range(0, n, tile):
        lds = np.full(tile + halo_max + 8, np.nan, dtype=f32)
        nst = (L + 8) // 4 * 4
        lds[:nst] = 0
        m = max(0, min(n - t0, nst))
        lds[:m] = y[t0:t0 + m]
        act = gi + 4 <= L
        Y = np.where(act[:, None], lds[np.minimum(gi[:, None] + np.arange(12)[None, :], len(lds) - 1)], f32(0))
        b2 = (Y[:, :10] + Y[:, 1:11]).astype(f32)
        b4 = (b2[:, :8] + b2[:, 2:10]).astype(f32)
        B = (b4[:, :4] + b4[:, 4:8]).astype(f32)
        for k, lv in enumerate([Y[:, :4], b2[:, :4], b4[:, :4], B]):
            if k <= kmax:
                emit(k, t0, lv[:own])
        lds[(gi[act][:, None] + four[None, :])] = B[act]
        for k in range(4, kmax + 1):
            w = 1 << (k - 1)
            ok = gi + w + 4 <= L
            B[ok] = (B[ok] + lds[(gi[ok] + w)[:, None] + four[None, :]]).astype(f32)
            emit(k, t0, B[:own])
            if k == kmax:
                break
            lds[(gi[ok][:, None] + four[None, :])] = B[ok]
    return best, arg


def sp_cluster_ref(events, dm_list, band_delay_per_dm: float, tsamp: float) -> List[Dict]:
    """Literal transcription of the clustering rule.  events: (sample,
    width_log2, snr, dm_idx) tuples.  Taken in descending S/N (ties: dm_idx,
    width_log2, sample); with t = sample + w / 2 an event joins the first
    accepted candidate with |t - t0| <= (w + w0) / 2 + |dm - dm0| *
    band_delay_per_dm / tsamp, else it founds a candidate."""
    order = sorted(events, key=lambda e: (-float(e[2]), int(e[3]), int(e[1]), int(e[0])))
    cands: List[Dict] = []
    for sample, k, snr, d in order:
        sample, k, d = int(sample), int(k), int(d)
        w = 1 << k
        dm = float(dm_list[d])
        t = sample + 0.5 * w
        for c in cands:
            slack = abs(dm - c["dm"]) * band_delay_per_dm / tsamp
            if abs(t - c["t"]) <= 0.5 * (w + c["width"]) + slack:
                c["members"] += 1
                c["first_sample"] = min(c["first_sample"], sample)
                c["last_sample"] = max(c["last_sample"], sample + w - 1)
                c["dm_idx_lo"] = min(c["dm_idx_lo"], d)
                c["dm_idx_hi"] = max(c["dm_idx_hi"], d)
                break
        else:
            cands.append({"sample": sample, "t": t, "time_s": t * tsamp, "width": w, "snr": float(snr), "dm": dm,
                          "dm_idx": d, "members": 1, "first_sample": sample, "last_sample": sample + w - 1,
                          "dm_idx_lo": d, "dm_idx_hi": d})
    return cands


# ------------------------------------------------------------ fold cubes ----
def fold_cube(values: np.ndarray, offsets: np.ndarray, period: float, af: float, tsamp: float, n: int, nints: int,
              nsub: int, nbins: int, killmask=None):
    """Filterbank fold cube of one candidate, written from the definition in
    csrc/include/psoup/foldcube.hpp.  values [nsamps, nchans] raw samples
    (>= 0), offsets int [nchans], af from accel_factor.  Returns (sums int64
    [nints, nsub, nbins], hits int32 [nints, nbins], nactive int32 [nsub])."""
    nsamps, nchans = values.shape
    kill = np.ones(nchans, bool) if killmask is None else np.asarray(killmask) != 0
    off = np.asarray(offsets, dtype=np.int64)
    if int(off.max()) + n > nsamps or int(off.min()) < 0:
        raise ValueError("fold_cube: max(off) + n <= nsamps is required")
    nps = n // nints
    h = n / 2.0
    d = np.arange(nints * nps, dtype=np.float64)
    subint = np.arange(nints * nps, dtype=np.int64) // nps
    tbp = float(np.float32(tsamp)) / float(period)
    frac = np.modf(d * tbp)[0]
    bins = np.clip(np.floor(frac * nbins), 0, nbins - 1).astype(np.int64)
    src = np.clip(np.rint(d + af * ((d - h) * (d - h) - h * h)), 0, n - 1).astype(np.int64)
    hits = np.zeros((nints, nbins), dtype=np.int64)
    np.add.at(hits, (subint, bins), 1)
    sums = np.zeros((nints, nsub, nbins), dtype=np.int64)
    nactive = np.zeros(nsub, dtype=np.int32)
    for c in np.nonzero(kill)[0]:
        s = (int(c) * nsub) // nchans
        nactive[s] += 1
        np.add.at(sums, (subint, s, bins), values[src + off[c], c].astype(np.int64))
    return sums, hits.astype(np.int32), nactive


# --------------------------------------------------------- burst cutouts ----
# NumPy oracle of csrc/include/psoup/burstcube.hpp, written from its
# definition in int64.
def burst_tscrunch(width: int, tscrunch: int = 0) -> int:
    return int(tscrunch) if tscrunch > 0 else max(1, int(width) // 2)


def burst_t0(sample: int, width: int, f: int, ntime: int) -> int:
    return int(sample) + int(width) // 2 - (int(ntime) // 2) * int(f)


def burst_dms(dm: float, ndm: int, dm_half_range: float = 0.0) -> np.ndarray:
    """float32 [ndm] DM rows of a candidate: row ndm // 2 is exactly ``dm``
    (as float32), the rows step by 2 half / ndm and none is negative."""
    d = float(np.float32(dm))
    hr = float(np.float32(dm_half_range))
    half = min(d, hr) if hr > 0 else d
    step = 2.0 * half / ndm
    j = np.arange(ndm, dtype=np.float64) - float(ndm // 2)
    return np.maximum(0.0, d + j * step).astype(np.float32)


def burst_rows(values: np.ndarray, chansets, offsets: np.ndarray, t0: int, f: int, ntime: int, nvalid: int = None):
    """sums, hits (int64 [nrows, ntime]) of rows r with channels chansets[r]
    and offsets[r] (int [nchans]): bin k sums values[u, c] over c in the set
    and u = t0 + k f + i + offsets[r][c], i in [0, f), where 0 <= u < nvalid."""
    n = values.shape[0] if nvalid is None else int(nvalid)
    prefix = np.zeros((values.shape[1], n + 1), dtype=np.int64)
    np.cumsum(values[:n].T.astype(np.int64), axis=1, out=prefix[:, 1:])
    k = np.arange(ntime, dtype=np.int64)
    nrows = len(chansets)
    sums = np.zeros((nrows, ntime), dtype=np.int64)
    hits = np.zeros((nrows, ntime), dtype=np.int64)
    for r in range(nrows):
        for c in chansets[r]:
            lo = int(t0) + k * int(f) + int(offsets[r][c])
            a, b = np.clip(lo, 0, n), np.clip(lo + int(f), 0, n)
            sums[r] += prefix[c, b] - prefix[c, a]
            hits[r] += b - a
    return sums, hits


def burst_cube_offsets(values: np.ndarray, ds_offsets: np.ndarray, dmt_offsets: np.ndarray, t0: int, f: int,
                       ntime: int, nsub: int, killmask=None, nvalid: int = None) -> Dict:
    """The cutout of one candidate at explicit offsets: ds_offsets int
    [nchans], dmt_offsets int [ndm, nchans].  Returns a dict of ds_sums,
    ds_hits (int32 [nsub, ntime]), dmt_sums, dmt_hits (int32 [ndm, ntime])
    and nactive (int32 [nsub])."""
    nchans = values.shape[1]
    kill = np.ones(nchans, bool) if killmask is None else np.asarray(killmask) != 0
    live = [int(c) for c in np.nonzero(kill)[0]]
    subs = [[c for c in live if (c * nsub) // nchans == s] for s in range(nsub)]
    ndm = len(dmt_offsets)
    ds, dh = burst_rows(values, subs, [ds_offsets] * nsub, t0, f, ntime, nvalid)
    ts, th = burst_rows(values, [live] * ndm, dmt_offsets, t0, f, ntime, nvalid)
    assert max(ds.max(initial=0), ts.max(initial=0)) < 2 ** 31
    return {"ds_sums": ds.astype(np.int32), "ds_hits": dh.astype(np.int32), "dmt_sums": ts.astype(np.int32),
            "dmt_hits": th.astype(np.int32), "nactive": np.array([len(s) for s in subs], dtype=np.int32)}


def burst_cube(values: np.ndarray, sample: int, width: int, dm: float, delays: np.ndarray, ntime: int, nsub: int,
               ndm: int, tscrunch: int = 0, dm_half_range: float = 0.0, killmask=None, nvalid: int = None) -> Dict:
    """The cutout of the candidate (sample, width, dm) of values [nsamps,
    nchans] (raw samples): burst_cube_offsets' dict plus tscrunch (the f
    used), t0 and dms (float32 [ndm])."""
    f = burst_tscrunch(width, tscrunch)
    t0 = burst_t0(sample, width, f, ntime)
    dms = burst_dms(dm, ndm, dm_half_range)
    out = burst_cube_offsets(values, dm_offsets([dm], delays)[0], dm_offsets(dms, delays), t0, f, ntime, nsub,
                             killmask, nvalid)
    out.update(tscrunch=f, t0=t0, dms=dms)
    return out


# ------------------------------------------------------------ RFI excision --
# NumPy oracles of csrc/include/psoup/rfi.hpp, written from its definition in
# int64 and float64.
def rfi_rdiv(a, n):
    """floor((2a + n) / (2n)) for a >= 0, n > 0 (integers or int64 arrays)."""
    return (2 * a + n) // (2 * n)


def rfi_block_lengths(nsamps: int, block: int) -> np.ndarray:
    nblk = -(-int(nsamps) // int(block))
    lens = np.full(nblk, int(block), dtype=np.int64)
    lens[-1] = int(nsamps) - (nblk - 1) * int(block)
    return lens


def rfi_block_sums(values: np.ndarray, block: int) -> Tuple[np.ndarray, np.ndarray]:
    """values: raw samples [nchans, nsamps].  Returns (S1, S2) uint64 [nchans, nblk]."""
    x = np.asarray(values).astype(np.int64)
    nchans, nsamps = x.shape
    starts = np.arange(0, nsamps, int(block))
    S1 = np.add.reduceat(x, starts, axis=1)
    S2 = np.add.reduceat(x * x, starts, axis=1)
    return S1.astype(np.uint64), S2.astype(np.uint64)


def _rfi_outliers(x: np.ndarray, thresh: float) -> Tuple[np.ndarray, float]:
    med = float(np.median(x))
    dev = np.abs(x - med)
    mad = float(np.median(dev))
    if mad == 0.0:
        return x != med, med
    return dev > (thresh * 1.4826) * mad, med


def rfi_flag(S1: np.ndarray, S2: np.ndarray, nsamps: int, block: int, killmask=None, thresh: float = 5.0,
             chan_frac: float = 0.3, block_frac: float = 0.3) -> Dict:
    """The host step: dict(chan_flag, block_flag, cell uint8; fill, G, nb int32;
    killmask int list), from the raw block sums [nchans, nblk]."""
    S1 = np.asarray(S1).astype(np.int64)
    S2 = np.asarray(S2).astype(np.int64)
    nchans, nblk = S1.shape
    lens = rfi_block_lengths(nsamps, block)
    assert lens.size == nblk
    live = np.ones(nchans, dtype=bool) if killmask is None or len(killmask) == 0 else np.asarray(killmask) != 0
    mean = S1.astype(np.float64) / lens.astype(np.float64)
    var = (lens * S2 - S1 * S1).astype(np.float64) / (lens * lens).astype(np.float64)
    pre = np.zeros((nchans, nblk), dtype=bool)
    for c in range(nchans):
        if not live[c]:
            pre[c] = True
            continue
        fm, _ = _rfi_outliers(mean[c], thresh)
        fv, med_v = _rfi_outliers(var[c], thresh)
        pre[c] = fm | fv
        if med_v == 0.0:
            pre[c] = True
    chan_flag = ~live
    block_flag = np.zeros(nblk, dtype=bool)
    for c in range(nchans):
        if live[c] and float(pre[c].sum()) / float(nblk) > chan_frac:
            chan_flag[c] = True
    nlive = int(live.sum())
    if nlive:
        for b in range(nblk):
            if float(pre[live, b].sum()) / float(nlive) > block_frac:
                block_flag[b] = True
    cell = pre | chan_flag[:, None] | block_flag[None, :]
    fill = np.zeros(nchans, dtype=np.int64)
    kill = np.ones(nchans, dtype=np.int64)
    for c in range(nchans):
        ok = ~cell[c]
        n = int(lens[ok].sum())
        if n:
            fill[c] = rfi_rdiv(int(S1[c][ok].sum()), n)
        if n == 0 or not live[c]:
            kill[c] = 0
    G = np.zeros(nblk, dtype=np.int64)
    nb = np.zeros(nblk, dtype=np.int64)
    for b in range(nblk):
        ok = ~cell[:, b]
        nb[b] = int(ok.sum())
        if nb[b]:
            G[b] = rfi_rdiv(int(fill[ok].sum()), int(nb[b]))
    return {"chan_flag": chan_flag.astype(np.uint8), "block_flag": block_flag.astype(np.uint8),
            "cell": cell.astype(np.uint8), "fill": fill.astype(np.int32), "G": G.astype(np.int32),
            "nb": nb.astype(np.int32), "killmask": [int(k) for k in kill]}


def rfi_apply(values: np.ndarray, mask: Dict, block: int, nbits: int, zero_dm: bool = False) -> np.ndarray:
    """Step 4 on raw samples [nchans, nsamps]; returns the cleaned raw samples (int64)."""
    x = np.asarray(values).astype(np.int64)
    nchans, nsamps = x.shape
    V = (1 << int(nbits)) - 1
    cell = np.asarray(mask["cell"]) != 0
    fill = np.asarray(mask["fill"]).astype(np.int64)
    G = np.asarray(mask["G"]).astype(np.int64)
    y = x.copy()
    for b in range(cell.shape[1]):
        sl = slice(b * int(block), min(nsamps, (b + 1) * int(block)))
        ok = ~cell[:, b]
        n = int(ok.sum())
        if zero_dm and n:
            Z = x[ok, sl].sum(axis=0)
            zbar = rfi_rdiv(Z, n)
            y[ok, sl] = np.clip(x[ok, sl] - zbar[None, :] + G[b], 0, V)
        y[~ok, sl] = fill[~ok, None]
    return y


def rfi_clean(values: np.ndarray, block: int, nbits: int, killmask=None, thresh: float = 5.0, chan_frac: float = 0.3,
              block_frac: float = 0.3, zero_dm: bool = False) -> Tuple[np.ndarray, Dict]:
    """The whole chain on raw samples [nchans, nsamps]: (cleaned, mask dict)."""
    S1, S2 = rfi_block_sums(values, block)
    mask = rfi_flag(S1, S2, values.shape[1], block, killmask, thresh, chan_frac, block_frac)
    return rfi_apply(values, mask, block, nbits, zero_dm), mask


# --------------------------------------------------------------- cubeopt ----
# NumPy oracle of csrc/include/psoup/cubeopt.hpp, written from its definition.
OPT_MAX_PLANE = 16384


def cube_opt_nwidths(nbins: int) -> int:
    nw, w = 1, 2
    while w <= nbins // 2:
        nw, w = nw + 1, w * 2
    return nw


def cube_opt_prepare(sums, hits, nactive, ndm: int, np_: int, npd: int, k: int = 0,
                     period: float = 1.0, dm: float = 0.0, acc: float = 0.0) -> Dict:
    """Step 1: dict(d int32 [nints, nsub, nbins], mtot, v2 (Python ints), v).
    Raises ValueError naming ``candidate k`` where the definition refuses."""
    sums = np.asarray(sums, dtype=np.int64)
    hits = np.asarray(hits, dtype=np.int64)
    nactive = np.asarray(nactive)
    nints, nsub, nbins = sums.shape
    who = f"cube opt: candidate {k} "
    if hits.shape != (nints, nbins) or nactive.shape != (nsub,):
        raise ValueError(who + "has the wrong shape")
    if (hits <= 0).any():
        raise ValueError(who + "has a phase bin without samples")
    if nints * nbins > OPT_MAX_PLANE:
        raise ValueError(who + f"nints * nbins exceeds {OPT_MAX_PLANE}")
    if ndm * np_ * npd * nbins >= 2 ** 31:
        raise ValueError(who + "the trial bins do not fit 31 bits")
    if not (math.isfinite(period) and period > 0 and math.isfinite(dm) and math.isfinite(acc)):
        raise ValueError(who + "bad period, DM or acceleration")
    href = hits.max(axis=1)
    # exact integers throughout: Python ints in object arrays
    S = sums.astype(object)
    H = hits.astype(object)[:, None, :]
    t = 2 * S * href.astype(object)[:, None, None]
    if max(abs(int(t.max())), abs(int(t.min()))) >= 2 ** 63:
        raise ValueError(who + "2 * sums * Href does not fit 63 bits")
    q = (t + H) // (2 * H)
    B = q.sum(axis=2) // nbins
    d = q - B[:, :, None]
    live = nactive > 0
    d[:, ~live, :] = 0
    maxabs = max(abs(int(d.max())), abs(int(d.min())))
    if maxabs >= 2 ** 31 or int(d.min()) < -2 ** 31:
        raise ValueError(who + "a baseline-subtracted value does not fit int32")
    if maxabs * nints * int(live.sum()) * (nbins // 2) >= 2 ** 31:
        raise ValueError(who + "the box sums do not fit int32")
    mtot = int(d.sum())
    v2 = int((d * d).sum())
    return {"d": d.astype(np.int32), "mtot": mtot, "v2": v2, "v": float(v2) / float(nbins)}


def _opt_reduce(x: float, nbins: int) -> int:
    return int(np.rint(x)) % nbins


def cube_opt_shifts(nints: int, nsub: int, nbins: int, nchans: int, tsamp: float, period: float, dm: float,
                    delays: np.ndarray, ndm: int, np_: int, npd: int, dm_half_range: float = 0.0,
                    p_step: float = 1.0, pd_step: float = 1.0) -> Dict:
    """Step 2: dict(dms float32 [ndm], sdm int32 [ndm, nsub], st int32 [np, npd, nints])."""
    dms = burst_dms(dm, ndm, dm_half_range)
    delays = np.asarray(delays, dtype=np.float32)
    sub_of = (np.arange(nchans, dtype=np.int64) * nsub) // nchans
    tbp = float(np.float32(tsamp)) / float(period)
    dm0 = float(np.float32(dm))
    sdm = np.zeros((ndm, nsub), dtype=np.int32)
    for s in range(nsub):
        ch = np.nonzero(sub_of == s)[0]
        dsub = 0.5 * (float(delays[ch[0]]) + float(delays[ch[-1]]))
        for kd in range(ndm):
            sdm[kd, s] = _opt_reduce((float(dms[kd]) - dm0) * dsub * tbp * nbins, nbins)
    st = np.zeros((np_, npd, nints), dtype=np.int32)
    for kp in range(np_):
        L = (kp - np_ // 2) * float(p_step)
        for kpd in range(npd):
            Q = (kpd - npd // 2) * float(pd_step)
            for i in range(nints):
                u = (i + 0.5) / nints
                st[kp, kpd, i] = _opt_reduce(L * (u - 0.5) + Q * (4.0 * u * (1.0 - u)), nbins)
    return {"dms": dms, "sdm": sdm, "st": st}


def cube_opt_profile(d: np.ndarray, sdm_row: np.ndarray, st_row: np.ndarray) -> np.ndarray:
    """prof int64 [nbins] of one trial."""
    nints, nsub, nbins = d.shape
    b = np.arange(nbins)
    A = np.zeros((nints, nbins), dtype=np.int64)
    for s in range(nsub):
        A += d[:, s, (b + int(sdm_row[s])) % nbins]
    prof = np.zeros(nbins, dtype=np.int64)
    for i in range(nints):
        prof += A[i, (b + int(st_row[i])) % nbins]
    return prof


def cube_opt_search(d: np.ndarray, sdm: np.ndarray, st: np.ndarray) -> Dict:
    """Step 3 from the definition: dict(best_val, best_idx, centre int32 [nw];
    dmcurve int32 [nw, ndm]; ppd int32 [nw, np, npd])."""
    d = np.asarray(d).astype(np.int64)
    sdm, st = np.asarray(sdm), np.asarray(st)
    nints, nsub, nbins = d.shape
    ndm, (np_, npd) = sdm.shape[0], st.shape[:2]
    nw = cube_opt_nwidths(nbins)
    b = np.arange(nbins)
    S = np.zeros((nw, ndm, np_ * npd, nbins), dtype=np.int64)
    rot = (b[None, None, :] + st.reshape(np_ * npd, nints)[:, :, None]) % nbins  # [trial, i, b]
    for kd in range(ndm):
        A = np.zeros((nints, nbins), dtype=np.int64)
        for s in range(nsub):
            A += d[:, s, (b + int(sdm[kd, s])) % nbins]
        prof = np.zeros((np_ * npd, nbins), dtype=np.int64)
        for i in range(nints):
            prof += A[i][rot[:, i, :]]
        box = prof
        for k in range(nw):
            S[k, kd] = box
            box = box + np.roll(box, -(1 << k), axis=1)
    assert np.abs(S).max(initial=0) < 2 ** 31
    flat = S.reshape(nw, -1)
    return {"best_val": flat.max(axis=1).astype(np.int32),
            "best_idx": flat.argmax(axis=1).astype(np.int32),  # the first occurrence
            "dmcurve": S.max(axis=(2, 3)).astype(np.int32),
            "ppd": S.max(axis=(1, 3)).reshape(nw, np_, npd).astype(np.int32),
            "centre": S[:, ndm // 2, (np_ // 2) * npd + npd // 2].max(axis=1).astype(np.int32)}


def cube_opt_snr(s: float, w: int, mtot: int, v: float, nbins: int) -> float:
    if not v > 0:
        return 0.0
    return (float(s) - w * float(mtot) / nbins) / math.sqrt(v * w * (1.0 - float(w) / nbins))


def cube_opt_finish(prep: Dict, shifts: Dict, found: Dict, period: float, acc: float, tsamp: float, fold_nsamps: int,
                    p_step: float = 1.0, pd_step: float = 1.0) -> Dict:
    """Step 4: the record of one candidate (the search outputs included)."""
    d = prep["d"]
    nints, nsub, nbins = d.shape
    ndm = len(shifts["dms"])
    np_, npd = shifts["st"].shape[:2]
    nw = cube_opt_nwidths(nbins)

    def best_of(vals):
        best, which = 0.0, 0
        for k in range(nw):
            s = cube_opt_snr(float(int(vals[k])), 1 << k, prep["mtot"], prep["v"], nbins)
            if k == 0 or s > best:
                best, which = s, k
        return best, which

    snr, kbest = best_of(found["best_val"])
    snr_in, _ = best_of(found["centre"])
    flags = 0
    if float(shifts["dms"][0]) == 0.0:
        snr_dm0, _ = best_of(found["dmcurve"][:, 0])
    else:
        snr_dm0, flags = 0.0, 1
    idx = int(found["best_idx"][kbest])
    opt_bin, t = idx % nbins, idx // nbins
    kpd, kp, kd = t % npd, (t // npd) % np_, t // npd // np_
    L = (kp - np_ // 2) * float(p_step)
    Q = (kpd - npd // 2) * float(pd_step)
    ts = float(np.float32(tsamp))
    n = float(int(fold_nsamps))
    T = n * ts
    out = {k: np.asarray(v).copy() for k, v in found.items()}
    out.update(snr=snr, snr_in=snr_in, snr_dm0=snr_dm0,
               opt_period=1.0 / (1.0 / float(period) - L / (nbins * T)),
               opt_acc=float(np.float32(acc)) - (8.0 * C_LIGHT * Q * float(period)) / (nbins * ts * ts * n * n),
               opt_dm=float(shifts["dms"][kd]), opt_width=1 << kbest, opt_bin=opt_bin, opt_kd=kd, opt_kp=kp,
               opt_kpd=kpd, flags=flags, mtot=prep["mtot"], v=prep["v"], dms=np.asarray(shifts["dms"]).copy(),
               profile=cube_opt_profile(d.astype(np.int64), shifts["sdm"][kd], shifts["st"][kp, kpd]).astype(np.int32))
    return out


def cube_optimise(cand: Dict, header: Dict, delays: np.ndarray, ndm: int = 64, np_: int = 65, npd: int = 33,
                  dm_half_range: float = 0.0, p_step: float = 1.0, pd_step: float = 1.0, k: int = 0) -> Dict:
    """The whole chain on one candidate dict (period, dm, acc, nactive, hits,
    sums) of a fold-cube file with ``header``: cube_opt_finish's record plus
    period, dm, acc."""
    prep = cube_opt_prepare(cand["sums"], cand["hits"], cand["nactive"], ndm, np_, npd, k, float(cand["period"]),
                            float(cand["dm"]), float(cand["acc"]))
    nints, nsub, nbins = prep["d"].shape
    sh = cube_opt_shifts(nints, nsub, nbins, int(header["nchans"]), float(header["tsamp"]), float(cand["period"]),
                         float(cand["dm"]), delays, ndm, np_, npd, dm_half_range, p_step, pd_step)
    found = cube_opt_search(prep["d"], sh["sdm"], sh["st"])
    rec = cube_opt_finish(prep, sh, found, float(cand["period"]), float(cand["acc"]), float(header["tsamp"]),
                          int(header["fold_nsamps"]), p_step, pd_step)
    rec.update(period=float(cand["period"]), dm=float(np.float32(cand["dm"])), acc=float(np.float32(cand["acc"])))
    return rec


# ---------------------------------------------------------------- burstopt --
# The oracle of csrc/include/psoup/burstopt.hpp, written from its definition
# in Python ints, int64 and float64.
def burst_opt_nwidths(ntime: int) -> int:
    nw, w = 1, 2
    while w <= ntime // 2:
        nw, w = nw + 1, w * 2
    return nw


def _bopt_off_pulse(ntime: int) -> np.ndarray:
    k = np.arange(ntime)
    return (k < ntime // 4) | (k >= ntime - ntime // 4)


def _bopt_rows(sums, hits):
    """Step 1 for the rows of one plane, in exact integers: (d, cnt, moff, v2) as object / int arrays."""
    sums = np.asarray(sums, dtype=np.int64)
    hits = np.asarray(hits, dtype=np.int64)
    nrows, ntime = sums.shape
    off = _bopt_off_pulse(ntime)
    d = np.zeros((nrows, ntime), dtype=object)
    cnt = np.zeros(nrows, dtype=np.int64)
    moff = [0] * nrows
    v2 = [0] * nrows
    for r in range(nrows):
        href = int(hits[r].max())
        filled = hits[r] > 0
        sel = filled & off
        if href <= 0 or not sel.any():
            continue
        q = {int(k): (2 * int(sums[r, k]) * href + int(hits[r, k])) // (2 * int(hits[r, k])) for k in np.nonzero(filled)[0]}
        cnt[r] = int(sel.sum())
        base = sum(q[int(k)] for k in np.nonzero(sel)[0]) // int(cnt[r])
        for k, v in q.items():
            d[r, k] = v - base
        moff[r] = sum(int(d[r, k]) for k in np.nonzero(sel)[0])
        v2[r] = sum(int(d[r, k]) ** 2 for k in np.nonzero(sel)[0])
    return d, cnt, moff, v2


def burst_opt_prepare(cand: Dict, k: int = 0) -> Dict:
    """Step 1 on a cutout dict (ds_sums, ds_hits, dmt_sums, dmt_hits; dm and
    tscrunch where present): dict(d_ds int32 [nsub, ntime], d_dmt int32 [ndm,
    ntime], cnt_ds, cnt_dmt int32, moff_ds, moff_dmt, v2_ds, v2_dmt int64, v,
    mbar_ds, mbar_dmt float64 [ndm]).  Raises ValueError naming ``candidate
    k`` where the definition refuses."""
    ds_sums = np.asarray(cand["ds_sums"])
    nsub, ntime = ds_sums.shape
    who = f"burst opt: candidate {k} "
    if ntime < 8:
        raise ValueError(who + f"ntime = {ntime} is below 8")
    dm = float(cand.get("dm", 0.0))
    if not (math.isfinite(dm) and dm >= 0) or int(cand.get("tscrunch", 1)) < 1:
        raise ValueError(who + "bad DM or tscrunch")
    d_ds, cnt_ds, moff_ds, v2_ds = _bopt_rows(ds_sums, cand["ds_hits"])
    nlive = int((cnt_ds > 0).sum())
    if nlive == 0:
        raise ValueError(who + "no waterfall row is live")
    d_dmt, cnt_dmt, moff_dmt, v2_dmt = _bopt_rows(cand["dmt_sums"], cand["dmt_hits"])
    max_ds = max(abs(int(d_ds.max())), abs(int(d_ds.min())))
    max_dmt = max(abs(int(d_dmt.max())), abs(int(d_dmt.min())))
    for d in (d_ds, d_dmt):
        if int(d.max()) > 2 ** 31 - 1 or int(d.min()) < -2 ** 31:
            raise ValueError(who + "a baseline-subtracted value does not fit int32")
    if max_ds * nlive * (ntime // 2) >= 2 ** 31:
        raise ValueError(who + "the waterfall's box sums do not fit int32")
    if max_dmt * (ntime // 2) >= 2 ** 31:
        raise ValueError(who + "the DM-time plane's box sums do not fit int32")
    v = mbar = 0.0
    for s in range(nsub):
        if cnt_ds[s] > 0:
            v = v + float(v2_ds[s]) / float(cnt_ds[s])
            mbar = mbar + float(moff_ds[s]) / float(cnt_ds[s])
    mbar_dmt = np.array([float(moff_dmt[j]) / float(cnt_dmt[j]) if cnt_dmt[j] > 0 else 0.0
                         for j in range(len(cnt_dmt))], dtype=np.float64)
    return {"d_ds": d_ds.astype(np.int32), "d_dmt": d_dmt.astype(np.int32), "cnt_ds": cnt_ds.astype(np.int32),
            "cnt_dmt": cnt_dmt.astype(np.int32), "moff_ds": np.array(moff_ds, dtype=np.int64),
            "moff_dmt": np.array(moff_dmt, dtype=np.int64), "v2_ds": np.array(v2_ds, dtype=np.int64),
            "v2_dmt": np.array(v2_dmt, dtype=np.int64), "v": v, "mbar_ds": mbar, "mbar_dmt": mbar_dmt}


def burst_opt_shifts(ntime: int, nsub: int, nchans: int, dm: float, f: int, dms, delays: np.ndarray, nfine: int = 65,
                     fine_half_range: float = 0.0) -> Dict:
    """Step 2: dict(dmf float32 [nfine], sf int32 [nfine, nsub])."""
    if nfine < 1 or nfine > 257 or nfine % 2 == 0 or not fine_half_range >= 0:
        raise ValueError("burst opt: nfine must be odd and in 1..257, fine_half_range non-negative")
    dms = np.asarray(dms, dtype=np.float32)
    ndm = len(dms)
    half = float(fine_half_range)
    if not half > 0:
        half = 0.0 if ndm == 1 else float(dms[ndm // 2]) - float(dms[ndm // 2 - 1])
    step = 0.0 if nfine == 1 else half / (nfine // 2)
    dm0 = float(np.float32(dm))
    dmf = np.array([max(0.0, dm0 + (kf - nfine // 2) * step) for kf in range(nfine)]).astype(np.float32)
    delays = np.asarray(delays, dtype=np.float32)
    sub_of = (np.arange(nchans, dtype=np.int64) * nsub) // nchans
    sf = np.zeros((nfine, nsub), dtype=np.int32)
    for s in range(nsub):
        ch = np.nonzero(sub_of == s)[0]
        dsub = 0.5 * (float(delays[ch[0]]) + float(delays[ch[-1]]))
        for kf in range(nfine):
            x = (float(dmf[kf]) - dm0) * dsub / float(int(f))
            sf[kf, s] = int(min(max(np.rint(x), -float(ntime)), float(ntime)))
    return {"dmf": dmf, "sf": sf}


def burst_opt_profile(d_ds: np.ndarray, sf_row: np.ndarray) -> np.ndarray:
    """P int64 [ntime] of one fine row: terms outside the window are 0."""
    d_ds = np.asarray(d_ds).astype(np.int64)
    nsub, ntime = d_ds.shape
    k = np.arange(ntime)
    prof = np.zeros(ntime, dtype=np.int64)
    for s in range(nsub):
        x = k + int(sf_row[s])
        ok = (x >= 0) & (x < ntime)
        prof[ok] += d_ds[s, x[ok]]
    return prof


def burst_opt_search(d_ds: np.ndarray, d_dmt: np.ndarray, sf: np.ndarray) -> Dict:
    """Step 3 from the definition: dict(best_val, best_idx int32 [2, nw] (the
    coarse plane first); curve, curve_bin int32 [nw, ndm + nfine])."""
    d_dmt = np.asarray(d_dmt).astype(np.int64)
    sf = np.asarray(sf)
    ndm, ntime = d_dmt.shape
    nfine = sf.shape[0]
    nw = burst_opt_nwidths(ntime)
    P = np.concatenate([d_dmt, np.stack([burst_opt_profile(d_ds, sf[kf]) for kf in range(nfine)])], axis=0)
    lowest = -2 ** 62
    csum = np.concatenate([np.zeros((P.shape[0], 1), dtype=np.int64), np.cumsum(P, axis=1)], axis=1)
    curve = np.zeros((nw, ndm + nfine), dtype=np.int64)
    curve_bin = np.zeros((nw, ndm + nfine), dtype=np.int64)
    best_val = np.zeros((2, nw), dtype=np.int64)
    best_idx = np.zeros((2, nw), dtype=np.int64)
    for kw in range(nw):
        w = 1 << kw
        S = np.full((ndm + nfine, ntime), lowest, dtype=np.int64)
        S[:, :ntime - w + 1] = csum[:, w:] - csum[:, :ntime - w + 1]
        assert np.abs(S[:, :ntime - w + 1]).max(initial=0) < 2 ** 31
        curve[kw] = S.max(axis=1)
        curve_bin[kw] = S.argmax(axis=1)  # the first occurrence
        for plane, rows in ((0, slice(0, ndm)), (1, slice(ndm, ndm + nfine))):
            flat = S[rows].reshape(-1)
            best_val[plane, kw] = flat.max()
            best_idx[plane, kw] = int(flat.argmax())
    return {"best_val": best_val.astype(np.int32), "best_idx": best_idx.astype(np.int32),
            "curve": curve.astype(np.int32), "curve_bin": curve_bin.astype(np.int32)}


def burst_opt_snr(s: float, w: int, mbar: float, v: float) -> float:
    if not v > 0:
        return 0.0
    return (float(s) - w * float(mbar)) / math.sqrt(v * w)


def burst_opt_finish(cand: Dict, prep: Dict, shifts: Dict, found: Dict) -> Dict:
    """Step 4: the record of one candidate (the search outputs included).
    ``cand`` needs tscrunch, t0 and dms."""
    d_ds = np.asarray(prep["d_ds"]).astype(np.int64)
    nsub, ntime = d_ds.shape
    dms = np.asarray(cand["dms"], dtype=np.float32)
    ndm = len(dms)
    nw = burst_opt_nwidths(ntime)
    f, t0 = int(cand["tscrunch"]), int(cand["t0"])
    v = prep["v"]

    def best_of(vals, mbars):
        best, which = 0.0, 0
        for k in range(nw):
            s = burst_opt_snr(float(int(vals[k])), 1 << k, float(mbars[k]), v)
            if k == 0 or s > best:
                best, which = s, k
        return best, which

    bv, bi = np.asarray(found["best_val"]), np.asarray(found["best_idx"])
    curve = np.asarray(found["curve"])
    snr_coarse, kc = best_of(bv[0], [prep["mbar_dmt"][int(bi[0, k]) // ntime] for k in range(nw)])
    coarse_row, coarse_bin = int(bi[0, kc]) // ntime, int(bi[0, kc]) % ntime
    snr_in, _ = best_of(curve[:, ndm // 2], [prep["mbar_dmt"][ndm // 2]] * nw)
    flags = 0
    if float(dms[0]) == 0.0:
        snr_dm0, _ = best_of(curve[:, 0], [prep["mbar_dmt"][0]] * nw)
    else:
        snr_dm0, flags = 0.0, 1
    snr, kb = best_of(bv[1], [prep["mbar_ds"]] * nw)
    w = 1 << kb
    opt_kf, opt_bin = int(bi[1, kb]) // ntime, int(bi[1, kb]) % ntime
    sf = np.asarray(shifts["sf"])[opt_kf]
    band = np.zeros(nsub, dtype=np.int64)
    nlive = npos = 0
    for s in range(nsub):
        if prep["cnt_ds"][s] == 0:
            continue
        x = opt_bin + np.arange(w) + int(sf[s])
        ok = (x >= 0) & (x < ntime)
        band[s] = int(d_ds[s, x[ok]].sum())
        nlive += 1
        if float(int(band[s])) - w * (float(int(prep["moff_ds"][s])) / float(int(prep["cnt_ds"][s]))) > 0:
            npos += 1
    out = {k: np.asarray(a).copy() for k, a in found.items()}
    out.update(snr=snr, snr_coarse=snr_coarse, snr_in=snr_in, snr_dm0=snr_dm0,
               frac_pos=float(npos) / float(nlive) if nlive else 0.0, v=v, mbar_ds=prep["mbar_ds"],
               opt_sample=t0 + opt_bin * f, opt_dm=float(shifts["dmf"][opt_kf]), coarse_dm=float(dms[coarse_row]),
               opt_width=w * f, opt_kf=opt_kf, opt_bin=opt_bin, coarse_row=coarse_row, coarse_width=(1 << kc) * f,
               coarse_bin=coarse_bin, flags=flags, dms=dms.copy(), dmf=np.asarray(shifts["dmf"]).copy(),
               mbar_dmt=np.asarray(prep["mbar_dmt"], dtype=np.float64).copy(), band=band.astype(np.int32),
               profile=burst_opt_profile(d_ds, sf).astype(np.int32))
    return out


def burst_optimise(cand: Dict, header: Dict, delays: np.ndarray, nfine: int = 65, fine_half_range: float = 0.0,
                   k: int = 0) -> Dict:
    """The whole chain on one cutout dict (``BurstCubeFile.candidate``'s keys,
    or reference.burst_cube's plus sample, width, dm) of a burst-cutout file
    with ``header`` (nchans): burst_opt_finish's record plus sample, width,
    tscrunch, t0, dm and cand_snr."""
    prep = burst_opt_prepare(cand, k)
    nsub, ntime = prep["d_ds"].shape
    sh = burst_opt_shifts(ntime, nsub, int(header["nchans"]), float(cand["dm"]), int(cand["tscrunch"]), cand["dms"],
                          delays, nfine, fine_half_range)
    found = burst_opt_search(prep["d_ds"], prep["d_dmt"], sh["sf"])
    rec = burst_opt_finish(cand, prep, sh, found)
    rec.update(sample=int(cand["sample"]), width=int(cand["width"]), tscrunch=int(cand["tscrunch"]),
               t0=int(cand["t0"]), dm=float(np.float32(cand["dm"])), cand_snr=float(np.float32(cand.get("snr", 0.0))))
    return rec


# -------------------------------------------------------------- filscrunch --
# The oracle of csrc/include/psoup/scrunch.hpp, written from its definition.
SCRUNCH_BLOCK = 4096


def scrunch_offsets(dm: float, delays: np.ndarray, nsub: int) -> Tuple[np.ndarray, int]:
    """Step 1: (rel int32 [nchans], R)."""
    nchans = len(delays)
    if nsub < 1 or nchans % nsub:
        raise ValueError("nsub must divide nchans")
    w = nchans // nsub
    off = dm_offsets([dm], np.asarray(delays, dtype=np.float32))[0].astype(np.int64)
    rel = off - off[np.arange(nchans) // w * w]
    if (rel < 0).any():
        raise ValueError("a channel leads its subband's first channel (foff must be < 0)")
    return rel.astype(np.int32), int(rel.max())


def scrunch_nout(nsamps: int, R: int, f: int) -> int:
    return (nsamps - R) // f if nsamps > R else 0


def scrunch_sums(values: np.ndarray, rel: np.ndarray, f: int, nsub: int, killmask=None, nvalid: int = None):
    """Steps 2 and 3 on raw ``values`` [nsamps, nchans] (the first ``nvalid``
    samples are valid, default all): A int64 [nsub, nout], nactive int32
    [nsub], S1 and S2 uint64 [nsub, nblk]."""
    nsamps, nchans = values.shape
    nsamps = nsamps if nvalid is None else int(nvalid)
    w = nchans // nsub
    kill = np.ones(nchans, bool) if killmask is None else np.asarray(killmask) != 0
    nout = scrunch_nout(nsamps, int(np.max(rel)), f)
    if nout < 1:
        raise ValueError("nout < 1")
    A = np.zeros((nsub, nout), dtype=np.int64)
    nactive = np.zeros(nsub, dtype=np.int32)
    for c in np.nonzero(kill)[0]:
        r = int(rel[c])
        A[c // w] += values[r:r + f * nout, c].astype(np.int64).reshape(nout, f).sum(axis=1)
        nactive[c // w] += 1
    S1, S2 = scrunch_block_sums(A)
    return A, nactive, S1, S2


def scrunch_block_sums(A: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    nsub, nout = A.shape
    nblk = -(-nout // SCRUNCH_BLOCK)
    S1 = np.zeros((nsub, nblk), dtype=np.uint64)
    S2 = np.zeros((nsub, nblk), dtype=np.uint64)
    a = A.astype(np.uint64)
    for b in range(nblk):
        seg = a[:, b * SCRUNCH_BLOCK:(b + 1) * SCRUNCH_BLOCK]
        S1[:, b] = seg.sum(axis=1, dtype=np.uint64)
        S2[:, b] = (seg * seg).sum(axis=1, dtype=np.uint64)
    return S1, S2


def _median(v: List[float]) -> float:
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def scrunch_scale(S1: np.ndarray, S2: np.ndarray, nout: int, nactive, sigma_out: float = 16.0) -> Dict:
    """Step 4: Python ints for the numerator, float64 otherwise."""
    nsub, nblk = S1.shape
    if nblk != -(-nout // SCRUNCH_BLOCK):
        raise ValueError("S1 / S2 must be [nsub, ceil(nout / L)]")
    lens = [SCRUNCH_BLOCK] * (nblk - 1) + [nout - (nblk - 1) * SCRUNCH_BLOCK]
    M = np.zeros(nsub, dtype=np.int32)
    live = np.zeros(nsub, dtype=np.uint8)
    sig = []
    for s in range(nsub):
        m, v = [], []
        for b, n in enumerate(lens):
            s1, s2 = int(S1[s, b]), int(S2[s, b])
            m.append(float(s1) / float(n))
            v.append(float(n * s2 - s1 * s1) / float(n * n))
        med_m, med_v = _median(m), _median(v)
        M[s] = math.floor(med_m + 0.5)
        if int(nactive[s]) > 0 and med_v > 0:
            live[s] = 1
            sig.append(math.sqrt(med_v))
    if not sig:
        raise ValueError("no live subband")
    sigma_ref = _median(sig)
    t = sigma_out / sigma_ref * 65536.0 + 0.5
    mul = 2 ** 31 - 1 if not t < 2.0 ** 31 else (1 if t < 1.0 else math.floor(t))
    return {"M": M, "live": live, "mul": int(mul), "sigma_ref": sigma_ref, "nlive": len(sig)}


def scrunch_quant(A: np.ndarray, M, mul: int, live) -> np.ndarray:
    """Step 5: uint8 [nsub, nout]."""
    d = ((np.asarray(A, dtype=np.int64) - np.asarray(M, dtype=np.int64)[:, None]) * int(mul) + 32768) >> 16
    y = np.clip(d + 128, 0, 255).astype(np.uint8)
    y[np.asarray(live) == 0] = 128
    return y


def scrunch_plan(tsamp: float, fch1: float, foff: float, nchans: int, dm_end: float) -> List[Tuple[float, float, int]]:
    """Step 7: (dm_lo, dm_hi, tscrunch) per tier over [0, dm_end]."""
    nu = min(fch1, fch1 + float(nchans - 1) * foff) / 1000.0
    unit = tsamp * (nu * nu * nu) / (8.3e-6 * abs(foff))
    tiers = []
    for k in range(7):
        lo = 0.0 if k == 0 else float(1 << k) * unit
        if k > 0 and not lo < dm_end:
            break
        nxt = float(2 << k) * unit
        tiers.append((lo, dm_end if (k == 6 or not nxt < dm_end) else nxt, 1 << k))
    return tiers


def scrunch_header(hdr: Dict, nsub: int, f: int, dm: float, nout: int) -> Dict:
    """Step 6: the output's header dict from the input's (a parsed header)."""
    out = dict(hdr)
    w = int(hdr["nchans"]) // nsub
    out.update(nchans=nsub, foff=float(w) * float(hdr["foff"]), tsamp=float(f) * float(hdr["tsamp"]), nbits=8,
               nsamples=nout if "nsamples" in hdr.get("_present", ()) else 0, refdm=float(np.float32(dm)))
    return out


def scrunch_filterbank(infile: str, outfile: str, dm: float = 0.0, nsub: int = 0, f: int = 1,
                       sigma_out: float = 16.0, killmask=None, kill_out: str = None) -> Dict:
    """The whole tool on the CPU: reads ``infile``, writes ``outfile`` (and the
    subband killfile ``kill_out``); returns the scale dict plus A, y, nout,
    rel and nactive."""
    import os

    from .sigproc import header_bytes, read_filterbank

    fb = read_filterbank(infile)
    hdr = fb.header
    nchans = int(hdr["nchans"])
    nsub = nsub or nchans
    if hdr["foff"] >= 0:
        raise ValueError("foff must be negative")
    if not 1 <= f <= 256 or nchans % nsub or not sigma_out > 0 or dm < 0:
        raise ValueError("bad scrunch parameters")
    delays = delay_table(nchans, hdr["tsamp"], hdr["fch1"], hdr["foff"])
    rel, R = scrunch_offsets(dm, delays, nsub)
    A, nactive, S1, S2 = scrunch_sums(fb.data, rel, f, nsub, killmask)
    V = (1 << int(hdr["nbits"])) - 1
    if V * f * int(nactive.max()) >= 1 << 26:
        raise ValueError("2^26 bound")
    nout = A.shape[1]
    sc = scrunch_scale(S1, S2, nout, nactive, sigma_out)
    y = scrunch_quant(A, sc["M"], sc["mul"], sc["live"])
    tmp = outfile + ".tmp"
    with open(tmp, "wb") as fo:
        fo.write(header_bytes(scrunch_header(hdr, nsub, f, dm, nout), keep_present=True))
        fo.write(np.ascontiguousarray(y.T).tobytes())
    os.replace(tmp, outfile)
    if kill_out:
        with open(kill_out, "w") as fo:
            fo.write("".join("1\n" if v else "0\n" for v in sc["live"]))
    return dict(sc, A=A, y=y, nout=nout, rel=rel, R=R, nactive=nactive, S1=S1, S2=S2)


# ----------------------------------------------------------------- fildigi --
# The oracle of csrc/include/psoup/digi.hpp, written from its definition.
DIGI_BLOCK = 4096


def digi_quantum(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Step 1 on one statistics block ``x`` [len, nchans]: (E int32 [nchans],
    q int64 [len, nchans]; q is 0 at the non-finite samples of float input)."""
    x = np.asarray(x)
    nchans = x.shape[1]
    if x.dtype != np.float32:
        return np.zeros(nchans, np.int32), x.astype(np.int64)
    bits = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    fin = (bits & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    amax = np.where(fin, bits, np.uint32(0)).max(axis=0)
    e = np.maximum((amax >> np.uint32(23)).astype(np.int32), 1)
    E = np.where(amax == 0, 0, e - 127 - 22).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(np.ldexp(np.where(fin, x, np.float32(0)).astype(np.float64), -E[None, :]))
    return E, q.astype(np.int64)


def digi_block_sums(x: np.ndarray) -> Dict:
    """Steps 1 and 2 on samples ``x`` [nsamps, nchans] (uint8, int8, uint16 or
    float32): N uint32, S1 int64, S2 uint64, E int32, all [nchans, nblk], and
    nbad uint64 [nchans]."""
    x = np.asarray(x)
    nsamps, nchans = x.shape
    nblk = -(-nsamps // DIGI_BLOCK)
    N = np.zeros((nchans, nblk), np.uint32)
    S1 = np.zeros((nchans, nblk), np.int64)
    S2 = np.zeros((nchans, nblk), np.uint64)
    E = np.zeros((nchans, nblk), np.int32)
    for b in range(nblk):
        seg = x[b * DIGI_BLOCK:(b + 1) * DIGI_BLOCK]
        fin = np.isfinite(seg) if seg.dtype == np.float32 else np.ones(seg.shape, bool)
        E[:, b], q = digi_quantum(seg)
        N[:, b] = fin.sum(axis=0)
        S1[:, b] = q.sum(axis=0)
        S2[:, b] = (q * q).astype(np.uint64).sum(axis=0, dtype=np.uint64)
    nbad = (nsamps - N.astype(np.int64).sum(axis=1)).astype(np.uint64)
    return {"N": N, "S1": S1, "S2": S2, "E": E, "nbad": nbad}


def digi_nint(nblk: int, J: int) -> int:
    return -(-nblk // J) if J > 0 else 1


def digi_scale(N, S1, S2, E, killmask=None, sigma_out: float = 16.0, scale: str = "channel", J: int = 0) -> Dict:
    """Steps 3 and 4: Python ints for the numerator, float64 otherwise,
    ``numpy.median`` for the medians.  mean, gain float64 and live uint8, all
    [nint, nchans] (gain and mean 0 where not live); alive [nchans]."""
    if not sigma_out > 0 or J < 0 or scale not in ("channel", "file"):
        raise ValueError("bad digi parameters")
    nchans, nblk = N.shape
    nint = digi_nint(nblk, J)
    per = J if J > 0 else nblk
    kill = np.ones(nchans, bool) if killmask is None or len(killmask) == 0 else np.asarray(killmask) != 0
    mean = np.zeros((nint, nchans))
    gain = np.zeros((nint, nchans))
    sig = np.zeros((nint, nchans))
    live = np.zeros((nint, nchans), np.uint8)
    for c in range(nchans):
        for j in range(nint):
            m, v = [], []
            for b in range(j * per, min(nblk, (j + 1) * per)):
                n, s1, s2, e = int(N[c, b]), int(S1[c, b]), int(S2[c, b]), int(E[c, b])
                if n == 0:
                    continue
                m.append(math.ldexp(float(s1) / float(n), e))
                v.append(math.ldexp(float(n * s2 - s1 * s1) / float(n * n), 2 * e))
            if not m:
                continue
            med_m, med_v = float(np.median(np.array(m))), float(np.median(np.array(v)))
            if kill[c] and med_v > 0:
                live[j, c] = 1
                mean[j, c] = med_m
                sig[j, c] = math.sqrt(med_v)
    if not live.any():
        raise ValueError("no live channel")
    for j in range(nint):
        on = live[j] != 0
        if scale == "file":
            if on.any():
                gain[j, on] = sigma_out / float(np.median(sig[j, on]))
        else:
            gain[j, on] = sigma_out / sig[j, on]
    alive = live.any(axis=0).astype(np.int64)
    g = gain[live != 0]
    return {"nint": nint, "mean": mean, "gain": gain, "live": live, "alive": alive, "nlive": int(alive.sum()),
            "gain_min": float(g.min()), "gain_max": float(g.max())}


def digi_quant(x: np.ndarray, mean, gain, J: int = 0, flip: bool = False) -> Tuple[np.ndarray, int]:
    """Steps 5 and 6: (y uint8 [nsamps, nchans] in output order, nclip).
    mean, gain [nint, nchans] in input channel order, gain 0 = not live."""
    x = np.asarray(x)
    nsamps, nchans = x.shape
    mean = np.asarray(mean, np.float64).reshape(-1, nchans)
    gain = np.asarray(gain, np.float64).reshape(-1, nchans)
    blk = np.arange(nsamps) // DIGI_BLOCK
    j = blk // J if J > 0 else np.zeros(nsamps, np.int64)
    good = (np.isfinite(x) if x.dtype == np.float32 else np.ones(x.shape, bool)) & (gain[j] != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((np.where(good, x, 0).astype(np.float64) - mean[j]) * gain[j]) + 128.0
    r = np.where(good, r, 128.0)
    nclip = int(((r < 0) | (r > 255)).sum())
    y = np.clip(r, 0, 255).astype(np.uint8)
    return (y[:, ::-1] if flip else y), nclip


def digi_band(fch1: float, foff: float, nchans: int) -> Tuple[bool, float, float]:
    """Step 6: (flip, fch1', foff')."""
    if foff > 0:
        return True, fch1 + float(nchans - 1) * foff, -foff
    return False, fch1, foff


def digi_header(hdr: Dict, nsamps: int) -> Dict:
    """Step 7: the output's header dict from the input's (a parsed header)."""
    out = dict(hdr)
    _, fch1, foff = digi_band(float(hdr["fch1"]), float(hdr["foff"]), int(hdr["nchans"]))
    present = [k for k in hdr.get("_present", ()) if k != "signed"]
    out.update(nbits=8, signed=0, fch1=fch1, foff=foff, nsamples=nsamps if "nsamples" in present else 0)
    out["_present"] = present
    return out


def digi_filterbank(infile: str, outfile: str, sigma_out: float = 16.0, scale: str = "channel", J: int = 0,
                    killmask=None, kill_out: str = None) -> Dict:
    """The whole tool on the CPU: reads ``infile``, writes ``outfile`` (and the
    killfile ``kill_out`` in output channel order); returns the block tables,
    the scale dict, y, nclip, flip and killmask."""
    import os

    from .sigproc import header_bytes, read_raw_filterbank

    hdr, x = read_raw_filterbank(infile)
    nsamps, nchans = x.shape
    if nsamps < 1:
        raise ValueError("shorter than one sample")
    sums = digi_block_sums(x)
    sc = digi_scale(sums["N"], sums["S1"], sums["S2"], sums["E"], killmask, sigma_out, scale, J)
    flip = digi_band(float(hdr["fch1"]), float(hdr["foff"]), nchans)[0]
    y, nclip = digi_quant(x, sc["mean"], sc["gain"], J, flip)
    kill = sc["alive"][::-1] if flip else sc["alive"]
    tmp = outfile + ".tmp"
    with open(tmp, "wb") as fo:
        fo.write(header_bytes(digi_header(hdr, nsamps), keep_present=True))
        fo.write(np.ascontiguousarray(y).tobytes())
    os.replace(tmp, outfile)
    if kill_out:
        with open(kill_out, "w") as fo:
            fo.write("".join("1\n" if v else "0\n" for v in kill))
    return dict(sums, **sc, y=y, nclip=nclip, flip=flip, killmask=[int(v) for v in kill])


# ---------------------------------------------------------------- fits2fil --
# The oracle of csrc/include/psoup/psrfits.hpp, written from its definition.
FITS_NAN = np.uint32(0x7FC00000)
FITS_TELESCOPES = {"ARECIBO": 1, "OOTY": 2, "NANCAY": 3, "PARKES": 4, "JODRELL": 5, "GBT": 6, "GMRT": 7,
                   "EFFELSBERG": 8, "LOFAR": 11, "VLA": 12, "MEERKAT": 64}


def fits_pols(npol: int, pol_type: str, pol: int = -1) -> Tuple[int, int]:
    """(a, b) with b = -1 when one polarisation is taken; ``pol`` -1 = auto."""
    if pol >= 0:
        if pol >= npol:
            raise ValueError(f"fits: --pol {pol} is not below NPOL = {npol}")
        return pol, -1
    if npol == 1:
        return 0, -1
    t = pol_type.strip().upper()
    if t.startswith("AABB"):
        return 0, 1
    if t == "IQUV":
        return 0, -1
    raise ValueError(f"fits: POL_TYPE '{pol_type}' with NPOL = {npol} needs --pol P")


def fits_row_slots(offs_sub, nrows: int, nsblk: int, tbin: float) -> Dict:
    """Rows and time: slot [nrows], slot_row [nslots] (-1 = dropped), nslots,
    nsamps, ndropped, offs_sub0 (as tstart takes it)."""
    half = (0.5 * nsblk) * tbin
    if offs_sub is None or not np.any(np.asarray(offs_sub) != 0):
        slot = np.arange(nrows, dtype=np.int64)
        o0 = half
    else:
        o = np.asarray(offs_sub, np.float64)
        if not np.isfinite(o).all():
            raise ValueError("fits: OFFS_SUB is not finite")
        q = (o - o[0]) / (float(nsblk) * tbin)
        k = np.rint(q)
        if (np.abs(q - k) > 1e-3).any():
            raise ValueError("fits: a row does not start on a whole row")
        slot = k.astype(np.int64)
        if slot[0] != 0 or (np.diff(slot) <= 0).any():
            raise ValueError("fits: the row slots do not increase strictly")
        o0 = float(o[0]) if o[0] != 0 else half
    nslots = int(slot[-1]) + 1
    if nslots > 2 * nrows:
        raise ValueError("fits: more than half the rows are dropped")
    if nslots * nsblk >= 1 << 31:
        raise ValueError("fits: too many samples for a SIGPROC header")
    slot_row = np.full(nslots, -1, np.int32)
    slot_row[slot] = np.arange(nrows, dtype=np.int32)
    return {"slot": slot, "slot_row": slot_row, "nslots": nslots, "nsamps": nslots * nsblk,
            "ndropped": nslots - nrows, "offs_sub0": o0}


def fits_band(freq, chan_bw: float = 0.0) -> Tuple[float, float]:
    """(fch1, foff) of the first row's DAT_FREQ (float64 [nchan])."""
    f = np.asarray(freq, np.float64)
    n = len(f)
    fch1 = float(f[0])
    foff = float(chan_bw) if n == 1 else float((f[n - 1] - f[0]) / float(n - 1))
    if not (math.isfinite(fch1) and math.isfinite(foff)) or foff == 0:
        raise ValueError("fits: foff must not be zero")
    if (np.abs(f - (fch1 + np.arange(n, dtype=np.float64) * foff)) > 0.01 * abs(foff)).any():
        raise ValueError("fits: DAT_FREQ is not evenly spaced")
    return fch1, foff


def fits_sexagesimal(text: str) -> float:
    s = text.strip()
    neg = s.startswith("-")
    if s[:1] in ("+", "-"):
        s = s[1:]
    parts = s.split(":", 2)
    if len(parts) != 3:
        return 0.0
    try:
        h, m, sec = int(parts[0]), int(parts[1]), float(parts[2].strip().replace("D", "E").replace("d", "E"))
    except ValueError:
        return 0.0
    if h < 0 or m < 0 or not sec >= 0 or not math.isfinite(sec):
        return 0.0
    v = (float(h) * 10000.0 + float(m) * 100.0) + sec
    return -v if neg else v


def fits_decode(raw: np.ndarray, scl, offs, wts, slot_row, pols, z: float = 0.0, t0: int = 0,
                count: Optional[int] = None) -> np.ndarray:
    """The decode of the definition.  raw: integer samples [nrows, nsblk, npol,
    nchan]; scl, offs float32 [nrows, npol, nchan]; wts float32 [nrows, nchan];
    slot_row [nslots] (file row or -1).  Float64 steps as defined and one
    rounding to float32; returns x float32 [count, nchan] of samples [t0, t0 +
    count) with the quiet NaN 0x7fc00000 for a dropped slot, a zero weight and
    a NaN result."""
    raw = np.asarray(raw)
    nrows, nsblk, npol, nchan = raw.shape
    slot_row = np.asarray(slot_row)
    nsamps = len(slot_row) * nsblk
    count = nsamps - t0 if count is None else count
    scl = np.asarray(scl, np.float32).astype(np.float64)
    offs = np.asarray(offs, np.float32).astype(np.float64)
    wts32 = np.asarray(wts, np.float32)
    zd = float(np.float32(z))
    out = np.full((nsamps, nchan), FITS_NAN, np.uint32)
    a, b = pols
    with np.errstate(all="ignore"):
        for k, r in enumerate(slot_row):
            if r < 0:
                continue
            u = (raw[r, :, a, :].astype(np.float64) - zd) * scl[r, a][None, :] + offs[r, a][None, :]
            if b >= 0:
                ub = (raw[r, :, b, :].astype(np.float64) - zd) * scl[r, b][None, :] + offs[r, b][None, :]
                u = u + ub
            v = u * wts32[r].astype(np.float64)[None, :]
            x = v.astype(np.float32).view(np.uint32)
            x = np.where(np.isnan(v) | (wts32[r] == 0)[None, :], FITS_NAN, x)
            out[k * nsblk:(k + 1) * nsblk] = x
    return np.ascontiguousarray(out[t0:t0 + count]).view(np.float32)


def fits_header(f: Dict, slots: Dict, band, telescope_id: int = -1, machine_id: int = 0, rawdatafile: str = "") -> Dict:
    """The output's header dict from a ``read_psrfits`` dict."""
    p = f["primary"]
    fch1, foff = band
    _, fch1, foff = digi_band(fch1, foff, f["nchan"])
    half = (0.5 * f["nsblk"]) * f["tbin"]

    def num(key):
        return float(p[key].strip().replace("D", "E").replace("d", "E"))

    secs = ((num("STT_SMJD") + num("STT_OFFS")) + slots["offs_sub0"]) - half
    tel = telescope_id if telescope_id >= 0 else FITS_TELESCOPES.get(p.get("TELESCOP", "").strip().upper(), 0)
    hdr = {"source_name": p.get("SRC_NAME", "").strip(), "rawdatafile": rawdatafile, "telescope_id": tel,
           "machine_id": machine_id, "data_type": 1, "src_raj": fits_sexagesimal(p.get("RA", "")),
           "src_dej": fits_sexagesimal(p.get("DEC", "")), "tstart": float(int(p["STT_IMJD"])) + secs / 86400.0,
           "tsamp": f["tbin"], "fch1": fch1, "foff": foff, "nchans": f["nchan"], "nbits": 8, "nifs": 1,
           "nsamples": slots["nsamps"], "barycentric": 0}
    present = ["telescope_id", "machine_id", "barycentric", "src_raj", "src_dej", "tstart", "nsamples"]
    try:
        hdr["ibeam"] = int(p["BEAM_ID"].strip())
        present.append("ibeam")
    except (KeyError, ValueError):
        pass
    hdr["_present"] = present
    return hdr


def fits_filterbank(infile, outfile: Optional[str] = None, sigma_out: float = 16.0, scale: str = "channel", J: int = 0,
                    killmask=None, kill_out: Optional[str] = None, pol: int = -1, no_scales: bool = False,
                    no_offsets: bool = False, no_weights: bool = False, telescope_id: int = -1, machine_id: int = 0,
                    rawdatafile: Optional[str] = None) -> Dict:
    """The whole tool on the CPU: reads ``infile`` (a path or the file's
    bytes), writes ``outfile`` (and the killfile ``kill_out`` in output channel
    order) when given; returns x, the block tables, the scale dict, y, nclip,
    flip, killmask, the header dict and its bytes."""
    import os

    from .psrfits import read_psrfits, unpack_samples
    from .sigproc import header_bytes

    f = read_psrfits(infile)
    nrows, nsblk, npol, nchan = f["nrows"], f["nsblk"], f["npol"], f["nchan"]
    slots = fits_row_slots(f["OFFS_SUB"], nrows, nsblk, f["tbin"])
    band = fits_band(f["DAT_FREQ"][0], f["chan_bw"])
    pols = fits_pols(npol, f["pol_type"], pol)
    if not sigma_out > 0 or J < 0 or scale not in ("channel", "file"):
        raise ValueError("bad digi parameters")
    raw = unpack_samples(f["DATA"], f["nbits"], bool(f["signint"])).reshape(nrows, nsblk, npol, nchan)
    scl = np.ones_like(f["DAT_SCL"]) if no_scales else f["DAT_SCL"]
    offs = np.zeros_like(f["DAT_OFFS"]) if no_offsets else f["DAT_OFFS"]
    wts = np.ones_like(f["DAT_WTS"]) if no_weights else f["DAT_WTS"]
    kill = np.ones(nchan, np.int64) if killmask is None or len(killmask) == 0 else (np.asarray(killmask) != 0).astype(np.int64)
    if len(kill) != nchan:
        raise ValueError("fits: killmask size != NCHAN")
    kill = kill * (wts != 0).any(axis=0)
    if not kill.any():
        raise ValueError("fits: no live channel")
    if rawdatafile is None:
        rawdatafile = os.path.basename(infile) if isinstance(infile, str) else ""
    hdr = fits_header(f, slots, band, telescope_id, machine_id, rawdatafile)
    x = fits_decode(raw, scl, offs, wts, slots["slot_row"], pols, f["z"])
    sums = digi_block_sums(x)
    sc = digi_scale(sums["N"], sums["S1"], sums["S2"], sums["E"], kill, sigma_out, scale, J)
    flip = band[1] > 0
    y, nclip = digi_quant(x, sc["mean"], sc["gain"], J, flip)
    alive = sc["alive"][::-1] if flip else sc["alive"]
    head = header_bytes(hdr, keep_present=True)
    if outfile:
        tmp = outfile + ".tmp"
        with open(tmp, "wb") as fo:
            fo.write(head)
            fo.write(np.ascontiguousarray(y).tobytes())
        os.replace(tmp, outfile)
    if kill_out:
        with open(kill_out, "w") as fo:
            fo.write("".join("1\n" if v else "0\n" for v in alive))
    return dict(sums, **sc, x=x, y=y, nclip=nclip, flip=flip, killmask=[int(v) for v in alive], header=hdr,
                header_bytes=head, slots=slots, pols=pols, z=f["z"], rows=nrows)


# --------------------------------------------------------------- filinject --
# The oracle of csrc/include/psoup/inject.hpp, written from its definition:
# uint64 / float64 NumPy, one correctly rounded operation at a time.
INJECT_BLOCK = 4096
INJECT_STEPS = 256
INJECT_TABLE_LEN = 6 * INJECT_STEPS + 1
INJECT_MAX_SIGNALS = 64
_INJ_GOLDEN = 0x9E3779B97F4A7C15
_INJ_M1 = 0xBF58476D1CE4E5B9
_INJ_M2 = 0x94D049BB133111EB
_INJ_MASK = (1 << 64) - 1


def inject_hash(seed: int, c: int, t: int) -> int:
    """The dither's 64-bit draw z of sample (c, t), in Python integers."""
    z = ((int(seed) + 1) * _INJ_GOLDEN + ((int(c) << 40) | int(t))) & _INJ_MASK
    z = ((z ^ (z >> 30)) * _INJ_M1) & _INJ_MASK
    z = ((z ^ (z >> 27)) * _INJ_M2) & _INJ_MASK
    return z ^ (z >> 31)


def inject_draws(seed: int, c: int, t: np.ndarray) -> np.ndarray:
    """z >> 33 (31 bits) for the absolute sample indices ``t`` (uint64) of channel c."""
    base = np.uint64(((int(seed) + 1) * _INJ_GOLDEN + (int(c) << 40)) & _INJ_MASK)
    with np.errstate(over="ignore"):
        z = base + np.asarray(t, dtype=np.uint64)   # (c << 40) | t == (c << 40) + t for t < 2^40
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_INJ_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_INJ_M2)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(33)


def inject_profile_table() -> np.ndarray:
    k = np.arange(INJECT_TABLE_LEN, dtype=np.float64)
    return np.rint(32768.0 * np.exp(-(k * k) / (2.0 * INJECT_STEPS * INJECT_STEPS))).astype(np.uint16)


def inject_check_signals(signals) -> None:
    """The refusals of the definition, by name (ValueError)."""
    if len(signals) == 0:
        raise ValueError("inject: no signal to inject")
    if len(signals) > INJECT_MAX_SIGNALS:
        raise ValueError("inject: more than 64 signals")
    for i, s in enumerate(signals):
        burst = not hasattr(s, "period")
        vals = [s.dm, s.amplitude, getattr(s, "alpha", 0.0)]
        vals += [s.time, s.width] if burst else [s.period, s.duty, s.accel, s.phase]
        if not all(math.isfinite(float(v)) for v in vals):
            raise ValueError(f"inject: signal {i}: a value is not finite")
        if s.amplitude < 0:
            raise ValueError(f"inject: signal {i}: amp must not be negative")
        if s.dm < 0:
            raise ValueError(f"inject: signal {i}: dm must not be negative")
        if burst:
            if not s.width > 0:
                raise ValueError(f"inject: signal {i}: width must be positive")
        else:
            if not s.period > 0:
                raise ValueError(f"inject: signal {i}: period must be positive")
            if not s.duty > 0:
                raise ValueError(f"inject: signal {i}: duty must be positive")
            if s.duty > 1:
                raise ValueError(f"inject: signal {i}: duty must not exceed 1")


def inject_parse(text: str) -> List:
    """The injection file's text -> PulsarSpec / BurstSpec list (checked)."""
    from .synthetic import BurstSpec, PulsarSpec

    out = []
    for n, line in enumerate(text.splitlines(), 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        if tok[0] not in ("pulsar", "burst"):
            raise ValueError(f"inject: line {n}: unknown kind '{tok[0]}' (pulsar or burst)")
        if len(tok) < 4:
            raise ValueError(f"inject: line {n}: {tok[0]} needs at least three columns")
        if len(tok) > (8 if tok[0] == "pulsar" else 6):
            raise ValueError(f"inject: line {n}: too many columns for a {tok[0]}")
        try:
            v = [float(x) for x in tok[1:]]
        except ValueError:
            raise ValueError(f"inject: line {n}: cannot read a column") from None
        if tok[0] == "pulsar":
            v += [0.05, 0.0, 0.0, 0.0][len(v) - 3:]
            out.append(PulsarSpec(period=v[0], dm=v[1], amplitude=v[2], duty=v[3], accel=v[4], phase=v[5], alpha=v[6]))
        else:
            v += [0.005, 0.0][len(v) - 3:]
            out.append(BurstSpec(time=v[0], dm=v[1], amplitude=v[2], width=v[3], alpha=v[4]))
        if len(out) > INJECT_MAX_SIGNALS:
            raise ValueError("inject: more than 64 signals")
    inject_check_signals(out)
    return out


def inject_sigma(S1: np.ndarray, S2: np.ndarray, nsamps: int) -> np.ndarray:
    """sigma[c] from the block sums [nchans, nblk] of blocks of 4096 samples:
    the square root of the median of (n S2 - S1^2) / n^2 over the full blocks
    (a shorter file: its one short block)."""
    S1 = np.asarray(S1)
    S2 = np.asarray(S2)
    nchans = S1.shape[0]
    nfull = int(nsamps) // INJECT_BLOCK
    n = INJECT_BLOCK if nfull else int(nsamps)
    nuse = nfull if nfull else 1
    sigma = np.zeros(nchans, dtype=np.float64)
    for c in range(nchans):
        v = [float(n * int(S2[c, b]) - int(S1[c, b]) ** 2) / float(n * n) for b in range(nuse)]
        sigma[c] = math.sqrt(float(np.median(np.array(v, dtype=np.float64))))
    return sigma


def inject_unit(sigma, killmask, nchans: int) -> np.ndarray:
    unit = np.ones(nchans, dtype=np.float64) if sigma is None else np.array(sigma, dtype=np.float64)
    if killmask is not None and len(killmask):
        unit[np.asarray(killmask) == 0] = 0.0
    return unit


def inject_tables(signals, header: Dict, unit, smear: bool = True) -> Dict:
    """The per-channel tables of the definition for PulsarSpec / BurstSpec
    ``signals``: sigc [nsig, 4], delay, inv_w, w [nsig, nchans] float64, A_q
    [nsig, nchans] uint32, T [1537] uint16, tsamp, nlive."""
    inject_check_signals(signals)
    nchans = int(header["nchans"])
    tsamp, fch1, foff = float(header["tsamp"]), float(header["fch1"]), float(header["foff"])
    unit = np.asarray(unit, dtype=np.float64)
    ns = len(signals)
    D = delay_table(nchans, tsamp, fch1, foff).astype(np.float64)
    f_c = fch1 + np.arange(nchans, dtype=np.float64) * foff
    f_mid = fch1 + foff * float(nchans - 1) / 2.0
    sigc = np.zeros((ns, 4), dtype=np.float64)
    delay = np.zeros((ns, nchans), dtype=np.float64)
    w = np.zeros((ns, nchans), dtype=np.float64)
    A_q = np.zeros((ns, nchans), dtype=np.uint32)
    for s, sg in enumerate(signals):
        burst = not hasattr(sg, "period")
        alpha = float(getattr(sg, "alpha", 0.0))
        if burst:
            sigc[s] = (1.0, float(sg.time) / tsamp, 0.0, 0.0)
            f0 = 0.0
            w0 = float(sg.width) / tsamp / 2.3548
        else:
            f0 = 1.0 / float(sg.period)
            sigc[s] = (0.0, float(sg.accel) / (2.0 * C_LIGHT), f0, float(sg.phase))
            w0 = float(sg.duty) / 2.3548
        delay[s] = float(sg.dm) * D
        if smear:
            fg = f_c / 1000.0
            sm_s = 8.3e-6 * float(sg.dm) * abs(foff) / (fg * fg * fg)
            sm = sm_s / tsamp if burst else sm_s * f0
            w[s] = np.sqrt(w0 * w0 + sm * sm)
        else:
            w[s] = w0
        a = float(sg.amplitude) * unit
        if alpha != 0.0:
            a = a * np.power(f_c / f_mid, alpha)
        a = a * (w0 / w[s])
        q = np.rint(65536.0 * a)
        if np.any(q >= 16777216.0):
            raise ValueError(f"inject: signal {s}: the amplitude reaches 256 levels (A_q >= 2^24)")
        A_q[s] = q.astype(np.uint32)
    return {"nsig": ns, "nchans": nchans, "tsamp": tsamp, "sigc": sigc, "delay": delay, "inv_w": float(INJECT_STEPS) / w,
            "w": w, "A_q": A_q, "T": inject_profile_table(), "nlive": int(np.count_nonzero(unit > 0))}


def inject_expected(tab: Dict, c: int, t: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """E (uint64, Q31 levels) of channel c at the absolute samples ``t``
    (uint64), and the touched count of every signal there."""
    tf = np.asarray(t, dtype=np.uint64).astype(np.float64)
    E = np.zeros(tf.shape, dtype=np.uint64)
    T = tab["T"].astype(np.uint64)
    tsamp = float(tab["tsamp"])
    touched = np.zeros(tab["nsig"], dtype=np.uint64)
    for s in range(tab["nsig"]):
        a = int(tab["A_q"][s, c])
        if a == 0:
            continue
        kind, k1, k2, k3 = (float(v) for v in tab["sigc"][s])
        x = tf - float(tab["delay"][s, c])
        if kind != 0.0:
            d = np.abs(x - k1)
        else:
            te = x * tsamp
            ph = (te - (k1 * te) * te) * k2 + k3
            ph = ph - np.floor(ph)
            d = np.minimum(ph, 1.0 - ph)
        u = d * float(tab["inv_w"][s, c])
        hit = u < (INJECT_TABLE_LEN - 1) + 0.5
        k = np.rint(u[hit]).astype(np.int64)
        E[hit] += np.uint64(a) * T[k]
        touched[s] = np.count_nonzero(hit)
    return E, touched


def inject_apply(values: np.ndarray, tab: Dict, nbits: int, seed: int = 0, t0: int = 0):
    """The per-sample step on raw samples ``values`` [nchans, nsamps] holding
    the file's samples from ``t0`` on.  Returns (out uint8, nclip, touched
    uint64 [nsig])."""
    x = np.asarray(values)
    nchans, nsamps = x.shape
    L = (1 << int(nbits)) - 1
    t = np.uint64(t0) + np.arange(nsamps, dtype=np.uint64)
    out = np.empty((nchans, nsamps), dtype=np.uint8)
    nclip = 0
    touched = np.zeros(tab["nsig"], dtype=np.uint64)
    for c in range(nchans):
        E, tc = inject_expected(tab, c, t)
        touched += tc
        add = (E + inject_draws(seed, c, t)) >> np.uint64(31)
        y = x[c].astype(np.uint64) + add
        nclip += int(np.count_nonzero(y > L))
        out[c] = np.minimum(y, np.uint64(L)).astype(np.uint8)
    return out, nclip, touched


def inject_truth(signals, tab: Dict, header: Dict, nsamps: int, unit, sigma) -> List[Tuple[int, float, float]]:
    """(npulses, peak, snr) per signal; sigma None (level units): snr 0."""
    tsamp = float(header["tsamp"])
    unit = np.asarray(unit, dtype=np.float64)
    live = unit > 0
    out = []
    for s, sg in enumerate(signals):
        kind, k1, k2, k3 = (float(v) for v in tab["sigc"][s])
        if kind != 0.0:
            npulses = 1 if 0 <= k1 < float(nsamps) else 0
        else:
            te = float(nsamps - 1) * tsamp
            n = math.floor((te - (k1 * te) * te) * k2 + k3) - math.ceil(k3) + 1
            npulses = max(0, int(n))
        a = tab["A_q"][s].astype(np.float64) / 65536.0
        peak = float(np.sum(a[live]) / np.count_nonzero(live)) if np.any(live) else 0.0
        snr = 0.0
        if sigma is not None:
            sg_ = np.asarray(sigma, dtype=np.float64)
            ok = live & (sg_ > 0)
            ws = tab["w"][s] if kind != 0.0 else tab["w"][s] * float(sg.period) / tsamp
            r = a[ok] / sg_[ok]
            snr = math.sqrt(float(np.sum(((r * r) * float(npulses)) * (ws[ok] * math.sqrt(math.pi)))))
        out.append((npulses, peak, snr))
    return out


def inject_filterbank(infile: str, outfile: Optional[str], signals, killmask=None, seed: int = 0, units: str = "sigma",
                      smear: bool = True) -> Dict:
    """The whole tool on the CPU: reads ``infile``, adds ``signals`` (a list of
    PulsarSpec / BurstSpec, or the injection file's text) and writes
    ``outfile`` (when given) with the header bytes verbatim.  Returns packed
    (the data block's bytes), values [nsamps, nchans], nclip, touched, sigma,
    the tables and truth."""
    import os

    from .sigproc import pack_samples, read_filterbank

    if units not in ("sigma", "level"):
        raise ValueError("inject: units must be sigma or level")
    if isinstance(signals, str):
        signals = inject_parse(signals)
    fb = read_filterbank(infile)
    hdr = fb.header
    nsamps, nchans = fb.data.shape
    nbits = int(hdr["nbits"])
    if nsamps < 1:
        raise ValueError("inject: the input is shorter than one sample")
    rows = np.ascontiguousarray(fb.data.T)
    sigma = None
    if units == "sigma":
        S1, S2 = rfi_block_sums(rows, INJECT_BLOCK)
        sigma = inject_sigma(S1, S2, nsamps)
    unit = inject_unit(sigma, killmask, nchans)
    tab = inject_tables(signals, hdr, unit, smear)
    out, nclip, touched = inject_apply(rows, tab, nbits, seed, 0)
    values = np.ascontiguousarray(out.T)
    packed = pack_samples(values, nbits)
    if outfile:
        with open(infile, "rb") as f:
            head = f.read(int(hdr["size"]))
        tmp = outfile + ".tmp"
        with open(tmp, "wb") as fo:
            fo.write(head)
            fo.write(packed.tobytes())
        os.replace(tmp, outfile)
    return {"packed": packed, "values": values, "nclip": nclip, "touched": touched, "sigma": sigma, "unit": unit,
            "tables": tab, "truth": inject_truth(signals, tab, hdr, nsamps, unit, sigma)}


# ------------------------------------------------------------------ jerk ----
# The definition at the top of csrc/include/psoup/jerk.hpp in NumPy int64 /
# float64: the oracle of csrc/kernels/jerk.hip and of the host steps.
JERK_MAX_SPAN = 1 << 26
JERK_MAX_TRIALS = 4096


def jerk_factor(jerk: float, tsamp: float) -> float:
    """jf of a jerk trial (m/s^3, float32) at the float32 tsamp."""
    return ((float(np.float32(jerk)) * float(np.float32(tsamp))) * float(np.float32(tsamp))) / (6 * C_LIGHT)


def jerk_shift(n: int, jf: float) -> np.ndarray:
    """s(i), i < n: int64 rint (half to even) of three float64 products."""
    i = np.arange(int(n), dtype=np.int64)
    h = int(n) // 2
    g = ((i.astype(np.float64) * (i - h).astype(np.float64)) * (i - int(n)).astype(np.float64)) * np.float64(jf)
    return np.rint(g).astype(np.int64)


def jerk_freq_factor(jerk: float, n: int, tsamp: float) -> float:
    """1 + jerk T^2 / (12 c), T = n tsamp: apparent over true frequency."""
    T = float(int(n)) * float(np.float32(tsamp))
    return 1.0 + ((float(np.float32(jerk)) * T) * T) / (12.0 * C_LIGHT)


def jerk_resample(x: np.ndarray, n: int, jf: float) -> np.ndarray:
    """y of one row x [nrow] (any dtype) for the span n <= nrow."""
    x = np.asarray(x)
    n = int(n)
    if not 1 <= n <= len(x):
        raise ValueError("jerk_resample: the span must be in 1..nrow")
    y = x.copy()
    i = np.arange(n, dtype=np.int64)
    y[:n] = x[np.clip(i + jerk_shift(n, jf), 0, n - 1)]
    return y


def jerk_check(n: int, jfs) -> None:
    if int(n) > JERK_MAX_SPAN:
        raise ValueError("jerk: series longer than 2^26 samples")
    for f in jfs:
        if not math.isfinite(f):
            raise ValueError("jerk: a non-finite value (jerk factor)")
        if (abs(f) * float(n)) * float(n) / 2.0 > 0.9:
            raise ValueError("jerk: a trial moves more than 0.9 samples per sample at the ends")


def jerk_width(dm: float, pulse_width: float, tsamp: float, cfreq: float, bw: float) -> float:
    """AccelPlan::step's effective width at a DM, in seconds (float32 microseconds inside)."""
    bw32, cf32, dm32 = float(np.float32(abs(bw))), float(np.float32(cfreq)), float(np.float32(dm))
    tdm = np.float32(math.pow(8.3 * bw32 / math.pow(cf32, 3.0) * dm32, 2.0))
    tpulse = np.float32(pulse_width) * np.float32(pulse_width)
    ttsamp = np.float32(tsamp) * np.float32(tsamp)
    w_us = np.sqrt(np.float32(np.float32(tdm + tpulse) + ttsamp))
    return float(np.float32(w_us)) * 1.0e-6


def jerk_plan(jerk_start: float, jerk_end: float, tol: float, step: float, pulse_width: float, n: int, tsamp: float,
              cfreq: float, bw: float, dm: float) -> np.ndarray:
    """The jerk trials (float32) of one DM: (float32)(k step) for every integer
    k with jerk_start <= k step <= jerk_end; the one value when start == end."""
    lo, hi = float(np.float32(jerk_start)), float(np.float32(jerk_end))
    if not all(math.isfinite(float(v)) for v in (lo, hi, tol, step, pulse_width, tsamp, cfreq, bw)):
        raise ValueError("jerk: a non-finite value (plan)")
    if lo > hi:
        raise ValueError("jerk: jerk_start > jerk_end")
    if lo == hi:
        return np.array([lo], dtype=np.float32)
    if float(np.float32(step)) > 0:
        st = float(np.float32(step))
    else:
        T = float(int(n)) * float(np.float32(tsamp))
        t = float(np.float32(tol))
        w = jerk_width(dm, pulse_width, tsamp, cfreq, bw)
        st = ((2.0 * w) * math.sqrt(t * t - 1.0)) * ((72.0 * math.sqrt(3.0)) * C_LIGHT) / ((T * T) * T)
    if not (math.isfinite(st) and st > 0):
        raise ValueError("jerk: a non-finite value (the jerk step)")
    ka, kb = math.ceil(lo / st), math.floor(hi / st)
    if kb - ka + 1 > 2 * JERK_MAX_TRIALS:
        raise ValueError("jerk: more than 4096 jerk trials per DM")
    k0, k1 = int(ka), int(kb)
    while float(k0) * st < lo:
        k0 += 1
    while float(k0 - 1) * st >= lo:
        k0 -= 1
    while float(k1) * st > hi:
        k1 -= 1
    while float(k1 + 1) * st <= hi:
        k1 += 1
    if k1 - k0 + 1 > JERK_MAX_TRIALS:
        raise ValueError("jerk: more than 4096 jerk trials per DM")
    if k1 < k0:
        raise ValueError("jerk: no trial k * step in the range")
    return np.array([float(k) * st for k in range(k0, k1 + 1)], dtype=np.float32)


def jerk_distill(cands, tobs: float, span_s: float, tol: float, keep: bool = True):
    """The jerk distillation of one DM: ``cands`` are (Cand, jerk) pairs; a
    stable descending-S/N sort, then AccelerationDistiller's relation with the
    edge f0 tol widened by f0 |jerk0 - jerk| T^2 / (12 c).  Returns the
    surviving pairs; with ``keep`` the absorbed ones are appended to their
    absorber's ``assoc``."""
    c = sorted(cands, key=lambda p: -p[0].snr)
    uniq = [True] * len(c)
    toc = f32(tobs) / C_LIGHT
    jw = (float(span_s) * float(span_s)) / (12.0 * C_LIGHT)
    for idx in range(len(c)):
        if not uniq[idx]:
            continue
        f0, a0, j0 = f32(c[idx][0].freq), f32(c[idx][0].acc), f32(c[idx][1])
        for ii in range(idx + 1, len(c)):
            f, a, j = f32(c[ii][0].freq), f32(c[ii][0].acc), f32(c[ii][1])
            edge = f0 * f32(tol) + (f0 * abs(j0 - j)) * jw
            af = f32(f0 + (a0 - a) * f0 * toc)
            rel = (f0 - edge < f < af + edge) if af > f0 else (af - edge < f < f0 + edge)
            if rel:
                if keep:
                    c[idx][0].assoc.append(c[ii][0])
                uniq[ii] = False
    return [p for p, u in zip(c, uniq) if u]


# ----------------------------------------------------------------- orbit ----
# The definition at the top of csrc/include/psoup/orbit.hpp in NumPy uint64 /
# int64: the oracle of csrc/kernels/orbit.hip and of the host steps.  The sine
# table is built with math.sin, the C library's double sine that the native
# table is built with.
ORBIT_MAX_SPAN = 1 << 26
ORBIT_MAX_TEMPLATES = 1 << 20
_ORBIT_TABLE = None


def orbit_sine_table() -> np.ndarray:
    """int32 T[0..4096]: a turn in 4096 steps, Q30, built from the first quadrant."""
    global _ORBIT_TABLE
    if _ORBIT_TABLE is None:
        t = np.zeros(4097, dtype=np.int64)
        for j in range(1025):
            t[j] = int(np.rint(math.ldexp(math.sin(float(j) * (math.pi / 2048)), 30)))
        for j in range(1025):
            t[2048 - j] = t[j]
        for j in range(2049):
            t[2048 + j] = -t[j]
        _ORBIT_TABLE = t.astype(np.int32)
        _ORBIT_TABLE.setflags(write=False)
    return _ORBIT_TABLE


def orbit_quantise(pb: float, a1: float, ph: float, tsamp: float) -> Tuple[int, int, int]:
    """(W, F, Aq) of a template at the float32 tsamp; raises ValueError by name."""
    pb, a1, ph, ts = float(pb), float(a1), float(ph), float(np.float32(tsamp))
    if not all(math.isfinite(v) for v in (pb, a1, ph, ts)):
        raise ValueError("orbit: a non-finite value")
    if pb < 64.0 * ts:
        raise ValueError("orbit: pb < 64 tsamp")
    if a1 < 0.0:
        raise ValueError("orbit: a1 < 0")
    W = int(np.rint(math.ldexp(ts / pb, 64)))
    r = ph - math.floor(ph)
    if r >= 1.0:
        r = 0.0
    F = int(math.ldexp(r, 64))
    aq = float(np.rint((a1 / ts) * 256.0))
    if aq >= 2.0 ** 30:
        raise ValueError("orbit: Aq >= 2^30")
    return W, F, int(aq)


def orbit_sine(th: np.ndarray) -> np.ndarray:
    """S(th) of uint64 phases, int64."""
    T = orbit_sine_table().astype(np.int64)
    th = np.asarray(th, dtype=np.uint64)
    j = (th >> np.uint64(52)).astype(np.int64)
    f = ((th >> np.uint64(32)) & np.uint64(0xFFFFF)).astype(np.int64)
    return T[j] + (((T[j + 1] - T[j]) * f + (1 << 19)) >> 20)


def orbit_shift(n: int, q: Tuple[int, int, int]) -> np.ndarray:
    """s(i), i < n, int64: wrapping uint64 phases, int64 arithmetic shifts."""
    W, F, Aq = (int(v) for v in q)
    with np.errstate(over="ignore"):
        th = np.uint64(F) + np.arange(int(n), dtype=np.uint64) * np.uint64(W)
    sf = int(orbit_sine(np.array([F], dtype=np.uint64))[0])
    return (np.int64(Aq) * (orbit_sine(th) - sf) + (1 << 37)) >> 38


def orbit_resample(x: np.ndarray, n: int, q: Tuple[int, int, int]) -> np.ndarray:
    """y of one row x [nrow] (any dtype) for the span n <= nrow."""
    x = np.asarray(x)
    n = int(n)
    if not 1 <= n <= len(x):
        raise ValueError("orbit_resample: the span must be in 1..nrow")
    y = x.copy()
    i = np.arange(n, dtype=np.int64)
    y[:n] = x[np.clip(i + orbit_shift(n, q), 0, n - 1)]
    return y


def orbit_beta(pb: float, a1: float) -> float:
    return ((2.0 * math.pi) * float(a1)) / float(pb)


def orbit_check(n: int, bank, tsamp: float) -> None:
    if int(n) > ORBIT_MAX_SPAN:
        raise ValueError("orbit: series longer than 2^26 samples")
    if len(bank) == 0:
        raise ValueError("orbit: an empty bank")
    if len(bank) > ORBIT_MAX_TEMPLATES:
        raise ValueError("orbit: more than 2^20 templates")
    for pb, a1, ph in bank:
        orbit_quantise(pb, a1, ph, tsamp)
        if orbit_beta(pb, a1) > 0.9:
            raise ValueError("orbit: a template moves more than 0.9 samples per sample")


def orbit_parse_bank(text: str) -> List[Tuple[float, float, float]]:
    """The (pb, a1, ph) of a bank file's text: `#` starts a comment, columns past the third are ignored."""
    bank = []
    for ln, line in enumerate(text.split("\n"), 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        try:
            if len(tok) < 3:
                raise ValueError
            bank.append(tuple(float(v) for v in tok[:3]))
        except ValueError:
            raise ValueError(f"orbit: bank line {ln} is malformed") from None
    return bank


def orbit_grid(pb_start: float, pb_end: float, npb: int, a1_start: float, a1_end: float, na1: int,
               nphase: int) -> List[Tuple[float, float, float]]:
    """The regular grid: pb geometric, a1 linear, phase k / nphase; pb slowest, phase fastest."""
    if min(npb, na1, nphase) < 1:
        raise ValueError("orbit: --npb, --na1 and --nphase must be at least 1")
    if npb * na1 * nphase > ORBIT_MAX_TEMPLATES:
        raise ValueError("orbit: more than 2^20 templates")
    bank = []
    for p in range(npb):
        pb = float(pb_start)
        if p > 0:
            pb = float(pb_end) if p == npb - 1 else \
                float(pb_start) * math.pow(float(pb_end) / float(pb_start), float(p) / float(npb - 1))
        for a in range(na1):
            a1 = float(a1_start)
            if a > 0:
                a1 = float(a1_end) if a == na1 - 1 else \
                    float(a1_start) + (float(a1_end) - float(a1_start)) * (float(a) / float(na1 - 1))
            for f in range(nphase):
                bank.append((pb, a1, float(f) / float(nphase)))
    return bank


def orbit_distill(cands, beta, tol: float, keep: bool = True):
    """The orbit distillation of one DM: ``cands`` are (Cand, template index)
    pairs, ``beta`` the templates' 2 pi a1 / pb.  A stable descending-S/N sort;
    a survivor absorbs a weaker candidate of another template when
    |f / f0 - 1| <= tol + beta0 + beta.  The plain scan, survivors times all
    candidates.  Returns the surviving pairs; with ``keep`` the absorbed ones
    are appended to their absorber's ``assoc``."""
    c = sorted(cands, key=lambda p: -p[0].snr)
    uniq = [True] * len(c)
    for idx in range(len(c)):
        if not uniq[idx]:
            continue
        f0, b0 = f32(c[idx][0].freq), float(beta[c[idx][1]])
        for ii in range(idx + 1, len(c)):
            if c[ii][1] == c[idx][1]:
                continue
            if abs(f32(c[ii][0].freq) / f0 - 1.0) <= (f32(tol) + b0) + float(beta[c[ii][1]]):
                if keep:
                    c[idx][0].assoc.append(c[ii][0])
                uniq[ii] = False
    return [p for p, u in zip(c, uniq) if u]


# ------------------------------------------------------------- sideband ----
# The sideband (phase-modulation) search of csrc/include/psoup/sideband.hpp in
# float64 NumPy.  An extension beyond the reference.
SB_RANGE = 4096
SB_RANGE_LANES = 256


def sideband_geometry(min_freq: float, max_freq: float, fft_size: int, tsamp: float, m_lo: int = 5, m_hi: int = 13) -> Dict:
    """The definition's T, k_lo, k_hi and segments per size (float32 inputs)."""
    T = float(fft_size) * float(np.float32(tsamp))
    top = fft_size // 2
    k_lo = int(min(max(math.ceil(float(np.float32(min_freq)) * T), 0), top))
    k_hi = int(min(max(math.floor(float(np.float32(max_freq)) * T), 0), top))
    k_hi = max(k_hi, k_lo)
    return {"tobs": T, "k_lo": k_lo, "k_hi": k_hi,
            "nseg": {m: sideband_nseg(k_hi - k_lo, m) for m in range(m_lo, m_hi + 1)}}


def sideband_nseg(band: int, m: int) -> int:
    M = 1 << m
    return 0 if band < M else (band - M) // (M // 2) + 1


def sideband_power(spec: np.ndarray, k_lo: int, k_hi: int, zapmask=None) -> Tuple[float, np.ndarray]:
    """Step 2 on one complex64 spectrum: (mu, P float32 [len(spec)], zero outside
    the band).  zapmask: a boolean array per bin (True = zapped) or None.  mu is
    summed in the definition's order."""
    spec = np.asarray(spec)
    re = spec.real.astype(np.float64)
    im = spec.imag.astype(np.float64)
    p = re * re + im * im
    zap = np.zeros(len(p), dtype=bool) if zapmask is None else np.asarray(zapmask, dtype=bool)
    band = k_hi - k_lo
    nranges = (band + SB_RANGE - 1) // SB_RANGE
    v = np.zeros(nranges * SB_RANGE)
    v[:band] = np.where(zap[k_lo:k_hi], 0.0, p[k_lo:k_hi])
    v = v.reshape(nranges, SB_RANGE // SB_RANGE_LANES, SB_RANGE_LANES)
    a = np.zeros((nranges, SB_RANGE_LANES))
    for u in range(SB_RANGE // SB_RANGE_LANES):
        a = a + v[:, u, :]
    s = SB_RANGE_LANES // 2
    while s >= 1:
        a = a[:, :s] + a[:, s:2 * s]
        s //= 2
    total = 0.0
    for r in range(nranges):
        total = total + float(a[r, 0])
    count = int(band - np.count_nonzero(zap[k_lo:k_hi]))
    if count < 1:
        raise ValueError("sideband: the band has no unzapped bin")
    mu = total / count
    P = np.zeros(len(p), dtype=np.float32)
    P[k_lo:k_hi] = np.where(zap[k_lo:k_hi], np.float32(1.0), (p[k_lo:k_hi] / mu).astype(np.float32))
    return mu, P


def sideband_spectra(P: np.ndarray, k_lo: int, k_hi: int, m: int, clip: float = 32.0) -> Tuple[np.ndarray, np.ndarray]:
    """Step 3 at one size on one float32 row: (S float64 [nseg, M/2], norm
    float64 [nseg] = ||x||_2 of each segment), by numpy.fft.rfft in float64."""
    M = 1 << m
    nseg = sideband_nseg(k_hi - k_lo, m)
    if nseg == 0:
        return np.zeros((0, M // 2)), np.zeros(0)
    x = np.minimum(np.asarray(P[k_lo:k_hi], dtype=np.float32), np.float32(clip)).astype(np.float64) - 1.0
    idx = (np.arange(nseg) * (M // 2))[:, None] + np.arange(M)[None, :]
    seg = x[idx]
    F = np.fft.rfft(seg, axis=1)[:, :M // 2]
    return (F.real ** 2 + F.imag ** 2) / M, np.sqrt((seg * seg).sum(axis=1))


def sideband_bound(S: np.ndarray, norm: np.ndarray, m: int) -> np.ndarray:
    """What a float32 radix FFT may differ from S by: t = 16 u log2(M) ||x||_2 on
    |F|, so (2 |F| t + t^2) / M on S (u = 2^-24)."""
    M = 1 << m
    t = 16.0 * 2.0 ** -24 * m * np.asarray(norm, dtype=np.float64)
    t = t.reshape((-1,) + (1,) * (np.ndim(S) - 1)) if np.ndim(S) > 1 else t
    return (2.0 * np.sqrt(np.asarray(S) * M) * t + t * t) / M


def sideband_search(P: np.ndarray, k_lo: int, k_hi: int, m_lo: int = 5, m_hi: int = 13, j_min: int = 2,
                    clip: float = 32.0, min_power: float = 30.0, dm_idx: int = 0) -> Dict:
    """Steps 3 and 4 on one float32 row.  Returns per size m: best_S, best_j
    (lowest j on a tie), bound (on best_S), gap (largest less second largest S)
    and the events (dm_idx, m, seg, j, S) of S >= min_power."""
    out = {"events": []}
    for m in range(m_lo, m_hi + 1):
        S, norm = sideband_spectra(P, k_lo, k_hi, m, clip)
        if S.shape[0] == 0:
            out[m] = {"best_S": np.zeros(0), "best_j": np.zeros(0, dtype=np.int64), "bound": np.zeros(0),
                      "gap": np.zeros(0)}
            continue
        A = S[:, j_min:]
        j = np.argmax(A, axis=1)  # the first of equal maxima
        best = A[np.arange(len(j)), j]
        if A.shape[1] > 1:
            part = np.partition(A, A.shape[1] - 2, axis=1)
            gap = part[:, -1] - part[:, -2]
        else:
            gap = np.full(len(j), np.inf)
        out[m] = {"best_S": best, "best_j": j + j_min, "bound": sideband_bound(best, norm, m), "gap": gap}
        for s in np.nonzero(best >= min_power)[0]:
            out["events"].append((int(dm_idx), m, int(s), int(j[s] + j_min), float(best[s])))
    return out


def sideband_related(e, c0) -> bool:
    """Step 5's two conditions, in exact integers."""
    _, m, seg, j, _ = e
    _, m0, seg0, j0, _ = c0
    M, M0 = 1 << m, 1 << m0
    c = seg * (M // 2) + M // 2
    cc = seg0 * (M0 // 2) + M0 // 2
    if abs(c - cc) > (M + M0) // 2:
        return False
    for r in range(1, 5):
        if abs(r * j * M0 - j0 * M) <= r * M0 + M or abs(j * M0 - r * j0 * M) <= M0 + r * M:
            return True
    return False


def sideband_cluster(events) -> List[Tuple[tuple, int, int, int]]:
    """Step 5: [(leading event, members, dm_lo, dm_hi)] in descending S."""
    ev = sorted((tuple(e) for e in events), key=lambda e: (-float(np.float32(e[4])), e[0], e[1], e[2]))
    out: List[list] = []
    for e in ev:
        for c in out:
            if sideband_related(e, c[0]):
                c[1] += 1
                c[2] = min(c[2], e[0])
                c[3] = max(c[3], e[0])
                break
        else:
            out.append([e, 1, e[0], e[0]])
    return [tuple(c) for c in out]


# ---------------------------------------------------------------- orbopt ----
# The oracle of csrc/include/psoup/orbopt.hpp, written from its definition in
# Python ints, int64 and float64; the fold is built on orbit_shift above.
OOPT_MAX_TEMPLATES = 4096


def orbopt_check_params(nbins: int = 64, nints: int = 16, npb: int = 9, na1: int = 9, nphase: int = 9, np_: int = 33,
                        p_step: float = 1.0, pb_step: float = 0.0, a1_step: float = 0.0, phase_step: float = 0.0) -> None:
    if not 2 <= nbins <= 256:
        raise ValueError("orbopt: nbins must be in 2..256")
    if not 1 <= nints <= 64:
        raise ValueError("orbopt: nints must be in 1..64")
    if min(npb, na1, nphase) < 1 or npb % 2 == 0 or na1 % 2 == 0 or nphase % 2 == 0:
        raise ValueError("orbopt: an even count (--npb, --na1 and --nphase must be odd and at least 1)")
    if not 1 <= np_ <= 257 or np_ % 2 == 0:
        raise ValueError("orbopt: an even count (--np must be odd and in 1..257)")
    if npb * na1 * nphase > OOPT_MAX_TEMPLATES:
        raise ValueError("orbopt: more than 4096 templates per candidate")
    if not all(math.isfinite(v) and v >= 0 for v in (p_step, pb_step, a1_step, phase_step)):
        raise ValueError("orbopt: the steps must be finite and non-negative")


def orbopt_grid(cand, n: int, tsamp: float, nbins: int = 64, npb: int = 9, na1: int = 9, nphase: int = 9,
                pb_step: float = 0.0, a1_step: float = 0.0, phase_step: float = 0.0, k: int = 0) -> Dict:
    """Step 1 and G for ``cand`` = (period, dm, acc, pb, a1, phase): dict(npb,
    na1, nphase, dpb, da1, dph, G, templates [(pb, a1, ph)] after the sign fold,
    quant [(W, F, Aq)]).  Raises ValueError naming ``candidate k``."""
    P, dm, acc, pb0, a10, ph0 = (float(v) for v in cand)
    ts = float(np.float32(tsamp))
    who = f"orbopt: candidate {k}"
    if int(n) > ORBIT_MAX_SPAN:
        raise ValueError("orbopt: series longer than 2^26 samples")
    if not math.isfinite(P) or P < 2.0 * ts:
        raise ValueError(who + ": the period is not finite or below 2 tsamp")
    if not math.isfinite(dm) or dm < 0:
        raise ValueError(who + ": a non-finite or negative DM")
    if not all(math.isfinite(v) for v in (acc, pb0, a10, ph0)):
        raise ValueError(who + ": orbit: a non-finite value")
    T = float(int(n)) * ts
    nb = float(nbins)
    da1 = float(a1_step) if a1_step > 0 else P / (2.0 * nb)
    if phase_step > 0:
        dph = float(phase_step)
    elif a10 == 0.0:
        dph, nphase = 0.0, 1
    else:
        dph = min(1.0 / 16.0, P / ((4.0 * math.pi) * abs(a10) * nb))
    if pb_step > 0:
        dpb = float(pb_step)
    elif a10 == 0.0:
        dpb, npb = 0.0, 1
    else:
        dpb = min(pb0 / 16.0, (pb0 * pb0 * P) / ((4.0 * math.pi) * abs(a10) * T * nb))
    G = int(np.rint(math.ldexp(ts / P, 64)))
    tmpl, quant = [], []
    for kb in range(npb):
        for ka in range(na1):
            for kp in range(nphase):
                pb = pb0 + float(kb - npb // 2) * dpb
                a1 = a10 + float(ka - na1 // 2) * da1
                ph = ph0 + float(kp - nphase // 2) * dph
                if a1 < 0.0:
                    a1, ph = -a1, ph + 0.5
                try:
                    quant.append(orbit_quantise(pb, a1, ph, ts))
                    if orbit_beta(pb, a1) > 0.9:
                        raise ValueError("orbit: a template moves more than 0.9 samples per sample")
                except ValueError as e:
                    raise ValueError(f"{who}: grid template {len(tmpl)}: {e}") from None
                tmpl.append((pb, a1, ph))
    return {"npb": npb, "na1": na1, "nphase": nphase, "dpb": dpb, "da1": da1, "dph": dph, "G": G, "templates": tmpl,
            "quant": quant}


def orbopt_bins(n: int, G: int, nints: int, nbins: int) -> np.ndarray:
    """The flat cell j(i) * nbins + b(i) of every sample, int64 [n]."""
    i = np.arange(int(n), dtype=np.uint64)
    with np.errstate(over="ignore"):
        phi = i * np.uint64(G)
    b = ((phi >> np.uint64(32)) * np.uint64(nbins)) >> np.uint64(32)
    j = (i * np.uint64(nints)) // np.uint64(n)
    return (j * np.uint64(nbins) + b).astype(np.int64)


def orbopt_hits(n: int, G: int, nints: int, nbins: int) -> np.ndarray:
    return np.bincount(orbopt_bins(n, G, nints, nbins), minlength=nints * nbins).astype(np.int32).reshape(nints, nbins)


def orbopt_fold_plain(y: np.ndarray, n: int, G: int, nints: int, nbins: int) -> np.ndarray:
    """The plain fold of one (already resampled) row's first n samples: int32 [nints, nbins], modulo 2^32."""
    cell = orbopt_bins(n, G, nints, nbins)
    s = np.zeros(nints * nbins, dtype=np.int64)
    np.add.at(s, cell, np.asarray(y[:int(n)], dtype=np.int64))
    return (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(nints, nbins)


def orbopt_fold(x: np.ndarray, n: int, G: int, quant, nints: int, nbins: int) -> np.ndarray:
    """Step 2 for one row: int32 [K, nints, nbins]."""
    x = np.asarray(x)
    n = int(n)
    cell = orbopt_bins(n, G, nints, nbins)
    i = np.arange(n, dtype=np.int64)
    out = np.zeros((len(quant), nints * nbins), dtype=np.int64)
    for k, q in enumerate(quant):
        src = np.clip(i + orbit_shift(n, q), 0, n - 1)
        out[k] = np.bincount(cell, weights=x[src].astype(np.float64), minlength=nints * nbins).astype(np.int64)
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(len(quant), nints, nbins)


def orbopt_moments(x: np.ndarray, n: int, k: int = 0) -> Tuple[int, int]:
    """Step 3's (m, V1) in Python ints; refuses candidate k at the int32 bound."""
    n = int(n)
    v = np.asarray(x[:n], dtype=np.int64)
    m = (int(v.sum()) + n // 2) // n
    v1 = int(((v - m) ** 2).sum())
    if max(m, 255 - m) * n >= 2 ** 31:
        raise ValueError(f"orbopt: candidate {k}: max(m, 255 - m) * n >= 2^31")
    return m, v1


def orbopt_drift_table(nints: int, nbins: int, np_: int, p_step: float = 1.0) -> np.ndarray:
    st = np.zeros((np_, nints), dtype=np.int32)
    for l in range(np_):
        L = (l - np_ // 2) * float(p_step)
        for j in range(nints):
            u = (j + 0.5) / nints
            st[l, j] = _opt_reduce(L * (u - 0.5), nbins)
    return st


def orbopt_search(fold: np.ndarray, hits: np.ndarray, m: int, st: np.ndarray) -> Dict:
    """Step 4 from the definition: dict(best_val, best_idx, centre int32 [nw];
    tcurve int32 [nw, K]; msum int64 [K])."""
    fold = np.asarray(fold)
    K, nints, nbins = fold.shape
    st = np.asarray(st)
    np_ = st.shape[0]
    nw = cube_opt_nwidths(nbins)
    # d modulo 2^32, read back as int32
    d = ((fold.astype(np.int64) - int(m) * np.asarray(hits, dtype=np.int64)[None]) & 0xFFFFFFFF).astype(np.uint32) \
        .view(np.int32).astype(np.int64)
    b = np.arange(nbins)
    rot = (b[None, None, :] + st[:, :, None]) % nbins                      # [l, j, b]
    S = np.zeros((nw, K, np_, nbins), dtype=np.int64)
    for k in range(K):
        prof = np.zeros((np_, nbins), dtype=np.int64)
        for j in range(nints):
            prof += d[k, j][rot[:, j, :]]
        box = prof
        for kw in range(nw):
            S[kw, k] = box
            box = box + np.roll(box, -(1 << kw), axis=1)
    assert np.abs(S).max(initial=0) < 2 ** 31
    flat = S.reshape(nw, -1)
    return {"best_val": flat.max(axis=1).astype(np.int32), "best_idx": flat.argmax(axis=1).astype(np.int32),
            "tcurve": S.max(axis=(2, 3)).astype(np.int32), "centre": S[:, K // 2, np_ // 2].max(axis=1).astype(np.int32),
            "msum": d.sum(axis=(1, 2)).astype(np.int64)}


def orbopt_snr(s: float, w: int, msum: int, v: float, nbins: int) -> float:
    if not v > 0:
        return 0.0
    return (float(s) - w * float(msum) / nbins) / math.sqrt(v * w * (1.0 - float(w) / nbins))


def orbopt_finish(cand, grid: Dict, n: int, tsamp: float, m: int, v1: int, hits: np.ndarray, st: np.ndarray,
                  found: Dict, fold: np.ndarray, p_step: float = 1.0) -> Dict:
    """Step 5: the record of one candidate.  ``fold`` is [K, nints, nbins]."""
    P, dm, acc, pb0, a10, ph0 = (float(v) for v in cand)
    K, nints, nbins = np.asarray(fold).shape
    np_ = np.asarray(st).shape[0]
    nw = cube_opt_nwidths(nbins)
    v = float(v1) / float(nbins)
    snr = snr_in = 0.0
    kbest = 0
    for kw in range(nw):
        k = int(found["best_idx"][kw]) // nbins // np_
        s = orbopt_snr(float(int(found["best_val"][kw])), 1 << kw, int(found["msum"][k]), v, nbins)
        if kw == 0 or s > snr:
            snr, kbest = s, kw
        si = orbopt_snr(float(int(found["centre"][kw])), 1 << kw, int(found["msum"][K // 2]), v, nbins)
        if kw == 0 or si > snr_in:
            snr_in = si
    idx = int(found["best_idx"][kbest])
    ob, ol, ok = idx % nbins, (idx // nbins) % np_, idx // nbins // np_
    ts = float(np.float32(tsamp))
    T = float(int(n)) * ts
    L = (ol - np_ // 2) * float(p_step)
    kp, ka, kb = ok % grid["nphase"], (ok // grid["nphase"]) % grid["na1"], ok // grid["nphase"] // grid["na1"]
    face = lambda i, c: c > 1 and i in (0, c - 1)  # noqa: E731
    flags = 1 if (face(kp, grid["nphase"]) or face(ka, grid["na1"]) or face(kb, grid["npb"]) or face(ol, np_)) else 0
    if ((abs(float(np.float32(acc))) * T * T) / ((2.0 * C_LIGHT) * P)) * nbins > 1.0:
        flags |= 2
    d = ((np.asarray(fold[ok], dtype=np.int64) - int(m) * np.asarray(hits, dtype=np.int64)) & 0xFFFFFFFF) \
        .astype(np.uint32).view(np.int32).astype(np.int64)
    bb = np.arange(nbins)
    prof = np.zeros(nbins, dtype=np.int64)
    for j in range(nints):
        prof += d[j, (bb + int(st[ol, j])) % nbins]
    out = {k2: np.asarray(v2).copy() for k2, v2 in found.items()}
    t = grid["templates"][ok]
    out.update(period=P, dm=float(np.float32(dm)), acc=float(np.float32(acc)), pb=pb0, a1=a10, phase=ph0,
               npb=grid["npb"], na1=grid["na1"], nphase=grid["nphase"], dpb=grid["dpb"], da1=grid["da1"],
               dph=grid["dph"], snr=snr, snr_in=snr_in, opt_period=1.0 / (1.0 / P - L / (nbins * T)), opt_pb=t[0],
               opt_a1=t[1], opt_phase=t[2], opt_width=1 << kbest, opt_bin=ob, opt_k=ok, opt_l=ol, flags=flags, m=int(m),
               v1=int(v1), hits=np.asarray(hits, dtype=np.int32).copy(), fold=np.asarray(fold[ok], dtype=np.int32).copy(),
               profile=(prof & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    return out


def orbit_optimise(x: np.ndarray, cand, n: int, tsamp: float, nbins: int = 64, nints: int = 16, npb: int = 9,
                   na1: int = 9, nphase: int = 9, np_: int = 33, p_step: float = 1.0, pb_step: float = 0.0,
                   a1_step: float = 0.0, phase_step: float = 0.0, k: int = 0) -> Dict:
    """The whole chain on one candidate (period, dm, acc, pb, a1, phase) and
    its dedispersed row ``x``: orbopt_finish's record."""
    orbopt_check_params(nbins, nints, npb, na1, nphase, np_, p_step, pb_step, a1_step, phase_step)
    grid = orbopt_grid(cand, n, tsamp, nbins, npb, na1, nphase, pb_step, a1_step, phase_step, k)
    m, v1 = orbopt_moments(x, n, k)
    hits = orbopt_hits(n, grid["G"], nints, nbins)
    fold = orbopt_fold(x, n, grid["G"], grid["quant"], nints, nbins)
    st = orbopt_drift_table(nints, nbins, np_, p_step)
    found = orbopt_search(fold, hits, m, st)
    return orbopt_finish(cand, grid, n, tsamp, m, v1, hits, st, found, fold, p_step)


def orbopt_parse_candidates(text: str):
    """The (period, dm, acc, pb, a1, phase) of a candidate file's text (dm and acc as float32)."""
    out = []
    for ln, line in enumerate(text.split("\n"), 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        try:
            if len(tok) < 6:
                raise ValueError
            v = [float(t) for t in tok[:6]]
        except ValueError:
            raise ValueError(f"orbopt: candidate line {ln} is malformed") from None
        out.append((v[0], float(np.float32(v[1])), float(np.float32(v[2])), v[3], v[4], v[5]))
    return out
