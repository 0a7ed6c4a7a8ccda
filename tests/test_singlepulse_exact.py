"""Single-pulse search at its tile, halo, trend and tie edges
(csrc/kernels/singlepulse.hip), against the float64 oracle of
peasoup_amd.utils.reference with a tolerance derived from the kernel's
arithmetic (reference.sp_error_bound), never a flat number, and against the
integer-exact oracle (reference.sp_boxcar_snr_exact) with no tolerance at all.

CPU: the float32 NumPy emulation of the kernel's order (reference.sp_search_f32,
window guards and stale partners included) stays inside the bound on every case
of this module and reproduces the exact cases bit for bit; every defect of
DEFECTS, implemented as a variant of the oracle, moves at least one case by
more than twice the bound; sp_baseline_samples against a transcription.
GPU: every ladder depth K = 2..12, depths limited by n, tile and halo edges,
the last valid start, trends (block means and sigma through
sp_trend_sigma_rows), extremes, row indexing, ties and records.

Largest observed |kernel - oracle| / bound per width on an MI355X (gfx950),
over every GPU case of the module (each test prints its own figures):

  width   1     2     4     8     16    32    64    128   256   512   1024  2048  4096
  ratio   0.189 0.207 0.228 0.227 0.234 0.232 0.237 0.230 0.223 0.219 0.202 0.166 0.124

all from trend-31251-31250, whose first 15625 samples lie before the first
block centre: there the rounding of one float32 mean, which the bound charges
in full, is the whole error.  Every other case stays below 0.19.  The
NumPy emulation gives the same figures to four digits.  The largest
|sigma - oracle sigma| / bound is 0.048.  No case found a defect in the
kernels."""
import collections
import functools
import math

import numpy as np
import pytest

from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref

T = C.SP_TILE
NONE = 0xFFFFFFFF

Case = collections.namedtuple("Case", "name rows n baseline wmax")


def _eff_baseline(b, n):
    return min(max(int(b), 64), int(n))


def _pack(xs, n, stride=None):
    """float rows -> uint8 [ndm, stride], rounded and clipped, the padding past
    n filled with 255 (a read past n would show)."""
    stride = stride or (n + 3) // 4 * 4 + 8
    assert stride % 4 == 0 and stride >= n
    rows = np.full((len(xs), stride), 255, dtype=np.uint8)
    for d, x in enumerate(xs):
        assert len(x) == n
        rows[d, :n] = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    rows.setflags(write=False)
    return rows


def _kmax(n, wmax):
    return len(ref.sp_widths(n, wmax)) - 1


# ----------------------------------------------------------------- cases ----
def _depth_case(wmax):
    """n = 2T + 37, H = 2^K.  Row 0: a top hat of H samples over [T - H/2,
    T + H/2) and one over the last H samples; row 1: H/2 samples ending at the
    tile boundary, and the last H; row 2: H samples from T - 1, the last start
    of tile 0, whose widest boxcar needs the whole halo."""
    n = 2 * T + 37
    H = 1 << _kmax(n, wmax)
    rng = np.random.default_rng(100 + wmax)
    xs = [rng.normal(100.0, 3.0, n) for _ in range(3)]
    xs[0][T - H // 2:T + H // 2] += 30.0
    xs[0][n - H:] += 30.0
    xs[1][T - H // 2:T] += 30.0
    xs[1][n - H:] += 20.0
    xs[2][T - 1:T - 1 + H] += 30.0
    return Case(f"depth-{wmax}", _pack(xs, n), n, _eff_baseline(4096, n), wmax)


def _noise_case(name, n, wmax, baseline, seed):
    """Two rows of N(100, 6) noise on ramps of 20 and 40 units, a 37-sample top
    hat across the first tile boundary where the row reaches it."""
    rng = np.random.default_rng(seed)
    xs = []
    for d in range(2):
        x = rng.normal(100.0, 6.0, n) + 20.0 * (d + 1) * np.arange(n) / n
        if n > T:
            x[T - 18:min(n, T + 19)] += 10.0
        xs.append(x)
    return Case(name, _pack(xs, n), n, _eff_baseline(baseline, n), wmax)


def _last_start_case(n, wmax, baseline):
    """One row per width w: N(100, 2) noise and 40 units over [n - w, n); the
    row stride is three times n."""
    widths = ref.sp_widths(n, wmax)
    rng = np.random.default_rng(7000 + n)
    xs = []
    for w in widths:
        x = rng.normal(100.0, 2.0, n)
        x[n - w:] += 40.0
        xs.append(x)
    stride = (3 * n + 3) // 4 * 4
    return Case(f"last-{n}-{wmax}", _pack(xs, n, stride), n, _eff_baseline(baseline, n), wmax)


def _trend_case(n, baseline):
    """Levels that move by tens of units per trend block: a square wave of
    period 5 blocks, a ramp of 45 units per block that saturates, a sawtooth
    of period 3.1 blocks; N(0, 2) noise on each."""
    b = _eff_baseline(baseline, n)
    rng = np.random.default_rng(9000 + n + baseline)
    i = np.arange(n, dtype=np.float64)
    step = np.where(np.floor(i / (2.5 * b)) % 2 == 0, 60.0, 180.0)
    ramp = np.clip(20.0 + 45.0 * i / b, 0.0, 235.0)
    saw = 40.0 + 160.0 * ((i / (3.1 * b)) % 1.0)
    xs = [v + rng.normal(0.0, 2.0, n) for v in (step, ramp, saw)]
    return Case(f"trend-{n}-{baseline}", _pack(xs, n), n, b, 4096)


def _extreme_case():
    n = T + 70
    rng = np.random.default_rng(31)
    alt = np.where(np.arange(n) % 2 == 0, 0.0, 255.0)
    step = np.where(np.arange(n) < 5000 + 21, 0.0, 255.0)  # 5021 % 64 == 29
    spike = np.full(n, 100.0)
    spike[3000] = 101.0
    live0 = rng.normal(100.0, 6.0, n)
    live1 = rng.normal(60.0, 3.0, n) + 30.0 * np.arange(n) / n
    xs = [alt, np.zeros(n), step, live0, np.full(n, 255.0), spike, live1]
    return Case("extremes", _pack(xs, n), n, 4096, 4096)


EXTREME_DEAD = (1, 4)
EXTREME_LIVE = (3, 6)


def _rows_case():
    """33 rows of 200 samples (4 trend blocks of 64), each with its own level,
    sigma and slope, and a pulse whose place depends on the row."""
    n, ndm = 200, 33
    rng = np.random.default_rng(33)
    xs = []
    for d in range(ndm):
        x = rng.normal(20.0 + 6.0 * d, 0.5 + 0.4 * d, n) + (d % 5) * 10.0 * np.arange(n) / n
        x[5 * d:5 * d + 1 + d % 7] += 4.0 * (0.5 + 0.4 * d)
        xs.append(x)
    return Case("rows-33", _pack(xs, n), n, 64, 64)


DEPTH_WMAX = [4 << j for j in range(11)] + [100, 4095]
NLIM_N = [64, 65, 66, 67, 127, 128, 129, 8191, 8192, 8193]
EDGE = [(K, n) for K in (12, 4) for n in (T - 1, T, T + 1, T + (1 << K) - 1, T + (1 << K), T + (1 << K) + 1, 2 * T)]
LAST = [(2 * T + 37, 4096, 4096), (T + 2, 4096, 4096), (T + 4096 + 3, 4096, 4096), (2 * T, 512, 100), (200, 64, 64),
        (67, 4096, 64)]
TREND = [(385, 64), (1000, 64), (1050, 100), (1000, 1000), (1000, 999), (2 * T + 37, 4096), (31251, 31250),
         (3 * T + 11, 4096)]


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [_depth_case(w) for w in DEPTH_WMAX]
    cs += [_noise_case(f"nlim-{n}", n, 4096, 64 if n < 4096 else 4096, 200 + n) for n in NLIM_N]
    cs += [_noise_case(f"edge-{K}-{n}", n, 1 << K, 4096, 300 + n + K) for K, n in EDGE]
    cs += [_last_start_case(*a) for a in LAST]
    cs += [_trend_case(*a) for a in TREND]
    cs += [_extreme_case(), _rows_case()]
    return collections.OrderedDict((c.name, c) for c in cs)


def _names(prefix):
    return [k for k in _cases() if k.startswith(prefix)]


def test_cases_cover_the_residues():
    ns = {c.n for c in _cases().values()}
    assert {n % 4 for n in ns} == {0, 1, 2, 3} and {0, 1, 63} <= {n % 64 for n in ns}
    assert {_kmax(c.n, c.wmax) for c in _cases().values()} >= set(range(2, 13))
    assert all(c.n <= 31251 and c.rows.shape[0] <= 40 for c in _cases().values())


Oracle = collections.namedtuple("Oracle", "widths snr bound maxima blockbound")


def _block_bound(bound, block=64):
    """Per width: the largest bound of each 64-start block (|max f - max g| <= max |f - g|)."""
    out = []
    for b in bound:
        nb = (len(b) + block - 1) // block
        out.append(np.array([b[j * block:(j + 1) * block].max() for j in range(nb)]))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Per row of the case: the float64 oracle and its bound; computed once."""
    c = _cases()[name]
    widths = ref.sp_widths(c.n, c.wmax)
    out = []
    for d in range(c.rows.shape[0]):
        u = c.rows[d, :c.n]
        snr = ref.sp_boxcar_snr(u, c.baseline, widths)
        bound = ref.sp_error_bound(u, c.baseline, widths)
        out.append(Oracle(widths, snr, bound, ref.sp_block_maxima(snr), _block_bound(bound)))
    return out


def _dense_from_snr(snr, n):
    """Dense (best, arg) [K + 1, ceil(n / 64)] of a list of float64 S/N arrays."""
    nb64 = (n + 63) // 64
    best = np.zeros((len(snr), nb64))
    arg = np.full((len(snr), nb64), NONE, dtype=np.uint32)
    for k, (mx, am) in enumerate(ref.sp_block_maxima([s for s in snr])):
        best[k, :len(mx)] = mx
        arg[k, :len(am)] = am
    return best, arg


def _ratios(name, d, best):
    """Per width: the largest |best - oracle block maximum| / bound of row d."""
    o = _oracle(name)[d]
    out = {}
    for k, w in enumerate(o.widths):
        mx, _ = o.maxima[k]
        nb = len(mx)
        diff = np.abs(np.asarray(best[k, :nb], dtype=np.float64) - mx)
        bb = o.blockbound[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0, 0.0, diff / bb)
        out[w] = float(np.max(r)) if nb else 0.0
    return out


def _params(c, thresh=1e30, capacity=1 << 16):
    p = C.SpParams()
    p.tsamp, p.min_snr, p.boxcar_max, p.baseline_samples, p.capacity = 1e-3, thresh, c.wmax, c.baseline, capacity
    return p


def _assert_dense(name, best, arg, tag="gpu"):
    """Shapes, validity and argmax of a dense output, and every block maximum
    within the derived bound of the oracle's.  Prints the largest ratio per
    width."""
    c = _cases()[name]
    rows = range(c.rows.shape[0])
    n = c.n
    widths = ref.sp_widths(n, c.wmax)
    assert C.sp_widths(n, c.wmax) == widths
    assert best.shape == arg.shape == (len(rows), len(widths), (n + 63) // 64)
    assert np.isfinite(best).all()
    worst = {}
    for j, d in enumerate(rows):
        o = _oracle(name)[d]
        for k, w in enumerate(widths):
            mx, _ = o.maxima[k]
            nb = len(mx)
            assert nb == (n - w + 1 + 63) // 64
            a = arg[j, k, :nb].astype(np.int64)
            assert np.array_equal(a // 64, np.arange(nb)) and (a + w <= n).all(), (name, d, w)
            assert (best[j, k, nb:] == 0).all() and (arg[j, k, nb:] == NONE).all()
            # the oracle's S/N at the kernel's argmax is the oracle's block maximum, within both bounds
            assert (mx - o.snr[k][a] <= o.bound[k][a] + o.blockbound[k]).all(), (name, d, w)
        for w, r in _ratios(name, d, best[j]).items():
            worst[w] = max(worst.get(w, 0.0), r)
    for w, r in sorted(worst.items()):
        print(f"sp-ratio {tag} {name} w={w} {r:.4f}")
    bad = {w: r for w, r in worst.items() if not r <= 1.0}
    assert not bad, (name, bad)


# ------------------------------------------------------------------- CPU ----
def test_sp_baseline_samples_matches_transcription():
    def expect(baseline_s, tsamp, samples, n):
        b = samples if samples else int(math.ceil(baseline_s / tsamp))
        return min(max(b, 64), n)

    for baseline_s, tsamp, samples, n in [(2.0, 64e-6, 0, 1 << 20), (2.0, 64e-6, 0, 31250), (2.0, 64e-6, 0, 31249),
                                          (2.0, 1e-3, 0, 70001), (0.5, 3e-4, 0, 70001), (1e-3, 1e-3, 0, 5000),
                                          (0.0635, 1e-3, 0, 5000), (0.0641, 1e-3, 0, 5000), (2.0, 1e-3, 0, 64),
                                          (2.0, 1e-3, 100, 5000), (2.0, 1e-3, 1, 5000), (2.0, 1e-3, 9999, 5000),
                                          (1.0, 1.0 / 3.0, 0, 100), (2.0, 1e-3, 63, 64)]:
        p = C.SpParams()
        p.tsamp, p.baseline_s, p.baseline_samples = tsamp, baseline_s, samples
        assert C.sp_baseline_samples(p, n) == expect(baseline_s, tsamp, samples, n), (baseline_s, tsamp, samples, n)
    p = C.SpParams()
    p.tsamp, p.baseline_s = 64e-6, 2.0
    assert C.sp_baseline_samples(p, 1 << 20) == 31250
    p.tsamp, p.baseline_s = 1e-3, 1e-3
    assert C.sp_baseline_samples(p, 5000) == 64 and C.sp_baseline_samples(p, 64) == 64


@functools.lru_cache(maxsize=None)
def _emulated(name):
    c = _cases()[name]
    K = _kmax(c.n, c.wmax)
    outs = [ref.sp_search_f32(c.rows[d, :c.n], c.baseline, K) for d in range(c.rows.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


@pytest.mark.parametrize("name", list(_cases()))
def test_f32_emulation_stays_inside_the_bound(name):
    best, arg = _emulated(name)
    _assert_dense(name, best, arg, tag="emulation")


# Defects, as variants of the float64 oracle.
def _defect_snr(u8, baseline, widths, defect, kmax):
    u = np.asarray(u8)
    n = len(u)
    sums, counts = ref.sp_block_means(u, baseline)
    M = sums / counts.astype(np.float64)
    nblk = len(M)
    i = np.arange(n, dtype=np.float64)
    if nblk == 1:
        trend = np.full(n, M[0])
    else:
        centres = np.arange(nblk) * float(baseline) + 0.5 * baseline
        if defect == "trend_half_sample":
            centres = centres - 0.5
        if defect == "last_block_own_centre":
            centres[-1] = (nblk - 1) * float(baseline) + 0.5 * counts[-1]
        trend = np.interp(i, centres, M)
        if defect == "pos_truncated_low" and baseline % 2 == 0:
            for j in range(1, nblk):
                s = j * baseline + baseline // 2  # an exact centre: pos == j
                if s < n:
                    trend[s] = M[j - 1]
    x = u.astype(np.float64) - trend
    sigma = math.sqrt(float((x * x).sum()) / ((n - 1) if defect == "sigma_n_minus_1" else n))
    c = np.concatenate([[0.0], np.cumsum(x)])
    out = []
    for w in widths:
        lo = np.arange(n + 1 - w)
        hi = lo + w
        if defect == "halo_one_level_short":
            hi = np.minimum(hi, lo // T * T + T + (1 << kmax) // 2)  # the tile sees zeros past T + H / 2
        s = c[hi] - c[lo]
        if defect == "last_start_one_short":
            s = s[:-1]
        ww = 2 * w if defect == "scale_of_next_level" else w
        out.append(s / (sigma * math.sqrt(ww)) if sigma > 0 else np.zeros_like(s))
    return out


DEFECTS = {  # defect -> the cases that must catch it
    "sigma_n_minus_1": ["nlim-64", "nlim-129", "nlim-8193"],
    "trend_half_sample": ["trend-385-64", "trend-1050-100", "trend-31251-31250"],
    "last_block_own_centre": ["trend-385-64", "trend-1000-999", "trend-31251-31250", "trend-1050-100"],
    "pos_truncated_low": ["trend-1000-64", "trend-1050-100", f"trend-{2 * T + 37}-4096"],
    "halo_one_level_short": [f"depth-{w}" for w in DEPTH_WMAX],
    "last_start_one_short": [f"last-{n}-{w}" for n, w, _ in LAST],
    "scale_of_next_level": ["depth-4", "depth-4096", "nlim-64"],
}


def _defect_worst(name, defect):
    c = _cases()[name]
    widths = ref.sp_widths(c.n, c.wmax)
    worst = 0.0
    for d in range(c.rows.shape[0]):
        snr = _defect_snr(c.rows[d, :c.n], c.baseline, widths, defect, len(widths) - 1)
        best, _ = _dense_from_snr(snr, c.n)
        worst = max(worst, max(_ratios(name, d, best).values()))
    return worst


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defective_oracles_leave_the_bound(defect):
    """Every case named for the defect differs from the true oracle by more
    than twice the bound in some block maximum: the dense comparison of this
    module fails on each of them."""
    for name in DEFECTS[defect]:
        r = _defect_worst(name, defect)
        assert r > 2.0, (defect, name, r)
    # and the true oracle, through the same path, is inside
    name = DEFECTS[defect][0]
    c = _cases()[name]
    for d in range(c.rows.shape[0]):
        best, _ = _dense_from_snr(_oracle(name)[d].snr, c.n)
        assert max(_ratios(name, d, best).values()) == 0.0


def test_halo_defect_is_caught_at_every_depth():
    """Row 2 of a depth case puts its widest boxcar's maximum at start T - 1,
    which needs all H samples of halo: one level short fails for every K."""
    for wmax in DEPTH_WMAX:
        name = f"depth-{wmax}"
        c = _cases()[name]
        widths = ref.sp_widths(c.n, c.wmax)
        snr = _defect_snr(c.rows[2, :c.n], c.baseline, widths, "halo_one_level_short", len(widths) - 1)
        best, _ = _dense_from_snr(snr, c.n)
        assert _ratios(name, 2, best)[widths[-1]] > 2.0, name
        o = _oracle(name)[2]
        assert o.maxima[-1][1][(T - 1) // 64] == T - 1


# ----------------------------------------------------- exact (tie) rows ----
def _exact_rows():
    """Rows of 100 +- sigma with as many of either sign (integer mean, sigma a
    power of two), one trend block: period 2 (ties among a thread's four
    starts at width 1, whole blocks of ties at every wider width), period 16
    (ties 16 starts apart: across the lanes of a row), the same at sigma 2 and
    4, and two seeded balanced shuffles."""
    n = T + 208  # a multiple of 16: whole periods
    i = np.arange(n)
    rng = np.random.default_rng(16)
    p2 = np.where(i % 2 == 0, 1, -1)
    p2r = -p2
    p16 = np.where(i % 16 < 8, 1, -1)
    p16b = np.where((i + 5) % 16 < 8, 1, -1)
    sh = np.array([1, -1] * (n // 2))
    sh1, sh2 = rng.permutation(sh), rng.permutation(sh)
    xs = [100 + p2, 100 + p2r, 100 + p16, 100 + 2 * p16b, 100 + 4 * sh1, 100 + sh2, 100 + 2 * p2, 37 + sh1]
    return n, _pack([x.astype(np.float64) for x in xs], n)


@functools.lru_cache(maxsize=None)
def _exact_oracle():
    n, rows = _exact_rows()
    widths = ref.sp_widths(n, 4096)
    out = []
    for d in range(rows.shape[0]):
        ex = ref.sp_boxcar_snr_exact(rows[d, :n], widths)
        nb64 = (n + 63) // 64
        best = np.zeros((len(widths), nb64), dtype=np.float32)
        arg = np.full((len(widths), nb64), NONE, dtype=np.uint32)
        arg_hi = arg.copy()
        for k, s in enumerate(ex["sums"]):
            for b in range((len(s) + 63) // 64):
                seg = s[b * 64:(b + 1) * 64]
                j = int(np.argmax(seg))  # the first maximum of the exact integer sums
                best[k, b], arg[k, b] = ex["snr32"][k][b * 64 + j], b * 64 + j
                arg_hi[k, b] = b * 64 + len(seg) - 1 - int(np.argmax(seg[::-1]))
        out.append((best, arg, arg_hi))
    return n, rows, widths, out


def test_exact_rows_tie_inside_threads_and_across_lanes():
    n, rows, widths, out = _exact_oracle()
    ex = ref.sp_boxcar_snr_exact(rows[0, :n], widths)
    s1 = ex["sums"][0]
    assert s1[0] == s1[2] == s1[:4].max()  # width 1, period 2: a tie among one thread's four starts
    ex = ref.sp_boxcar_snr_exact(rows[2, :n], widths)
    s8 = ex["sums"][3]
    assert s8[0] == s8[16] == s8[32] == s8[:64].max() and (s8[1:16] < s8[0]).all()  # ties 4 lanes apart
    # "highest index on a tie" differs from the rule in the exact outputs
    assert all((arg != arg_hi).any() for (_, arg, arg_hi) in out)
    # the tolerance-based oracle agrees with the exact one
    snr = ref.sp_boxcar_snr(rows[4, :n], n, widths)
    ex = ref.sp_boxcar_snr_exact(rows[4, :n], widths)
    for k in range(len(widths)):
        np.testing.assert_allclose(snr[k], ex["snr"][k], rtol=0, atol=1e-9)


def test_f32_emulation_equals_exact_oracle():
    n, rows, widths, out = _exact_oracle()
    for d, (best, arg, _) in enumerate(out):
        ebest, earg = ref.sp_search_f32(rows[d, :n], n, len(widths) - 1)
        assert np.array_equal(earg, arg), d
        assert np.array_equal(ebest.view(np.uint32), best.view(np.uint32)), d


def _records_from_dense(best, arg, thresh, dm_idx0=0, strict=False):
    """{(d, k, arg, best) : best >= thresh} of a dense output, in record order."""
    out = []
    for d in range(best.shape[0]):
        for k in range(best.shape[1]):
            for b in range(best.shape[2]):
                if arg[d, k, b] == NONE:
                    continue
                v = best[d, k, b]
                if (v > thresh) if strict else (v >= thresh):
                    out.append((d + dm_idx0, k, int(arg[d, k, b]), float(v)))
    return sorted(out, key=lambda t: t[:3])


def _record_thresholds(best, arg):
    """A value that occurs (about 40 records at or above it), its float32
    neighbour above, and the middle of the gap to the next value above."""
    vals = np.unique(best[arg != NONE])
    assert len(vals) > 60
    v = vals[-40]
    up = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
    assert vals[-39] > up
    mid = np.float32(0.5 * (float(v) + float(vals[-39])))
    assert v < mid < vals[-39]
    return [float(v), float(up), float(mid)]


def test_threshold_defect_changes_the_records():
    best, arg = _emulated("depth-4096")
    for t in _record_thresholds(best, arg)[:1]:
        a, b = _records_from_dense(best, arg, t), _records_from_dense(best, arg, t, strict=True)
        assert len(a) == len(b) + 1  # '>' loses exactly the record at the threshold
    t_at, t_up, _ = _record_thresholds(best, arg)
    assert len(_records_from_dense(best, arg, t_up)) == len(_records_from_dense(best, arg, t_at)) - 1


def test_last_start_is_the_strict_maximum_by_twice_the_bound():
    for nn, wmax, _ in LAST:
        name = f"last-{nn}-{wmax}"
        c = _cases()[name]
        for k, w in enumerate(ref.sp_widths(c.n, c.wmax)):
            assert _last_start_margin(name, k, w) > 2.0, (name, w)


def _last_start_margin(name, k, w):
    """(oracle S/N at start n - w - the largest other S/N of its block) / bound, row k."""
    c = _cases()[name]
    o = _oracle(name)[k]
    s, a = o.snr[k], c.n - w
    seg = s[a // 64 * 64:a]  # the block's other starts all lie before n - w
    other = seg.max() if len(seg) else -np.inf
    return (s[a] - other) / o.blockbound[k][a // 64]


# ------------------------------------------------------------------- GPU ----
def _run(name, **kw):
    c = _cases()[name]
    return C.sp_search_rows(c.rows, c.n, _params(c, **kw), dense=True)


def _dense_case(name):
    events, reruns, best, arg = _run(name)
    assert events == [] and reruns == 0
    _assert_dense(name, best, arg)
    return best, arg


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("depth-"))
def test_sp_every_ladder_depth(name):
    _dense_case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("nlim-"))
def test_sp_depth_limited_by_n(name):
    best, _ = _dense_case(name)
    c = _cases()[name]
    assert best.shape[1] == len(ref.sp_widths(c.n, 4096)) == min(12, int(math.log2(c.n // 2))) + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("edge-"))
def test_sp_tile_and_halo_edges(name):
    _dense_case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("last-"))
def test_sp_last_valid_start(name):
    c = _cases()[name]
    _, arg = _dense_case(name)
    for k, w in enumerate(ref.sp_widths(c.n, c.wmax)):
        assert _last_start_margin(name, k, w) > 2.0
        assert arg[k, k, (c.n - w) // 64] == c.n - w, (name, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("trend-"))
def test_sp_trend_means_sigma_and_search(name):
    c = _cases()[name]
    means, partials = C.sp_trend_sigma_rows(c.rows, c.n, c.baseline)
    ndm = c.rows.shape[0]
    nblk = (c.n + c.baseline - 1) // c.baseline
    assert means.shape == (ndm, nblk) and means.dtype == np.float32
    assert partials.shape == (ndm, 64) and partials.dtype == np.float64
    span = (c.n + 63) // 64
    for d in range(ndm):
        u = c.rows[d, :c.n]
        sums, counts = ref.sp_block_means(u, c.baseline)
        exp = (sums.astype(np.float64) / counts.astype(np.float64)).astype(np.float32)
        assert np.array_equal(means[d].view(np.uint32), exp.view(np.uint32)), (name, d)
        sigma = ref.sp_sigma(u, c.baseline)
        rel = ref.sp_sigma_rel_bound(u, c.baseline)
        got = math.sqrt(partials[d].sum() / c.n)
        print(f"sp-sigma {name} row {d} {abs(got - sigma) / (rel * sigma):.4f}")
        assert abs(got - sigma) <= rel * sigma, (name, d, got, sigma)
        empty = np.arange(64) * span >= c.n
        assert (partials[d][empty] == 0).all() and (partials[d][~empty] > 0).all()
    _dense_case(name)


@pytest.mark.gpu
def test_sp_extremes():
    name = "extremes"
    c = _cases()[name]
    events, reruns, best, arg = _run(name, thresh=3.0)
    _assert_dense(name, best, arg)
    for d in EXTREME_DEAD:
        assert (best[d] == 0).all()
    got = [e.astuple() for e in events]
    assert got == _records_from_dense(best, arg, np.float32(3.0))
    assert got and not any(d in EXTREME_DEAD for (d, _, _, _) in got)
    # the spike row: S/N close to sqrt(n) at width 1
    assert best[5, 0].max() > 0.99 * math.sqrt(c.n)
    for d in EXTREME_LIVE:
        ev1, _, best1, arg1 = C.sp_search_rows(c.rows[d:d + 1], c.n, _params(c, thresh=3.0), dense=True, dm_idx0=d)
        assert np.array_equal(best1[0].view(np.uint32), best[d].view(np.uint32)) and np.array_equal(arg1[0], arg[d])
        assert [e.astuple() for e in ev1] == [t for t in got if t[0] == d]


@pytest.mark.gpu
def test_sp_row_indexing():
    name = "rows-33"
    c = _cases()[name]
    events, _, best, arg = _run(name, thresh=3.0)
    _assert_dense(name, best, arg)
    got = [e.astuple() for e in events]
    assert got == _records_from_dense(best, arg, np.float32(3.0)) and len({t[0] for t in got}) > 20
    means, partials = C.sp_trend_sigma_rows(c.rows, c.n, c.baseline)
    single = []
    for d in range(c.rows.shape[0]):
        ev1, _, best1, arg1 = C.sp_search_rows(c.rows[d:d + 1], c.n, _params(c, thresh=3.0), dense=True, dm_idx0=d)
        assert np.array_equal(best1[0].view(np.uint32), best[d].view(np.uint32)) and np.array_equal(arg1[0], arg[d]), d
        single += [e.astuple() for e in ev1]
        m1, p1 = C.sp_trend_sigma_rows(c.rows[d:d + 1], c.n, c.baseline)
        assert np.array_equal(m1[0], means[d]) and np.array_equal(p1[0], partials[d]), d
    assert single == got


@pytest.mark.gpu
def test_sp_ties_resolve_to_the_lowest_index_exactly():
    n, rows, widths, out = _exact_oracle()
    p = C.SpParams()
    p.tsamp, p.min_snr, p.boxcar_max, p.baseline_samples = 1e-3, 1e30, 4096, n
    _, _, best, arg = C.sp_search_rows(rows, n, p, dense=True)
    assert best.shape == (rows.shape[0], len(widths), (n + 63) // 64)
    for d, (ebest, earg, _) in enumerate(out):
        assert np.array_equal(arg[d], earg), d
        assert np.array_equal(best[d].view(np.uint32), ebest.view(np.uint32)), d


@pytest.mark.gpu
def test_sp_records_are_the_thresholded_dense_output():
    name = "depth-4096"
    c = _cases()[name]
    _, _, best, arg = _run(name)
    counts = []
    for t in _record_thresholds(best, arg):
        exp = _records_from_dense(best, arg, np.float32(t))
        counts.append(len(exp))
        E = len(exp)
        assert E > 8
        for capacity, reruns_ok in [(1 << 16, lambda r: r == 0), (E, lambda r: r == 0), (E - 1, lambda r: r == 1),
                                    (1, lambda r: r >= 1)]:
            ev, reruns, _, _ = C.sp_search_rows(c.rows, c.n, _params(c, thresh=t, capacity=capacity), dense=False)
            assert reruns_ok(reruns), (t, capacity, reruns)
            assert [e.astuple() for e in ev] == exp, (t, capacity)
    assert counts[1] == counts[0] - 1 and counts[2] == counts[1]
