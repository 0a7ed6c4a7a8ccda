"""SearchEngine's candidates against a float64 oracle of the whole DM trial.

Under test: everything SearchEngine::search_trial / search_prepared /
search_prepared_many make of their stages (engine.cpp): the per-level search
ranges, bin_width and the per-level factor, the flat trial list (series,
acceleration and whitening stats per batch slot), the mean and sigma handed to
the spectrum pass, and the hand-over from cluster peaks to Candidates and on
to the two distillers.  The oracle (utils/reference.py search_trial64 and its
pieces search_levels64 / search_candidates64) is the search from its
definition: whiten64 -> n irfft(D) -> search_spectrum per acceleration at
(mean, std) n -> float64 harmonic sums -> crossings strictly above min_snr
inside peak_bounds -> unique_peaks -> (dm, dm_idx, acc, nh, snr, float32(idx
factor)) -> the Python harmonic distiller per trial -> the Python acceleration
distiller per DM.  tobs, bin_width, the ranges, the threshold, the frequency
and the distillers' tolerances are float32 where the engine forms them so.

Rule (GPU tests): the engine's list equals the oracle's in length, order,
(dm, dm_idx, acc, nh, freq) bit for bit and count_assoc(); snr within TOL.

Inputs: uint8 trials rint(N(128, 6)) clipped, one seed per case: pure noise,
and noise plus two trains of one-sample pulses (and one of six-sample pulses),
the second accelerated so that it peaks at trial 6 of the 9-trial list;
amplitudes and accelerations scale with the length so that S/N and shift in
samples are those of 2^15.  One zap entry (the second harmonic of
the first train) is in every case's parameters.  Acceleration lists (_accs)
are symmetric about 0 and include 0, up to +-A_MAX, which moves the read
position by SHIFT_15 = 8.6 samples at 2^15 (an even count adds 0.4321 A_MAX at
the end).  test_search_spectrum_exact's ACCS[15] holds no "safe" value between
a shift of 0.5 and of 2457 samples, so the values are this module's own and
test_accelerations_are_safe holds every one used, at every length used, to
that module's "safe" rule (no read position within 1e-6 of a rounding tie).

min_snr per case is the midpoint of the widest gap between consecutive sorted
oracle level values (all levels, all trials) within WINDOW of the case's
wanted threshold.  With G = 1e-2, test_conditions_hold_for_the_committed_seeds
asserts per case that no level value lies within G of min_snr, that every
cluster's peak exceeds its runner-up by G, that no two candidates which the
harmonic (per trial) or the acceleration (per DM) relation joins in either
direction are within G in S/N -- and, because both distillers sort by S/N and
the rule compares the order, that no two candidates of one distiller input
are within ORDER_GAP = 2 x the S/N cap of each other.  Across the cases it
asserts >= 3 candidates on every level 0..5, a cluster of >= 10 crossings,
candidates lost to each distiller, a crossing within two bins of a level's
start and a case whose highest searched bin lies below nb.

Defective oracles (test_defective_oracles_change_the_candidates): start[h] +
1, end[h] - 1, trial k at the acceleration of trial k + 1, another series'
stats, level scales from the next level, no 2^(h-1) in the index, factor
without 2^-h, min_gap - 1.  Each must change the candidate list of at least
one of DEFECT_CASES at that case's own min_snr (the number of cases changed is
printed).  Two do NOT: start + 1 and end - 1 change no list (4 -> 4, 4 -> 4,
4 -> 4, 5 -> 5, 1 -> 1 candidates), because no cluster of these cases peaks on
the first or last bin of a range and a crossing there only joins a cluster
that peaks further in; the min_freq 209.45 case does put crossings within two
bins of start (asserted).  Their test prints the figures and asserts nothing;
a range off by one shows only where a peak sits on the edge.

FFT paths not covered: rows_ext exists only from 2^26 and is out of scope, as
are odd lengths and the multi-rank drivers (their engine calls are these).

Tolerance on S/N, per level h: min(4 x MEASURED[h], cap), cap = 2^(h/2)
(test_search_spectrum_exact.TOL_CAP[0] + test_whiten_exact.TOL_CAP[0]) +
2^-20 |snr| (one bin of P summed over 2^h bins and scaled by 2^(-h/2); the
whitened spectrum likewise; bright lines and the float32 stats).  Every
tolerance is below G / 10 (asserted).

Measured |snr_gpu - snr_oracle| (MI355X, worst over every GPU case of this
module, as of its first commit):

    level   max error   candidates
      0     5.34e-06     3   (nharmonics 1)
      1     5.22e-06     5   (three DMs in one flat list, raw, job 2)
      2     5.70e-06    14   (fft_size 3 * 2^14)
      3     7.52e-06    82   (nharmonics 3)
      4     1.14e-05   202   (fft_size 2^17)
      5     3.61e-06     3   (max_freq 200)

The engine agreed with the oracle on every axis in candidates, order,
frequencies and associations.  Two faults of the glue were found and fixed
with this module, both a refusal to search rather than a wrong candidate:
  * min_freq beyond a level's last bin (min_freq 209.45 at 2^15: level 5
    would start at bin 28110 of 16385).  The empty range's start went into
    hi_, the highest searched bin, and the spectrum pass refused nbins_out >
    M + 1.  Empty ranges no longer count towards hi_.
  * fft_size 3 * 2^14: the four-step geometry does not exist, the engine fell
    back to fft_mode 1, whose fused r2c indexes by powers of two and refused
    M = 3 * 2^13.  Such lengths now take fft_mode 0 (asserted below).
"""
import collections
import functools
import types

import numpy as np
import pytest
from test_search_spectrum_exact import TOL_CAP as SPECTRUM_CAP
from test_search_spectrum_exact import _tie_distance
from test_whiten_exact import TOL_CAP as WHITEN_CAP

from peasoup_amd.utils import reference as ref

dev = "cuda"
TSAMP = 64e-6
N15, N16, N17, N3 = 1 << 15, 1 << 16, 1 << 17, 3 << 14
G = 1e-2
WINDOW = 0.5
A_MAX = 300000.0
SHIFT_15 = 8.6  # samples at the centre of a 2^15 series at A_MAX

# largest |snr_gpu - snr_oracle| per level (module docstring)
MEASURED = {0: 5.335e-6, 1: 5.218e-6, 2: 5.700e-6, 3: 7.520e-6, 4: 1.135e-5, 5: 3.614e-6}


def snr_cap(h, snr):
    return 2.0 ** (0.5 * h) * (SPECTRUM_CAP[0] + WHITEN_CAP[0]) + 2.0 ** -20 * abs(snr)


def snr_tol(h, snr):
    cap = snr_cap(h, snr)
    return cap if MEASURED[h] is None else min(4.0 * MEASURED[h], cap)


ORDER_GAP = 2.0 * snr_cap(5, 64.0)

# ------------------------------------------------------------------ inputs --
# name -> ([(period in samples, pulse width in samples, amplitude, index into _accs(9) of its acceleration)],
# dm, dm_idx).  One-sample pulses spread over every harmonic below Nyquist and peak on the top level, the
# six-sample ones lower.
TRIALS = {
    "noise": ([], 0.0, 0),
    "pulses": ([(37.3, 1, 5.0, 4), (53.71, 1, 4.5, 6), (97.7, 6, 1.6, 4)], 10.0, 3),
    "pulses2": ([(41.9, 1, 4.5, 4), (61.3, 1, 5.0, 2)], 23.5, 7),
}
EXTRA = 1013  # samples past n in every row


def _accs(K, n=N15):
    """The list scales with (2^15 / n)^2, so A_MAX shifts by SHIFT_15 samples at every length.  Neighbouring trials must differ by a shift of about a sample, or they resample alike and their candidates
    tie in S/N: the 40-trial list spans +-3.1 A_MAX."""
    m = K if K % 2 else K - 1
    amax = (A_MAX if K <= 17 else 3.1 * A_MAX) * (float(N15) / n) ** 2
    v = [0.0] if m == 1 else [amax * (2.0 * j / (m - 1) - 1.0) for j in range(m)]
    if K % 2 == 0:
        v.append(0.4321 * amax)
    return [float(np.float32(a)) for a in v]


@functools.lru_cache(maxsize=None)
def _trial(name, n, seed):
    """uint8 [n + EXTRA]: rint(N(128, 6)) plus one-sample pulses, periodic in the index that resample_ii at the
    train's acceleration reads (to first order in the shift), clipped"""
    trains, _, _ = TRIALS[name]
    length = n + EXTRA
    x = np.random.default_rng(seed).normal(128.0, 6.0, length)
    j = np.arange(length, dtype=np.float64)
    for period, width, amp, k in trains:
        af = ref.accel_factor(_accs(9, n)[k], TSAMP)
        ph = (j - af * j * (j - n)) / period
        x = x + amp * np.sqrt(float(N15) / n) * ((ph % 1.0) < width / period)  # the same S/N at every length
    r = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    r.setflags(write=False)
    return r


ZAP = ([float(np.float32(2.0 / (37.3 * TSAMP)))], [float(np.float32(1.5))])
BASE = dict(tsamp=TSAMP, min_freq=0.1, max_freq=1100.0, nharmonics=4, freq_tol=1e-4, max_harm=16,
            boundary_5_freq=0.05, boundary_25_freq=0.5, zap_freqs=ZAP[0], zap_widths=ZAP[1], min_gap=30)

Case = collections.namedtuple("Case", "trial seed n nsamps K wanted over")


def case(seed, trial="pulses", n=N15, nsamps=None, K=9, wanted=6.0, **over):
    return Case(trial, seed, n, n if nsamps is None else nsamps, K, wanted, tuple(sorted(over.items())))


def _params(c, min_snr=None):
    p = types.SimpleNamespace(**BASE)
    p.fft_size = c.n
    for k, v in c.over:
        setattr(p, k, v)
    p.min_snr = c.wanted - WINDOW if min_snr is None else min_snr
    return p


@functools.lru_cache(maxsize=None)
def _levels(c):
    return ref.search_levels64(_trial(c.trial, c.n, c.seed), c.nsamps, _params(c), _accs(c.K, c.n), c.wanted - WINDOW)


def _level_values(lev):
    return np.concatenate([v for rows in lev["trials"] for (_, v) in rows])


def _threshold_from_oracle(levs, wanted):
    """Midpoint of the widest gap between consecutive sorted oracle level values within WINDOW of `wanted`,
    as float32 (the engine's min_snr)"""
    vals = np.sort(np.concatenate([_level_values(lev) for lev in levs]))
    vals = vals[(vals > wanted - WINDOW) & (vals < wanted + WINDOW)]
    assert len(vals) >= 2
    gaps = np.diff(vals)
    i = int(np.argmax(gaps))
    return ref.f32(0.5 * (vals[i] + vals[i + 1]))


@functools.lru_cache(maxsize=None)
def _oracle(c, raw=False, group=None):
    """The oracle of case c at the min_snr of its group (an engine has one min_snr for all its jobs): the
    cases whose pooled level values the threshold is taken from, default c alone."""
    lev = _levels(c)
    _, dm, dm_idx = TRIALS[c.trial]
    thr = _threshold_from_oracle([_levels(x) for x in (group or (c,))], c.wanted)
    return ref.search_candidates64(lev, _params(c, thr), thr, dm, dm_idx, raw)


def _sig(cands):
    return [(c.dm_idx, c.acc, c.nh, c.freq, len(c.assoc)) for c in cands]


# ------------------------------------------------------------------- cases --
# The seed of each case is the first of 1, 2, ... at which check_conditions holds for it.
BASE_CASE = case(10)
NOISE_CASE = case(1, "noise")
NH_SEEDS = {0: 1, 1: 13, 2: 1, 3: 8, 4: 10, 5: 10}  # (1: the first with three candidates on level 1)
NH_CASES = {nh: case(NH_SEEDS[nh], nharmonics=nh) for nh in (0, 1, 2, 3, 4, 5)}
# a quarter of Nyquist is 1953 Hz: levels 0 and 1 end below the last bin, level 2 reaches it
RANGE_CASES = {"default": BASE_CASE, "max_freq 2000": case(14, max_freq=2000.0),
               # start = 4.194 min_freq 2^h: 14055 at level 4, one bin below the first train's fundamental
               "min_freq 209.45": case(1, min_freq=209.45, nharmonics=5),
               # every level ends below nb = 16385 (13421 at level 5): the pruned spectrum
               "max_freq 200": case(8, max_freq=200.0, nharmonics=5)}
NSAMPS_CASES = {"n": BASE_CASE, "0.8 n": case(14, nsamps=int(0.8 * N15)), "n + 1000": case(10, nsamps=N15 + 1000)}
GAP_CASES = {30: BASE_CASE, 5: case(10, min_gap=5), 31: case(10, min_gap=31)}
BATCH_CASES = {1: case(1, K=1), 7: case(10, K=7), 8: case(10, K=8), 9: BASE_CASE, 17: case(1, K=17, wanted=7.0),
               40: case(1, K=40, wanted=9.0)}
LENGTH_CASES = {N16: case(24, n=N16), N17: case(1, n=N17), N3: case(2, n=N3)}
MULTI_CASES = (case(1, "pulses", K=5), case(101, "noise"), case(201, "pulses2", K=3))  # one engine, one min_snr
ALL_CASES = list(dict.fromkeys([NOISE_CASE] + list(NH_CASES.values()) + list(RANGE_CASES.values()) +
                               list(NSAMPS_CASES.values()) + list(GAP_CASES.values()) + list(BATCH_CASES.values()) +
                               list(LENGTH_CASES.values())))
# (case, the group its threshold comes from or None)
ALL_ORACLES = [(c, None) for c in ALL_CASES] + [(c, MULTI_CASES) for c in MULTI_CASES]
DEFECT_CASES = [BASE_CASE, NH_CASES[5], RANGE_CASES["min_freq 209.45"], RANGE_CASES["max_freq 200"], NOISE_CASE]


# --------------------------------------------------------------- CPU tests --
def _close_pairs(cands, gap):
    """index pairs (i < j in descending S/N) of candidates within `gap` in S/N"""
    order = sorted(range(len(cands)), key=lambda i: -cands[i].snr)
    out = []
    for a, i in enumerate(order):
        for j in order[a + 1:]:
            if cands[i].snr - cands[j].snr >= gap:
                break
            out.append((i, j))
    return out


def _harm_joined(p, a, b):
    return any(ref.harm_related(x.freq, [y.freq], [y.nh], p.freq_tol, ref.f32(p.max_harm), True)[0]
               for x, y in ((a, b), (b, a)))


def _acc_joined(p, tobs, a, b):
    return any(ref.acc_related(x.freq, x.acc, y.freq, y.acc, tobs, p.freq_tol) for x, y in ((a, b), (b, a)))


def _case_id(c):
    return "-".join(map(str, c[:6])) + "".join(f"-{k}={v}" for k, v in c.over)


@pytest.mark.parametrize("c,group", ALL_ORACLES, ids=[_case_id(c) + ("-multi" if g else "") for c, g in ALL_ORACLES])
def test_conditions_hold_for_the_committed_seeds(c, group):
    check_conditions(c, group)


def check_conditions(c, group=None):
    lev, res = _levels(c), _oracle(c, False, group)
    p = _params(c, res["min_snr"])
    thr = res["min_snr"]
    vals = _level_values(lev)
    assert abs(thr - c.wanted) < WINDOW and thr - G > lev["floor"]
    assert not len(vals) or np.abs(vals - thr).min() >= G, "a level value within G of min_snr"
    for cl in res["clusters"]:
        for level in cl:
            for _, peak, second, _ in level:
                assert peak - second >= G, "a cluster whose two largest crossings are within G"
    for trial in res["harm_in"]:
        for i, j in _close_pairs(trial, G):
            assert not _harm_joined(p, trial[i], trial[j]), "harmonically related cluster peaks within G in S/N"
        assert not _close_pairs(trial, ORDER_GAP), "the harmonic distiller's order hangs on float32 rounding"
    per_dm = [x for t in res["per_trial"] for x in t]
    for i, j in _close_pairs(per_dm, G):
        assert not _acc_joined(p, lev["tobs"], per_dm[i], per_dm[j]), "acceleration-related candidates within G"
    assert not _close_pairs(per_dm, ORDER_GAP), "the acceleration distiller's order hangs on float32 rounding"
    for x in per_dm:
        assert snr_tol(x.nh, x.snr) <= snr_cap(x.nh, x.snr) < G / 10
    print(f"ENGINE_ORACLE {c}: min_snr {thr:.4f} crossings {int((vals > thr).sum())} "
          f"clusters {sum(len(t) for t in res['harm_in'])} after harmonic {len(per_dm)} final {len(res['cands'])} "
          f"by level {np.bincount([x.nh for x in res['cands']], minlength=6)}")


def test_the_cases_cover_what_the_engine_can_get_wrong():
    by_level = np.zeros(6, dtype=int)
    biggest, harm_lost, acc_lost, near_start, pruned = 0, 0, 0, 0, 0
    for c, group in ALL_ORACLES:
        lev, res = _levels(c), _oracle(c, False, group)
        by_level += np.bincount([x.nh for x in res["cands"]], minlength=6)
        biggest = max([biggest] + [k[3] for cl in res["clusters"] for level in cl for k in level])
        harm_lost += sum(len(a) > len(b) for a, b in zip(res["harm_in"], res["per_trial"]))
        acc_lost += sum(len(t) for t in res["per_trial"]) > len(res["cands"])
        for rows in lev["trials"]:
            for h, (idx, val) in enumerate(rows):
                s = lev["bounds"][h][0]
                near_start += int(s > 0 and ((idx[val > res["min_snr"]] - s) <= 2).any())
        pruned += max(e for _, e, _ in lev["bounds"]) < lev["nb"]
    print(f"ENGINE_ORACLE candidates by level {by_level}, largest cluster {biggest} crossings, trials that lose "
          f"candidates to the harmonic distiller {harm_lost}, DMs that lose to the acceleration distiller "
          f"{acc_lost}, (trial, level)s with a crossing within two bins of start {near_start}, pruned cases {pruned}")
    assert (by_level >= 3).all(), by_level
    assert biggest >= 10 and harm_lost >= 1 and acc_lost >= 1 and near_start >= 1 and pruned >= 1


def test_search_ranges_are_where_the_cases_say():
    su = ref.search_setup(_params(RANGE_CASES["max_freq 2000"]))
    ends = [e for _, e, _ in su["bounds"]]
    assert ends[0] < ends[1] < su["nb"] and ends[2] == su["nb"]
    su = ref.search_setup(_params(RANGE_CASES["min_freq 209.45"]))
    assert su["bounds"][su["nlevels"]][0] > 1000
    su = ref.search_setup(_params(RANGE_CASES["max_freq 200"]))
    assert max(e for _, e, _ in su["bounds"]) < su["nb"]
    su = ref.search_setup(_params(BASE_CASE))
    assert su["tobs"] == ref.f32(np.float32(N15) * np.float32(TSAMP)) and su["bin_width"] == ref.f32(1.0 / su["tobs"])


def test_accelerations_are_safe():
    used = sorted({(c.n, c.K) for c, _ in ALL_ORACLES})
    for n, K in used:
        accs = _accs(K, n)
        assert len(accs) == K and 0.0 in accs and len(set(accs)) == K
        m = K if K % 2 else K - 1
        assert accs[:m] == [-a for a in accs[:m][::-1]], "symmetric about 0"
        for a in accs:
            # beyond 2^15 a margin of 1e-6 is luck (2e-6 n samples lie that near a tie once the shift exceeds a
            # sample): there the floor is that module's "ulp" rule
            assert ref.f32(a) == a and _tie_distance(a, n) >= (1e-6 if n == N15 else 2e-8), (n, K, a)
    shift = abs(ref.accel_factor(A_MAX, TSAMP)) * N15 * N15 / 4
    assert abs(shift - SHIFT_15) < 0.05
    # the second train of "pulses" peaks at the trial of its own acceleration, which is not 0
    lev = _levels(BASE_CASE)
    f2 = 1.0 / (53.71 * TSAMP)
    best = []
    for rows in lev["trials"]:
        idx, val = rows[4]
        near = np.abs(idx * lev["bounds"][4][2] - f2) < 0.1
        best.append(val[near].max() if near.any() else 0.0)
    assert int(np.argmax(best)) == 6 and _accs(9)[6] != 0.0, best


def _defective(name, c):
    lev = _levels(c)
    p = _params(c, _oracle(c)["min_snr"])
    accs = _accs(c.K, c.n)
    kw, gap = {}, None
    b = list(lev["bounds"])
    if name == "start + 1":
        kw["bounds"] = [(s + 1, e, f) for s, e, f in b]
    if name == "end - 1":
        kw["bounds"] = [(s, e - 1, f) for s, e, f in b]
    if name == "acceleration of trial k + 1":
        kw["search_accs"] = accs[1:] + accs[:1]
    if name == "another series' stats":
        other = _levels(NOISE_CASE if c.trial != "noise" else BASE_CASE)["stats"]
        kw["stats"] = (other[0], other[2])
    if name == "scale of the next level":
        kw["scales"] = ref.LEVEL_SCALE[1:] + [0.125]
    if name == "no rounding term":
        kw["rounding"] = False
    if name == "factor without 2^-h":
        kw["bounds"] = [(s, e, b[0][2]) for s, e, f in b]
    if name == "min_gap - 1":
        gap = p.min_gap - 1
    dlev = ref.search_levels64(_trial(c.trial, c.n, c.seed), c.nsamps, p, accs, p.min_snr, **kw) if kw else lev
    _, dm, dm_idx = TRIALS[c.trial]
    return ref.search_candidates64(dlev, p, p.min_snr, dm, dm_idx, min_gap=gap)


DEFECTS = ["start + 1", "end - 1", "acceleration of trial k + 1", "another series' stats", "scale of the next level",
           "no rounding term", "factor without 2^-h", "min_gap - 1"]


DEFECT_NOTES = {
    "start + 1": "no cluster of these cases peaks on the first bin of a range, and a crossing there only joins a "
                 "cluster that peaks further in",
    "end - 1": "no cluster of these cases peaks on the last bin of a range",
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_defective_oracles_change_the_candidates(defect):
    changed = {}
    for c in DEFECT_CASES + ([GAP_CASES[5]] if defect == "min_gap - 1" else []):
        good, bad = _oracle(c)["cands"], _defective(defect, c)["cands"]
        same = _sig(good) == _sig(bad) and all(abs(a.snr - b.snr) <= snr_tol(a.nh, a.snr) for a, b in zip(good, bad))
        changed[c] = not same
        print(f"ENGINE_DEFECT {defect}: {len(good)} -> {len(bad)} candidates, changed {not same}: {c}")
    if defect in DEFECT_NOTES:  # changes nothing here (module docstring); the figures are printed, nothing is loosened
        print(f"ENGINE_DEFECT {defect}: {sum(changed.values())} of {len(changed)} cases change; {DEFECT_NOTES[defect]}")
        return
    assert any(changed.values()), f"{defect}: no case's candidate list changes"


def test_oracle_pieces_agree():
    """harmonic_levels64 against the float32 harmonic_sums, cluster_peaks64 against unique_peaks, the vectorised
    harmonic relation against its loop, search_trial64 against its two halves."""
    rng = np.random.default_rng(3)
    P = rng.normal(0, 1, 4099)
    L64 = ref.harmonic_levels64(P, 5)
    for h, L32 in enumerate(ref.harmonic_sums(P.astype(np.float32), 5), start=1):
        assert np.abs(L64[h] - L32).max() < 1e-4
    i = np.arange(len(P))
    assert np.allclose(L64[3], sum(P[(i * m + 4) >> 3] for m in range(1, 9)) / np.sqrt(8.0), atol=1e-12)
    idx = np.sort(rng.choice(5000, 400, replace=False))
    val = rng.uniform(6, 30, 400)
    for gap in (5, 30, 31):
        assert [(a, b) for a, b, _, _ in ref.cluster_peaks64(idx, val, gap)] == ref.unique_peaks(idx, val, gap)
        assert sum(k[3] for k in ref.cluster_peaks64(idx, val, gap)) == 400
    for f0, f, nh in ((10.0, 20.0, 1), (10.0, 5.0003, 3), (10.0, 5.002, 3), (7.0, 10.5, 1), (7.0, 10.5, 0)):
        loop = sum(1 for jj in range(1, 17) for kk in range(1, 2 ** nh + 1)
                   if 1 - ref.f32(1e-4) < kk * f / (jj * f0) < 1 + ref.f32(1e-4))
        assert ref.harm_related(f0, [f], [nh], 1e-4, 16.0, True)[0] == loop
    c = BASE_CASE
    res = _oracle(c)
    _, dm, dm_idx = TRIALS[c.trial]
    whole = ref.search_trial64(_trial(c.trial, c.n, c.seed), c.nsamps, _params(c, res["min_snr"]), _accs(c.K, c.n), dm, dm_idx)
    assert _sig(whole["cands"]) == _sig(res["cands"]) and [x.snr for x in whole["cands"]] == [x.snr for x in res["cands"]]
    raw = _oracle(c, True)
    assert [t[:4] for t in _sig(raw["cands"])] == [t[:4] for t in _sig([x for t in res["per_trial"] for x in t])]
    assert not any(x.assoc for x in raw["cands"])


# --------------------------------------------------------------- GPU tests --
def _search_params(c, group=None, **engine):
    import peasoup_amd._C as C

    o = _params(c, _oracle(c, False, group)["min_snr"])
    p = C.SearchParams()
    for k in ("fft_size", "tsamp", "min_snr", "min_freq", "max_freq", "nharmonics", "freq_tol", "max_harm",
              "boundary_5_freq", "boundary_25_freq", "zap_freqs", "zap_widths", "min_gap"):
        setattr(p, k, getattr(o, k))
    p.accel_batch = 8
    for k, v in engine.items():
        setattr(p, k, v)
    return p


def _engine(c, **engine):
    import torch

    import peasoup_amd._C as C

    return C.SearchEngine(_search_params(c, **engine), torch.cuda.current_stream().cuda_stream)


def _rows(cases):
    """the cases' trials as rows of one device buffer, 255 between them; (tensor, row stride)"""
    import torch

    n = cases[0].n
    rs = (n + EXTRA + 255) // 256 * 256
    buf = np.full((len(cases), rs), 255, dtype=np.uint8)
    for b, c in enumerate(cases):
        assert c.n == n
        buf[b, :n + EXTRA] = _trial(c.trial, n, c.seed)
    return torch.from_numpy(buf).to(dev), rs


def _job(b, c, raw=None):
    _, dm, dm_idx = TRIALS[c.trial]
    return (b, dm, dm_idx, _accs(c.K, c.n)) + (() if raw is None else (raw,))


def _compare(label, got, c, raw=False, group=None):
    exp = _oracle(c, raw, group)["cands"]
    _, dm, _ = TRIALS[c.trial]
    worst = {}
    for g, e in zip(got, exp):
        worst[e.nh] = max(worst.get(e.nh, 0.0), abs(g.snr - e.snr))
    print(f"ENGINE_EXACT {label}: {len(got)} candidates (oracle {len(exp)}), count {np.bincount([e.nh for e in exp], minlength=6)} "
          + " ".join(f"L{h}={v:.3e}" for h, v in sorted(worst.items())))
    gsig = [(g.dm_idx, g.acc, g.nh, g.freq, g.count_assoc()) for g in got]
    if gsig != _sig(exp):
        k = next((i for i, (a, b) in enumerate(zip(gsig, _sig(exp))) if a != b), min(len(got), len(exp)))
        show = lambda s, x: [t + (round(v.snr, 4),) for t, v in zip(s[k:k + 3], x[k:k + 3])]  # noqa: E731
        pytest.fail(f"{label}: {len(got)} candidates, the oracle has {len(exp)}; first difference at {k}: "
                    f"engine {show(gsig, got)} oracle {show(_sig(exp), exp)}")
    assert len(exp) > 0 or group, label  # (a noise job among several may hold nothing at the shared min_snr)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dm == ref.f32(dm), (label, k)
        assert abs(g.snr - e.snr) <= snr_tol(e.nh, e.snr), (label, k, e.nh, g.snr, e.snr, snr_tol(e.nh, e.snr))


def _search_trial(label, c, **engine):
    d, _ = _rows([c])
    e = _engine(c, **engine)
    _, dm, dm_idx = TRIALS[c.trial]
    got = e.search_trial(d.data_ptr(), c.nsamps, dm, dm_idx, _accs(c.K, c.n))
    _compare(label, got, c)
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("fft_mode", [2, 1, 0])
@pytest.mark.parametrize("which", ["pulses", "noise"])
def test_fft_modes(fft_mode, which):
    e = _search_trial(f"fft_mode {fft_mode} {which}", BASE_CASE if which == "pulses" else NOISE_CASE,
                      fft_mode=fft_mode)
    assert e.fft_mode == fft_mode and not e.rows_ext and not e.whiten_mixed_radix


@pytest.mark.gpu
def test_whitening_with_rocfft(monkeypatch):
    monkeypatch.setenv("PSOUP_WHITEN_ROCFFT", "1")
    assert _search_trial("PSOUP_WHITEN_ROCFFT=1", BASE_CASE).fft_mode == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N16, N17, N3])
def test_other_lengths(n):
    e = _search_trial(f"n {n}", LENGTH_CASES[n])
    if n == N3:  # the whitener is mixed-radix; mode 1's fused r2c needs a power of two, so the search takes mode 0
        assert e.fft_mode == 0 and e.whiten_mixed_radix
    else:
        assert e.fft_mode == 2 and not e.whiten_mixed_radix


HARM_FLAGS = {"default": lambda f: f, "unfused": lambda f: f & ~64, "screen off": lambda f: f | 4,
              "sums from X": lambda f: (f & ~64) | 8, "group screen off": lambda f: f & ~262144,
              "other tile": lambda f: f ^ 65536}


@pytest.mark.gpu
@pytest.mark.parametrize("flags", list(HARM_FLAGS))
@pytest.mark.parametrize("which", ["nh 4", "nh 5"])
def test_harmonic_flags(flags, which):
    import peasoup_amd._C as C

    old = C.kernels.harmonic_flags()
    try:
        C.kernels.harmonic_set_flags(HARM_FLAGS[flags](old))
        _search_trial(f"harmonic flags {flags} {which}", NH_CASES[int(which[-1])])
    finally:
        C.kernels.harmonic_set_flags(old)


@pytest.mark.gpu
@pytest.mark.parametrize("nh", list(NH_CASES))
def test_nharmonics(nh):
    _search_trial(f"nharmonics {nh}", NH_CASES[nh])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RANGE_CASES))
def test_search_ranges(name):
    _search_trial(f"range {name}", RANGE_CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NSAMPS_CASES))
def test_series_length(name):
    _search_trial(f"nsamps {name}", NSAMPS_CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("min_gap", list(GAP_CASES))
@pytest.mark.parametrize("cluster,distill", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")])
def test_clustering_and_distilling(monkeypatch, min_gap, cluster, distill):
    monkeypatch.setenv("PSOUP_GPU_CLUSTER", cluster)
    monkeypatch.setenv("PSOUP_GPU_DISTILL", distill)
    e = _search_trial(f"min_gap {min_gap} PSOUP_GPU_CLUSTER={cluster} PSOUP_GPU_DISTILL={distill}", GAP_CASES[min_gap])
    ctr = e.counters()
    on_device = cluster == "1" and distill == "1" and min_gap <= 30  # min_gap 31 clusters (and so distils) on the host
    assert (ctr["gpu_distilled"] > 0) == on_device and (ctr["host_distilled"] == 0) == on_device


@pytest.mark.gpu
@pytest.mark.parametrize("log2", [0, 6])
@pytest.mark.parametrize("nh", [4, 5])
def test_peak_regions(log2, nh):
    _search_trial(f"peak_region_log2 {log2} nh {nh}", NH_CASES[nh], peak_region_log2=log2)


@pytest.mark.gpu
@pytest.mark.parametrize("K", list(BATCH_CASES))
def test_batches_of_8(K):
    e = _search_trial(f"accel_batch 8, {K} trials", BATCH_CASES[K], accel_batch=8)
    assert e.batch_size == 8 and e.last_batch == 8


@pytest.mark.gpu
@pytest.mark.parametrize("K", [9, 17, 40])
@pytest.mark.parametrize("batch", ["16/8", "auto"])
def test_other_batchings(K, batch):
    eng = dict(accel_batch=16, sub_batch=8) if batch == "16/8" else dict(accel_batch=0)
    e = _search_trial(f"accel_batch {batch}, {K} trials", BATCH_CASES[K], **eng)
    assert (e.batch_size, e.sub_batch) == (16, 8) if batch == "16/8" else e.batch_size > 40


def _multi_engine(**engine):
    import torch

    import peasoup_amd._C as C

    e = C.SearchEngine(_search_params(MULTI_CASES[0], MULTI_CASES, **engine), torch.cuda.current_stream().cuda_stream)
    assert e.max_prepare >= len(MULTI_CASES) and e.fft_mode == 2
    return e


def _compare_multi(label, lists, order, raw=False):
    assert len(lists) == len(order) and sum(map(len, lists)) > 0
    for got, k in zip(lists, order):
        _compare(f"{label} job {k}", got, MULTI_CASES[k], raw, MULTI_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("raw", [False, True])
def test_several_dms_in_one_flat_list(raw):
    """jobs of 5, 9 and 3 accelerations: the flat list of 17 straddles the batches of 8 at trials 8 and 16"""
    d, rs = _rows(MULTI_CASES)
    e = _multi_engine()
    e.prepare(d.data_ptr(), rs, N15, 3)
    if raw:
        lists = e.collect(e.search_prepared_many_async([_job(b, c, True) for b, c in enumerate(MULTI_CASES)]))
    else:
        lists = e.search_prepared_many([_job(b, c) for b, c in enumerate(MULTI_CASES)])
    _compare_multi(f"search_prepared_many raw={raw}", lists, [0, 1, 2], raw)


@pytest.mark.gpu
def test_second_half_of_the_prepared_slots():
    d, rs = _rows(MULTI_CASES)
    e = _multi_engine()
    e.reserve(3, 17, True)
    first = e.max_prepare
    e.prepare(d.data_ptr(), rs, N15, 3, first)
    lists = e.search_prepared_many([_job(first + b, c) for b, c in enumerate(MULTI_CASES)])
    _compare_multi("prepare(first = max_prepare)", lists, [0, 1, 2])


@pytest.mark.gpu
def test_launch_prepare_finish():
    """search_launch of block A, prepare of block B (the same trials in another order) into the other half of
    the slots, search_finish; then block B's search from that half."""
    order = [2, 0, 1]
    dA, rs = _rows(MULTI_CASES)
    dB, _ = _rows([MULTI_CASES[k] for k in order])
    e = _multi_engine()
    e.reserve(3, 17, True)
    first = e.max_prepare
    e.prepare(dA.data_ptr(), rs, N15, 3)
    h = e.search_launch([_job(b, c, False) for b, c in enumerate(MULTI_CASES)])
    e.prepare(dB.data_ptr(), rs, N15, 3, first)
    e.search_finish(h)
    _compare_multi("search_launch/finish block A", e.collect(h), [0, 1, 2])
    h = e.search_launch([_job(first + b, MULTI_CASES[k], False) for b, k in enumerate(order)])
    e.search_finish(h)
    _compare_multi("search_launch/finish block B", e.collect(h), order)
