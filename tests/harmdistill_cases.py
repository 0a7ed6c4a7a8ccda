"""Trials shared by test_harmdistill_gpu.py (kern::harm_distill_batch) and test_candidates.py (the
host HarmonicDistiller): per parameter set a batch of trials in the layout of the device
distiller's input (per level ascending idx, S/N as float32) and the oracle's answer,
reference.py_distill with reference.harm_cond(tol, max_harm, keep=False, frac=True).

What each trial is for (csrc/kernels/harmdistill.hip):
  sizes 1 .. harm_cap   the 256-thread kernel up to 1024 peaks and the 512-thread one above it, the
                        bitonic sort's padding (sizes around powers of two), whole and part 64-blocks
                        of the greedy scan (63, 64, 65)
  all-related           every candidate an exact (sub)harmonic of the strongest: step 3 (iii) clears
                        every later word, one survivor
  unrelated             no relation bit anywhere: every candidate survives, in S/N order
  top idx               idx up to 2^29 - 1 at the top level: the idx | level << 29 packing
  edges                 frequency ratios planted on both sides of (1 - tol, 1 + tol) for j up to
                        max_harm and k up to 2^level: the prefilter and the exact test of harm_related
  tie                   two equal S/N: the trial is handed to the host (kHarmHost)
No two S/N of a trial are equal except in the tie trial."""
import functools

import numpy as np

from peasoup_amd.utils import reference as ref

HARM_CAP = 4096  # kernels.hpp kHarmCap (the tests check it against the extension's)
DF = 1.0 / ((1 << 26) * 64e-6)  # level-0 bin width; level h: DF / 2^h
FACTOR = [DF / 2 ** h for h in range(6)]
# (nlev, tol, max_harm): every level count but the old test's 3, every (tol, max_harm) pair, level 5 at tol 1e-3
PARAMS = [(0, 1e-4, 16), (1, 1e-3, 16), (2, 1e-4, 1), (4, 1e-5, 32), (5, 1e-3, 16)]
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049, HARM_CAP]
TOP = (1 << 29) - 1


def _snr(rng, n):
    """n distinct S/N, exact in float32, in random order."""
    return (9.0 + rng.permutation(n) / 64.0).astype(np.float32)


def _levels(cands, snr):
    """[(level, idx)] distinct, with one S/N each -> per level (idx ascending, snr)."""
    nlev = max(h for h, _ in cands)
    out = []
    for h in range(nlev + 1):
        rows = sorted((i, float(s)) for (hh, i), s in zip(cands, snr) if hh == h)
        out.append((np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float32)))
    return out


def _pad_levels(levels, nlev):
    return levels + [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * (nlev + 1 - len(levels))


def _bin(f, h):
    return int(round(f / FACTOR[h]))


def family_trial(rng, n, nlev, tol, max_harm, lone):
    """n peaks: harmonics j / k of four fundamentals (jitter around the tolerance), a fraction
    `lone` of unrelated bins; above 1024 peaks the fundamentals are the strongest, so the oracle's
    scan stays short."""
    funds = [_bin(f, 0) for f in rng.uniform(20.0, 200.0, 4)]
    seen, cands = set(), []
    for i0 in funds:
        seen.add((0, i0))
        cands.append((0, i0))
    while len(cands) < max(n, 4):
        h = int(rng.integers(0, nlev + 1))
        if rng.random() < lone:
            f = rng.uniform(5.0, 3000.0)
        else:
            f = funds[rng.integers(4)] * FACTOR[0] * rng.integers(1, int(max_harm) + 1) / rng.integers(1, 2 ** h + 1)
            f *= 1.0 + rng.normal(0, 0.5 * tol)
        b = _bin(f, h)
        if 0 < b <= TOP and (h, b) not in seen:
            seen.add((h, b))
            cands.append((h, b))
    cands = cands[:n] if n >= 4 else cands[3:3 + n]
    snr = _snr(rng, len(cands))
    if n > 1024:  # the fundamentals (the first four) first in S/N order
        snr = np.sort(snr)[::-1].copy()
        snr[4:] = snr[4:][rng.permutation(len(snr) - 4)]
    return _pad_levels(_levels(cands, snr), nlev)


def related_trial(rng, nlev, max_harm):
    """Every candidate an exact harmonic or sub-harmonic j / k (k <= 2^level) of the strongest."""
    i0 = 720720  # level-0 bin of the fundamental: divisible by 1..16
    cands = [(0, i0)]
    for h in range(nlev + 1):
        for k in range(1, 2 ** h + 1):
            for j in range(1, int(max_harm) + 1):
                num = i0 * 2 ** h * j
                if num % k == 0 and num // k <= TOP and (h, num // k) not in cands:
                    cands.append((h, num // k))
    cands = [cands[0]] + [cands[1 + k] for k in rng.permutation(len(cands) - 1)[:300]]
    snr = np.sort(_snr(rng, len(cands)))[::-1].copy()  # the fundamental the strongest
    snr[1:] = snr[1:][rng.permutation(len(snr) - 1)]
    return _pad_levels(_levels(cands, snr), nlev)


def unrelated_trial(rng, nlev, tol, max_harm, want=70):
    """Candidates no stronger one is related to (screened here at twice the tolerance; the test
    asserts that the oracle removes none)."""
    cands, freqs = [], []
    snr = np.sort(_snr(rng, want))[::-1]
    for _ in range(20000):
        if len(cands) == want:
            break
        h = int(rng.integers(0, nlev + 1))
        b = _bin(rng.uniform(50.0, 3000.0), h)
        f = ref.f32(b * FACTOR[h])
        if (h, b) in cands:
            continue
        if freqs and ref.harm_related(1.0, f / np.array(freqs), [h] * len(freqs), 2 * tol, max_harm, True).any():
            continue
        cands.append((h, b))
        freqs.append(f)
    snr = snr[:len(cands)].copy()
    return _pad_levels(_levels(cands, snr), nlev)


def top_trial(rng, nlev, max_harm):
    """idx up to 2^29 - 1 at the top level, the same frequencies at the levels below, harmonics."""
    cands = [(nlev, TOP), (nlev, TOP - 1), (nlev, TOP - 63), (nlev, TOP - 64), (nlev, TOP // 2), (nlev, TOP // 3)]
    for h in range(nlev):
        cands += [(h, TOP >> (nlev - h)), (h, (TOP >> (nlev - h)) - 1), (h, (TOP // 2) >> (nlev - h))]
    while len(cands) < 90:
        h = int(rng.integers(0, nlev + 1))
        b = int(rng.integers(1 << 24, 1 << 29)) if rng.random() < 0.5 else TOP * int(rng.integers(1, 17)) // int(rng.integers(17, 64))
        if (h, b) not in cands and 0 < b <= TOP:
            cands.append((h, b))
    return _pad_levels(_levels(cands, _snr(rng, len(cands))), nlev)


def edge_trial(rng, nlev, tol, max_harm):
    """Around a fundamental f0 (the strongest, level 0): f0 j / k (1 +- tol (1 +- 2^-10)), j up to
    max_harm, k up to 2^level, each rounded to a bin of its level.  Returns the levels and the
    planted (level, idx)."""
    i0 = (1 << 29) // (2 ** nlev * int(max_harm)) - 9  # the largest that keeps every planted idx below 2^29:
    f0 = i0 * FACTOR[0]                                # the bins are fine next to tol 2^-10 where they can be
    triples = [(h, j, k) for h in range(nlev + 1) for k in range(1, 2 ** h + 1) for j in range(1, int(max_harm) + 1)]
    pick = [triples[t] for t in rng.permutation(len(triples))[:60]]
    pick += [(nlev, int(max_harm), 1), (nlev, 1, 2 ** nlev), (nlev, int(max_harm), 2 ** nlev), (0, 1, 1)]
    cands, planted = [(0, i0)], []
    for h, j, k in pick:
        for sa in (-1.0, 1.0):
            for sb in (-1.0, 1.0):
                b = _bin(f0 * j / k * (1.0 + sa * tol * (1.0 + sb * 2.0 ** -10)), h)
                if 0 < b <= TOP and (h, b) not in cands:
                    cands.append((h, b))
                    planted.append((h, b))
    snr = np.sort(_snr(rng, len(cands)))[::-1].copy()
    snr[1:] = snr[1:][rng.permutation(len(snr) - 1)]
    return _pad_levels(_levels(cands, snr), nlev), planted


def tie_trial(rng, nlev, tol, max_harm):
    lv = family_trial(rng, 200, nlev, tol, max_harm, 0.3)
    idx, snr = lv[0]
    snr = snr.copy()
    snr[2] = snr[0]
    return [(idx, snr)] + lv[1:]


@functools.lru_cache(maxsize=None)
def batch(p):
    """The trials of parameter set PARAMS[p]: dict(nlev, tol, max_harm, trials [per-level lists],
    kind [name per trial], planted {trial: [(level, idx)]})."""
    nlev, tol, max_harm = PARAMS[p]
    rng = np.random.default_rng(500 + p)
    trials, kind, planted = [], [], {}
    for n in SIZES:
        trials.append(family_trial(rng, n, nlev, tol, max_harm, 0.15 if n <= 1025 else 0.03))
        kind.append(f"size{n}")
    trials.append(_pad_levels([], nlev))
    kind.append("empty")
    trials.append(related_trial(rng, nlev, max_harm))
    kind.append("related")
    trials.append(unrelated_trial(rng, nlev, tol, max_harm))
    kind.append("unrelated")
    trials.append(top_trial(rng, nlev, max_harm))
    kind.append("top")
    lv, pl = edge_trial(rng, nlev, tol, max_harm)
    planted[len(trials)] = pl
    trials.append(lv)
    kind.append("edges")
    trials.append(tie_trial(rng, nlev, tol, max_harm))
    kind.append("tie")
    return dict(nlev=nlev, tol=tol, max_harm=max_harm, trials=trials, kind=kind, planted=planted)


def tuples(levels):
    """The candidates of one trial as Candidate constructor arguments, in load order."""
    return [(10.0, 3, 0.0, h, float(v), float(np.float32(int(i) * FACTOR[h])))
            for h, (idx, snr) in enumerate(levels) for i, v in zip(idx, snr)]


@functools.lru_cache(maxsize=None)
def oracle(p, k):
    """Trial k of set p distilled by the Python oracle: [(level, snr, float32 freq)] in descending S/N."""
    b = batch(p)
    out = ref.py_distill([ref.Cand(*t) for t in tuples(b["trials"][k])], ref.harm_cond(b["tol"], b["max_harm"], False, True))
    return [(c.nh, c.snr, c.freq) for c in out]
