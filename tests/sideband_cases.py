"""Shared cases of the sideband tests: seeded inputs, the float64 oracle's
results (computed once and left unchanged) and the comparison rules.

Tolerance (derived, not measured): a radix FFT of M points in float32 (unit
roundoff u = 2^-24, twiddles rounded once from double) obeys Higham's bound
||F - F_ref||_2 <= log2(M) eta ||x||_2 with eta about 7u.  Every |F_j - F_ref,j|
is allowed t = 16 u log2(M) ||x||_2 (the 16 covers eta, the clip and the
subtraction), so S = |F|^2 / M may differ by (2 |F_ref,j| t + t^2) / M
(``reference.sideband_bound``).  The winner j must be the oracle's except where
the oracle's two largest S are closer than twice that bound, and those segments
may be at most 1% of all (asserted on the oracle alone, without a GPU)."""
import functools
import math
import os

import numpy as np

from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import write_filterbank
from peasoup_amd.utils.synthetic import PulsarSpec

M_LO, M_HI = 5, 13
WINDOW, HOP = 8192, 4096

# ---- every size: 3 rows of exponential noise, an unaligned head, several windows, a partial last one and a
# remainder that is no multiple of any hop; NaN outside the band
K_LO = 37
BAND = 3 * 8192 + 4096 + 611
K_HI = K_LO + BAND
STRIDE = (K_HI + 3) // 4 * 4 + 4
SEED_ALL = 11


def noise_rows(nrows, stride, k_lo, k_hi, seed, outside=np.nan):
    rng = np.random.default_rng(seed)
    P = np.full((nrows, stride), outside, dtype=np.float32)
    P[:, k_lo:k_hi] = rng.exponential(1.0, size=(nrows, k_hi - k_lo)).astype(np.float32)
    return P


@functools.lru_cache(maxsize=None)
def all_sizes():
    P = noise_rows(3, STRIDE, K_LO, K_HI, SEED_ALL)
    P.setflags(write=False)
    oracle = [ref.sideband_search(P[r], K_LO, K_HI, M_LO, M_HI, 2, 32.0, 30.0, r) for r in range(3)]
    return P, oracle


def ambiguous(o):
    """Segments of one size's oracle record whose winner a float32 transform may miss."""
    return o["gap"] < 2.0 * o["bound"]


def compare_dense(best_S, best_j, oracle_rows, nseg, m_lo=M_LO, m_hi=M_HI, what=""):
    """best_S / best_j [nrows, nm, seg_stride] against the oracle records of every row: S within the bound, j equal
    outside the ambiguous segments, nothing written past a size's segments.  Returns (segments, ambiguous ones)."""
    total = amb = 0
    for r, orow in enumerate(oracle_rows):
        for m in range(m_lo, m_hi + 1):
            o = orow[m]
            n = len(o["best_S"])
            assert n == nseg[m - m_lo], (what, m, n, nseg)
            S = np.asarray(best_S[r, m - m_lo, :n], dtype=np.float64)
            j = np.asarray(best_j[r, m - m_lo, :n])
            assert np.all(np.isfinite(S)), (what, r, m)
            a = ambiguous(o)
            same = j == o["best_j"]
            assert np.all(same | a), (what, r, m, np.nonzero(~(same | a))[0][:5])
            err = np.abs(S - o["best_S"])
            ok = err <= o["bound"]
            # an ambiguous segment that chose the runner-up is within the gap plus the bound of the oracle's best
            ok |= a & ~same & (err <= o["gap"] + 2.0 * o["bound"])
            assert np.all(ok), (what, r, m, float(err.max()), np.nonzero(~ok)[0][:5])
            total += n
            amb += int(np.count_nonzero(a))
    return total, amb


# ---- planted combs: x_i = A cos(2 pi j0 i / M) on P = 1 gives S_j0 = A^2 M / 4
COMB_A = 0.5
COMB_K_LO = 3
COMB_BAND = 2 * 8192 + 4096


def comb_rows(m, j_min=2):
    """6 rows at size m: j0 = j_min and M/2 - 1 in the first segment, the last one and the last one a window owns.
    Returns (P [6, stride], [(seg, j0)] per row)."""
    M = 1 << m
    nseg = ref.sideband_nseg(COMB_BAND, m)
    owned_last = 1 if m == 13 else (HOP - M // 2) // (M // 2)
    stride = (COMB_K_LO + COMB_BAND + 3) // 4 * 4
    cases = [(seg, j0) for seg in (0, nseg - 1, owned_last) for j0 in (j_min, M // 2 - 1)]
    P = np.ones((len(cases), stride), dtype=np.float32)
    i = np.arange(M)
    for r, (seg, j0) in enumerate(cases):
        s = COMB_K_LO + seg * (M // 2)
        P[r, s:s + M] = (1.0 + COMB_A * np.cos(2.0 * np.pi * ((j0 * i) % M) / M)).astype(np.float32)
    return P, cases


# ---- clip: one bin of 10^6 in noise.  Clipped to 32 the bin alone carries x = 31, that is S = 31^2 / M at every j
# of a segment covering it: 30.03 at M = 32 and 15.02 at M = 64, at or close to the threshold of 30 by the definition
# itself, whatever the seed.  "No event" is therefore asserted on M >= 128 (7.5 and below), on a seed for which the
# oracle has none; every size, 32 and 64 included, is compared with the oracle.
CLIP_K_LO = 5
CLIP_BAND = 8192 + 4096 + 123
CLIP_BIN = CLIP_K_LO + 6000
CLIP_SEED = 4
CLIP_QUIET_M_LO = 7


@functools.lru_cache(maxsize=None)
def clip_case():
    stride = (CLIP_K_LO + CLIP_BAND + 3) // 4 * 4
    P = noise_rows(1, stride, CLIP_K_LO, CLIP_K_LO + CLIP_BAND, CLIP_SEED)
    P[0, CLIP_BIN] = 1.0e6
    P.setflags(write=False)
    o32 = ref.sideband_search(P[0], CLIP_K_LO, CLIP_K_LO + CLIP_BAND, M_LO, M_HI, 2, 32.0, 30.0, 0)
    obig = ref.sideband_search(P[0], CLIP_K_LO, CLIP_K_LO + CLIP_BAND, M_LO, M_HI, 2, 1.0e9, 30.0, 0)
    return P, o32, obig


def covering(m, k_lo, k_bin, nseg):
    """Segments of size m that hold bin k_bin."""
    M = 1 << m
    return [s for s in range(nseg) if k_lo + s * (M // 2) <= k_bin < k_lo + s * (M // 2) + M]


def split_events(oracle_rows, min_power, m_lo=M_LO, m_hi=M_HI):
    """The oracle's events of several rows as {(dm_idx, m, seg): (j, S, bound, ambiguous)} in two sets: `sure` (S
    above the threshold by more than the bound) and `border` (within the bound of it, either side)."""
    sure, border = {}, {}
    for r, orow in enumerate(oracle_rows):
        for m in range(m_lo, m_hi + 1):
            o = orow[m]
            a = ambiguous(o)
            for s in range(len(o["best_S"])):
                S, b = float(o["best_S"][s]), float(o["bound"][s])
                rec = (int(o["best_j"][s]), S, b, bool(a[s]))
                if S - b >= min_power:
                    sure[(r, m, s)] = rec
                elif S + b >= min_power:
                    border[(r, m, s)] = rec
    return sure, border


def check_events(events, sure, border, complete):
    """Every event is one of the oracle's (S within the bound, j equal unless ambiguous), none twice; with `complete`
    every sure one is there.  Border events (within the bound of the threshold) may be there or not; they are at most
    1% of the set."""
    seen = set()
    for e in events:
        key = (int(e[0]), int(e[1]), int(e[2]))
        assert key not in seen, key
        seen.add(key)
        rec = sure.get(key) or border.get(key)
        assert rec is not None, ("not an event of the oracle", e)
        j, S, b, amb = rec
        assert amb or int(e[3]) == j, (e, rec)
        assert abs(float(e[4]) - S) <= (b if int(e[3]) == j else 3.0 * b + 1e-30) or amb, (e, rec)
    if complete:
        missing = [k for k in sure if k not in seen]
        assert not missing, missing[:5]
    assert len(border) <= 0.01 * max(len(sure), 1) or len(border) <= 1, (len(border), len(sure))


# ---- end to end: 2^17 samples of 1 ms, 16 channels, 8 bits; a 50 Hz pulsar (Gaussian pulses of sigma 0.03 turns:
# FWHM 0.0706) on a circular orbit of pb = T / 16 with 2 pi f a1 = 20 rad.  0.15 channel sigma per channel is 16 x
# 0.15 / sqrt(16) = 0.6 sigma per sample of the dedispersed series.  The DM steps are made wide (a 2 ms pulse width
# for the DM plan) so that a neighbouring trial smears the 20 ms period visibly; the pulsar sits on the third of the
# four trials.
NS = 1 << 17
TSAMP = 1e-3
F0 = 50.0
E2E_SEED = 2
E2E_DM_OPTS = ["--dm_start", "0", "--dm_end", "500", "--dm_pulse_width", "2000", "--dm_tol", "1.5"]
E2E_DM_IDX = 2


def e2e_tobs():
    return NS * float(np.float32(TSAMP))


def e2e_header():
    hdr = dict(synthetic.make_header(nchans=16, nbits=8, tsamp=TSAMP))
    hdr["nsamples"] = NS
    return hdr


def e2e_values(dm_list):
    T = e2e_tobs()
    spec = PulsarSpec(period=1.0 / F0, dm=float(dm_list[E2E_DM_IDX]), duty=0.0706, amplitude=0.15,
                      orbit=(T / 16.0, 20.0 / (2.0 * math.pi * F0), 0.0))
    return synthetic.generate(NS, e2e_header(), [spec], seed=E2E_SEED)


def e2e_file(tmp, dm_list, name="sideband.fil"):
    path = os.path.join(str(tmp), name)
    write_filterbank(path, e2e_header(), e2e_values(dm_list))
    return path


def empty_file(tmp, name="empty.fil", nsamples=NS):
    """The end-to-end file's shape with zeros for data: enough for the setup (the DM list, every refusal)."""
    path = os.path.join(str(tmp), name)
    hdr = e2e_header()
    hdr["nsamples"] = nsamples
    write_filterbank(path, hdr, np.zeros((nsamples, 16), dtype=np.uint8))
    return path


def big_file(tmp, name="big.fil"):
    """A span above 2^26 from the header alone: a sparse 1-bit file whose data block is never read."""
    path = os.path.join(str(tmp), name)
    hdr = synthetic.make_header(nchans=8, nbits=1, tsamp=64e-6)
    hdr["nsamples"] = (1 << 27) + 4096
    write_filterbank(path, hdr, np.zeros((0, 8), dtype=np.uint8))
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) + hdr["nsamples"])
    return path


def cand_lines(path):
    with open(path) as f:
        return [ln for ln in f.read().splitlines() if ln and not ln.startswith("#")]
