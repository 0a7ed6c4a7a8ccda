"""Staging of the two-level screen (harmsum.hip harmonic_peaks_q8g_kernel):
the chunks of all gather ranges are dealt to the 256 threads round-robin, and
the LDS image (bytes and block maxima) must be what the range-by-range staging
left.  The screen only decides where the exact sums run, so under every flag
set the records must equal the unscreened fp32 kernel's on the same P.

Planted on exponential noise: harmonic families whose fundamental is the first
and the last bin of a tile (their terms are then the first and the last bytes
each gather range stages, next to the neighbouring tile's), one byte of each
out-of-range code, and a last trial whose every byte is out of range.  Every
trial must give between 1 and 1000 records by the NumPy model
(utils/reference.py harmonic_sums), so no comparison is between empty lists."""
import functools

import numpy as np
import pytest
import torch

from peasoup_amd.utils.reference import harmonic_sums, q8

pytestmark = pytest.mark.gpu
dev = "cuda"

GROUPS = 1 << 18  # the two-level screen
WIDE = 1 << 16    # 16 bins per thread (4096-bin tiles) up to 3 levels; cleared: 2048-bin tiles
THRESH = {1: 6.0, 3: 9.0}
TILE = 4096       # a multiple of both tile sizes
STARTS = [19, 35, 67, 131, 259, 515]  # lo = 19: the tiles start at bin 16


def _records(r):
    return sorted(zip(*[t.tolist() for t in r]))


def _idx(i, h, m):
    return (i * m + (1 << (h - 1))) >> h


def _ends(nb):
    return [nb, nb - 7, nb, nb - 100, nb, nb]


def _flag_sets(old):
    """The default and the other tile size (another chunk count, another deal).
    No flag bit was kept: the range-by-range staging and the measured pre-pass
    for the block maxima (docs/ROADMAP.md) were both deleted."""
    return [old, old ^ WIDE]


def _plant_family(row, i, nlev, amp):
    """Fundamental i and every term of every level at `amp`: no single bin
    crosses, the sums of levels >= 1 do."""
    row[i] = amp
    for h in range(1, nlev + 1):
        for m in range(1, 1 << h, 2):
            row[_idx(i, h, m)] = amp


@functools.lru_cache(maxsize=None)
def _case(log2n, Kb, nlev):
    """(P, per-trial list of planted (level-free) bins) -- built once per shape."""
    n = 1 << log2n
    rng = np.random.default_rng(1000 * log2n + 10 * Kb + nlev)
    P = (rng.exponential(1.0, (Kb, n)) - 1.0).astype(np.float32)
    b0 = STARTS[0] & ~15
    ntile = (n - b0) // TILE
    planted = []
    for k in range(Kb - 1):
        T = 1 + (3 * k + 1) % (ntile - 2)
        first, lastb = b0 + T * TILE, b0 + (T + 1) * TILE - 1
        # >= 5.0 per term: level 1 gives 10 / sqrt 2 = 7.07 > 6, level 2 gives 10 > 9.  Every family its own
        # amplitude (and sums): family 0 has the smallest, 5.0, and alone of all its single bins stay below
        # both thresholds; from 6.0 (1 level) or 9.0 (3 levels) on a family's bins cross at level 0 too.
        _plant_family(P[k], first, nlev, 5.0 + 0.25 * (2 * k))
        _plant_family(P[k + 1 if k + 1 < Kb - 1 else 0], lastb, nlev, 5.0 + 0.25 * (2 * k + 1))
        planted.append((k, first))
        planted.append((k + 1 if k + 1 < Kb - 1 else 0, lastb))
    P[0, b0 + 2 * TILE + 1000] = 1e6    # byte 254
    P[1, b0 + 2 * TILE + 1007] = -50.0  # byte 255
    P[Kb - 1, :] = -50.0                # every byte out of range (255) ...
    P[Kb - 1, b0 + 3 * TILE + 8] = 1e6  # ... and one 254: the only bins that cross
    P.setflags(write=False)
    return P, tuple(planted)


def _model_counts(P, nlev, starts, ends, thresh):
    out = []
    for k in range(P.shape[0]):
        lev = [P[k]] + harmonic_sums(P[k], nlev)
        out.append(sum(int((lev[h][starts[h]:ends[h]] > np.float32(thresh)).sum()) for h in range(nlev + 1)))
    return out


@pytest.mark.parametrize("limit", [False, True])
@pytest.mark.parametrize("nlev", [1, 3])
@pytest.mark.parametrize("Kb", [3, 9])
@pytest.mark.parametrize("log2n", [15, 17])
def test_screened_equals_exact(log2n, Kb, nlev, limit):
    import peasoup_amd._C as C
    from peasoup_amd import ops

    P, planted = _case(log2n, Kb, nlev)
    n = P.shape[1]
    nb = n - 1003 if limit else n  # rows longer than the spectrum: the clamped tail chunks
    starts, ends = STARTS, _ends(nb)
    thresh = THRESH[nlev]
    counts = _model_counts(P, nlev, starts, ends, thresh)
    print("records per trial (model):", counts)
    assert all(1 <= c <= 1000 for c in counts), counts
    Qh = q8(P)
    assert (Qh[0] == 254).sum() == 1 and (Qh[1] == 255).sum() == 1 and (Qh[Kb - 1] >= 254).all()
    Pt = torch.tensor(P, device=dev)
    Q = ops.quantize_q8(Pt)
    old = C.kernels.harmonic_flags()
    assert old & GROUPS
    ref = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, nbins=nb))
    per_trial = np.bincount([r[0] for r in ref], minlength=Kb)
    assert per_trial.tolist() == counts
    keys = {(r[0], r[2]) for r in ref}
    assert all(p in keys for p in planted), "every planted tile-edge bin crosses"
    try:
        for flags in _flag_sets(old):
            C.kernels.harmonic_set_flags(flags)
            got = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, nbins=nb, Q=Q))
            assert got == ref, (hex(flags), len(got), len(ref))
    finally:
        C.kernels.harmonic_set_flags(old)


@pytest.mark.parametrize("nlev", [1, 3])
def test_threshold_at_a_planted_sum(nlev):
    """The threshold (and with it every screening bound derived from it) set
    exactly at the top level's sum of a planted tile-edge bin: no record there
    (the comparison is strict); one float below: the record.  The sum is the
    fp32 kernel's own value at a lower threshold."""
    import peasoup_amd._C as C
    from peasoup_amd import ops

    log2n, Kb = 15, 3
    P, planted = _case(log2n, Kb, nlev)
    n = P.shape[1]
    starts, ends = STARTS, _ends(n)
    Pt = torch.tensor(P, device=dev)
    Q = ops.quantize_q8(Pt)
    k, i = planted[0]
    low = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, THRESH[nlev]))
    at = [r[3] for r in low if (r[0], r[1], r[2]) == (k, nlev, i)]
    assert len(at) == 1
    v = np.float32(at[0])
    old = C.kernels.harmonic_flags()
    try:
        for thresh, present in ((float(v), False), (float(np.nextafter(v, np.float32(-np.inf))), True)):
            counts = _model_counts(P, nlev, starts, ends, thresh)
            assert all(1 <= c <= 1000 for c in counts), counts
            C.kernels.harmonic_set_flags(old)
            ref = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh))
            assert ((k, nlev, i) in {(r[0], r[1], r[2]) for r in ref}) == present
            for flags in _flag_sets(old):
                C.kernels.harmonic_set_flags(flags)
                got = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, Q=Q))
                assert got == ref, (hex(flags), thresh, len(got), len(ref))
    finally:
        C.kernels.harmonic_set_flags(old)


_SCALE = [1.0, 0.70710678118654752440, 0.5, 0.35355339059327376220, 0.25, 0.17677669529663688110]


def _lim(thresh, h):
    """The screening bound of level h in byte-sum units as harmonic_peaks_batch
    derives it from the threshold (harmsum.hip: pre.lo[h], then lim.v[h])."""
    t = float(np.float32(thresh)) / _SCALE[h]
    lo = t - abs(t) * 1e-5 - 1e-30
    f = np.float32(lo)
    if float(f) > lo:
        f = np.nextafter(f, np.float32(-np.inf))
    n = float(1 << h)
    return int(np.floor(4.0 * (float(f) - n / 8.0 - 0.25) + 127.0 * n)) - 1


def _thresh_for_lim(target, h):
    """A float32 threshold whose derived lim[h] is `target`."""
    n = float(1 << h)
    lo = (target + 1.5 - 127.0 * n) / 4.0 + n / 8.0 + 0.25  # the middle of the step
    t = float(np.float32(lo * _SCALE[h] / (1.0 - 1e-5)))
    assert _lim(t, h) == target, (t, _lim(t, h), target)
    return t


@pytest.mark.parametrize("nlev", [1, 3])
def test_screening_bound_at_a_planted_byte_sum(nlev):
    """The top level's screening bound lim[h] set exactly at the byte sum of a
    planted tile-edge bin (first bin of a tile: its bytes are the first ones
    each range stages), so the screen's strict comparison does not pass that
    bin on level h, and one below it, so it does.  Records equal the fp32
    kernel's both times."""
    import peasoup_amd._C as C
    from peasoup_amd import ops

    log2n, Kb = 15, 3
    P, planted = _case(log2n, Kb, nlev)
    n = P.shape[1]
    starts, ends = STARTS, _ends(n)
    k, i = planted[0]
    assert (i - (STARTS[0] & ~15)) % TILE == 0
    Qh = q8(P)
    S = int(Qh[k, i]) + sum(int(Qh[k, _idx(i, h, m)]) for h in range(1, nlev + 1) for m in range(1, 1 << h, 2))
    assert int(Qh[k].max()) == 254 and S < 254 * (1 << nlev)
    Pt = torch.tensor(P, device=dev)
    Q = ops.quantize_q8(Pt)
    old = C.kernels.harmonic_flags()
    try:
        for target in (S, S - 1):
            thresh = _thresh_for_lim(target, nlev)
            assert (S > _lim(thresh, nlev)) == (target == S - 1)
            counts = _model_counts(P, nlev, starts, ends, thresh)
            print("lim", target, "thresh", thresh, "records per trial (model):", counts)
            assert all(1 <= c <= 1000 for c in counts), counts
            C.kernels.harmonic_set_flags(old)
            ref = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh))
            assert np.bincount([r[0] for r in ref], minlength=Kb).tolist() == counts
            for flags in _flag_sets(old):
                C.kernels.harmonic_set_flags(flags)
                got = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, Q=Q))
                assert got == ref, (hex(flags), thresh, len(got), len(ref))
    finally:
        C.kernels.harmonic_set_flags(old)
