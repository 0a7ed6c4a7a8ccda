"""Shapes, templates, planes and the recovery pulsar shared by test_orbopt.py
(host transcriptions) and test_orbopt_gpu.py (kernels): the same cases reach the
same paths.  The oracle's resampled rows are computed once per shape and shared."""
import functools
import os

import numpy as np

import orbit_cases as oc
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import write_filterbank
from peasoup_amd.utils.synthetic import PulsarSpec

TS = oc.TS
SHAPES = [(17, 0), (4101, 37), (65539, 0)]
NINTS = (1, 3, 16)
NBINS = (2, 7, 64, 256)


def periods(n):
    """In samples: the bin changes every sample; a few samples per bin; a whole wave in one bin."""
    return (2.5, 64.3, max(2.5, n / 3.0))


def phase_step(period_samples):
    """G of a period given in samples (ts / P = 1 / period_samples)."""
    return int(np.rint(np.ldexp(1.0 / float(period_samples), 64)))


def combos(n):
    """(nints, nbins, [G of candidate 0, 1, 2]): every nints with every nbins, the three periods dealt to the three
    rows in an order that turns with the combination, so every (nints, nbins, period) is folded."""
    g = [phase_step(p) for p in periods(n)]
    out = []
    for a, nints in enumerate(NINTS):
        for b, nbins in enumerate(NBINS):
            r = (a + b) % 3
            out.append((nints, nbins, g[r:] + g[:r]))
    return out


@functools.lru_cache(maxsize=None)
def shape_case(n, pad):
    """x uint8 [3, stride] (stride a multiple of 256), the 60 templates of orbit_cases.templates(n) and the oracle's
    resampled spans y uint8 [3, 60, n]; read-only."""
    nrow = n + pad
    x = oc.rows(3, (nrow + 255) // 256 * 256, 7 * n + pad)
    tpl = oc.templates(n)
    i = np.arange(n, dtype=np.int64)
    y = np.empty((3, len(tpl), n), dtype=np.uint8)
    for k, q in enumerate(tpl):
        y[:, k] = x[:, np.clip(i + ref.orbit_shift(n, q), 0, n - 1)]
    x.setflags(write=False)
    y.setflags(write=False)
    return x, tpl, y


def want_fold(y, k0, k1, n, Gs, nints, nbins):
    """The oracle's planes int32 [3, k1 - k0, nints, nbins] from the resampled spans."""
    out = np.empty((y.shape[0], k1 - k0, nints, nbins), dtype=np.int32)
    for c in range(y.shape[0]):
        cell = ref.orbopt_bins(n, Gs[c], nints, nbins)
        for k in range(k0, k1):
            s = np.bincount(cell, weights=y[c, k].astype(np.float64), minlength=nints * nbins).astype(np.int64)
            out[c, k - k0] = (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(nints, nbins)
    return out


def group_bounds(ntpl):
    """K of 1, 5 and 13 (and the rest): every template is used once."""
    out, k = [], 0
    for size in (1, 5, 13, 13, 13, ntpl):
        if k < ntpl:
            out.append((k, min(ntpl, k + size)))
            k += size
    return out


# ------------------------------------------------------------------ planes ----
def search_planes(kind, K, nints, nbins, seed=0):
    """(fold int32 [K, nints, nbins], hits int32 [nints, nbins], m) whose d = fold - m hits is `kind`:
    'bound': random over the whole range in which every box sum still fits an int32;
    'equal': one value everywhere (every maximum is a tie)."""
    rng = np.random.default_rng(seed)
    hits = rng.integers(1, 40, (nints, nbins)).astype(np.int64)
    m = int(rng.integers(0, 256))
    wmax = 1 << (ref.cube_opt_nwidths(nbins) - 1)  # the widest box
    lim = (2 ** 31 - 1) // (nints * wmax)
    if kind == "bound":
        d = rng.integers(-lim, lim + 1, (K, nints, nbins))
        d[0, :, :wmax] = lim        # the largest box sum there is
        d[K - 1, :, :wmax] = -lim
    else:
        d = np.full((K, nints, nbins), 3, dtype=np.int64)
    fold = ((d + m * hits[None]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return fold, hits.astype(np.int32), m


# ------------------------------------------------------------ small files ----
CAND_TEXT = """# period_s dm acc pb_s a1_ls phase freq nh snr folded_snr dm_idx
0.0123 12.5 0 40 0.004 0.3 81.3 1 20 0 0

0.0301 3 1.5 25.5 0 0.6 33.2 0 15 0 0   # a1 = 0: one pb, one phase
"""
SMALL_OPTS = ["--nbins", 16, "--nints", 4, "--npb", 3, "--na1", 3, "--nphase", 3, "--np", 5]
SMALL_PARAMS = dict(nbins=16, nints=4, npb=3, na1=3, nphase=3, np_=5)


def small_file(tmp):
    fil = os.path.join(str(tmp), "small.fil")
    hdr = synthetic.make_header(nchans=16, nbits=8, tsamp=320e-6)
    synthetic.write(fil, 1 << 14, hdr, [PulsarSpec(period=0.0123, dm=12.5, duty=0.08, amplitude=0.5)], seed=3)
    cand = os.path.join(str(tmp), "cands.txt")
    with open(cand, "w") as f:
        f.write(CAND_TEXT)
    return fil, cand


def refusal_cases(tmp):
    """(candidate text or None, extra options, the name the refusal carries), shared by the module and the binary."""
    good = "0.0123 12.5 0 40 0.004 0.3\n"
    return [
        (good, ["--npb", 4], "an even count"),
        (good, ["--np", 10], "an even count"),
        (good, ["--nbins", 300], "nbins must be in 2..256"),
        (good, ["--nints", 0], "nints must be in 1..64"),
        (good, ["--npb", 17, "--na1", 17, "--nphase", 17], "more than 4096 templates"),
        ("# nothing\n\n", [], "an empty candidate file"),
        (good, ["--limit", 0], "an empty candidate file"),
        (good + "0.0123 12.5 0 40 0.004\n", [], "candidate line 2 is malformed"),
        (good + "0.0001 12.5 0 40 0.004 0.3\n", [], "candidate 1"),
        (good + "0.0001 12.5 0 40 0.004 0.3\n", [], "below 2 tsamp"),
        ("nan 12.5 0 40 0.004 0.3\n", [], "below 2 tsamp"),
        ("0.0123 -1 0 40 0.004 0.3\n", [], "non-finite or negative DM"),
        ("0.0123 nan 0 40 0.004 0.3\n", [], "non-finite or negative DM"),
        ("0.0123 12.5 0 inf 0.004 0.3\n", [], "non-finite value"),
        ("0.0123 12.5 0 0.01 0.004 0.3\n", [], "pb < 64 tsamp"),
        ("0.0123 12.5 0 1e9 2000 0.3\n", [], "Aq >= 2^30"),
        ("0.0123 12.5 0 100 20 0\n", [], "0.9 samples per sample"),
        (None, [], "cannot open the candidate file"),
    ]


# ---------------------------------------------------------------- recovery ----
NS = 1 << 17
P0 = 0.0101
TRUTH = (60.0, 0.0096, 0.75)
START = (63.0, 0.0088, 0.72)
DM0 = 20.0
# S/N of the CPU oracle (reference.orbit_optimise with a 1 x 1 x 1 grid, 33 drift trials) on this file: at the
# injected template and at the starting one.  profiles/orbopt/SUMMARY.md records how they were obtained.
SNR_TRUTH = 46.30460193034741
SNR_START = 13.939439352387177


def recovery_values():
    """The filterbank of the orbsearch recovery test: 2^17 samples at 320 us, 64 channels, P = 10.1 ms, DM 20,
    pb 60 s, a1 0.0096 ls, phase 0.75."""
    hdr = dict(synthetic.make_header(nchans=64, nbits=8, tsamp=320e-6))
    hdr["nsamples"] = NS
    spec = dict(period=P0, dm=DM0, duty=0.05, amplitude=0.1)
    return hdr, synthetic.generate(NS, hdr, [PulsarSpec(orbit=TRUTH, **spec)], seed=1)


def recovery_row():
    """The dedispersed row of that file at DM 20 from the CPU oracle, and its span n."""
    from peasoup_amd import _C as C

    hdr, values = recovery_values()
    geom = C.DedispGeometry.make(hdr, NS, [DM0], [1] * 64)
    offs = np.asarray(geom.offsets(0, 1)).reshape(1, 64)
    row = ref.dedisperse(values, offs, 8, None, int(geom.out_nsamps))[0]
    return row, min(len(row), NS)


def recovery_file(tmp):
    hdr, values = recovery_values()
    fil = os.path.join(str(tmp), "orbital.fil")
    write_filterbank(fil, hdr, values)
    cand = os.path.join(str(tmp), "start.txt")
    with open(cand, "w") as f:
        f.write(f"{P0!r} {DM0!r} 0 {START[0]!r} {START[1]!r} {START[2]!r}\n")
    return fil, cand
