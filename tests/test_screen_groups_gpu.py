"""Two-level screen of the screened harmonic sum (harmsum.hip
harmonic_peaks_q8g_kernel, harmonic flag bit 18): groups of 8 bins are screened
on block maxima of the screening bytes before any single bin.  The records must
equal the unscreened fp32 kernel's, and the per-bin screen's (bit 18 cleared),
for every level count, at the edges of the groups' gather windows, around
out-of-range bytes, on dense tiles and on the spectrum passes' own Q layouts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

GROUPS = 262144  # harmonic flag bit 18: the two-level screen
THRESH = {0: 5.0, 1: 6.0, 2: 7.5, 3: 9.0, 4: 10.0, 5: 10.0}


def _records(r):
    return sorted(zip(*[t.tolist() for t in r]))


def _idx(i, h, m):
    """The bin term (h, m) of bin i reads (the reference index expression)."""
    return (i * m + (1 << (h - 1))) >> h


def _ranges(n):
    """Per-level [start, end) that cut inside groups of 8 bins: start = 3,
    end = 5 (mod 8), different per level."""
    base = (n // 8) * 8 - 3
    starts = [3, 11, 19, 35, 67, 131]
    ends = [base, base - 8 * 13, base - 8, base - 8 * 40, base, base - 16]
    assert all(s % 8 == 3 for s in starts) and all(e % 8 == 5 for e in ends)
    return starts, ends


def _three_way(Pt, Q, nlev, starts, ends, thresh, bases, **kw):
    """Records of the unscreened kernel, and for each base flag set those of the
    screened kernel with the group screen on and off; all must be equal."""
    import peasoup_amd._C as C
    from peasoup_amd import ops

    old = C.kernels.harmonic_flags()
    assert old & GROUPS, "the two-level screen is on by default"
    ref = _records(ops.harmonic_peaks(kw.pop("Pnat", Pt), nlev, starts, ends, thresh))
    try:
        for base in bases(old):
            C.kernels.harmonic_set_flags(base | GROUPS)
            on = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, Q=Q, **kw))
            C.kernels.harmonic_set_flags(base & ~GROUPS)
            off = _records(ops.harmonic_peaks(Pt, nlev, starts, ends, thresh, Q=Q, **kw))
            assert on == ref, (base, len(on), len(ref))
            assert off == ref, (base, len(off), len(ref))
    finally:
        C.kernels.harmonic_set_flags(old)
    return ref


@pytest.mark.parametrize("nlev", [0, 1, 2, 3, 4, 5])
def test_every_level_count(nlev):
    from peasoup_amd import ops

    thresh = THRESH[nlev]
    rng = np.random.default_rng(180 + nlev)
    n, Kb = 131075, 8  # 32 tiles of 4096 bins and a clamped tail; not a multiple of 16
    P = (rng.exponential(1.0, (Kb, n)) - 1.0).astype(np.float32)
    for k in range(Kb):  # harmonic families with amplitudes around the threshold
        for f0 in rng.uniform(40.0, n / 40.0, 3):
            amp = rng.uniform(0.4, 2.5) * thresh
            for hm in range(1, 33):
                b = int(f0 * hm)
                if b < n:
                    P[k, b] += amp / np.sqrt(hm)
    starts, ends = _ranges(n)
    Pt = torch.from_numpy(P).to(dev)
    Q = ops.quantize_q8(Pt)
    # bit 1: pre-threshold off (every group flagged, every bin exact); bit 16 toggled: the other tile size
    ref = _three_way(Pt, Q, nlev, starts, ends, thresh,
                     lambda old: (old, old | 2, old ^ 65536, (old ^ 65536) | 2))
    assert len(ref) > 20


@pytest.mark.parametrize("nlev", [3, 5])
def test_window_edges(nlev):
    """For every term (h, m): one bin whose read is the last bin of its
    group's window and the first byte of a block, and one whose read is the
    first bin of the window and the last byte of a block.  That one bin of the
    spectrum carries the whole crossing; everything else is at the noise floor.
    With P in natural order the groups start on multiples of 8, and a few terms
    have no such bin: a window of one bin ((4, 1), (5, 1): 8 bins read one
    index) is then taken on the block edge, and for (2, 3) (windows 6 g .. 6 g
    + 5, never odd, never ending on a multiple of 8) a window that spans two
    blocks, planted at its last and at its first bin."""
    from peasoup_amd import ops

    thresh = 5.0
    rng = np.random.default_rng(7 + nlev)
    n, Kb = 90003, 8
    P = rng.normal(0.0, 0.05, (Kb, n)).astype(np.float32)
    scale = [1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25, 2 ** -2.5]
    terms = [(h, m) for h in range(1, nlev + 1) for m in range(1, 1 << h, 2)]
    planted, strict = {}, {}
    slot = 0
    for h, m in terms:
        for edge in ("last", "first"):
            k = slot % Kb
            g0 = 1500 + 260 * (slot // Kb)  # groups far apart within a trial
            slot += 1
            found = None
            for pref in (0, 1, 2):
                for g in range(g0, g0 + 256):
                    f = 8 * g
                    a, b = _idx(f, h, m), _idx(f + 7, h, m)
                    on_edge = b % 8 == 0 if edge == "last" else a % 8 == 7
                    ok = (on_edge and b > a, on_edge, a >> 3 != b >> 3)[pref]
                    if ok:
                        found = (f + 7, b) if edge == "last" else (f, a)
                        break
                if found:
                    break
            strict[(h, m, edge)] = pref == 0
            i, j = found
            P[k, j] = 1.1 * thresh / scale[h]  # < 31.5: inside the byte range
            planted[(h, m, edge)] = (k, h, i)
    assert len(planted) == 2 * len(terms), "an edge case for every term"
    # the terms whose windows cannot end on a block edge with groups on multiples of 8
    loose = {(h, m) for h, m in terms if not (strict[(h, m, "last")] or strict[(h, m, "first")])}
    assert loose == {t for t in [(2, 3), (4, 1), (5, 1)] if t in terms}
    starts, ends = _ranges(n)
    Pt = torch.from_numpy(P).to(dev)
    Q = ops.quantize_q8(Pt)
    assert int(Q.max()) < 254
    ref = _three_way(Pt, Q, nlev, starts, ends, thresh, lambda old: (old, old ^ 65536))
    got = {(r[0], r[1], r[2]) for r in ref}
    for h, m in terms:
        assert planted[(h, m, "last")] in got or planted[(h, m, "first")] in got, (h, m)
    assert all(v in got for v in planted.values())


@pytest.mark.parametrize("nlev", [3, 5])
def test_out_of_range_bytes(nlev):
    """A single 254 (large value, NaN) and a single 255 (below -32) on a block
    boundary and on the last bin of a row, in otherwise quiet trials."""
    from peasoup_amd import ops

    thresh = 6.0
    rng = np.random.default_rng(21 + nlev)
    n, Kb = 70003, 8
    P = rng.normal(0.0, 0.05, (Kb, n)).astype(np.float32)
    spots = {0: (40000, 1e6), 1: (40007, 1e6), 2: (n - 1, 1e6), 3: (24008, np.nan), 4: (n - 1, np.nan),
             5: (32000, -50.0), 6: (32007, -50.0), 7: (n - 1, -50.0)}
    for k, (b, v) in spots.items():
        P[k, b] = v
        P[k, 3001 + 8 * k] = 3.0 * thresh  # one plain peak per trial
    # a value below the range next to bins that cross without it
    P[5, 16000] = 30.0
    starts = [3, 11, 19, 35, 67, 131]
    ends = [n] * 6  # the last bin of the row is searched
    Pt = torch.from_numpy(P).to(dev)
    Q = ops.quantize_q8(Pt)
    Qh = Q.cpu().numpy()
    for k, (b, v) in spots.items():
        assert Qh[k, b] == (255 if v < 0 else 254), (k, b, Qh[k, b])
        assert b % 8 in (0, 7) or b == n - 1
    assert int((Qh[:, :n] >= 254).sum()) == len(spots)
    ref = _three_way(Pt, Q, nlev, starts, ends, thresh, lambda old: (old, old ^ 65536))
    assert len(ref) > 20


def test_dense_tiles():
    """Most groups flagged: every record exactly once from the flagged-group path."""
    from peasoup_amd import ops

    rng = np.random.default_rng(33)
    n, Kb = 100003, 8
    P = (rng.exponential(1.0, (Kb, n)) - 1.0).astype(np.float32)
    starts, ends = _ranges(n)
    Pt = torch.from_numpy(P).to(dev)
    Q = ops.quantize_q8(Pt)
    ref = _three_way(Pt, Q, 3, starts, ends, 5.0, lambda old: (old, old ^ 65536))
    assert len(ref) > 1000
    assert len(set((r[0], r[1], r[2]) for r in ref)) == len(ref)


def _series(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) * 64e-6
    x = rng.standard_normal(n)
    ph = (t / 0.00731) % 1.0
    x += 2.0 * (np.minimum(ph, 1 - ph) < 0.03)
    return torch.from_numpy(x.astype(np.float32)).to(dev)


@pytest.mark.parametrize("nlev,thresh", [(3, 6.0), (4, 7.0)])
def test_r2c_screening_rows(nlev, thresh):
    """Q as the tiled r2c kernel writes it (natural P, no shift)."""
    from peasoup_amd import ops

    n = 1 << 17
    x = _series(n, 5)
    accs = [float(a) for a in np.linspace(-60, 60, 8)]
    st = torch.tensor([0.0, 0.0, 0.5 / np.sqrt(n), 0.0], dtype=torch.float32, device=dev)
    P, Q = ops.fft4_resample_interbin(x, accs, 64e-6, st, float(n), screen=True)
    M = n // 2
    starts = [3, 11, 19, 35, 67, 131]
    ends = [M + 1, M - 3, M + 1, M - 99, M + 1, M + 1]
    ref = _three_way(P, Q, nlev, starts, ends, thresh, lambda old: (old, old ^ 65536))
    assert len(ref) > 20


@pytest.mark.parametrize("nlev,thresh", [(3, 6.0), (4, 7.0), (1, 5.5)])
def test_blocked_spectrum_shifted_rows(nlev, thresh):
    """The fused spectrum pass's layouts: blocked P and Q rows shifted by
    spec_q_shift (the tiles then start below bin 0 of the row)."""
    import peasoup_amd._C as C
    from peasoup_amd import ops

    n = 1 << 17
    x = _series(n, 9)
    accs = [float(a) for a in np.linspace(-60, 60, 8)]
    st = torch.tensor([0.0, 0.0, 0.5 / np.sqrt(n), 0.0], dtype=torch.float32, device=dev)
    Pb, Q, g = ops.fft4_spectrum_pass(x, accs, 64e-6, st, float(n))
    assert C.kernels.spec_q_shift % 16 != 0
    Pn = ops.spec_unblock(Pb, g).contiguous()
    M = g.n1 * g.n2
    starts = [3, 11, 19, 35, 67, 131]
    ends = [M + 1, M - 3, M + 1, M - 99, M + 1, M + 1]
    ref = _three_way(Pb, Q, nlev, starts, ends, thresh, lambda old: (old, old ^ 65536), Pnat=Pn, nbins=M + 1, pblk=g)
    assert len(ref) > 20


def test_engine_groups_equal_per_bin():
    """SearchEngine.search_trial with the group screen on and off: identical
    candidates, S/N bit for bit (both read the same P), on the fused spectrum
    pass (blocked P) and with the exact sums recomputed from the spectrum."""
    import peasoup_amd._C as C

    rng = np.random.default_rng(5)
    n = (1 << 21) + 100
    t = np.arange(n) * 64e-6
    x = rng.normal(128, 6, n)
    ph = (t / 0.0123) % 1.0
    x += 25.0 * (np.minimum(ph, 1 - ph) < 0.02)
    trial = torch.from_numpy(np.clip(np.rint(x), 0, 255).astype(np.uint8)).to(dev)
    accs = [float(a) for a in np.linspace(-40, 40, 17)]
    old = C.kernels.harmonic_flags()
    out = {}
    try:
        for name, base in (("fused", old | 64), ("fromx", (old & ~64) | 8)):
            for on in (True, False):
                C.kernels.harmonic_set_flags(base | GROUPS if on else base & ~GROUPS)
                p = C.SearchParams()
                p.fft_size, p.tsamp, p.nharmonics = 1 << 21, 64e-6, 4
                eng = C.SearchEngine(p, torch.cuda.current_stream().cuda_stream)
                c = eng.search_trial(trial.data_ptr(), n, 10.0, 3, accs)
                out[(name, on)] = [(x.dm_idx, x.acc, x.nh, x.snr, x.freq, x.count_assoc()) for x in c]
    finally:
        C.kernels.harmonic_set_flags(old)
    for name in ("fused", "fromx"):
        assert out[(name, True)] == out[(name, False)] and len(out[(name, True)]) > 0
