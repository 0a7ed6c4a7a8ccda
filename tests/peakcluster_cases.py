"""Cases shared by test_peakcluster_cases.py (CPU audit), test_peakcluster_paths_gpu.py and
test_peakcluster_gpu.py: the record format of the harmonic kernel, segments built to reach named
branches of csrc/kernels/peakcluster.hip, and the oracle (reference.unique_peaks).

A case is a dict: name, gap, nseg, region_log2, cap, records (uint32 [rows, 3], rows > cap: the
slack holds stale chunks), counts (uint32, one per record region) and segs {segment: (idx int32
ascending distinct, snr float32)} -- the crossings the clustering has to see.

Families and the branch each was built for (kernel names as in peakcluster.hip):
  sizes          n on the row / wave edges of both peak_cluster_kernel instances, the raw hand-off
                 (n > cluster_cap), nseg = 18: blockIdx = segment.
  radix_small    step 1's LSD radix sort in the 512-thread kernel: m = 512 (last rank sort), 513,
                 4..8 passes from first-idx spans on both sides of 2^16, 2^20, 2^24, 2^28 and the
                 largest idx below 2^31 - 64, chunks arriving ascending / descending, chunks of
                 every length 1..64 (step 2's gather).
  radix_large    the same in the 1024-thread kernel: m = 1024, 1025, m near n, n = cluster_cap.
  one            nseg = 1.
  shapes_g*      steps 3a-4 on structured S/N (gaps 1, 2, 29, 30), in both kernels, >= 2 rows:
                 falling / rising / equal / sawtooth on consecutive bins (3a's fast path, step 4's
                 long chain), spacing gap and gap - 1 (the `< gap` boundary, 3a's and 3c's binary
                 searches), stretches of dense and sparse bins switching at multiples of 64 and at
                 the row length +- 1 (3b's block / row stitching), equal-S/N pairs.
  gap_*          every gap 1..30, nseg = 8 (the XCD segment remap), all segments distinct.
  lds_limit      nseg = 8192: seg_hist_kernel / seg_scatter_kernel at kSegLds, remapped.
  global         nseg = 8200: seg_hist_global_kernel / seg_scatter_global_kernel.
  regions3, global_regions   region_log2 > 0: RecRegions / region_end in both pairs of kernels.
  over_cap, stale, bad_desc, regions_damaged   chunk_ok: see the builders' docstrings."""
import functools

import numpy as np

from peasoup_amd.utils import reference as ref

CHUNK = 0x80000000   # kernels.hpp kPeakChunk
RAW = 0x80000000     # kClusterRaw
SMALL = 4096         # peakcluster.hip kClSmall
TH_SMALL, TH_LARGE = 512, 1024  # threads = row length of the two kernels
SEG_LDS = 8192       # kSegLds
STRIDE = 32          # kPeakRegionStride
BLOCK = 4096         # records per hist / scatter block: a region is a whole number of them
CAP_SEG = 14000      # kClusterCap (the audit checks it against the extension's)
SLACK = 256
SHAPE_GAPS = (1, 2, 29, 30)


# ---------------------------------------------------------------- records ----
def chunks_of(segs):
    """The chunks (segment, idx, snr) of every segment: one per 64-bin group with crossings."""
    out = []
    for s, (idx, snr) in segs.items():
        if len(idx) == 0:
            continue
        cuts = np.flatnonzero(np.diff(idx >> 6)) + 1
        for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(idx)]):
            out.append((s, idx[a:b], snr[a:b]))
    return out


def chunk_rows(chunks, base=0):
    """Chunks laid down from row `base`: descriptor {CHUNK | count << 16 | segment, first idx,
    absolute position of the first crossing}, then the crossings {segment, idx, snr bits}."""
    rows, pos = [], base
    for s, ci, cs in chunks:
        c = len(ci)
        rows.append(np.array([[CHUNK | (c << 16) | s, int(ci[0]), pos + 1]], np.uint32))
        rows.append(np.stack([np.full(c, s, np.uint32), ci.view(np.uint32), cs.view(np.uint32)], axis=1))
        pos += 1 + c
    return np.concatenate(rows) if rows else np.zeros((0, 3), np.uint32)


def shuffled(chunks, rng, order=None):
    """Chunks in any order; order = {segment: "asc" | "desc"} sorts that segment's chunks by
    first idx within the slots they drew."""
    perm = [chunks[k] for k in rng.permutation(len(chunks))]
    for s, how in (order or {}).items():
        slots = [k for k, c in enumerate(perm) if c[0] == s]
        mine = sorted((perm[k] for k in slots), key=lambda c: int(c[1][0]), reverse=(how == "desc"))
        for k, c in zip(slots, mine):
            perm[k] = c
    return perm


def chunked_records(segs, rng, order=None):
    """Records as harmonic_peaks_batch emits them: per segment, runs of idx-ascending crossings
    of one 64-bin group, each behind its descriptor; chunks in any order (kernels.hpp kPeakChunk)."""
    return chunk_rows(shuffled(chunks_of(segs), rng, order))


def stale_rows(rng, nrows, base, nseg):
    """Exactly nrows rows of well-formed left-over chunks (positions absolute from `base`, segment
    below nseg, S/N above every live crossing: clustering one of them changes the answer)."""
    chunks, left = [], nrows
    while left >= 2:
        c = int(min(left - 1, rng.integers(1, 65)))
        off = np.sort(rng.choice(64, c, replace=False))
        chunks.append((int(rng.integers(0, nseg)), (64 * int(rng.integers(0, 1 << 14)) + off).astype(np.int32),
                       (5000.0 + 100.0 * rng.random(c)).astype(np.float32)))
        left -= 1 + c
    rows = chunk_rows(chunks, base)
    if left:  # one row over: a crossing of no chunk
        rows = np.concatenate([rows, np.array([[0, 7, 0x43FA0000]], np.uint32)])
    return rows


def held_chunks(case):
    """The documented rule (peakcluster.hip chunk_ok) read off the buffer: per segment the
    descriptors (row, first idx, position, count) a clustering may use, in buffer order."""
    rec, cap, log2 = case["records"], case["cap"], case["region_log2"]
    capr = cap >> log2
    out = {}
    for r in range(1 << log2):
        end = r * capr + min(int(case["counts"][r]), capr)
        rows = np.arange(r * capr, end)
        d = rec[rows]
        ok = ((d[:, 0] & CHUNK) != 0) & ((d[:, 0] & 0xFFFF) < case["nseg"]) & \
            (d[:, 2].astype(np.int64) + ((d[:, 0] >> 16) & 0x7F) <= end)
        for row in rows[ok]:
            f = int(rec[row, 0])
            out.setdefault(f & 0xFFFF, []).append((int(row), int(rec[row, 1]), int(rec[row, 2]), (f >> 16) & 0x7F))
    return out


def held_segments(case):
    """The segments those descriptors describe, crossings in idx order."""
    rec, out = case["records"], {}
    for s, ds in held_chunks(case).items():
        rows = np.concatenate([np.arange(p, p + c) for _, _, p, c in sorted(ds, key=lambda d: d[1])])
        out[s] = (rec[rows, 1].view(np.int32), rec[rows, 2].view(np.float32))
    return out


def lay_out(name, segs, gap, nseg, seed, region_log2=0, order=None):
    """An undamaged batch: chunks shuffled (dealt round-robin to the regions), stale chunks in the
    unused part of every region and in the slack behind the capacity."""
    rng = np.random.default_rng(seed)
    chunks = shuffled(chunks_of(segs), rng, order)
    R = 1 << region_log2
    if region_log2 == 0:
        rows = chunk_rows(chunks)
        cap = len(rows) + 100
        parts, counts = [rows, stale_rows(rng, cap + SLACK - len(rows), len(rows), nseg)], [len(rows)]
    else:
        deal = [chunks[r::R] for r in range(R)]
        need = max(sum(1 + len(c[1]) for c in d) for d in deal)
        capr = BLOCK * max(1, -(-need // BLOCK))
        cap, parts, counts = R * capr, [], []
        for r in range(R):
            rows = chunk_rows(deal[r], r * capr)
            parts += [rows, stale_rows(rng, capr - len(rows), r * capr + len(rows), nseg)]
            counts.append(len(rows))
        parts.append(stale_rows(rng, SLACK, cap, nseg))
    return dict(name=name, gap=gap, nseg=nseg, region_log2=region_log2, cap=cap, records=np.concatenate(parts),
                counts=np.array(counts, np.uint32), segs={s: v for s, v in segs.items() if len(v[0])})


# --------------------------------------------------------------- segments ----
def bumpy(rng, idx, ties):
    """Bumps (runs of crossings rising to a peak and falling) plus noise; ties: S/N in halves,
    so equal neighbours meet the strict '>' rule."""
    n = len(idx)
    snr = 9.0 + 40.0 * rng.random(n)
    lo, hi = int(idx[0]), int(idx[-1]) + 1
    for c in rng.integers(lo, hi, max(1, n // 200)):
        snr += 200.0 * np.exp(-0.5 * ((idx - c) / (5 + 40 * rng.random())) ** 2)
    if ties:
        snr = np.round(snr * 2) / 2
    return snr.astype(np.float32)


def random_seg(rng, n, spread, base=0, ties=False):
    """n crossings drawn from n * spread + 10 bins from `base`: dense (1) to sparse."""
    idx = (base + np.sort(rng.choice(n * spread + 10, n, replace=False))).astype(np.int32)
    return idx, bumpy(rng, idx, ties)


def seg_of_chunks(rng, groups, counts, offs=None, ties=False):
    """One chunk per 64-bin group: counts[j] distinct bins of group groups[j], the lowest at
    offs[j] where given."""
    parts = []
    for j, (g, c) in enumerate(zip(groups, counts)):
        o = None if offs is None else offs[j]
        if o is None:
            b = np.sort(rng.choice(64, c, replace=False))
        else:
            b = np.r_[o, o + 1 + np.sort(rng.choice(63 - o, c - 1, replace=False))] if c > 1 else np.array([o])
        parts.append(64 * int(g) + b)
    idx = np.concatenate(parts).astype(np.int32)
    assert np.all(np.diff(idx) > 0)
    return idx, bumpy(rng, idx, ties)


def seg_m(rng, n, m, g0, span=None, ties=False):
    """n crossings in exactly m chunks whose first idx run from 64 g0 to 64 g0 + span (both
    ends one-crossing chunks); span None: groups one or two apart."""
    if span is None:
        groups = g0 + np.cumsum(np.r_[0, rng.integers(1, 3, m - 1)])
        last_off = 0
    else:
        g1, last_off = g0 + (span >> 6), span & 63
        mid = set()
        while len(mid) < m - 2:
            mid.update(rng.integers(g0 + 1, g1, m - 2 - len(mid)).tolist())
        groups = np.r_[g0, np.sort(np.fromiter(mid, np.int64)), g1]
    extra = np.bincount(rng.choice((m - 2) * 63, n - m, replace=False) // 63, minlength=m - 2)
    counts = np.r_[1, 1 + extra, 1]
    offs = [0] + [None] * (m - 2) + [last_off]
    return seg_of_chunks(rng, groups, counts, offs, ties)


def shape_segments(gap, seed):
    """The structured S/N shapes at one gap, each in the small kernel (1100 crossings: 3 rows of
    512) and the large one (4500: 5 rows of 1024); {segment: (name, idx, snr)}, all distinct."""
    rng = np.random.default_rng(seed)
    out = {}

    def add(name, idx, snr):
        s = len(out)
        idx = np.asarray(idx, np.int64) + 100000 * s + 7 * s  # no two segments alike
        out[s] = (name, idx.astype(np.int32), np.asarray(snr, np.float32))

    for n, row in ((1100, TH_SMALL), (4500, TH_LARGE)):
        i = np.arange(n)
        add("falling", i, 3000.0 - 0.5 * i)       # all survive; one run: step 4 follows n / gap jumps
        add("rising", i, 10.0 + 0.5 * i)          # one survivor, the last crossing
        add("equal", i, np.full(n, 25.0))         # every crossing survives
        for p in sorted({max(1, gap - 1), gap, gap + 1}):
            add(f"saw{p - gap:+d}", i, 10.0 + (i % p))
        add("spaced_gap", gap * i, bumpy(rng, gap * i, True))              # every crossing its own cluster
        if gap > 1:
            add("spaced_gap-1", (gap - 1) * i, bumpy(rng, (gap - 1) * i, True))  # one chain
        # dense and sparse stretches switching at multiples of 64 and at the row length +- 1
        cuts = sorted({64, 128, 192, 320, row - 1, row + 1, row + 64, 2 * row - 1, 2 * row + 1, 2 * row + 128}
                      | {3 * row - 1, 3 * row + 1, 4 * row - 64, 4 * row + 1})
        cuts = [c for c in cuts if c < n]
        step, dense, sparse = np.ones(n, np.int64), True, [max(2, gap - 1), max(2, gap), gap + 5]
        for a, b in zip([0] + cuts, cuts + [n]):
            if not dense:
                step[a:b] = [sparse[k % 3] for k in range(b - a)]
            dense = not dense
        idx = np.cumsum(step)
        add("alternating", idx, bumpy(rng, idx, True))
        # equal-S/N pairs gap - 1 (where that is a spacing) and gap apart, 3 gap between pairs
        d = np.array([gap - 1 if (k % 2 == 0 and gap > 1) else gap for k in range(n // 2)])
        a0 = np.cumsum(np.r_[0, d[:-1] + 3 * gap])
        v = (9.0 + rng.integers(0, 40, n // 2)).astype(np.float32)
        add("pairs", np.stack([a0, a0 + d], axis=1).reshape(-1), np.repeat(v, 2))
    return out


# ------------------------------------------------------------------ cases ----
def _sizes():
    rng = np.random.default_rng(101)
    sizes = [63, 64, 65, 0, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, CAP_SEG - 1, CAP_SEG, CAP_SEG + 1, 0, 1]
    segs = {s: random_seg(rng, n, 1 + s % 4, base=977 * s, ties=s % 2 == 0) for s, n in enumerate(sizes) if n}
    return lay_out("sizes", segs, 30, len(sizes), 1)


RADIX_SPANS = [(1 << 16) - 1, 1 << 16, (1 << 20) - 1, 1 << 20, (1 << 24) - 1, 1 << 24, (1 << 28) - 1, 1 << 28,
               (1 << 31) - 65]


def _radix_small():
    rng = np.random.default_rng(102)
    segs = {}
    for s, span in enumerate(RADIX_SPANS):  # 0..8: the pass counts; the last starts at idx 0
        segs[s] = seg_m(rng, 1500 + 300 * s, 520 + 7 * s, 0 if span == (1 << 31) - 65 else 3 + s, span, ties=s % 2 == 1)
    segs[9] = seg_m(rng, 2000, 512, 50)    # last rank sort
    segs[10] = seg_m(rng, 2001, 513, 60)   # first radix sort
    segs[11] = seg_m(rng, 3000, 700, 70, ties=True)   # chunks arrive ascending
    segs[12] = seg_m(rng, 3100, 800, 80, ties=True)   # chunks arrive descending
    segs[13] = seg_m(rng, 4096, 4000, 90)  # m near n at the small kernel's capacity
    lens = rng.permutation(64) + 1         # chunks of every length 1..64
    segs[14] = seg_of_chunks(rng, 1000 + 2 * np.arange(64), lens)
    segs[15] = seg_of_chunks(rng, 2000 + np.arange(192), np.r_[lens, lens[::-1], lens], ties=True)
    return lay_out("radix_small", segs, 30, 16, 2, order={11: "asc", 12: "desc"})


def _radix_large():
    rng = np.random.default_rng(103)
    segs = {0: seg_m(rng, 6000, 1024, 5),            # last rank sort of the large kernel
            1: seg_m(rng, 6001, 1025, 9),            # first radix sort
            2: seg_m(rng, 5000, 4990, 11, ties=True),    # almost every crossing its own chunk
            3: seg_m(rng, CAP_SEG, 2000, 13, (1 << 24) + 77),
            4: seg_m(rng, CAP_SEG - 1, 13000, 17, (1 << 31) - 65 - 64 * 17, ties=True),
            5: seg_m(rng, 4097, 1500, 19, (1 << 20) - 1),
            6: seg_m(rng, 9000, 3000, 23, (1 << 22) + 5, ties=True),
            7: seg_m(rng, 7000, 1100, 29, 1 << 28)}
    return lay_out("radix_large", segs, 7, 8, 3, order={6: "desc", 7: "asc"})


def _one():
    rng = np.random.default_rng(104)
    return lay_out("one", {0: seg_m(rng, 2500, 600, 4, ties=True)}, 5, 1, 4)


def _shapes(gap):
    segs = {s: (idx, snr) for s, (_, idx, snr) in shape_segments(gap, 200 + gap).items()}
    return lay_out(f"shapes_g{gap}", segs, gap, 64, 10 + gap)


def _gap(gap):
    rng = np.random.default_rng(300 + gap)
    segs = {0: random_seg(rng, 100 + gap, 3, 0, True), 1: random_seg(rng, 513 + gap, 1 + gap % 3, 500),
            2: random_seg(rng, 700, 2, 900 + gap, True), 3: random_seg(rng, 1500, 1, 70 * gap),
            4: seg_m(rng, 2500, 600 + gap, 3 + gap, ties=True), 5: random_seg(rng, 4500, 1 + gap % 2, 11 * gap, True),
            6: seg_m(rng, 6000, 1100 + gap, 7), 7: random_seg(rng, 37 + gap, 20, 5)}
    return lay_out(f"gap_{gap}", segs, gap, 8, 20 + gap, order={4: "asc" if gap % 2 else "desc"})


def _many(name, nseg, ids, seed, region_log2=0):
    rng = np.random.default_rng(seed)
    segs = {}
    for k, s in enumerate(ids):
        segs[s] = seg_m(rng, 1200 + 100 * k, 520 + k, 3 + k) if k % 4 == 1 else \
            random_seg(rng, 40 + 333 * k, 1 + k % 3, base=13 * s + k, ties=k % 2 == 0)
    return lay_out(name, segs, 30, nseg, seed, region_log2)


def _regions3():
    rng = np.random.default_rng(105)
    segs = {0: random_seg(rng, 5000, 1, 0, True), 1: seg_m(rng, 3000, 700, 5), 2: random_seg(rng, 900, 3, 50),
            3: random_seg(rng, 4096, 2, 99, True), 4: seg_m(rng, 8000, 1300, 8, ties=True), 5: random_seg(rng, 64, 1, 7),
            7: random_seg(rng, 513, 1, 300)}
    return lay_out("regions3", segs, 12, 8, 5, region_log2=3)


def _live(rng, sizes, nseg_live):
    """Mixed live segments of a damaged batch; S/N below the stale chunks' 5000."""
    return {s: (seg_m(rng, n, n // 4, 3 + s, ties=True) if s % 3 == 2 and n >= 16 else
                random_seg(rng, n, 1 + s % 3, 40 * s, s % 2 == 0)) for s, n in zip(range(nseg_live), sizes) if n}


def _without(segs, chunk):
    """segs with one chunk (segment, idx, snr) removed."""
    s, ci, _ = chunk
    idx, snr = segs[s]
    keep = ~np.isin(idx, ci)
    out = dict(segs)
    out[s] = (idx[keep], snr[keep])
    return {k: v for k, v in out.items() if len(v[0])}


def _over_cap():
    """*d_count = cap + 37; the last chunk's descriptor lies below cap, its crossings end past
    it (chunk_ok's position + count <= n with n = min(count, cap)): the chunk is dropped."""
    rng = np.random.default_rng(106)
    segs = _live(rng, [3000, 700, 5000, 64, 1500, 2200, 513, 90], 8)
    chunks = shuffled(chunks_of(segs), rng)
    k = max(range(len(chunks)), key=lambda j: (len(chunks[j][1]) >= 8 and chunks[j][0] == 0, j))
    cut = chunks.pop(k)
    cut = (cut[0], cut[1], (cut[2] + np.float32(300.0)).astype(np.float32))  # it would win its neighbourhood
    segs[0] = (segs[0][0], np.where(np.isin(segs[0][0], cut[1]), segs[0][1] + np.float32(300.0), segs[0][1]).astype(np.float32))
    rows = chunk_rows(chunks + [cut])
    cap = len(rows) - len(cut[1]) // 2  # the descriptor and half the crossings below cap
    rec = np.concatenate([rows, stale_rows(rng, cap + 37 + SLACK - len(rows), len(rows), 8)])
    return dict(name="over_cap", gap=30, nseg=8, region_log2=0, cap=cap, records=rec,
                counts=np.array([cap + 37], np.uint32), segs=_without(segs, cut), full=segs)


def _stale():
    """Well-formed descriptors of well-formed crossings beyond *d_count (hist / scatter stop at
    region_end): ignored.  lay_out() puts them there; here they fill five blocks."""
    rng = np.random.default_rng(107)
    segs = _live(rng, [2000, 4500, 300, 65, 1025, 800, 0, 3000, 1, 0, 700, 130], 12)
    rows = chunk_rows(shuffled(chunks_of(segs), rng))
    cap = len(rows) + 5 * BLOCK
    rec = np.concatenate([rows, stale_rows(rng, cap + SLACK - len(rows), len(rows), 12)])
    return dict(name="stale", gap=9, nseg=12, region_log2=0, cap=cap, records=rec,
                counts=np.array([len(rows)], np.uint32), segs={s: v for s, v in segs.items() if len(v[0])})


def _bad_desc():
    """Inside the count: descriptors of segments >= nseg (chunk_ok's chunk_seg < nseg) with their
    crossings, and crossings of no chunk whose idx / snr fields look like positions: ignored."""
    rng = np.random.default_rng(108)
    nseg = 18
    segs = _live(rng, [1500, 4200, 600, 64, 2049, 900, 333, 5000, 77], 9)
    chunks = shuffled(chunks_of(segs), rng)
    alien = [(s, c[1], (c[2] + np.float32(400.0)).astype(np.float32)) for s, c in
             zip([18, 19, 31, 0x7FFF, 0xFFFF, 18 + 256, 18, 4096], chunks[:8])]  # copies of live chunks, elsewhere
    mixed = chunks + alien
    mixed = [mixed[k] for k in rng.permutation(len(mixed))]
    parts, pos = [], 0
    for k, c in enumerate(mixed):
        parts.append(chunk_rows([c], pos))
        pos += 1 + len(c[1])
        if k % 7 == 3:  # a crossing of no chunk: segment in range, fields that are valid positions
            parts.append(np.array([[k % nseg, pos - 5, pos - 3], [k % nseg, 3, 1]], np.uint32))
            pos += 2
    rows = np.concatenate(parts)
    cap = len(rows) + 100
    rec = np.concatenate([rows, stale_rows(rng, cap + SLACK - len(rows), len(rows), nseg)])
    return dict(name="bad_desc", gap=30, nseg=nseg, region_log2=0, cap=cap, records=rec,
                counts=np.array([len(rows)], np.uint32), segs=segs)


def _regions_damaged():
    """region_log2 = 2, cap = 4 x 4096.  Region 0: stale descriptors after its count; region 1:
    empty (count 0, stale chunks in it); region 2: count above capr and a chunk cut at the region's
    end (its missing crossings would be region 3's first records); region 3: plain."""
    rng = np.random.default_rng(109)
    capr, cap = BLOCK, 4 * BLOCK
    segs = _live(rng, [2600, 2000, 1500, 1200, 900, 600, 300, 65], 8)
    chunks = shuffled(chunks_of(segs), rng)
    r2, rows2 = [], 0
    while True:  # region 2: whole chunks, then the one that does not fit
        c = chunks.pop()
        if rows2 + 1 + len(c[1]) > capr:
            cut = c
            break
        r2.append(c)
        rows2 += 1 + len(c[1])
    assert rows2 < capr and len(cut[1]) >= 2  # the descriptor is held, the crossings are not all
    cut = (cut[0], cut[1], (cut[2] + np.float32(300.0)).astype(np.float32))
    full = dict(segs)
    i_, s_ = segs[cut[0]]
    full[cut[0]] = (i_, np.where(np.isin(i_, cut[1]), s_ + np.float32(300.0), s_).astype(np.float32))
    half = len(chunks) // 2
    r0, r3 = chunks[:half], chunks[half:]
    p0, p3 = chunk_rows(r0, 0), chunk_rows(r3, 3 * capr)
    assert len(p0) < capr - 200 and len(p3) < capr - 200
    p2 = chunk_rows(r2 + [cut], 2 * capr)[:capr]
    rec = np.concatenate([p0, stale_rows(rng, capr - len(p0), len(p0), 8),
                          stale_rows(rng, capr, capr, 8),
                          p2,
                          p3, stale_rows(rng, capr - len(p3), 3 * capr + len(p3), 8),
                          stale_rows(rng, SLACK, cap, 8)])
    counts = np.array([len(p0), 0, rows2 + 1 + len(cut[1]) + 100, len(p3)], np.uint32)
    return dict(name="regions_damaged", gap=30, nseg=8, region_log2=2, cap=cap, records=rec, counts=counts,
                segs=_without(full, cut), full=full)


BUILDERS = {"sizes": _sizes, "radix_small": _radix_small, "radix_large": _radix_large, "one": _one,
            **{f"shapes_g{g}": functools.partial(_shapes, g) for g in SHAPE_GAPS},
            **{f"gap_{g}": functools.partial(_gap, g) for g in range(1, 31)},
            "lds_limit": functools.partial(_many, "lds_limit", 8192, [0, 1, 7, 8, 1023, 1024, 4097, 8184, 8191], 110),
            "global": functools.partial(_many, "global", 8200, [0, 9, 1025, 4096, 8191, 8192, 8193, 8199], 111),
            "regions3": _regions3,
            "global_regions": functools.partial(_many, "global_regions", 8200, [0, 5, 8191, 8192, 8199], 112, 2)}
DAMAGED = {"over_cap": _over_cap, "stale": _stale, "bad_desc": _bad_desc, "regions_damaged": _regions_damaged}
NAMES = list(BUILDERS)
DAMAGED_NAMES = list(DAMAGED)


@functools.lru_cache(maxsize=None)
def case(name):
    return (BUILDERS.get(name) or DAMAGED[name])()


def cluster(idx, snr, gap):
    """The oracle on one segment: (idx int32, snr float32) of its cluster peaks."""
    pk = ref.unique_peaks(idx.tolist(), snr.tolist(), gap)
    return np.array([p[0] for p in pk], np.int32), np.array([p[1] for p in pk], np.float32)


@functools.lru_cache(maxsize=None)
def expected(name, cap_seg=CAP_SEG):
    """{segment: oracle peaks} of every segment the device clusters (n <= cap_seg)."""
    c = case(name)
    return {s: cluster(idx, snr, c["gap"]) for s, (idx, snr) in c["segs"].items() if len(idx) <= cap_seg}


def path(idx, cap_seg=CAP_SEG):
    """What peak_cluster_batch does with a segment, from its crossings alone: the kernel, the
    chunk count m, step 1's sort and, for the radix sort, its passes."""
    n = len(idx)
    first = idx[np.r_[True, np.diff(idx >> 6) != 0]] if n else idx
    m = len(first)
    kernel = "empty" if n == 0 else "small" if n <= SMALL else "large" if n <= cap_seg else "raw"
    out = dict(n=n, m=m, kernel=kernel, sort=None, passes=None, span=None,
               lens=np.unique(idx >> 6, return_counts=True)[1])
    if kernel in ("small", "large"):
        radix = m > (TH_SMALL if kernel == "small" else TH_LARGE)
        out["sort"] = "radix" if radix else "rank"
        if radix:
            span = int(first[-1]) - int(first[0])
            out["span"] = span
            out["passes"] = 1 if span == 0 else (span.bit_length() + 3) // 4
    return out
