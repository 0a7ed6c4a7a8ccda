"""CPU audit of the peak-clustering sweep (peakcluster_cases.py): the two host implementations of the
reference's rule agree on every case, bit for bit, and the case data alone proves which branch of
csrc/kernels/peakcluster.hip each family reaches -- the kernel (n == 0 / small n <= 4096 / large
n <= cluster_cap / raw), the chunk count m, step 1's sort (rank m <= threads, else radix) and the
radix pass count (bits(first-idx span) + 3) / 4 -- as peak_cluster_kernel computes them.  The record
buffers are read back with the documented validity rule (chunk_ok) and must describe exactly the
segments of the case, the damaged ones included."""
import numpy as np
import pytest

import peakcluster_cases as pc

ALL = pc.NAMES + pc.DAMAGED_NAMES


def test_constants_are_the_kernels(C):
    K = C.kernels
    assert int(K.cluster_cap) == pc.CAP_SEG and int(K.peak_region_stride) == pc.STRIDE


@pytest.mark.parametrize("name", ALL)
def test_host_scans_agree(C, name):
    """C.identify_unique_peaks == reference.unique_peaks, idx and S/N bits, on every segment."""
    c = pc.case(name)
    exp = pc.expected(name)
    assert exp
    for s, (idx, snr) in c["segs"].items():
        if s not in exp:
            assert len(idx) > pc.CAP_SEG
            continue
        gi, gs = C.identify_unique_peaks(idx.tolist(), snr.tolist(), c["gap"])
        assert np.array_equal(np.array(gi, np.int32), exp[s][0]), (name, s)
        assert np.array_equal(np.array(gs, np.float32).view(np.uint32), exp[s][1].view(np.uint32)), (name, s)


@pytest.mark.parametrize("name", ALL)
def test_records_hold_the_segments(name):
    """The buffer, read with the validity rule, holds exactly the case's segments: ascending distinct
    idx, chunks of one 64-bin group, positions inside the records held."""
    c = pc.case(name)
    assert len(c["records"]) >= c["cap"] + pc.SLACK  # every row a kernel may read is allocated and defined
    if c["region_log2"]:
        assert (c["cap"] >> c["region_log2"]) % pc.BLOCK == 0
    got = pc.held_segments(c)
    assert sorted(got) == sorted(c["segs"])
    for s, (idx, snr) in c["segs"].items():
        assert idx.dtype == np.int32 and snr.dtype == np.float32 and np.all(np.diff(idx) > 0) and idx[0] >= 0
        assert 0 <= s < c["nseg"]
        assert np.array_equal(got[s][0], idx) and np.array_equal(got[s][1].view(np.uint32), snr.view(np.uint32))
        assert float(snr.max()) < 5000.0  # below every stale crossing
    for s, ds in pc.held_chunks(c).items():
        assert len(ds) == pc.path(c["segs"][s][0])["m"]


def test_damaged_cases_lose_what_they_must():
    """The dropped chunk matters: clustering it too gives another answer."""
    for name in ("over_cap", "regions_damaged"):
        c = pc.case(name)
        differs = 0
        for s, (idx, snr) in c["full"].items():
            a = pc.cluster(idx, snr, c["gap"])
            b = pc.expected(name).get(s)
            differs += b is None or len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0])
        assert differs == 1, name
    c = pc.case("over_cap")
    assert int(c["counts"][0]) == c["cap"] + 37
    c = pc.case("regions_damaged")
    capr = c["cap"] >> 2
    assert c["region_log2"] == 2 and c["cap"] == 4 * 4096
    assert c["counts"][1] == 0 and c["counts"][2] > capr and 0 < c["counts"][0] < capr and 0 < c["counts"][3] < capr
    # descriptors lie in the rows the count excludes (regions 0 and 1) and one is cut at region 2's end
    rec = c["records"]
    for lo, hi in ((int(c["counts"][0]), capr), (capr, 2 * capr)):
        d = rec[lo:hi]
        assert np.count_nonzero((d[:, 0] & pc.CHUNK != 0) & ((d[:, 0] & 0xFFFF) < 8)) > 10
    d = rec[2 * capr:3 * capr]
    cut = (d[:, 0] & pc.CHUNK != 0) & (d[:, 2].astype(np.int64) + ((d[:, 0] >> 16) & 0x7F) > 3 * capr)
    assert np.count_nonzero(cut) == 1
    c = pc.case("bad_desc")
    d = c["records"][:int(c["counts"][0])]
    assert np.count_nonzero((d[:, 0] & pc.CHUNK != 0) & ((d[:, 0] & 0xFFFF) >= c["nseg"])) == 8
    assert np.count_nonzero((d[:, 0] & pc.CHUNK == 0) & (d[:, 2] < len(d)) & (d[:, 1] < len(d))) >= 10
    c = pc.case("stale")
    d = c["records"][int(c["counts"][0]):c["cap"]]
    assert np.count_nonzero((d[:, 0] & pc.CHUNK != 0) & ((d[:, 0] & 0xFFFF) < c["nseg"])) > 100


def _arrival(c, s):
    """First idx of segment s's descriptors in buffer order."""
    return [d[1] for d in sorted(pc.held_chunks(c)[s])]


def test_sweep_covers_what_it_must():
    """Each item of the coverage list, from the case data alone."""
    seen = set()
    sizes = {"small": set(), "large": set(), "raw": set(), "empty": set()}
    lens = set()
    for name in pc.NAMES:
        c = pc.case(name)
        seen.add(("gap", c["gap"]))
        seen.add(("nseg", c["nseg"]))
        if c["region_log2"]:
            seen.add("regions")
        if c["nseg"] > pc.SEG_LDS:
            seen.add("global-hist")
            assert {0, 8191, 8192, 8199} <= set(c["segs"]) and len(c["segs"]) < 12
        if c["nseg"] % 8 == 0:  # the remap: no two segments alike, so no wrong one passes for another
            keys = [idx.tobytes() + snr.tobytes() for idx, snr in c["segs"].values()]
            assert len(set(keys)) == len(keys)
            if c["nseg"] == 8:
                assert len(keys) >= 7
        if len(c["segs"]) < c["nseg"]:
            sizes["empty"].add(0)
        for s, (idx, snr) in c["segs"].items():
            p = pc.path(idx)
            k = p["kernel"]
            sizes[k].add(p["n"])
            lens.update(p["lens"].tolist())
            full = np.flatnonzero(p["lens"] == 64)
            if len(full):
                seen.add("full-chunk")  # 64 crossings: every bin of the group, consecutive
            if p["sort"] == "rank":
                seen.add((k, "rank", p["m"]))
            if p["sort"] == "radix":
                assert p["passes"] >= (4 if k == "small" else 5)  # m distinct 64-bin groups span >= 64 (m - 1)
                seen.add((k, "radix", p["m"]))
                seen.add((k, "passes", p["passes"]))
                seen.add((k, "span", p["span"]))
                arr = _arrival(c, s)
                if arr == sorted(arr):
                    seen.add((k, "ascending"))
                if arr == sorted(arr, reverse=True):
                    seen.add((k, "descending"))
                if k == "large" and p["m"] >= 0.99 * p["n"]:
                    seen.add("large-m-near-n")
                if k == "large" and p["n"] == pc.CAP_SEG and p["m"] > pc.TH_LARGE:
                    seen.add("large-radix-at-cap")
                assert int(idx[-1]) < 2 ** 31 - 64
    need = {("small", "rank", 512), ("small", "radix", 513), ("large", "rank", 1024), ("large", "radix", 1025),
            ("small", "ascending"), ("small", "descending"), "large-m-near-n", "large-radix-at-cap", "full-chunk",
            "regions", "global-hist"}
    need |= {("small", "passes", k) for k in (4, 5, 6, 7, 8)} | {("large", "passes", k) for k in (5, 6, 7, 8)}
    need |= {("small", "span", v) for e in (16, 20, 24, 28) for v in (2 ** e - 1, 2 ** e)} | {("small", "span", 2 ** 31 - 65)}
    need |= {("gap", g) for g in range(1, 31)} | {("nseg", v) for v in (1, 8, 18, 64, 8192, 8200)}
    assert need <= seen, need - seen
    # the pass count on both sides of every power of 16 the first-idx span can cross
    for e, k in ((16, 4), (20, 5), (24, 6), (28, 7)):
        assert ((2 ** e - 1).bit_length() + 3) // 4 == k and ((2 ** e).bit_length() + 3) // 4 == k + 1
    assert lens == set(range(1, 65))
    cap = pc.CAP_SEG
    assert {63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096} <= sizes["small"]
    assert {4097, cap - 1, cap} <= sizes["large"] and cap + 1 in sizes["raw"] and sizes["empty"]


def test_shapes_are_what_they_claim():
    """The structured shapes: present at gaps 1, 2, 29 and 30 in both kernels with at least two
    rows, and the oracle gives the result the shape was built for."""
    for gap in pc.SHAPE_GAPS:
        c = pc.case(f"shapes_g{gap}")
        exp = pc.expected(c["name"])
        assert c["gap"] == gap and c["nseg"] == 64
        have = set()
        for s, (name, idx, snr) in pc.shape_segments(gap, 200 + gap).items():
            assert np.array_equal(c["segs"][s][0], idx) and np.array_equal(c["segs"][s][1], snr)
            p = pc.path(idx)
            assert p["n"] > 2 * (pc.TH_SMALL if p["kernel"] == "small" else pc.TH_LARGE)
            have.add((name, p["kernel"]))
            pi, ps = exp[s]
            n, d = len(idx), np.diff(idx)
            if name in ("falling", "rising", "equal") or name.startswith("saw"):
                assert np.all(d == 1)
            if name == "falling":
                assert np.all(np.diff(snr) < 0) and np.array_equal(pi, idx[::gap])  # one run, n / gap chain steps
            if name == "rising":
                assert np.all(np.diff(snr) > 0)
                if gap > 1:  # one peak, the last crossing (gap 1 joins no two distinct bins)
                    assert pi.tolist() == [idx[-1]] and ps[0] == snr[-1]
                else:
                    assert np.array_equal(pi, idx)
            if name == "equal":
                assert len(set(snr.tolist())) == 1 and np.array_equal(pi, idx[::gap])
            if name.startswith("saw"):
                per = gap + int(name[3:])
                assert per >= 1 and np.array_equal(snr, (10.0 + np.arange(n) % per).astype(np.float32))
            if name == "spaced_gap":
                assert np.all(d == gap) and np.array_equal(pi, idx)  # every crossing its own cluster
            if name == "spaced_gap-1":
                assert np.all(d == gap - 1) and len(pi) < n
            if name == "alternating":
                row = pc.TH_SMALL if p["kernel"] == "small" else pc.TH_LARGE
                turns = set((np.flatnonzero((d[1:] == 1) != (d[:-1] == 1)) + 2).tolist())  # first position of a stretch
                assert {64, 128, 192, row - 1, row + 1, 2 * row - 1, 2 * row + 1} <= turns, (gap, sorted(turns))
                assert {max(2, gap - 1), max(2, gap), gap + 5} <= set(d.tolist())
            if name == "pairs":
                assert np.array_equal(snr[0::2], snr[1::2])
                assert set(d[0::2].tolist()) == ({gap - 1, gap} if gap > 1 else {gap})
        names = {"falling", "rising", "equal", "saw+0", "saw+1", "spaced_gap", "alternating", "pairs"}
        names |= {"saw-1", "spaced_gap-1"} if gap > 1 else set()
        assert {(nm, k) for nm in names for k in ("small", "large")} <= have, gap
