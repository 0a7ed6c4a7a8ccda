"""kern::peak_cluster_batch (csrc/kernels/peakcluster.hip) on every code path, against the plain
Python scan reference.unique_peaks: segtab, the peaks (idx and S/N bit patterns) and *d_total are
equal, raw segments hold exactly their crossings.  The cases come from peakcluster_cases.py;
test_peakcluster_cases.py proves on the CPU which branch each reaches and that the second host
implementation agrees with the oracle.  Per family, the branch it was built for:

  sizes            rows / waves of peak_cluster_kernel<4096, 512> and <14000, 1024> at n = 63 .. 14000,
                   the raw hand-off at 14001, the empty entry; blockIdx = segment (nseg = 18)
  radix_small/large, one   step 1's radix sort: m on both sides of the thread count, 4..8 passes,
                   counts aliasing jmp, keys aliasing kmem; step 2's gather of chunks of 1..64
  shapes_g1/2/29/30        step 3a's consecutive-bin fast path next to its binary search, 3b / 3c
                   across 64-position blocks and rows, step 4's long chain, ties and the `< gap` edge
  gap_1 .. gap_30  every gap the host accepts, nseg = 8: the XCD remap
                   seg = (blockIdx & 7) * (nseg >> 3) + (blockIdx >> 3)
  lds_limit        seg_hist_kernel / seg_scatter_kernel with nseg = kSegLds = 8192
  global, global_regions   seg_hist_global_kernel / seg_scatter_global_kernel (nseg = 8200)
  regions3, regions_damaged, global_regions   RecRegions / region_end with region_log2 > 0
  over_cap, stale, bad_desc, regions_damaged   chunk_ok: a chunk cut at the capacity (or at its
                   region's end), descriptors after the count, segments >= nseg.  The buffers are
                   allocated and defined past the capacity, so a kernel without the check reads
                   stale chunks and gives another answer; nothing reads outside an allocation."""
import numpy as np
import pytest
import torch

import peakcluster_cases as pc

pytestmark = pytest.mark.gpu
dev = "cuda"


def _run(K, c):
    cap, nseg, stride = c["cap"], c["nseg"], int(K.peak_region_stride)
    peaks = torch.from_numpy(c["records"].reshape(-1).view(np.int32).copy()).to(dev)
    cnt = np.zeros(stride * len(c["counts"]), np.uint32)
    cnt[::stride] = c["counts"]
    count = torch.from_numpy(cnt.view(np.int32)).to(dev)
    work = torch.empty(5 * nseg, dtype=torch.int32, device=dev)
    srt = torch.zeros(4 * cap, dtype=torch.int32, device=dev)
    out = torch.zeros(2 * cap, dtype=torch.int32, device=dev)
    tab = torch.full((2 * nseg,), -1, dtype=torch.int32, device=dev)
    tot = torch.full((1,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    K.peak_cluster_batch(peaks.data_ptr(), count.data_ptr(), cap, nseg, c["gap"], work.data_ptr(), srt.data_ptr(),
                         out.data_ptr(), tab.data_ptr(), tot.data_ptr(), s, region_log2=c["region_log2"])
    torch.cuda.synchronize()
    return (tab.cpu().numpy().view(np.uint32).reshape(nseg, 2), out.cpu().numpy().view(np.uint32).reshape(cap, 2),
            srt.cpu().numpy().view(np.uint32).reshape(2 * cap, 2)[cap:], int(tot.item()), count)


def _check(K, c, exp, tab, out, raw, tot):
    name, cap_seg = c["name"], int(K.cluster_cap)
    live = np.zeros(c["nseg"], bool)
    live[list(c["segs"])] = True
    assert not tab[~live].any(), (name, np.flatnonzero(tab[~live].any(axis=1))[:8])  # empty segments: {0, 0}
    total, spans = 0, []
    for s, (idx, snr) in c["segs"].items():
        first, cnt = int(tab[s, 0]), int(tab[s, 1])
        if len(idx) > cap_seg:  # left to the host: the raw crossings of exactly this segment, any order
            assert cnt == (len(idx) | pc.RAW), (name, s, hex(cnt))
            got = raw[first:first + len(idx)]
            o = np.argsort(got[:, 0].view(np.int32), kind="stable")
            assert np.array_equal(got[o, 0].view(np.int32), idx), (name, s)
            assert np.array_equal(got[o, 1], snr.view(np.uint32)), (name, s)
            continue
        ei, es = exp[s]
        assert cnt == len(ei), (name, s, len(idx), cnt, len(ei))
        got = out[first:first + cnt]
        assert np.array_equal(got[:, 0].view(np.int32), ei), (name, s)
        assert np.array_equal(got[:, 1], es.view(np.uint32)), (name, s)
        total += cnt
        spans.append((first, cnt))
    assert tot == total, name
    spans.sort()  # the segments' peaks are packed: disjoint ranges filling [0, total)
    assert [a for a, _ in spans] == np.r_[0, np.cumsum([n for _, n in spans])][:-1].tolist(), name


@pytest.mark.parametrize("name", pc.NAMES)
def test_peak_cluster_paths(C, name):
    K = C.kernels
    assert int(K.cluster_cap) == pc.CAP_SEG
    c = pc.case(name)
    tab, out, raw, tot, _ = _run(K, c)
    _check(K, c, pc.expected(name), tab, out, raw, tot)


@pytest.mark.parametrize("name", pc.DAMAGED_NAMES)
def test_peak_cluster_uses_whole_valid_chunks_only(C, name):
    """One kind of damage per case (peakcluster_cases.py): the result is the clustering of the
    chunks wholly held, whatever lies behind the counts."""
    K = C.kernels
    c = pc.case(name)
    tab, out, raw, tot, count = _run(K, c)
    _check(K, c, pc.expected(name), tab, out, raw, tot)
    if c["region_log2"]:
        # peak_regions_total (kernels.hpp): the records held in the regions, or, when one
        # overflowed, 2^region_log2 x the fullest region's count
        stride, R = int(K.peak_region_stride), 1 << c["region_log2"]
        capr = c["cap"] >> c["region_log2"]
        held = np.minimum(c["counts"], capr)
        fits = np.zeros(stride * R, np.uint32)
        fits[::stride] = held
        t = torch.full((2,), -1, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        K.peak_regions_total(count.data_ptr(), c["region_log2"], c["cap"], t.data_ptr(), s)
        d_fits = torch.from_numpy(fits.view(np.int32)).to(dev)
        K.peak_regions_total(d_fits.data_ptr(), c["region_log2"], c["cap"], t.data_ptr() + 4, s)
        torch.cuda.synchronize()
        got = t.cpu().numpy().view(np.uint32)
        assert int(c["counts"].max()) > capr
        assert int(got[0]) == R * int(c["counts"].max()) > c["cap"]
        assert int(got[1]) == int(held.sum())
