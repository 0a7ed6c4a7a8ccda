#!/usr/bin/env python3
"""Burst-cutout throughput on one GPU: BurstCutter.cut on a synthetic noise
filterbank (1024 channels by default) at the default cutout (256 time bins, 256
subbands, 256 DM rows), for candidates of several widths spread over DM.

    python tools/burst_bench.py [--log2n 21] [--nchans 1024] [--nbits 2|8] [--cands 16] [--reps 7]
                                [--widths 1,32,4096] [--dm_max 100] [--ntime 256] [--nsub 256] [--ndm 256]

One JSON line per width: the median over --reps timed calls after a warm-up
(device-synchronised host clock; cut() ends with its results on the host) as
candidates/s and ms per candidate, and the rate of the row bytes the outputs
sum ((ndm + 1) x ntime x f x nchans per candidate).  For scale it also times
one Dedisperser.run_list of the --ndm DM rows of the middle candidate over a
filterbank of the cutout's length (ntime x f samples plus the largest delay):
what a user would otherwise run per candidate.  Nothing else uses the GPU
while a call is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from peasoup_amd import _C  # noqa: E402
from peasoup_amd.utils import reference as ref  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402


def _median_time(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=21, help="filterbank length 2^log2n samples")
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--nbits", type=int, default=2, choices=[2, 8])
    ap.add_argument("--tsamp", type=float, default=64e-6)
    ap.add_argument("--cands", type=int, default=16)
    ap.add_argument("--dm_max", type=float, default=100.0)
    ap.add_argument("--widths", default="1,32,4096")
    ap.add_argument("--ntime", type=int, default=256)
    ap.add_argument("--nsub", type=int, default=256)
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "burst_bench needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    nsamps = 1 << a.log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=a.nbits, tsamp=a.tsamp, foff=-0.25)
    delays = ref.delay_table(a.nchans, a.tsamp, hdr["fch1"], hdr["foff"])
    packed = synthetic.generate_packed_torch(nsamps, hdr, [], seed=1)  # noise only, as bench.py's default
    ones = [1] * a.nchans
    dfb = _C.DeviceFilterbank(_C.DedispGeometry.make(hdr, nsamps, [0.0], ones), stream)
    dfb.load_packed_device(packed.data_ptr())
    torch.cuda.synchronize()
    nsub = min(a.nsub, a.nchans)
    dms = [float(x) for x in np.linspace(a.dm_max / a.cands, a.dm_max, a.cands).astype(np.float32)]
    for width in [int(w) for w in a.widths.split(",")]:
        f = ref.burst_tscrunch(width)
        samples = [int(x) for x in np.linspace(nsamps // 2, 3 * (nsamps // 4), a.cands)]
        cands = [_C.BurstCandidate(s, width, d) for s, d in zip(samples, dms)]
        cutter = _C.BurstCutter(dfb, _C.BurstParams(a.ntime, nsub, a.ndm), stream)
        cutter.cut(cands)  # warm-up
        tiles, single = cutter.tiles, cutter.single_row_tiles
        dt = _median_time(lambda: cutter.cut(cands), a.reps)  # ends in a stream synchronise
        # the yardstick: the ndm DM rows of the middle candidate, dedispersed over the cutout's length
        mid = dms[len(dms) // 2]
        rows = [float(x) for x in ref.burst_dms(mid, a.ndm)]
        need = a.ntime * f + int(ref.dm_offsets([rows[-1]], delays).max()) + 1
        n2 = min(nsamps, max(need, 4096))
        g2 = _C.DedispGeometry.make(hdr, n2, rows, ones)
        fb2 = _C.DeviceFilterbank(g2, stream)
        fb2.load_packed_device(packed.data_ptr())  # time-major bytes: the first n2 samples
        dd = _C.Dedisperser(fb2, stream)
        rs = _C.Dedisperser.row_stride(int(g2.out_nsamps))
        trials = torch.empty(a.ndm * rs, dtype=torch.uint8, device="cuda")

        def run_list():
            dd.run_list(list(range(a.ndm)), trials.data_ptr(), rs)
            torch.cuda.synchronize()

        run_list()  # warm-up
        dt_list = _median_time(run_list, a.reps)
        summed = float(a.ndm + 1) * a.ntime * f * a.nchans
        print(json.dumps({"metric": "burst cutouts: candidates / s", "value": round(a.cands / dt, 3),
                          "ms_per_candidate": round(1e3 * dt / a.cands, 4),
                          "summed_row_GB_per_s": round(a.cands * summed / dt / 1e9, 1),
                          "run_list_ndm_trials_ms": round(1e3 * dt_list, 4), "run_list_out_nsamps": int(g2.out_nsamps),
                          "width": width, "tscrunch": f, "cands": a.cands, "log2n": a.log2n, "nchans": a.nchans,
                          "nbits": a.nbits, "ntime": a.ntime, "nsub": nsub, "ndm": a.ndm, "dm_max": a.dm_max,
                          "row_tiles_per_candidate": tiles // a.cands, "one_row_dm_tiles": single, "reps": a.reps}),
              flush=True)
        del dd, fb2, trials


if __name__ == "__main__":
    main()
