#!/usr/bin/env python3
"""Filterbank fold-cube throughput on one GPU: CubeFolder.fold on a synthetic
noise filterbank (1024 channels by default), candidates spread over DM, period
and acceleration.

    python tools/cube_bench.py [--log2n 23] [--nchans 1024] [--nbits 2|8] [--cands 16] [--reps 3]
                               [--nints 16] [--nsub 32] [--nbins 64] [--period 0.0123] [--once]

One JSON line: candidates/s, ms per candidate and the effective rate of the
int8 rows read (nchans x fold_nsamps bytes per candidate) over --reps calls
after a warm-up (device-synchronised host clock; fold() ends with its results
on the host).  It also times one Dedisperser.run_list of a single DM on the
same filterbank: that launch reads the same rows once and is the natural
yardstick.  --period fixes every candidate's period (s) instead of the spread
(1 ms .. 1 s): long periods put a whole wave into one phase bin.  --once runs
one fold and one run_list and nothing else (the shape of a kernel-trace run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from peasoup_amd import _C  # noqa: E402
from peasoup_amd.utils import reference as ref  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=23, help="fold length 2^log2n samples")
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--nbits", type=int, default=2, choices=[2, 8])
    ap.add_argument("--tsamp", type=float, default=64e-6)
    ap.add_argument("--cands", type=int, default=16)
    ap.add_argument("--dm_max", type=float, default=100.0)
    ap.add_argument("--period", type=float, default=0.0, help="every candidate's period (s); 0 = 1 ms .. 1 s")
    ap.add_argument("--nints", type=int, default=16)
    ap.add_argument("--nsub", type=int, default=32)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cube_bench needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    n = 1 << a.log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=a.nbits, tsamp=a.tsamp, foff=-0.25)
    delays = ref.delay_table(a.nchans, a.tsamp, hdr["fch1"], hdr["foff"])
    dms = [float(x) for x in np.linspace(0.0, a.dm_max, max(2, a.cands)).astype(np.float32)][: a.cands]
    nsamps = n + int(ref.dm_offsets([a.dm_max], delays).max()) + 1
    packed = synthetic.generate_packed_torch(nsamps, hdr, [], seed=1)  # noise only, as bench.py's default
    geom = _C.DedispGeometry.make(hdr, nsamps, dms if len(dms) > 1 else dms + [a.dm_max], [1] * a.nchans)
    dfb = _C.DeviceFilterbank(geom, stream)
    dfb.load_packed_device(packed.data_ptr())
    torch.cuda.synchronize()
    del packed
    periods = [a.period] * a.cands if a.period > 0 else [float(p) for p in np.geomspace(1e-3, 1.0, a.cands)]
    accs = [float(x) for x in np.linspace(-50.0, 50.0, a.cands)] if a.cands > 1 else [0.0]
    cands = [_C.CubeCandidate(p, d, x) for p, d, x in zip(periods, dms, accs)]
    folder = _C.CubeFolder(dfb, _C.CubeParams(a.nints, min(a.nsub, a.nchans), a.nbins, n), stream)
    dd = _C.Dedisperser(dfb, stream)
    rs = _C.Dedisperser.row_stride(int(geom.out_nsamps))
    trial = torch.empty(rs, dtype=torch.uint8, device="cuda")

    def run_list():
        dd.run_list([len(dms) // 2], trial.data_ptr(), rs)
        torch.cuda.synchronize()

    folder.fold(cands)  # warm-up (and the --once run)
    run_list()
    if a.once:
        print(json.dumps({"cands": a.cands, "log2n": a.log2n, "nchans": a.nchans, "nbits": a.nbits}))
        return
    t0 = time.perf_counter()
    for _ in range(a.reps):
        folder.fold(cands)  # ends in a stream synchronise
    dt = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        run_list()
    dt_list = (time.perf_counter() - t0) / a.reps
    row_bytes = float(a.nchans) * n
    print(json.dumps({"metric": "fold cubes: candidates / s", "value": round(a.cands / dt, 3),
                      "ms_per_candidate": round(1e3 * dt / a.cands, 4),
                      "row_GB_per_s": round(a.cands * row_bytes / dt / 1e9, 1),
                      "run_list_one_dm_ms": round(1e3 * dt_list, 4),
                      "run_list_row_GB_per_s": round(row_bytes / dt_list / 1e9, 1),
                      "cands": a.cands, "log2n": a.log2n, "nchans": a.nchans, "nbits": a.nbits, "nints": a.nints,
                      "nsub": min(a.nsub, a.nchans), "nbins": a.nbins, "period": a.period,
                      "batches_per_fold": folder.batches // (a.reps + 1)}))


if __name__ == "__main__":
    main()
