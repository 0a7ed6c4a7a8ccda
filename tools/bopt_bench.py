#!/usr/bin/env python3
"""Throughput of burstopt (csrc/kernels/burstopt.hip) at burstcube's default
shape (ntime = nsub = ndm = 256, nfine = 65) and at the largest (1024 / 256 /
1024 / 257), against ``BurstCutter.cut`` of the same candidates, the stage it
follows.

    python tools/bopt_bench.py [--cands 32] [--log2n 20] [--nchans 256]

Cuts noise at ``--cands`` candidates, then times ``BurstOptimiser.optimise``
(prepare and shifts on the host, upload, search, download, finish), the search
with its transfers (``BurstOptimiser.search``) and the kernels alone on tables
that are already on the device (``search_device``, timed with events).  Prints
one JSON line per shape.
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


def bench_shape(a, dfb, hdr, delays, n, ntime, nsub, ndm, nfine, stream):
    rng = np.random.default_rng(1)
    nsub = min(nsub, a.nchans)
    samples = [int(s) for s in rng.integers(n // 4, 3 * n // 4, a.cands)]
    dms = [float(x) for x in np.linspace(20.0, 200.0, a.cands).astype(np.float32)]
    cands = [_C.BurstCandidate(s, 16, d, 10.0) for s, d in zip(samples, dms)]
    cutter = _C.BurstCutter(dfb, _C.BurstParams(ntime, nsub, ndm, 0, 0.0), stream)
    cuts = cutter.cut(cands)  # warm-up
    t0 = time.perf_counter()
    for _ in range(a.reps):
        cutter.cut(cands)
    dt_cut = (time.perf_counter() - t0) / a.reps

    geom = _C.BurstOptGeom(ntime, nsub, ndm, a.nchans, a.tsamp, hdr["fch1"], hdr["foff"])
    opt = _C.BurstOptimiser(geom, _C.BurstOptGrid(nfine, 0.0), stream)
    inputs = [dict(c, sample=s, width=16, dm=d, snr=10.0) for c, s, d in zip(cuts, samples, dms)]
    dl = [float(x) for x in delays]
    opt.optimise(inputs, dl)  # warm-up
    t0 = time.perf_counter()
    for _ in range(a.reps):
        opt.optimise(inputs, dl)
    dt_opt = (time.perf_counter() - t0) / a.reps
    # the search with its transfers, the host steps left out
    d_ds = rng.integers(-2000, 2000, (a.cands, nsub, ntime)).astype(np.int32)
    d_dmt = rng.integers(-2000, 2000, (a.cands, ndm, ntime)).astype(np.int32)
    sf = rng.integers(-ntime // 8, ntime // 8 + 1, (a.cands, nfine, nsub)).astype(np.int32)
    opt.search(d_ds, d_dmt, sf)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        opt.search(d_ds, d_dmt, sf)
    dt_search = (time.perf_counter() - t0) / a.reps
    # the kernels alone
    dev = [torch.from_numpy(x).cuda() for x in (d_ds, d_dmt, sf)]
    nw = opt.nwidths
    outs = [torch.empty((a.cands,) + s, dtype=torch.int32, device="cuda")
            for s in ((2, nw), (2, nw), (nw, ndm + nfine), (nw, ndm + nfine))]
    args = [t.data_ptr() for t in dev] + [a.cands] + [t.data_ptr() for t in outs]
    opt.search_device(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        opt.search_device(*args)
    e1.record()
    torch.cuda.synchronize()
    dt_kernel = e0.elapsed_time(e1) / 1e3 / a.reps
    reads = float(nfine) * nsub * ntime * 4  # LDS bytes of the fine rows' gather, per candidate
    print(json.dumps({"metric": "burstopt: candidates / s", "value": round(a.cands / dt_opt, 2),
                      "ms_per_candidate": round(1e3 * dt_opt / a.cands, 3),
                      "search_only_candidates_per_s": round(a.cands / dt_search, 2),
                      "kernel_only_candidates_per_s": round(a.cands / dt_kernel, 2),
                      "kernel_only_us_per_candidate": round(1e6 * dt_kernel / a.cands, 2),
                      "kernel_only_lds_read_TB_per_s": round(a.cands * reads / dt_kernel / 1e12, 3),
                      "cut_candidates_per_s": round(a.cands / dt_cut, 2),
                      "cut_ms_per_candidate": round(1e3 * dt_cut / a.cands, 3),
                      "cands": a.cands, "ntime": ntime, "nsub": nsub, "ndm": ndm, "nfine": nfine,
                      "log2n": a.log2n, "nchans": a.nchans}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20, help="filterbank length 2^log2n samples")
    ap.add_argument("--nchans", type=int, default=256)
    ap.add_argument("--tsamp", type=float, default=64e-6)
    ap.add_argument("--cands", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="256,256,256,65;1024,256,1024,257", help="ntime,nsub,ndm,nfine;...")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bopt_bench needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    n = 1 << a.log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=8, tsamp=a.tsamp, foff=-0.25)
    delays = ref.delay_table(a.nchans, a.tsamp, hdr["fch1"], hdr["foff"])
    packed = synthetic.generate_packed_torch(n, hdr, [], seed=1)
    geom = _C.DedispGeometry.make(hdr, n, [0.0, 400.0], [1] * a.nchans)
    dfb = _C.DeviceFilterbank(geom, stream)
    dfb.load_packed_device(packed.data_ptr())
    torch.cuda.synchronize()
    del packed
    for shape in a.shapes.split(";"):
        ntime, nsub, ndm, nfine = (int(x) for x in shape.split(","))
        bench_shape(a, dfb, hdr, delays, n, ntime, nsub, ndm, nfine, stream)


if __name__ == "__main__":
    main()
