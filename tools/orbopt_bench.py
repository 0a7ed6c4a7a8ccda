#!/usr/bin/env python3
"""orbopt's three costs on one GPU:

    python tools/orbopt_bench.py [--log2n 23] [--count 9] [--nints 16] [--nbins 64] [--np 33] [--reps 5]
                                 [--cands 16] [--nchans 64]

One JSON line.  (1) The median time (device events, after a warm-up) of
``orbopt_fold`` of one row of 2^log2n samples at count^3 templates (729 at the
default) into nints x nbins planes, against ``orbit_resample`` writing the same
count^3 resampled rows, and against the floor of that, a device-to-device copy
of those bytes, all timed in the same session.  The fold reads the row count^3
times (through L2) and writes count^3 small planes; the resample writes count^3
rows.  The timed calls are the torch ops: they include the upload of the
quantised templates.  (2) ``orbopt_search`` of those planes, per candidate.
(3) The host wall time of ``OrbitOptimiser.optimise`` of ``cands`` candidates at
two DMs on a synthetic filterbank of 2^log2n samples, end to end (dedispersion,
row moments and hits on the host, fold, search, finish).
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
from peasoup_amd import _C, ops  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402

TSAMP = 64e-6


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def candidate(n, dm=5.0):
    T = n * float(np.float32(TSAMP))
    return (0.0123, dm, 0.0, 0.8 * T, 200.0 * TSAMP, 0.37)


def kernel_part(a, out):
    n, K = 1 << a.log2n, a.count ** 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(64, 192, (1, n), dtype=torch.uint8, device="cuda", generator=g)
    p = _C.OrbOptParams(nbins=a.nbins, nints=a.nints, npb=a.count, na1=a.count, nphase=a.count, np=a.np)
    grid = _C.oopt_grid(0, p, candidate(n), n, TSAMP)
    q = [tuple(int(v) for v in t) for t in grid["quant"]]
    fold = torch.empty((1, K, a.nints, a.nbins), dtype=torch.int32, device="cuda")
    fold_ms = timed(lambda: ops.orbopt_fold(x, n, [grid["G"]], [q], a.nints, a.nbins, out=fold), a.reps)
    y = torch.empty((1, K, n), dtype=torch.uint8, device="cuda")
    resample_ms = timed(lambda: ops.orbit_resample(x, n, (), 0.0, out=y, quant=q), a.reps)
    src = torch.empty_like(y)
    copy_ms = timed(lambda: y.copy_(src), a.reps)
    del src, y
    hits = torch.from_numpy(_C.oopt_hits(grid["G"], n, a.nints, a.nbins)).cuda().view(1, a.nints, a.nbins)
    m = torch.tensor([128], dtype=torch.int32, device="cuda")
    st = _C.oopt_drift_table(p)
    search_ms = timed(lambda: ops.orbopt_search(fold, hits, m, st), a.reps)
    out.update(templates=K, fold_ms=round(fold_ms, 3), resample_ms=round(resample_ms, 3), copy_ms=round(copy_ms, 3),
               fold_over_resample=round(fold_ms / resample_ms, 3), fold_over_copy=round(fold_ms / copy_ms, 3),
               fold_source_GB_per_s=round(K * n / fold_ms / 1e6, 1), search_ms_per_candidate=round(search_ms, 3))


def optimise_part(a, out):
    ns = 1 << a.log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=8, tsamp=TSAMP)
    hdr["nsamples"] = ns
    packed = synthetic.generate_packed_torch(ns, hdr, [synthetic.PulsarSpec(period=0.0123, dm=5.0, amplitude=0.05)],
                                             seed=1)
    torch.cuda.synchronize()
    dms = [5.0, 7.5]
    stream = _C.GpuStream()
    geom = _C.DedispGeometry.make(hdr, ns, dms, [1] * a.nchans)
    dfb = _C.DeviceFilterbank(geom, stream.handle)
    dfb.load_packed_device(packed.data_ptr())
    stream.synchronize()
    p = _C.OrbOptParams(nbins=a.nbins, nints=a.nints, npb=a.count, na1=a.count, nphase=a.count, np=a.np)
    opt = _C.OrbitOptimiser(p, dfb, ns, stream.handle)
    n = int(opt.span)
    cands = [candidate(n, dms[i % 2]) for i in range(a.cands)]
    opt.optimise(cands[:2])  # warm-up: buffers, code objects, the dedispersion tables
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        opt.optimise(cands)
        ts.append(time.perf_counter() - t0)
    out.update(optimise_cands=a.cands, optimise_s=round(statistics.median(ts), 4), span=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=23)
    ap.add_argument("--count", type=int, default=9, help="npb = na1 = nphase")
    ap.add_argument("--nints", type=int, default=16)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--np", type=int, default=33)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cands", type=int, default=16)
    ap.add_argument("--nchans", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "orbopt_bench needs a GPU"
    out = {"metric": "orbopt", "log2n": a.log2n, "nints": a.nints, "nbins": a.nbins, "np": a.np}
    kernel_part(a, out)
    if a.cands > 0:
        optimise_part(a, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
