#!/usr/bin/env python3
"""Throughput of cubeopt (csrc/kernels/cubeopt.hip) at the default grid (64 DM
x 65 period x 33 acceleration trials), against ``CubeFolder.fold`` of the same
candidates, the stage it follows.

    python tools/opt_bench.py [--cands 64] [--log2n 22] [--nchans 256]

Folds noise at ``--cands`` candidates, then times ``CubeOptimiser.optimise``
(prepare and shift tables on the host, upload, search, download, finish) and,
separately, the search with its transfers (``CubeOptimiser.search``).  Prints
one JSON line: candidates / s, trial profiles / s and the LDS read rate of the
trial loop (nints x nbins dword reads per trial profile, the box-sum ladder
not counted) next to the time of the fold.
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
    ap.add_argument("--log2n", type=int, default=22, help="fold length 2^log2n samples")
    ap.add_argument("--nchans", type=int, default=256)
    ap.add_argument("--tsamp", type=float, default=64e-6)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--nints", type=int, default=16)
    ap.add_argument("--nsub", type=int, default=32)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--ndm", type=int, default=64)
    ap.add_argument("--np", type=int, default=65)
    ap.add_argument("--npd", type=int, default=33)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "opt_bench needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    n = 1 << a.log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=2, tsamp=a.tsamp, foff=-0.25)
    delays = ref.delay_table(a.nchans, a.tsamp, hdr["fch1"], hdr["foff"])
    dms = [float(x) for x in np.linspace(10.0, 100.0, max(2, a.cands)).astype(np.float32)][: a.cands]
    nsamps = n + int(ref.dm_offsets([100.0], delays).max()) + 1
    packed = synthetic.generate_packed_torch(nsamps, hdr, [], seed=1)
    geom = _C.DedispGeometry.make(hdr, nsamps, dms if len(dms) > 1 else dms + [100.0], [1] * a.nchans)
    dfb = _C.DeviceFilterbank(geom, stream)
    dfb.load_packed_device(packed.data_ptr())
    torch.cuda.synchronize()
    del packed
    periods = [float(p) for p in np.geomspace(5e-3, 1.0, a.cands)]
    cands = [_C.CubeCandidate(p, d, 0.0) for p, d in zip(periods, dms)]
    nsub = min(a.nsub, a.nchans)
    folder = _C.CubeFolder(dfb, _C.CubeParams(a.nints, nsub, a.nbins, n), stream)
    cubes = folder.fold(cands)  # warm-up
    t0 = time.perf_counter()
    for _ in range(a.reps):
        folder.fold(cands)
    dt_fold = (time.perf_counter() - t0) / a.reps

    og = _C.CubeOptGeom(a.nints, nsub, a.nbins, a.nchans, n, a.tsamp, hdr["fch1"], hdr["foff"])
    grid = _C.CubeOptGrid(a.ndm, 0.0, a.np, 1.0, a.npd, 1.0)
    opt = _C.CubeOptimiser(og, grid, stream)
    inputs = [dict(c, period=p, dm=d, acc=0.0) for c, p, d in zip(cubes, periods, dms)]
    dl = [float(x) for x in delays]
    opt.optimise(inputs, dl)  # warm-up
    t0 = time.perf_counter()
    for _ in range(a.reps):
        opt.optimise(inputs, dl)
    dt_opt = (time.perf_counter() - t0) / a.reps
    # the search with its transfers, the host steps left out
    rng = np.random.default_rng(0)
    d = rng.integers(-2000, 2000, (a.cands, a.nints, nsub, a.nbins)).astype(np.int32)
    sdm = rng.integers(0, a.nbins, (a.cands, a.ndm, nsub)).astype(np.int32)
    st = rng.integers(0, a.nbins, (a.cands, a.np, a.npd, a.nints)).astype(np.int32)
    opt.search(d, sdm, st)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        opt.search(d, sdm, st)
    dt_search = (time.perf_counter() - t0) / a.reps
    trials = a.ndm * a.np * a.npd
    reads = float(trials) * a.nints * a.nbins * 4
    print(json.dumps({"metric": "cubeopt: candidates / s", "value": round(a.cands / dt_opt, 2),
                      "trial_profiles_per_s": round(a.cands * trials / dt_opt, 0),
                      "search_only_candidates_per_s": round(a.cands / dt_search, 2),
                      "search_only_trial_profiles_per_s": round(a.cands * trials / dt_search, 0),
                      "search_only_lds_read_TB_per_s": round(a.cands * reads / dt_search / 1e12, 3),
                      "fold_candidates_per_s": round(a.cands / dt_fold, 2),
                      "ms_per_candidate": round(1e3 * dt_opt / a.cands, 3),
                      "fold_ms_per_candidate": round(1e3 * dt_fold / a.cands, 3),
                      "cands": a.cands, "trials_per_candidate": trials, "nints": a.nints, "nsub": nsub,
                      "nbins": a.nbins, "log2n": a.log2n, "nchans": a.nchans}))


if __name__ == "__main__":
    main()
