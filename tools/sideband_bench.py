#!/usr/bin/env python3
"""The sideband search's cost per DM on one GPU:

    python tools/sideband_bench.py [--log2n 23] [--rows 8] [--reps 7] [--tsamp 64e-6]

One JSON line.  ``rows`` spectra of 2^log2n / 2 + 1 bins of complex noise
(unit power, so P is exponential noise as after whitening) go through
``sb_power`` and ``sb_search`` over the default band and sizes; the times are
medians of device-event timings after a warm-up, divided by ``rows``.  Beside
them: a device-to-device copy of the P rows (the floor of anything that reads
P once and writes as much), and the host wall time of one zero-acceleration
``SearchEngine.search_trial`` of one 8-bit noise row of the same length, which
includes that trial's whitening.  The timed sb_search includes its dense test
outputs being off and an event buffer that nothing reaches at min_power 30.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=23)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tsamp", type=float, default=64e-6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sideband_bench needs a GPU"
    n, rows = 1 << a.log2n, a.rows
    nb = n // 2 + 1
    g = _C.sb_geometry(0.1, 1100.0, n, a.tsamp)
    k_lo, k_hi = int(g.k_lo), int(g.k_hi)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    spec = torch.view_as_complex(torch.randn((rows, nb, 2), dtype=torch.float32, device="cuda", generator=gen) *
                                 (0.5 ** 0.5))
    P = torch.zeros((rows, (nb + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    power_ms = timed(lambda: ops.sideband_power(spec, k_lo, k_hi, out=P), a.reps)
    res = {}

    def search():
        res["r"] = ops.sideband_search(P, k_lo, k_hi, dense=False, capacity=1 << 16)

    search_ms = timed(search, a.reps)
    src = torch.empty_like(P)
    copy_ms = timed(lambda: src.copy_(P), a.reps)
    del src

    # one zero-acceleration trial of the plain search on an 8-bit noise row of the same length
    sp = _C.SearchParams()
    sp.fft_size = n
    sp.tsamp = a.tsamp
    stream = _C.GpuStream()
    eng = _C.SearchEngine(sp, stream.handle)
    row = torch.randint(96, 160, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    eng.search_trial(row.data_ptr(), n, 0.0, 0, [0.0])
    ts = []
    for _ in range(max(3, a.reps)):
        t0 = time.perf_counter()
        eng.search_trial(row.data_ptr(), n, 0.0, 0, [0.0])
        ts.append(time.perf_counter() - t0)
    trial_ms = statistics.median(ts) * 1e3

    band = k_hi - k_lo
    out = {"metric": "sbsearch", "log2n": a.log2n, "rows": rows, "band_bins": band, "windows_per_row": int(g.nwin),
           "segments_per_row": int(sum(g.nseg)), "events": int(res["r"]["count"]),
           "sb_power_ms_per_dm": round(power_ms / rows, 4), "sb_search_ms_per_dm": round(search_ms / rows, 4),
           "sideband_ms_per_dm": round((power_ms + search_ms) / rows, 4),
           "copy_P_ms_per_dm": round(copy_ms / rows, 4),
           "zero_acc_search_trial_ms": round(trial_ms, 4),
           "sideband_over_trial": round((power_ms + search_ms) / rows / trial_ms, 3),
           "sb_search_over_copy": round(search_ms / copy_ms, 2),
           "P_read_GB_per_s": round(2.0 * 4.0 * band * rows / search_ms / 1e6, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
