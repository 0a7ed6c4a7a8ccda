#!/usr/bin/env python3
"""filinject's kernel on one GPU, on 8-bit channel-major rows (1024 channels x
2^20 samples by default) that are resident on the device:

    python tools/inject_bench.py [--log2n 20] [--nchans 1024] [--reps 7]

One JSON line with the median time (device events, after a warm-up) of the
inject op for three cases -- one pulsar, eight pulsars, one burst (which shows
the tile skip) -- the GB/s of row bytes moved at one read and one write of the
rows (2 nchans nsamps), and the ratio to the yardstick, a plain
device-to-device copy of the same rows (which also reads and writes them once)
timed in the same session.  The timed call is the torch op: it includes the
upload of the tables, the zeroing and read-back of the counters and a stream
synchronisation.  The rows are injected into again and again; the samples
saturate slowly, which changes no work the kernel does.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from peasoup_amd import _C, ops  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402
from peasoup_amd.utils.synthetic import BurstSpec, PulsarSpec  # noqa: E402


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
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "inject_bench needs a GPU"
    n, nchans = 1 << a.log2n, a.nchans
    hdr = synthetic.make_header(nchans=nchans, nbits=8, tsamp=64e-6, fch1=1500.0, foff=-300.0 / nchans)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = (torch.randn((nchans, n), device="cuda", generator=g) * 16.0).round().clamp(-128, 127).to(torch.int8)
    moved = 2.0 * n * nchans
    out = {"metric": "filinject kernel", "log2n": a.log2n, "nchans": nchans, "rows_GB": round(n * nchans / 1e9, 3),
           "tile": int(_C.inject_tile())}
    dst = torch.empty_like(x)
    copy_ms = timed(lambda: dst.copy_(x), a.reps)
    del dst
    out["copy_ms"] = round(copy_ms, 3)
    out["copy_GB_per_s"] = round(moved / copy_ms / 1e6, 1)
    unit = np.full(nchans, 16.0)
    t_obs = n * float(hdr["tsamp"])
    cases = {
        "one_pulsar": [PulsarSpec(period=0.0123, dm=100.0, amplitude=0.05)],
        "eight_pulsars": [PulsarSpec(period=0.003 * (k + 1) + 0.0007, dm=20.0 * (k + 1), amplitude=0.05, phase=0.1 * k)
                          for k in range(8)],
        "one_burst": [BurstSpec(time=0.5 * t_obs, dm=300.0, width=2e-3, amplitude=3.0)],
    }
    for name, sig in cases.items():
        tab = ops.inject_tables(sig, hdr, n, unit)
        res = {}

        def run():
            res["r"] = ops.inject(x, n, 8, tab, seed=1, bias=128)

        ms = timed(run, a.reps)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_GB_per_s"] = round(moved / ms / 1e6, 1)
        out[name + "_over_copy"] = round(ms / copy_ms, 3)
        out[name + "_touched_fraction"] = round(float(np.sum(res["r"][2])) / (len(sig) * n * nchans), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
