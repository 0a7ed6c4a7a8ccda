#!/usr/bin/env python3
"""fildigi passes on one GPU, on a synthetic float32 filterbank (1024 channels
x 2^20 samples by default) that is resident on the device:

    python tools/digi_bench.py [--log2n 20] [--nchans 1024] [--reps 7]

One JSON line with the median time (device events, after a warm-up) of
digi_block_sums and digi_quant, the GB/s of input bytes (4 nchans nsamps) and
the ratio to the yardstick, a plain device-to-device copy of the same input
bytes timed in the same session.  The stats pass reads the float input twice
and the quant pass once, so they are reported against 2x and 1x the copy's
time.  The timed calls are the torch ops: digi_block_sums includes the
allocation of its four small tables and a stream synchronisation, digi_quant
the upload of its table, the allocation of y and the read-back of nclip.
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
    assert torch.cuda.is_available(), "digi_bench needs a GPU"
    n, nchans = 1 << a.log2n, a.nchans
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    gains = 10.0 ** torch.linspace(-2.0, 2.0, nchans, device="cuda")
    x = torch.randn((n, nchans), device="cuda", generator=g) * gains + 3.0 * gains
    in_bytes = 4.0 * n * nchans
    out = {"metric": "fildigi passes", "log2n": a.log2n, "nchans": nchans, "input_GB": round(in_bytes / 1e9, 3),
           "stat_block": int(_C.digi_stat_block())}
    dst = torch.empty_like(x)
    copy_ms = timed(lambda: dst.copy_(x), a.reps)
    del dst
    out["copy_ms"] = round(copy_ms, 3)
    out["copy_input_GB_per_s"] = round(in_bytes / copy_ms / 1e6, 1)
    res = {}

    def sums():
        res["s"] = ops.digi_block_sums(x)

    ms = timed(sums, a.reps)
    out["sums_ms"] = round(ms, 3)
    out["sums_input_GB_per_s"] = round(in_bytes / ms / 1e6, 1)
    out["sums_over_2x_copy"] = round(ms / (2 * copy_ms), 3)
    s = res["s"]
    sc = _C.digi_scale(s["N"].cpu().numpy().astype(np.uint32), s["S1"].cpu().numpy(),
                       s["S2"].cpu().numpy().view(np.uint64), s["E"].cpu().numpy(), [], _C.DigiParams())
    for flip in (False, True):
        ms = timed(lambda: ops.digi_quant(x, sc["mean"], sc["gain"], 0, flip), a.reps)
        key = "quant_flip" if flip else "quant"
        out[key + "_ms"] = round(ms, 3)
        out[key + "_input_GB_per_s"] = round(in_bytes / ms / 1e6, 1)
        out[key + "_over_1x_copy"] = round(ms / copy_ms, 3)
    y, nclip = ops.digi_quant(x, sc["mean"], sc["gain"], 0, False)
    out["nclip"] = nclip
    out["y_sigma_ch0"] = round(float(y[:, 0].float().std()), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
