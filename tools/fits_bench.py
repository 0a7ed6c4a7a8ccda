"""Times fits2fil's decode kernel and its two whole passes (decode + block sums,
decode + requantise) on a 4096-channel, 2^20-sample, two-polarisation file at 2,
8 and 16 bits, each next to a device-to-device copy of the bytes the kernels
read plus write, in the same run.  Prints one JSON line per width.

    python tools/fits_bench.py [--nsamps N] [--nchan C] [--reps R]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peasoup_amd import ops  # noqa: E402


def timed(fn, reps, warmup=2):
    """Median and minimum over ``reps`` timed calls (ms), after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsamps", type=int, default=1 << 20)
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--nsblk", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nrows, npol, nchan = a.nsamps // a.nsblk, 2, a.nchan
    g = torch.Generator(device=dev).manual_seed(1)
    scl = (torch.rand((nrows, npol, nchan), device=dev, generator=g) + 0.5).contiguous()
    offs = torch.randn((nrows, npol, nchan), device=dev, generator=g).contiguous()
    wts = torch.ones((nrows, nchan), device=dev)
    slots = list(range(nrows))
    mean = np.zeros((1, nchan))
    gain = np.full((1, nchan), 0.25)
    for nbits in (2, 8, 16):
        row_bytes = a.nsblk * npol * nchan * nbits // 8
        data = torch.randint(0, 256, (nrows, row_bytes), dtype=torch.uint8, device=dev, generator=g)
        x = {}

        def decode():
            x["x"] = ops.fits_decode(data, scl, offs, wts, slots, a.nsblk, nbits, False, (0, 1), 0.0)

        def pass1():
            decode()
            ops.digi_block_sums(x["x"])

        def pass2():
            decode()
            ops.digi_quant(x["x"], mean, gain, 0, True)

        in_b, out_b = nrows * row_bytes, a.nsamps * nchan * 4
        moved = {"decode": in_b + out_b, "pass1": in_b + 2 * out_b, "pass2": in_b + 2 * out_b + a.nsamps * nchan}
        res = {"nbits": nbits, "nsamps": a.nsamps, "nchan": nchan, "npol": npol}
        for name, fn in (("decode", decode), ("pass1", pass1), ("pass2", pass2)):
            half = torch.empty(moved[name] // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(half)
            med, lo = timed(fn, a.reps)
            cmed, clo = timed(lambda: dst.copy_(half), a.reps)
            del half, dst
            res[name] = {"ms": round(med, 3), "ms_min": round(lo, 3), "GBps": round(moved[name] / med / 1e6, 1),
                         "copy_ms": round(cmed, 3), "copy_GBps": round(moved[name] / cmed / 1e6, 1),
                         "ratio_to_copy": round(med / cmed, 2)}
        print(json.dumps(res), flush=True)
        del data, x
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
