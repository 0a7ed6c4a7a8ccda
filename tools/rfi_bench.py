#!/usr/bin/env python3
"""RFI excision passes on one GPU, on a synthetic noise filterbank (1024
channels x 2^23 samples by default):

    python tools/rfi_bench.py [--log2n 23] [--nchans 1024] [--nbits 2|8] [--block 4096] [--reps 7] [--once KERNEL]

One JSON line with the median time (device events, after a warm-up) and the
GB/s of int8 row bytes (nchans x nsamps) of rfi_block_sums, rfi_apply in place
without and with zero-DM (the kernel launch alone: the flag tables are
uploaded once, outside the events; "apply_call" is a whole RfiCleaner.apply
with its table upload), pack_transpose and, as the
yardsticks, unpack_transpose over the same rows and one 32-DM dedispersion
chunk.  The mask applied is the one rfi_clean finds on the noise (false
positives only), so without zero-DM almost every tile returns at once; the
"flagged" figure applies a mask with one flagged cell in every block instead.
--once KERNEL (sums | apply | apply_flagged | apply_zdm | pack) runs that pass once after the
set-up and nothing else (the shape of a counter or kernel-trace run).
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
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--nbits", type=int, default=2, choices=[2, 8])
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rfi_bench needs a GPU"
    n, nchans, nbits = 1 << a.log2n, a.nchans, a.nbits
    bias = 128 if nbits == 8 else 0
    hdr = synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=64e-6, foff=-0.25)
    packed = synthetic.generate_packed_torch(n, hdr, [], seed=1)
    stride = (n + 255) // 256 * 256
    rows = ops.unpack_transpose(packed, n, nchans, nbits, bias, stride=stride)
    torch.cuda.synchronize()
    _, mask = ops.rfi_clean(rows.clone(), n, nbits, bias, block=a.block)
    nblk = int(mask.nblk)
    # one flagged cell in every block: every tile has a row to fill
    cell = np.zeros((nchans, nblk), dtype=np.uint8)
    cell[np.arange(nblk) % nchans, np.arange(nblk)] = 1
    some = {"chan_flag": np.zeros(nchans, np.uint8), "block_flag": np.zeros(nblk, np.uint8), "cell": cell,
            "fill": np.asarray(mask.fill), "G": np.asarray(mask.G), "nb": np.full(nblk, nchans - 1, np.int32),
            "killmask": [1] * nchans}
    some = _C.RfiMask(n, a.block, some["chan_flag"], some["block_flag"], some["cell"], some["fill"], some["G"],
                      some["nb"], some["killmask"])
    stream = torch.cuda.current_stream().cuda_stream

    def launcher(m, zero_dm):  # tables on the device once; the call is the kernel launch
        cl = _C.RfiCleaner(_C.RfiParams(a.block, 0.0, 0.0, 0.0, zero_dm), stream)
        cl.set_mask(m)
        return lambda: cl.apply_uploaded(rows.data_ptr(), stride, rows.data_ptr(), stride, nchans, n, nbits, bias)

    passes = {
        "sums": lambda: ops.rfi_block_sums(rows, n, a.block, bias),
        "apply": launcher(mask, False),
        "apply_flagged": launcher(some, False),
        "apply_zdm": launcher(mask, True),
        "apply_call": lambda: ops.rfi_apply(rows, n, nbits, mask, a.block, bias, zero_dm=True),
        "pack": lambda: ops.pack_transpose(rows, n, nbits, bias),
        "unpack": lambda: _C.kernels.unpack_transpose(packed.data_ptr(), n, nchans, nbits, rows.data_ptr(), stride,
                                                      bias, torch.cuda.current_stream().cuda_stream),
    }
    if a.once:
        passes[a.once]()
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "log2n": a.log2n, "nchans": nchans, "nbits": nbits}))
        return
    row_bytes = float(nchans) * n
    out = {"metric": "rfi excision passes", "log2n": a.log2n, "nchans": nchans, "nbits": nbits, "block": a.block,
           "tile": ops.rfi_tile(), "flagged_cells": int(mask.flagged_cells), "cells": nchans * nblk}
    for name in ("unpack", "sums", "apply", "apply_flagged", "apply_zdm", "apply_call", "pack"):
        ms = timed(passes[name], a.reps)
        out[name + "_ms"] = round(ms, 3)
        out[name + "_row_GB_per_s"] = round(row_bytes / ms / 1e6, 1)
    # one 32-DM dedispersion chunk of the same filterbank
    del rows
    dms = [float(x) for x in np.linspace(0.0, 20.0, 32).astype(np.float32)]
    geom = _C.DedispGeometry.make(hdr, n, dms, [1] * nchans)
    dfb = _C.DeviceFilterbank(geom, stream)
    dfb.load_packed_device(packed.data_ptr())
    dd = _C.Dedisperser(dfb, stream)
    rs = _C.Dedisperser.row_stride(int(geom.out_nsamps))
    trials = torch.empty(32 * rs, dtype=torch.uint8, device="cuda")
    ms = timed(lambda: dd.run(0, 32, trials.data_ptr(), rs, stream=stream), a.reps)
    out["dedisp_32dm_ms"] = round(ms, 3)
    out["dedisp_32dm_row_GB_per_s"] = round(row_bytes / ms / 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
