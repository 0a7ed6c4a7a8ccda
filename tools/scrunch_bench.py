#!/usr/bin/env python3
"""filscrunch passes on one GPU, on a synthetic noise filterbank (1024 channels
x 2^22 samples by default):

    python tools/scrunch_bench.py [--log2n 22] [--nchans 1024] [--nbits 2|8] [--dm 100] [--reps 7]

One JSON line with the median time (device events, after a warm-up) and the
GB/s of int8 row bytes (nchans x nsamps) of scrunch_sums and scrunch_quant at
(nsub = nchans / 16, f = 1), (nsub = nchans, f = 4) and (nchans / 16, 4), and,
as the yardsticks, unpack_transpose over the same rows and one 32-DM
dedispersion chunk, which reads the same bytes.  The timed calls are the torch
ops: scrunch_sums includes the upload of its small tables and the zeroing of
the block sums, scrunch_quant a padded copy of A (its own figure counts the
row bytes too, to compare; the pass itself moves 5 bytes per output sample).
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
from peasoup_amd.utils import reference as ref  # noqa: E402
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
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--nbits", type=int, default=2, choices=[2, 8])
    ap.add_argument("--dm", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "scrunch_bench needs a GPU"
    n, nchans, nbits = 1 << a.log2n, a.nchans, a.nbits
    bias = 128 if nbits == 8 else 0
    hdr = synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=64e-6, foff=-0.25)
    packed = synthetic.generate_packed_torch(n, hdr, [], seed=1)
    stride = (n + 255) // 256 * 256
    rows = ops.unpack_transpose(packed, n, nchans, nbits, bias, stride=stride)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    delays = ref.delay_table(nchans, hdr["tsamp"], hdr["fch1"], hdr["foff"])
    row_bytes = float(nchans) * n
    out = {"metric": "filscrunch passes", "log2n": a.log2n, "nchans": nchans, "nbits": nbits, "dm": a.dm,
           "tile": ops.scrunch_tile(), "stat_block": int(_C.scrunch_stat_block())}
    ms = timed(lambda: _C.kernels.unpack_transpose(packed.data_ptr(), n, nchans, nbits, rows.data_ptr(), stride, bias,
                                                   stream), a.reps)
    out["unpack_ms"] = round(ms, 3)
    out["unpack_row_GB_per_s"] = round(row_bytes / ms / 1e6, 1)
    for nsub, f in ((nchans // 16, 1), (nchans, 4), (nchans // 16, 4)):
        rel, R = ref.scrunch_offsets(a.dm if nsub < nchans else 0.0, delays, nsub)
        nout = (n - R) // f
        key = f"nsub{nsub}_f{f}"
        res = {}

        def sums():
            res["A"], res["S1"], res["S2"] = ops.scrunch_sums(rows, n, rel, f, nsub, nout, bias=bias)

        ms = timed(sums, a.reps)
        out[key + "_sums_ms"] = round(ms, 3)
        out[key + "_sums_row_GB_per_s"] = round(row_bytes / ms / 1e6, 1)
        S1, S2 = (t.cpu().numpy().view(np.uint64) for t in (res["S1"], res["S2"]))
        sc = _C.scrunch_scale(S1, S2, nout, np.full(nsub, nchans // nsub, np.int32), 16.0)
        A = res["A"]
        ms = timed(lambda: ops.scrunch_quant(A, sc["M"], sc["mul"], sc["live"]), a.reps)
        out[key + "_quant_ms"] = round(ms, 3)
        out[key + "_quant_row_GB_per_s"] = round(row_bytes / ms / 1e6, 1)
        out[key + "_mul"] = int(sc["mul"])
        del A, res
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
