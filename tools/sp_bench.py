#!/usr/bin/env python3
"""Single-pulse search throughput on one GPU: SinglePulseEngine.search_block on
chunks of DM trials dedispersed from the bench's synthetic 2-bit filterbank.

    python tools/sp_bench.py [--dms 32 64] [--log2n 20 23] [--nchans 64] [--reps 10] [--once] [--dedisp_kernel packed2]

Per (DMs, samples) one JSON line: ms per chunk (device-synchronised host clock
over --reps calls after a warm-up), samples x DMs per second, and the uint8 row
traffic the three launches need (block means and sigma read every row once, the
search once plus its halo of boxcar_max per 8192-sample tile) per second.
--once runs one dedispersion + one search per shape and nothing else (the
shape of a kernel-trace run).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from peasoup_amd import _C, dedisp_kernel  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dms", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--log2n", type=int, nargs="+", default=[20, 23])
    ap.add_argument("--nchans", type=int, default=64)
    ap.add_argument("--tsamp", type=float, default=64e-6)
    ap.add_argument("--boxcar_max", type=int, default=4096)
    ap.add_argument("--min_snr", type=float, default=6.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--dedisp_kernel", default="packed2", help="the chunk's dedispersion (the trace's yardstick)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sp_bench needs a GPU"
    stream = torch.cuda.current_stream().cuda_stream
    for log2n in a.log2n:
        nsamps = 1 << log2n
        hdr = synthetic.make_header(nchans=a.nchans, nbits=2, tsamp=a.tsamp)
        packed = synthetic.generate_packed_torch(nsamps, hdr, [], seed=1)  # noise only, as bench.py's default
        ndm_max = max(a.dms)
        dm_list = [0.5 * i for i in range(ndm_max)]
        geom = _C.DedispGeometry.make(hdr, nsamps, dm_list, [1] * a.nchans)
        dfb = _C.DeviceFilterbank(geom, stream)
        dfb.load_packed_device(packed.data_ptr())
        dd = _C.Dedisperser(dfb, stream)
        n = int(geom.out_nsamps)
        rs = _C.Dedisperser.row_stride(n)
        trials = torch.empty(ndm_max * rs, dtype=torch.uint8, device="cuda")
        p = _C.SpParams()
        p.tsamp, p.boxcar_max, p.min_snr = a.tsamp, a.boxcar_max, a.min_snr
        eng = _C.SinglePulseEngine(p, n, stream)
        for ndm in a.dms:
            dd.run(0, ndm, trials.data_ptr(), rs, dedisp_kernel(a.dedisp_kernel))
            ev = eng.search_block(trials.data_ptr(), rs, ndm, 0)  # warm-up (and the --once run)
            torch.cuda.synchronize()
            if a.once:
                print(json.dumps({"dms": ndm, "log2n": log2n, "nsamps": n, "events": len(ev)}))
                continue
            t0 = time.perf_counter()
            for _ in range(a.reps):
                eng.search_block(trials.data_ptr(), rs, ndm, 0)  # ends in a stream synchronise
            dt = (time.perf_counter() - t0) / a.reps
            tiles = (n + _C.SP_TILE - 1) // _C.SP_TILE
            row_bytes = ndm * (3 * n + tiles * max(eng.widths))
            print(json.dumps({"metric": "single-pulse samples x DMs / s", "value": round(ndm * n / dt, 1),
                              "ms_per_chunk": round(1e3 * dt, 4), "dms": ndm, "log2n": log2n, "nsamps": n,
                              "widths": len(eng.widths), "baseline": eng.baseline,
                              "row_bytes_per_s": round(row_bytes / dt, 1), "events": len(ev),
                              "reruns": eng.reruns}))
        del eng, dd, dfb, trials, packed


if __name__ == "__main__":
    main()
