#!/usr/bin/env python3
"""The jerk search's two costs on one GPU:

    python tools/jerk_bench.py [--log2n 23] [--rows 32] [--jerks 16] [--reps 7]
                               [--search_log2n 23] [--nchans 64] [--dms 8] [--acc 500]

One JSON line.  (1) The median time (device events, after a warm-up) and the
GB/s of ``jerk_resample`` for ``rows`` x 2^log2n samples x ``jerks`` jerk
trials (bytes counted: the output written once and as many source bytes read,
2 x rows x jerks x n), against the floor, a device-to-device copy of the same
output bytes timed in the same session.  The timed call is the torch op: it
includes the upload of the ``jerks`` factors.  (2) The host wall time of one DM
chunk (``dms`` DMs) of ``JerkSearcher`` with ``jerks`` jerk trials on a
synthetic filterbank of 2^search_log2n samples searched over +-``acc`` m/s^2
(685 acceleration trials per DM at the defaults, the headline bench's, so that
the plain chunk is bound by throughput, not by latency), against ``jerks``
times the same chunk through the plain search: the same searcher, and so the
unchanged engine, at the jerk grid {0}.  That plain run still copies each row
once through the resample at factor 0, which is left in its time.  The share
(t_jerk - jerks x t_plain) / t_jerk is what the loop adds in resampling,
repeated whitening and distillation.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from peasoup_amd import _C, ops  # noqa: E402
from peasoup_amd.utils import synthetic  # noqa: E402
from peasoup_amd.utils.sigproc import header_bytes  # noqa: E402


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


def kernel_part(a, out):
    n, rows, K = 1 << a.log2n, a.rows, a.jerks
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(0, 256, (rows, n), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.empty((rows, K, n), dtype=torch.uint8, device="cuda")
    # jerk factors up to a shift of 400 samples, both signs (0 included)
    jf = np.linspace(-1.0, 1.0, K) * 400.0 * 12.0 * np.sqrt(3.0) / float(n) ** 3
    moved = 2.0 * rows * K * n
    src = torch.empty_like(y)
    copy_ms = timed(lambda: y.copy_(src), a.reps)
    del src
    ms = timed(lambda: ops.jerk_resample(x, n, (), 0.0, out=y, factors=jf), a.reps)
    out.update(resample_ms=round(ms, 3), resample_GB_per_s=round(moved / ms / 1e6, 1), copy_ms=round(copy_ms, 3),
               copy_GB_per_s=round(moved / copy_ms / 1e6, 1), resample_over_copy=round(ms / copy_ms, 3),
               output_GB=round(rows * K * n / 1e9, 3))


def search_part(a, out):
    ns = 1 << a.search_log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=8, tsamp=64e-6)
    hdr["nsamples"] = ns
    # the samples stay on the device; the file holds the header and a sparse data block (the setup reads the header)
    packed = synthetic.generate_packed_torch(ns, hdr, [synthetic.PulsarSpec(period=0.0123, dm=5.0, amplitude=0.05)],
                                             seed=1)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.fil")
        with open(path, "wb") as f:
            f.write(header_bytes(hdr))
            f.truncate(f.tell() + ns * a.nchans)
        base = ["jerksearch", "-i", path, "--dm_start", "0", "--dm_end", str(a.dm_end), "--acc_start", str(-a.acc),
                "--acc_end", str(a.acc), "--fft_size", str(ns)]

        def run(extra, reps):
            ok, _, args = _C.parse_jerk_cmdline(base + extra)
            assert ok
            setup = _C.jerk_setup(args)
            stream = _C.GpuStream()
            dfb = _C.DeviceFilterbank(setup.geometry, stream.handle)
            dfb.load_packed_device(packed.data_ptr())
            stream.synchronize()
            js = _C.JerkSearcher(setup, dfb, stream.handle)
            d1 = min(a.dms, len(setup.dm_list))
            js.search(0, d1)  # warm-up: buffers, code objects, FFT plans
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                js.search(0, d1)
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts), d1, len(setup.jerks[0]), len(setup.accel_plan.generate(0.0))

        step = 0.9 * 1.8 * 6 * 299792458.0 / (ns * 64e-6) ** 2 / a.jerks  # inside the refusal rule
        t_plain, d1, _, nacc = run([], max(3, a.reps))
        t_jerk, _, nj, _ = run(["--jerk_start", "0", "--jerk_end", repr(step * (a.jerks - 1) * 1.0001),
                                "--jerk_step", repr(step)], 3)
    out.update(search_log2n=a.search_log2n, chunk_dms=d1, jerk_trials=nj, accel_trials_per_dm=nacc,
               jerk_chunk_s=round(t_jerk, 4), plain_chunk_s=round(t_plain, 4),
               plain_times_jerks_s=round(t_plain * nj, 4),
               jerk_loop_share=round((t_jerk - t_plain * nj) / t_jerk, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=23)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--jerks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--search_log2n", type=int, default=23)
    ap.add_argument("--nchans", type=int, default=64)
    ap.add_argument("--dms", type=int, default=8)
    ap.add_argument("--acc", type=float, default=500.0, help="search +-acc m/s^2")
    ap.add_argument("--dm_end", type=float, default=30.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jerk_bench needs a GPU"
    out = {"metric": "jerksearch", "log2n": a.log2n, "rows": a.rows, "jerks": a.jerks, "tile": int(_C.JERK_TILE)}
    kernel_part(a, out)
    search_part(a, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
