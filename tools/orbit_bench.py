#!/usr/bin/env python3
"""The orbit search's two costs on one GPU:

    python tools/orbit_bench.py [--log2n 23] [--rows 32] [--templates 16] [--reps 7]
                                [--search_log2n 23] [--nchans 64] [--dms 8] [--acc 500]
                                [--search_templates 64]

One JSON line.  (1) The median time (device events, after a warm-up) and the
GB/s of ``orbit_resample`` for ``rows`` x 2^log2n samples x ``templates``
templates (bytes counted: the output written once and as many source bytes
read, 2 x rows x templates x n), against the floor, a device-to-device copy of
the same output bytes timed in the same session.  The timed call is the torch
op: it includes the upload of the quantised templates.  (2) The host wall time
of one DM chunk (``dms`` DMs) of ``OrbitSearcher`` with ``search_templates``
templates on a synthetic filterbank of 2^search_log2n samples searched over
+-``acc`` m/s^2 (685 acceleration trials per DM at the defaults, the headline
bench's), against ``search_templates`` times the same chunk through the plain
search: the same searcher, and so the unchanged engine, at the one-template
identity bank.  That plain run still copies each row once through the resample
at a1 = 0, which is left in its time.  The share (t_orbit - templates x
t_plain) / t_orbit is what the loop adds in resampling, repeated whitening and
distillation.
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


def bank(count, n):
    """``count`` templates with orbits of 0.5 to 3 spans and amplitudes up to 400 samples, every phase."""
    T = n * float(np.float32(TSAMP))
    return [(T * (0.5 + 2.5 * k / max(count - 1, 1)), 400.0 * TSAMP * k / max(count - 1, 1), (0.37 * k) % 1.0)
            for k in range(count)]


def kernel_part(a, out):
    n, rows, K = 1 << a.log2n, a.rows, a.templates
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(0, 256, (rows, n), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.empty((rows, K, n), dtype=torch.uint8, device="cuda")
    q = ops.orbit_quantise(bank(K, n), TSAMP)
    moved = 2.0 * rows * K * n
    src = torch.empty_like(y)
    copy_ms = timed(lambda: y.copy_(src), a.reps)
    del src
    ms = timed(lambda: ops.orbit_resample(x, n, (), 0.0, out=y, quant=q), a.reps)
    out.update(resample_ms=round(ms, 3), resample_GB_per_s=round(moved / ms / 1e6, 1), copy_ms=round(copy_ms, 3),
               copy_GB_per_s=round(moved / copy_ms / 1e6, 1), resample_over_copy=round(ms / copy_ms, 3),
               output_GB=round(rows * K * n / 1e9, 3))


def search_part(a, out):
    ns = 1 << a.search_log2n
    hdr = synthetic.make_header(nchans=a.nchans, nbits=8, tsamp=TSAMP)
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
        base = ["orbsearch", "-i", path, "--dm_start", "0", "--dm_end", str(a.dm_end), "--acc_start", str(-a.acc),
                "--acc_end", str(a.acc), "--fft_size", str(ns)]

        def run(templates, reps):
            bankfile = os.path.join(tmp, f"bank{len(templates)}.txt")
            with open(bankfile, "w") as f:
                f.writelines(f"{pb!r} {a1!r} {ph!r}\n" for pb, a1, ph in templates)
            ok, _, args = _C.parse_orbit_cmdline(base + ["--bankfile", bankfile])
            assert ok
            setup = _C.orbit_setup(args)
            stream = _C.GpuStream()
            dfb = _C.DeviceFilterbank(setup.geometry, stream.handle)
            dfb.load_packed_device(packed.data_ptr())
            stream.synchronize()
            osr = _C.OrbitSearcher(setup, dfb, stream.handle)
            d1 = min(a.dms, len(setup.dm_list))
            osr.search(0, d1)  # warm-up: buffers, code objects, FFT plans
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                osr.search(0, d1)
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts), d1, len(setup.bank), len(setup.accel_plan.generate(0.0))

        t_plain, d1, _, nacc = run([(100.0, 0.0, 0.0)], max(3, a.reps))
        t_orbit, _, nt, _ = run(bank(a.search_templates, ns), 3)
    out.update(search_log2n=a.search_log2n, chunk_dms=d1, search_templates=nt, accel_trials_per_dm=nacc,
               orbit_chunk_s=round(t_orbit, 4), plain_chunk_s=round(t_plain, 4),
               plain_times_templates_s=round(t_plain * nt, 4),
               orbit_loop_share=round((t_orbit - t_plain * nt) / t_orbit, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=23)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--search_log2n", type=int, default=23)
    ap.add_argument("--search_templates", type=int, default=64)
    ap.add_argument("--nchans", type=int, default=64)
    ap.add_argument("--dms", type=int, default=8)
    ap.add_argument("--acc", type=float, default=500.0, help="search +-acc m/s^2")
    ap.add_argument("--dm_end", type=float, default=30.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "orbit_bench needs a GPU"
    out = {"metric": "orbsearch", "log2n": a.log2n, "rows": a.rows, "templates": a.templates,
           "tile": int(_C.ORBIT_TILE), "tiles_per_group": int(_C.ORBIT_TILES_PER_GROUP)}
    kernel_part(a, out)
    if a.search_templates > 0:
        search_part(a, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
