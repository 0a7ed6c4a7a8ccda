"""The circular-orbit search behind ``python -m peasoup_amd orb``: orbit
templates as an outer loop over the acceleration search
(csrc/include/psoup/orbit.hpp).

Each template (pb, a1, phase) re-indexes the dedispersed rows by the Roemer
delay of a circular orbit (csrc/kernels/orbit.hip), which makes them uniform in
the orbit frame; the unchanged ``SearchEngine`` then searches the re-indexed
rows over its acceleration list.  The filterbank is made resident through
torch; the native ``OrbitSearcher`` does the search on it, so this driver and
``bin/orbsearch`` write the same candidates.  One device: under
``torch.distributed.run`` rank 0 does the work and the other ranks return;
checkpoints are not supported.

An extension beyond the reference, which stops at a constant acceleration.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List

import torch

from .. import _C


@dataclass
class OrbitResult:
    candidates: List["_C.OrbitCandidate"]
    setup: "_C.OrbitSetup"
    accel_trials: int = 0
    template_trials: int = 0
    timers: Dict[str, float] = field(default_factory=dict)


def run_orbit_search(args, write: bool = True):
    """Runs the orbit search ``args`` (an ``OrbitCmdLineOptions``) describes on
    the current device and, with ``write``, writes ``args.outfilename``.
    Returns an :class:`OrbitResult` on rank 0 (None elsewhere).  Every refusal
    of the definition is raised (by ``_C.orbit_setup``) before any device work."""
    import time

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    t0 = time.perf_counter()
    setup = _C.orbit_setup(args)
    fb = _C.Filterbank.from_file(args.search.infilename)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP devices visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    packed = torch.from_numpy(fb.data().copy()).to(dev)
    t1 = time.perf_counter()
    stream = _C.GpuStream()
    torch.cuda.synchronize(dev)  # the upload ran on torch's stream
    dfb = _C.DeviceFilterbank(setup.geometry, stream.handle)
    dfb.load_packed_device(packed.data_ptr())
    stream.synchronize()
    del packed
    osr = _C.OrbitSearcher(setup, dfb, stream.handle)
    cands = osr.search()
    cands = _C.orbit_global_distill(cands, args, setup)
    t2 = time.perf_counter()
    if args.search.npdmp > 0:
        cands = osr.fold(cands, args.search.npdmp)
    t3 = time.perf_counter()
    cands = cands[:max(int(args.search.limit), 0)]
    if write:
        _C.write_orbit_output(args, setup, cands)
    res = OrbitResult(cands, setup, int(osr.accel_trials), int(osr.template_trials),
                      {"reading": t1 - t0, "searching": t2 - t1, "folding": t3 - t2, "total": time.perf_counter() - t0})
    del osr, dfb
    return res
