"""The sideband (phase-modulation) search behind ``python -m peasoup_amd sb``
(csrc/include/psoup/sideband.hpp): for orbits shorter than the observation.

Every dedispersed row is whitened and transformed by the unchanged
``Whitener``; short FFTs of the band-normalised powers of that spectrum
(csrc/kernels/sideband.hip) peak at ``j = M pb / T`` where a pulsar's sidebands
lie.  The filterbank is made resident through torch; the native
``SidebandSearcher`` does the search on it, so this driver and ``bin/sbsearch``
write the same candidates.  One device: under ``torch.distributed.run`` rank 0
does the work and the other ranks return; checkpoints are not supported.

An extension beyond the reference, which has no Fourier-domain binary search.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List

import torch

from .. import _C


@dataclass
class SidebandResult:
    candidates: List["_C.SbCandidate"]
    setup: "_C.SbSetup"
    events: int = 0
    reruns: int = 0
    timers: Dict[str, float] = field(default_factory=dict)


def run_sideband_search(args, write: bool = True, capacity: int = 1 << 16):
    """Runs the sideband search ``args`` (an ``SbCmdLineOptions``) describes on
    the current device and, with ``write``, writes ``args.outfilename``.
    Returns a :class:`SidebandResult` on rank 0 (None elsewhere).  Every
    refusal of the definition is raised (by ``_C.sb_setup``) before any device
    work."""
    import time

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    t0 = time.perf_counter()
    setup = _C.sb_setup(args)
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
    ss = _C.SidebandSearcher(setup, dfb, stream.handle, int(capacity))
    events = ss.search()
    cands = _C.sb_cluster_candidates(events)
    t2 = time.perf_counter()
    cands = cands[:max(int(args.search.limit), 0)]
    if write:
        _C.write_sb_output(args, setup, cands)
    res = SidebandResult(cands, setup, len(events), int(ss.reruns),
                         {"reading": t1 - t0, "searching": t2 - t1, "total": time.perf_counter() - t0})
    del ss, dfb
    return res
