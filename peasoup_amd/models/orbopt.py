"""orbopt behind ``python -m peasoup_amd oopt``: refines orbsearch candidates
(period, dm, pb, a1, phase) by folding their dedispersed rows on a dense local
grid of circular-orbit templates in one fused pass (csrc/kernels/orbopt.hip)
and searching every fold plane over period drift and boxcar width
(csrc/include/psoup/orbopt.hpp): the refined orbit and period, the S/N, the
S/N over the template grid and the fold at the optimum per candidate.

The filterbank is made resident through torch; the native ``OrbitOptimiser``
does the work on it and ``utils.outputs.write_orbopt_file`` writes the records,
so this driver and ``bin/orbopt`` write the same bytes.  One device: under
``torch.distributed.run`` rank 0 does the work and the other ranks return.

An extension beyond the reference, which stops at a constant acceleration.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List

from .. import _C
from ..utils import outputs


@dataclass
class OrbOptRun:
    header: Dict
    records: List[Dict]
    timers: Dict[str, float] = field(default_factory=dict)


def run_orbit_optimise(args, write: bool = True):
    """Optimises the candidates ``args`` (an ``OrbOptCmdLineOptions``) names on
    the current device and, with ``write``, writes ``args.outfilename``.
    Returns an :class:`OrbOptRun` on rank 0 (None elsewhere).  Every refusal of
    the definition is raised by name before any device work."""
    import time

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    t0 = time.perf_counter()
    if args.max_num_threads != 1:
        raise RuntimeError("orbopt: orbopt runs on one device (-t 1); multi-GPU runs are not supported")
    params = _C.oopt_params_of(args)
    _C.oopt_check_params(params)
    try:
        with open(args.candfilename) as f:
            text = f.read()
    except OSError:
        raise RuntimeError(f"orbopt: cannot open the candidate file {args.candfilename}") from None
    cands = _C.oopt_parse_candidates(text)
    if not cands:
        raise RuntimeError(f"orbopt: an empty candidate file ({args.candfilename})")
    cands = cands[:max(int(args.limit), 0)]
    if not cands:
        raise RuntimeError("orbopt: an empty candidate file (--limit 0)")
    dm_list = _C.oopt_dm_list(cands)
    hdr = _C.read_header(args.infilename)
    nchans, nsamps = int(hdr["nchans"]), int(hdr["nsamples"])
    killmask = _C.read_killfile(args.killfilename, nchans) if args.killfilename else [1] * nchans
    fft_size = int(args.size) if args.size else int(_C.prev_power_of_two(nsamps))
    geom = _C.DedispGeometry.make(hdr, nsamps, dm_list, killmask)
    if geom.out_nsamps < 1:
        raise RuntimeError("orbopt: the dedispersed series is empty")
    n = min(int(geom.out_nsamps), fft_size)
    for k, c in enumerate(cands):
        _C.oopt_grid(k, params, c, n, float(hdr["tsamp"]))

    import torch

    fb = _C.Filterbank.from_file(args.infilename)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP devices visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    packed = torch.from_numpy(fb.data().copy()).to(dev)
    t1 = time.perf_counter()
    stream = _C.GpuStream()
    torch.cuda.synchronize(dev)  # the upload ran on torch's stream
    geom = _C.DedispGeometry.make(fb.header, fb.nsamps, dm_list, killmask)
    dfb = _C.DeviceFilterbank(geom, stream.handle)
    dfb.load_packed_device(packed.data_ptr())
    stream.synchronize()
    del packed
    opt = _C.OrbitOptimiser(params, dfb, fft_size, stream.handle)
    records = opt.optimise(cands)
    t2 = time.perf_counter()
    header = dict(nints=params.nints, nbins=params.nbins, npb=params.npb, na1=params.na1, nphase=params.nphase,
                  np=params.np, nw=int(opt.nwidths), n=int(opt.span), tsamp=float(opt.tsamp), p_step=params.p_step)
    if write:
        outputs.write_orbopt_file(args.outfilename, header, records)
    header["ncand"] = len(records)
    del opt, dfb
    return OrbOptRun(header, records, {"reading": t1 - t0, "searching": t2 - t1, "total": time.perf_counter() - t0})


def print_records(run) -> None:
    """One line per candidate, as ``bin/orbopt -v``."""
    print("# period opt_period dm acc pb opt_pb a1 opt_a1 phase opt_phase width snr snr_in flags")
    for r in run.records:
        print(_C.oopt_verbose_line(r))
