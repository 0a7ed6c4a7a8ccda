"""Burst cutouts behind ``python -m peasoup_amd burst``: for each single-pulse
candidate the dedispersed dynamic spectrum (waterfall) and the DM-time plane
around it are cut out of the filterbank (csrc/kernels/burstcube.hip,
``BurstCutter``), the data of the two standard diagnostic panels of a transient
candidate.

The candidates come from an ``spsearch`` output (``--spfile``: its S/N, sample,
width and DM columns) or from a text file (``--candfile``: ``sample width dm
[snr]`` per line), as for ``bin/burstcube``.  The cut itself is the native
pipeline on one device, so both entry points write the same bytes.  Under
``torch.distributed.run`` rank 0 does the work and the other ranks return.

An extension beyond the reference.
"""
from __future__ import annotations

import os

from .. import _C


def run_burst_cutouts(args):
    """Cuts out the candidates ``args`` (a ``BurstCubeCmdLineOptions``) names and
    writes ``args.outfilename``; returns the ``BurstRun`` on rank 0 (None elsewhere)."""
    if bool(args.spfilename) == bool(args.candfilename):
        raise ValueError("give exactly one of --spfile and --candfile")
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    return _C.run_burst_pipeline(args)
