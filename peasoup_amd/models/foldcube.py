"""Filterbank fold cubes behind ``python -m peasoup_amd cube``: for each
periodicity candidate the filterbank is folded into a subint x subband x phase
cube (csrc/kernels/foldcube.hip, ``CubeFolder``), the data of the
frequency-phase and time-phase diagnostic panels.

The candidates come from a text file (``--candfile``: ``period_s dm acc`` per
line, as ``bin/foldcube``) or from the ``overview.xml`` of a finished search
(``--overview``, the first ``--top`` candidates: ``opt_period`` where it is
positive, else ``period``, with the candidate's DM and acceleration).  The fold
itself is the native pipeline on one device, so both entry points write the
same bytes.  Under ``torch.distributed.run`` rank 0 does the work and the
other ranks return.

An extension beyond the reference, whose fold_filterbank_kernel is commented out.
"""
from __future__ import annotations

import os
from typing import List

from .. import _C
from ..utils.outputs import OverviewFile


def overview_candidates(path: str, top: int) -> List["_C.CubeCandidate"]:
    """The first ``top`` candidates of an overview.xml as CubeCandidates."""
    ov = OverviewFile(path)
    out = []
    for i in range(min(int(top), len(ov))):
        c = ov.get_candidate(i)
        period = c["opt_period"] if c["opt_period"] > 0 else c["period"]
        out.append(_C.CubeCandidate(float(period), float(c["dm"]), float(c["acc"])))
    return out


def run_fold_cubes(args):
    """Folds the candidates ``args`` (a ``FoldCubeCmdLineOptions``) names and
    writes ``args.outfilename``; returns the ``CubeRun`` on rank 0 (None elsewhere)."""
    if bool(args.candfilename) == bool(args.overviewfilename):
        raise ValueError("give exactly one of --candfile and --overview")
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    if args.overviewfilename:
        cands = overview_candidates(args.overviewfilename, args.top)
        if not cands:
            raise ValueError(f"{args.overviewfilename}: no candidates")
    else:
        cands = _C.read_cube_candfile(args.candfilename, args.limit)
    return _C.run_cube_pipeline(args, cands)
