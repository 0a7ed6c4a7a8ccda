"""cubeopt behind ``python -m peasoup_amd opt``: a brute-force search over DM,
period-drift and acceleration-drift trials on the fold cubes ``foldcube``
wrote (csrc/kernels/cubeopt.hip, ``CubeOptimiser``), the prepfold / pdmp step:
an S/N-versus-DM curve, a P-Pdot plane, the optimum trial and its profile per
candidate.

The search itself is the native pipeline on one device, so this entry point
and ``bin/cubeopt`` write the same bytes.  Under ``torch.distributed.run`` rank
0 does the work and the other ranks return.

An extension beyond the reference, whose FoldOptimiser refines the period only
and never sees frequency.
"""
from __future__ import annotations

import os

from .. import _C


def run_cube_opt(args):
    """Searches the cubes ``args`` (a ``CubeOptCmdLineOptions``) names and
    writes ``args.outfilename``; returns the ``CubeOptRun`` on rank 0 (None
    elsewhere)."""
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    return _C.run_opt_pipeline(args)


def print_records(run) -> None:
    """One line per candidate, as ``bin/cubeopt -v``."""
    print("# period opt_period dm opt_dm acc opt_acc width snr snr_in snr_dm0")
    for i in range(run.ncand):
        r = run.result(i)
        print("%.12g %.12g %.6g %.6g %.6g %.6g %u %.3f %.3f %.3f" % (
            r["period"], r["opt_period"], r["dm"], r["opt_dm"], r["acc"], r["opt_acc"], r["opt_width"], r["snr"],
            r["snr_in"], r["snr_dm0"]))
