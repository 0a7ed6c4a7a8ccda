"""burstopt behind ``python -m peasoup_amd bopt``: a search over DM rows,
boxcar widths and start bins on the burst cutouts ``burstcube`` wrote
(csrc/kernels/burstopt.hip, ``BurstOptimiser``): per pulse the refined DM,
width and arrival sample, the S/N at the optimum, at the candidate's DM and at
DM 0, the S/N-versus-DM curves of both planes and the pulse energy per subband.

The search itself is the native pipeline on one device, so this entry point
and ``bin/burstopt`` write the same bytes.  Under ``torch.distributed.run`` rank
0 does the work and the other ranks return.

An extension beyond the reference, which has no single-pulse search.
"""
from __future__ import annotations

import os

from .. import _C


def run_burst_opt(args):
    """Searches the cutouts ``args`` (a ``BurstOptCmdLineOptions``) names and
    writes ``args.outfilename``; returns the ``BurstOptRun`` on rank 0 (None
    elsewhere)."""
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    return _C.run_bopt_pipeline(args)


def print_records(run) -> None:
    """One line per candidate, as ``bin/burstopt -v``."""
    print("# sample opt_sample width opt_width dm opt_dm snr snr_coarse snr_in snr_dm0 frac_pos")
    for i in range(run.ncand):
        r = run.result(i)
        print("%d %d %u %u %.6g %.6g %.3f %.3f %.3f %.3f %.3f" % (
            r["sample"], r["opt_sample"], r["width"], r["opt_width"], r["dm"], r["opt_dm"], r["snr"],
            r["snr_coarse"], r["snr_in"], r["snr_dm0"], r["frac_pos"]))
