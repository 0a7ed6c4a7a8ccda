"""fits2fil behind ``python -m peasoup_amd fits``: read one search-mode PSRFITS
file and convert it on the device (csrc/kernels/psrfits.hip and the fildigi
kernels, ``FitsDigitiser``) into an 8-bit, descending-frequency SIGPROC
filterbank, byte for byte as ``bin/fits2fil``.

The file is read into a NumPy array, converted by the native ``FitsDigitiser``
in time chunks and written from Python with the header built here.  Under
``torch.distributed.run`` rank 0 does the work and the other ranks return.
"""
from __future__ import annotations

import os

import numpy as np

from .. import _C
from ..utils.sigproc import header_bytes


def convert_psrfits(args):
    """Converts the PSRFITS file ``args`` (a ``FitsCmdLineOptions``) names and
    writes the outputs it names; returns the result dict on rank 0 (None
    elsewhere)."""
    from .. import ops

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    params = _C.fits_digi_params_from(args)
    _C.digi_check_params(params)
    opt = _C.fits_options_from(args)
    data = np.fromfile(args.infilename, dtype=np.uint8)
    nchan = int(_C.fits_inspect(data, opt, "")["nchan"])  # the native reader's refusals, by name
    kill = None
    if args.killfilename:
        kill, _ = _C.read_killfile(args.killfilename, nchan)
    y, res = ops.fits_digitise(data, params.sigma_out, params.scale, params.rescale_blocks, kill, opt.pol,
                               opt.no_scales, opt.no_offsets, opt.no_weights, opt.telescope_id, opt.machine_id,
                               os.path.basename(args.infilename))
    tmp = args.outfilename + ".tmp"
    with open(tmp, "wb") as f:
        f.write(header_bytes(res["header"], keep_present=True))
        f.write(np.ascontiguousarray(y).tobytes())
    os.replace(tmp, args.outfilename)
    if args.killoutfilename:
        _C.write_killfile(args.killoutfilename, [int(k) for k in res["killmask"]])
    return res
