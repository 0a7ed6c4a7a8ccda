"""fildigi behind ``python -m peasoup_amd digi``: digitise a SIGPROC filterbank
of 8, 16 or 32 bits and either band order on the device (csrc/kernels/digi.hip,
``Digitiser``) into an 8-bit, descending-frequency file, byte for byte as
``bin/fildigi``.

The file's samples are read into a NumPy array, digitised by the native
``Digitiser`` in time chunks and written from Python with the rewritten header.
Under ``torch.distributed.run`` rank 0 does the work and the other ranks
return.
"""
from __future__ import annotations

import os

import numpy as np

from .. import _C
from ..utils.reference import digi_header
from ..utils.sigproc import header_bytes, read_raw_filterbank


def digitise_filterbank(args):
    """Digitises the filterbank ``args`` (a ``DigiCmdLineOptions``) names and
    writes the outputs it names; returns the result dict on rank 0 (None
    elsewhere)."""
    from .. import ops

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    params = _C.digi_params_from(args)
    _C.digi_check_params(params)
    _C.read_raw_filterbank_info(args.infilename)  # the native reader's refusals, by name
    hdr, data = read_raw_filterbank(args.infilename)
    nsamps, nchans = data.shape
    kill = None
    if args.killfilename:
        kill, _ = _C.read_killfile(args.killfilename, nchans)
    y, res = ops.digitise(data, float(hdr["foff"]), params.sigma_out, params.scale, params.rescale_blocks, kill)
    tmp = args.outfilename + ".tmp"
    with open(tmp, "wb") as f:
        f.write(header_bytes(digi_header(hdr, nsamps), keep_present=True))
        f.write(np.ascontiguousarray(y).tobytes())
    os.replace(tmp, args.outfilename)
    if args.killoutfilename:
        _C.write_killfile(args.killoutfilename, [int(k) for k in res["killmask"]])
    return res
