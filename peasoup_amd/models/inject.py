"""filinject behind ``python -m peasoup_amd inject``: add dispersed pulsars and
single bursts to a SIGPROC filterbank of 1, 2, 4 or 8 bits on the device
(csrc/kernels/inject.hip, ``Injector``) and write a file of the same width,
byte for byte as ``bin/filinject``.

The file's data block is read into a NumPy array, injected by the native
``Injector`` in time chunks and written from Python behind the header bytes of
the input, copied verbatim.  Under ``torch.distributed.run`` rank 0 does the
work and the other ranks return.
"""
from __future__ import annotations

import os

import numpy as np

from .. import _C
from ..utils.sigproc import read_header


def inject_filterbank(args):
    """Injects into the filterbank ``args`` (an ``InjectCmdLineOptions``) names
    and writes the outputs it names; returns the result dict on rank 0 (None
    elsewhere)."""
    from .. import ops

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    if args.units not in ("sigma", "level"):
        raise ValueError(f"inject: units must be sigma or level, got {args.units}")
    if not args.injfilename:
        raise ValueError("inject: no injection file (--injfile)")
    signals = _C.inject_read_file(args.injfilename)
    hdr = read_header(args.infilename)
    nchans, nbits, nsamps = int(hdr["nchans"]), int(hdr["nbits"]), int(hdr["nsamples"])
    _C.inject_check_geometry(nchans, nbits, nsamps, float(hdr["tsamp"]), float(hdr["fch1"]), float(hdr["foff"]))
    nbytes = nsamps * nchans * nbits // 8
    with open(args.infilename, "rb") as f:
        head = f.read(int(hdr["size"]))
    packed = np.fromfile(args.infilename, dtype=np.uint8, count=nbytes, offset=int(hdr["size"]))
    if packed.size < nbytes:
        raise ValueError("filinject: truncated filterbank")
    kill = None
    if args.killfilename:
        kill, _ = _C.read_killfile(args.killfilename, nchans)
    y, res = ops.inject_filterbank_bytes(packed, hdr, nsamps, signals, kill, int(args.seed), args.units,
                                         not args.no_smear)
    tmp = args.outfilename + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head)
        f.write(np.ascontiguousarray(y).tobytes())
    os.replace(tmp, args.outfilename)
    if args.truthfilename:
        tmp = args.truthfilename + ".tmp"
        with open(tmp, "w") as f:
            f.write(_C.inject_truth_text(signals, [tuple(t) for t in res["truth"]], args.units, int(args.seed)))
        os.replace(tmp, args.truthfilename)
    res["signals"] = signals
    return res
