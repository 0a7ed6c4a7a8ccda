"""filscrunch behind ``python -m peasoup_amd scrunch``: subband and
time-scrunch a filterbank on the device (csrc/kernels/scrunch.hip,
``Scruncher``) into an 8-bit SIGPROC file, byte for byte as ``bin/filscrunch``.

The packed bytes are uploaded and unpacked with the torch ops, scrunched by the
native ``Scruncher``, turned back to time-major bytes by ``pack_transpose`` and
written from Python with the rewritten header.  ``--plan`` prints the
time-scrunch tiers from the header alone.  Under ``torch.distributed.run`` rank
0 does the work and the other ranks return.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _C
from ..utils.sigproc import header_bytes, read_header


def scrunched_header(hdr: dict, nsub: int, tscrunch: int, dm: float, nout: int) -> dict:
    """The output's header: every key of the input, with nchans, foff, tsamp,
    nbits, nsamples (where present) and refdm changed."""
    out = dict(hdr)
    w = int(hdr["nchans"]) // nsub
    out.update(nchans=nsub, foff=float(w) * float(hdr["foff"]), tsamp=float(tscrunch) * float(hdr["tsamp"]), nbits=8,
               nsamples=nout if "nsamples" in hdr.get("_present", ()) else 0, refdm=float(np.float32(dm)))
    return out


def print_plan(args) -> None:
    hdr = read_header(args.infilename)
    for lo, hi, f in _C.scrunch_plan(float(hdr["tsamp"]), float(hdr["fch1"]), float(hdr["foff"]), int(hdr["nchans"]),
                                     float(args.dm_end)):
        print(f"{lo:.6f} {hi:.6f} {f}")


def scrunch_filterbank(args):
    """Scrunches the filterbank ``args`` (a ``ScrunchCmdLineOptions``) names
    and writes the outputs it names; returns the result dict on rank 0 (None
    elsewhere)."""
    from .. import ops

    if int(os.environ.get("RANK", "0")) != 0:
        return None
    fb = _C.Filterbank.from_file(args.infilename)
    hdr = read_header(args.infilename)
    nchans, nbits, nsamps = int(fb.nchans), int(fb.nbits), int(fb.nsamps)
    if not float(hdr["foff"]) < 0:
        raise ValueError(f"scrunch: foff must be negative (channels in descending frequency), got {hdr['foff']}")
    params = _C.scrunch_check_params(_C.scrunch_params_from(args), nchans)
    kill = None
    if args.killfilename:
        kill, _ = _C.read_killfile(args.killfilename, nchans)
    nbytes = nsamps * nchans * nbits // 8
    packed = torch.from_numpy(np.array(fb.data()[:nbytes], copy=True)).cuda()
    bias = 128 if nbits == 8 else 0
    stride = (nsamps + 255) // 256 * 256
    rows = ops.unpack_transpose(packed, nsamps, nchans, nbits, bias, stride)
    del packed
    delays = _C.generate_delay_table(nchans, float(hdr["tsamp"]), float(hdr["fch1"]), float(hdr["foff"]))
    y, res = ops.scrunch(rows, nsamps, nbits, delays, params.dm, params.nsub, params.tscrunch, params.sigma_out, bias,
                         kill, float(hdr["foff"]))
    nout = int(res["nout"])
    data = ops.pack_transpose(y, nout, 8, 128).cpu().numpy()
    tmp = args.outfilename + ".tmp"
    with open(tmp, "wb") as f:
        f.write(header_bytes(scrunched_header(hdr, params.nsub, params.tscrunch, params.dm, nout), keep_present=True))
        f.write(data.tobytes())
    os.replace(tmp, args.outfilename)
    if args.killoutfilename:
        _C.write_killfile(args.killoutfilename, [int(k) for k in res["killmask"]])
    return res
