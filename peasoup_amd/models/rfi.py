"""RFI excision behind ``python -m peasoup_amd clean``: a block-statistics
mask and a zero-DM filter on the device filterbank (csrc/kernels/rfi.hip,
``RfiCleaner``); writes the cleaned ``.fil`` (header bytes verbatim), the mask
file and a killfile, byte for byte as ``bin/rficlean``.

The packed bytes are uploaded with torch, cleaned in place by the native
cleaner (unpack, block sums, host flags, apply, pack) and written from Python
(``utils.outputs.write_rfi_mask``).  Under ``torch.distributed.run`` rank 0
does the work and the other ranks return.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _C
from ..utils.outputs import write_rfi_mask


def mask_dict(mask) -> dict:
    """A ``_C.RfiMask`` as the dict of arrays ``write_rfi_mask`` takes."""
    return {"chan_flag": mask.chan_flag, "block_flag": mask.block_flag, "cell": mask.cell, "fill": mask.fill,
            "G": mask.G, "nb": mask.nb, "killmask": list(mask.killmask)}


def clean_packed(packed: torch.Tensor, nchans: int, nsamps: int, nbits: int, params, killmask=None):
    """Cleans packed SIGPROC bytes on the device in place; returns the ``_C.RfiMask``."""
    if not packed.is_cuda or packed.dtype != torch.uint8 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous uint8 HIP tensor")
    kill = [] if killmask is None else [int(k) for k in killmask]
    cleaner = _C.RfiCleaner(params, torch.cuda.current_stream().cuda_stream)
    return cleaner.clean_packed(packed.data_ptr(), int(nchans), int(nsamps), int(nbits), kill)


def clean_filterbank(args):
    """Cleans the filterbank ``args`` (an ``RfiCmdLineOptions``) names and
    writes the outputs it names; returns the ``_C.RfiMask`` on rank 0 (None
    elsewhere)."""
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    params = _C.rfi_params_from(args)
    fb = _C.Filterbank.from_file(args.infilename)
    nchans, nbits, nsamps = int(fb.nchans), int(fb.nbits), int(fb.nsamps)
    kill = None
    if args.killfilename:
        kill, _ = _C.read_killfile(args.killfilename, nchans)
    nbytes = nsamps * nchans * nbits // 8
    packed = torch.from_numpy(np.array(fb.data()[:nbytes], copy=True)).cuda()
    mask = clean_packed(packed, nchans, nsamps, nbits, params, kill)
    if args.outfilename:
        with open(args.infilename, "rb") as f:
            head = f.read(int(fb.header["size"]))
        tmp = args.outfilename + ".tmp"
        with open(tmp, "wb") as f:
            f.write(head)
            f.write(packed.cpu().numpy().tobytes())
        os.replace(tmp, args.outfilename)
    if args.maskfilename:
        write_rfi_mask(args.maskfilename,
                       {"nbits": nbits, "zero_dm": params.zero_dm, "nsamps": nsamps, "block": params.block,
                        "tsamp": float(fb.tsamp), "thresh": params.thresh, "chan_frac": params.chan_frac,
                        "block_frac": params.block_frac}, mask_dict(mask))
    if args.killoutfilename:
        _C.write_killfile(args.killoutfilename, list(mask.killmask))
    return mask
