"""Distributed single-pulse search: one process per GPU (torchrun), the same
distribution model as the FFA search (models/ffa.py):

1. rank 0 reads the ``.fil``; the packed bytes are RCCL-broadcast and every
   rank keeps a channel-major filterbank resident in HBM;
2. each rank dedisperses a contiguous DM shard in chunks and runs the native
   ``SinglePulseEngine`` on every chunk (block means, sigma, fused boxcar
   search; csrc/kernels/singlepulse.hip);
3. the events are gathered to rank 0, which clusters them across DMs
   (``sp_cluster``) and writes the text output.

An extension beyond the reference, which searches periodicities only.
"""
from __future__ import annotations

import struct
import time
from typing import List, Optional

import torch

from .. import _C, dedisp_kernel
from ..parallel import dist as pdist
from ..utils.timing import Stopwatch
from .search import load_packed_for_rank

_REC = struct.Struct("<Iifi")  # sample, width_log2, snr, dm_idx (the device record)


def encode_events(events) -> bytes:
    return struct.pack("<i", len(events)) + b"".join(
        _REC.pack(e.sample, e.width_log2, e.snr, e.dm_idx) for e in events)


def decode_events(b: bytes) -> list:
    (n,) = struct.unpack_from("<i", b, 0)
    return [_C.SpEvent(*_REC.unpack_from(b, 4 + i * _REC.size)) for i in range(n)]


class RankSinglePulse:
    """Per-rank state: resident filterbank, dedisperser, single-pulse engine."""

    def __init__(self, args, header: dict, packed: Optional[torch.Tensor], nsamps: int):
        self.ctx = pdist.context()
        self.args = args
        self.header = dict(header)
        self.dm_list = list(_C.generate_dm_list(args.dm_start, args.dm_end, header["tsamp"], args.dm_pulse_width,
                                                header["fch1"], header["foff"], header["nchans"], args.dm_tol))
        kill = [1] * int(header["nchans"])
        if args.killfilename:
            kill = list(_C.read_killfile(args.killfilename, int(header["nchans"]))[0])
        self.stream = torch.cuda.current_stream().cuda_stream
        # --rfi: every rank cleans its own copy of the packed bytes in place
        # (the stage is deterministic, so the copies stay identical); the
        # flagged channels join the killmask before the geometry is made
        self.rfi_mask = None
        self.rfi_params = None
        if args.rfi or args.zero_dm:
            if packed is None or not packed.is_cuda:
                raise ValueError("--rfi needs the packed filterbank on a HIP device")
            self.rfi_params = _C.sp_rfi_params(args)
            cleaner = _C.RfiCleaner(self.rfi_params, self.stream)
            self.rfi_mask = cleaner.clean_packed(packed.data_ptr(), int(header["nchans"]), int(nsamps),
                                                 int(header["nbits"]), kill)
            kill = [int(bool(a) and bool(b)) for a, b in zip(kill, self.rfi_mask.killmask)]
        self.geom = _C.DedispGeometry.make(self.header, int(nsamps), self.dm_list, kill)
        self.dfb = _C.DeviceFilterbank(self.geom, self.stream)
        if packed is not None:
            if packed.is_cuda:
                self.dfb.load_packed_device(packed.data_ptr())
            else:
                self.dfb.load_packed_host(packed.data_ptr())
        self.dedisperser = _C.Dedisperser(self.dfb, self.stream)
        self.kernel = dedisp_kernel(args.dedisp_kernel)
        self.params = _C.sp_params_from(args, float(header["tsamp"]))
        self.engine = _C.SinglePulseEngine(self.params, int(self.geom.out_nsamps), self.stream)
        self.row_stride = _C.Dedisperser.row_stride(self.geom.out_nsamps)
        self._trials: Optional[torch.Tensor] = None

    @property
    def band_delay_per_dm(self) -> float:
        """Dispersion delay across the band per unit DM (s): the delay
        table's last entry (samples) times tsamp, as run_sp_pipeline."""
        delays = self.geom.delays
        return float(delays[-1]) * float(self.header["tsamp"]) if len(delays) else 0.0

    def search(self, dm_indices, chunk: int = 32) -> list:
        from .search import RankSearcher

        out: list = []
        # chunks cut at multiples of the dedispersion tile (resident plans)
        for d0, d1 in RankSearcher.chunk_ranges(dm_indices, chunk):
            need = (d1 - d0) * self.row_stride
            if self._trials is None or self._trials.numel() < need:
                self._trials = torch.empty(need, dtype=torch.uint8, device=self.ctx.device)
            self.dedisperser.run(d0, d1, self._trials.data_ptr(), self.row_stride, self.kernel)
            out.extend(self.engine.search_block(self._trials.data_ptr(), self.row_stride, d1 - d0, d0))
        return out


def run_single_pulse_search(args, write: bool = True):
    """Distributed single-pulse search; returns the SpResult on rank 0 (None elsewhere)."""
    ctx = pdist.init()
    timers = {k: Stopwatch() for k in ("reading", "searching", "total")}
    timers["total"].start()
    timers["reading"].start()
    header, packed, nsamps = load_packed_for_rank(args.infilename, ctx)
    timers["reading"].stop()
    rs = RankSinglePulse(args, header, packed, nsamps)
    del packed
    shard = pdist.shard_range(len(rs.dm_list), ctx.world_size, ctx.rank)
    pdist.barrier()
    timers["searching"].start()
    t0 = time.perf_counter()
    local = rs.search(shard)
    torch.cuda.synchronize()
    wall = pdist.all_reduce_max_float(time.perf_counter() - t0)
    timers["searching"].stop()
    blobs = pdist.gather_bytes(encode_events(local), dst=0)
    if not ctx.is_root:
        return None
    events: List = []
    for b in blobs:
        events.extend(decode_events(b))
    events.sort(key=lambda e: (e.dm_idx, e.width_log2, e.sample))
    cands = _C.sp_cluster(events, rs.dm_list, rs.band_delay_per_dm, float(header["tsamp"]))
    if args.limit >= 0:
        cands = cands[: args.limit]
    timers["total"].stop()
    res = _C.SpResult()
    res.candidates = cands
    res.dm_list = rs.dm_list
    res.devices = list(range(ctx.world_size))
    res.timers = {k: v.get_time() for k, v in timers.items()} | {"searching_wall": wall}
    res.nsamps = int(rs.geom.out_nsamps)
    res.tsamp = float(header["tsamp"])
    res.widths = list(rs.engine.widths)
    res.baseline = int(rs.engine.baseline)
    res.events = len(events)
    if rs.rfi_mask is not None:
        res.rfi_comment = _C.rfi_summary_comment(rs.rfi_mask, rs.rfi_params)
        if args.rfi_maskfilename:
            from .rfi import mask_dict
            from ..utils.outputs import write_rfi_mask

            p = rs.rfi_params
            write_rfi_mask(args.rfi_maskfilename,
                           {"nbits": int(header["nbits"]), "zero_dm": p.zero_dm, "nsamps": int(nsamps),
                            "block": p.block, "tsamp": float(header["tsamp"]), "thresh": p.thresh,
                            "chan_frac": p.chan_frac, "block_frac": p.block_frac}, mask_dict(rs.rfi_mask))
    if write:
        _C.write_sp_output(args.outfilename, args, res)
    return res
