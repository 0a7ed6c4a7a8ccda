"""Dedispersion at its accumulator limits and in every kernel variant
(kernels and launchers in csrc/kernels/dedisperse.hip, dispatch in
Dedisperser::run / run_list of csrc/src/engine.cpp).

Oracle: int32 sums over NumPy slices in channel chunks (`_oracle`), the float32
scale and truncation of `ref.dedisperse`; a CPU test holds it equal to
`ref.dedisperse` itself.  It shares nothing with the kernels.  Every comparison
is `np.array_equal`: there is no tolerance in this file.

Inputs.  The fast kernels sum in sub-word lanes and spill on a fixed cadence
sized so that all-maximum input just fits (17 x 15 = 255 in a byte lane of
4-bit data, 16 x 12 = 192 in a byte lane of the 2-bit kernel, 3 x 21845 =
65535 in its 16-bit lanes, ...).  Uniform random samples never get near those
limits (`test_why_saturated_inputs`), so the lane cases use `saturated` (every
sample the maximum) and `near` (the maximum but for a seeded 3 % of entries,
which keeps the test sensitive to a shifted or swapped sample).

Variants.  Every run is made under the launch trace (`C.kernels.dedisp_trace`)
and asserts the set of kernel instantiations it launched, so a moved dispatch
threshold cannot silently take a case off the kernel it was written for.  The
expected tags come from `_expected`, a model of the dispatch written from the
host quantities `_measure` recomputes out of `g.offsets`; the cases that exist
for one variant also name it literally (`tag`, for the case's first kind).

Stores.  Outputs are pre-filled with 0xA5, with one guard row on each side.
Every kernel's store is guarded per byte: the vector store is taken only where
all of its samples lie below out_nsamps (`t + 4 <=`, `t + 8 <=`, `t + 16 <=`,
`t + 32 <= out_nsamps`), the tail loops stop at out_nsamps, and the direct
kernel tests each sample.  So the bytes [out_nsamps, stride) of every row and
both guard rows must be untouched, and that is what is asserted.

Geometry "L": tsamp 64 us, 400 MHz down over 200 MHz, 64 DMs base + step * k
(two 32-DM tiles), 3109 output samples (past the 1024- and 2048-sample tiles,
a tail that is no multiple of 16 or 32)."""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import sigproc, synthetic

dev = "cuda"
TSAMP, FCH1, BAND = 64e-6, 400.0, 200.0
OUT_NSAMPS = 3109
FILL = 0xA5

# DM lists (base, step) and the regime each is named for: the byte kernel taken ("one" / "two" LDS passes or the
# "global" valu kernel), whether the 2-bit kernel's window fits, whether the LDS-fed MFMA tile fits
LOW, MID, TWO, TWO_NO2, GLOBAL = (0.0, 0.002), (0.0, 0.02), (1.0, 0.1), (1.0, 0.15), (1.0, 0.3)
REGIME = {LOW: ("one", True, True), MID: ("one", True, False), TWO: ("two", True, False),
          TWO_NO2: ("two", False, False), GLOBAL: ("global", False, False)}

Case = collections.namedtuple("Case", "nbits nchans nactive dm ndm pattern kinds ranges tag")
Case.__new__.__defaults__ = (None,)


def _id(c):
    return f"{c.nbits}bit-{c.nactive}of{c.nchans}-dm{c.dm[0]:g}+{c.dm[1]:g}x{c.ndm}-{c.pattern}"


ALL_KINDS2 = ("Packed2", "Valu", "Mfma", "Direct")
FULL_AND_PARTS = ((0, 64), (5, 13), (8, 16))  # (8, 16): the dpw = 2 / dpt = 2 workgroups

# 1. lane limits of the 2-bit kernel (nibble 4 x 3, byte 16 x 12) and of the byte kernels on the same data (85 x 3,
#    255 x 1): active counts that are no multiple of 4, 8 or 64
LANE2 = [Case(2, nch, na, MID, 64, p, ALL_KINDS2, FULL_AND_PARTS)
         for na, nch in ((61, 64), (64, 64), (67, 96), (1021, 1024)) for p in ("saturated", "near")]
LANE2 += [Case(1, 64, 64, MID, 64, p, ALL_KINDS2, FULL_AND_PARTS) for p in ("saturated", "near")]
LANE2 += [Case(1, 1024, 1021, MID, 64, "saturated", ("Packed2", "Valu", "Direct"), ((0, 64),))]

# 2. the 2-bit kernel's channel limit: 3 x 21845 = 65535 fills its 16-bit lanes exactly.  Packed 2-bit samples need
#    a channel count that is a multiple of 4 (sigproc.pack_samples and the file format: whole bytes per sample), so
#    21845 channels cannot be a header's nchans: the limit is reached as 21845 active of 21848 channels.
LIMIT2 = [Case(2, 21848, 21845, LOW, 8, p, ("Packed2", "Direct"), ((0, 8),), "2bit<dpw=2>")
          for p in ("near", "saturated")]

# 3. byte lanes of the LDS kernel on 4-bit data: spilled every 17 channels (17 x 15 = 255)
BYTES4 = [Case(4, nch, na, dm, 64, p, ("Valu", "Mfma", "Auto", "Direct"), ((0, 64), (8, 16)))
          for na, nch in ((17, 64), (18, 64), (35, 64), (1024, 1024)) for dm in (MID, LOW)
          for p in ("saturated", "near")]

# 4. the 16-bit limit of the non-wide kernels (max raw value x active channels <= 65535)
LIMIT16 = [Case(nb, nch, na, MID, 40, p, ("Valu", "Direct"), ((0, 40),), tag)
           for nb, nch, na, tag in ((4, 4370, 4369, "lds<xor=0,passes=1,dpt=4,bytes=1>"),
                                    (4, 4370, 4370, "valu<dpt=4,wide=1,xor=0>"),
                                    (8, 258, 257, "lds<xor=1,passes=1,dpt=4,bytes=0>"),
                                    (8, 258, 258, "valu<dpt=4,wide=1,xor=1>"))
           for p in ("near", "saturated")]

# 5. the wide kernel's spill to 32 bits every 256 channels (256 x 255 = 65280): on the boundary, off it, odd
WIDE8 = [Case(8, 1024, na, MID, 64, p, ("Valu", "Mfma", "Direct"), ((0, 64), (5, 13)))
         for na in (1024, 769, 513) for p in ("saturated", "near")]

# 6. the two-pass LDS kernel, the fall-backs and the global kernels, on random data
TWOPASS = [
    Case(4, 64, 64, TWO, 64, "random", ("Valu", "Mfma", "Direct"), ((0, 64),), "lds<xor=0,passes=2,dpt=4,bytes=0>"),
    Case(8, 64, 64, TWO, 64, "random", ("Valu", "Mfma", "Direct"), ((0, 64),), "lds<xor=1,passes=2,dpt=4,bytes=0>"),
    # the 2-bit kernel with its window near the bound (364 of 384 dwords)
    Case(2, 64, 64, TWO, 64, "random", ("Packed2", "Valu", "Direct"), ((0, 64), (5, 37)), "2bit<dpw=4>"),
    # a Packed2 request whose window does not fit: the byte kernels take it
    Case(2, 64, 64, TWO_NO2, 64, "random", ("Packed2", "Auto", "Direct"), ((0, 64), (33, 64)),
         "lds<xor=0,passes=2,dpt=4,bytes=0>"),
    Case(4, 64, 64, GLOBAL, 64, "random", ("Valu", "Mfma", "Direct"), ((0, 64), (5, 37)), "valu<dpt=8,wide=0,xor=0>"),
    Case(8, 64, 61, GLOBAL, 64, "random", ("Valu", "Mfma", "Direct"), ((0, 64), (5, 37)), "valu<dpt=8,wide=0,xor=1>"),
]
# 1024 channels with 3 % killed against NumPy (the older 1024-channel tests compare with the direct kernel)
KILLED1024 = [Case(nb, 1024, 993, MID, 64, "random", kinds, ((0, 64), (5, 37), (33, 64)))
              for nb, kinds in ((2, ("Packed2", "Valu", "Mfma", "Auto", "Direct")),
                                (4, ("Valu", "Mfma", "Auto", "Direct")))]

# 7. run_list (always the global valu kernel) on the case-4 and case-6 geometries
LISTS = [(Case(8, 258, 258, MID, 40, "near", (), ()), "valu<dpt=4,wide=1,xor=1>"),
         (Case(4, 64, 64, TWO, 64, "random", (), ()), "valu<dpt=8,wide=0,xor=0>"),
         (Case(8, 64, 64, TWO, 64, "random", (), ()), "valu<dpt=8,wide=0,xor=1>")]

# 8. a compact set that launches every variant
COVER = [
    Case(2, 64, 61, LOW, 64, "near", ("Packed2", "Mfma", "Direct"), ((0, 64), (8, 16))),
    Case(4, 64, 35, MID, 64, "near", ("Valu", "Mfma"), ((0, 64), (8, 16))),
    Case(4, 64, 64, TWO, 64, "random", ("Valu",), ((0, 64),)),
    Case(4, 64, 64, GLOBAL, 64, "random", ("Valu",), ((0, 64),)),
    Case(4, 4370, 4370, MID, 40, "near", ("Valu",), ((0, 40),)),
    Case(8, 258, 257, MID, 40, "near", ("Valu",), ((0, 40), (8, 16))),
    Case(8, 258, 258, MID, 40, "near", ("Valu",), ((0, 40),)),
    Case(8, 64, 64, TWO, 64, "random", ("Valu",), ((0, 64),)),
    Case(8, 64, 61, GLOBAL, 64, "random", ("Valu",), ((0, 64),)),
]
# Every instantiation the launchers can start.  Not in the list, and unreachable from the dispatch:
# dedisperse_lds_kernel<false, 1, *, 1, false> (tags lds<xor=0,passes=1,dpt=2|4,bytes=0>).  XOR = false means bias 0,
# DedispGeometry::make gives bias 0 to every width but 8 bits, the widths are 1, 2, 4 and 8, and dedisperse_lds
# takes the byte-lane kernel for nbits <= 4 unless the window needs two passes.
ALL_TAGS = {
    "direct", "mfma", "mfma_lds", "pack2", "2bit<dpw=2>", "2bit<dpw=4>",
    "valu<dpt=4,wide=1,xor=0>", "valu<dpt=4,wide=1,xor=1>", "valu<dpt=8,wide=0,xor=0>", "valu<dpt=8,wide=0,xor=1>",
    "lds<xor=0,passes=1,dpt=4,bytes=1>", "lds<xor=0,passes=1,dpt=2,bytes=1>", "lds<xor=0,passes=2,dpt=4,bytes=0>",
    "lds<xor=1,passes=1,dpt=4,bytes=0>", "lds<xor=1,passes=1,dpt=2,bytes=0>", "lds<xor=1,passes=2,dpt=4,bytes=0>",
}

EVERY_CASE = LANE2 + LIMIT2 + BYTES4 + LIMIT16 + WIDE8 + TWOPASS + KILLED1024 + [c for c, _ in LISTS] + COVER


# ------------------------------------------------------------------ inputs --
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _killmask(nchans, nactive):
    kill = np.ones(nchans, dtype=np.int64)
    if nactive < nchans:
        rng = np.random.default_rng(_seed("kill", nchans, nactive))
        kill[rng.choice(nchans, nchans - nactive, replace=False)] = 0
    return kill


@functools.lru_cache(maxsize=None)
def _geometry(c):
    foff = -BAND / c.nchans
    dms = [c.dm[0] + c.dm[1] * k for k in range(c.ndm)]
    delays = C.generate_delay_table(c.nchans, TSAMP, FCH1, foff)
    nsamps = OUT_NSAMPS + C.compute_max_delay(dms, delays)
    hdr = synthetic.make_header(nchans=c.nchans, nbits=c.nbits, tsamp=TSAMP, fch1=FCH1, foff=foff, nsamples=nsamps)
    g = C.DedispGeometry.make(hdr, nsamps, dms, [int(k) for k in _killmask(c.nchans, c.nactive)])
    assert g.out_nsamps == OUT_NSAMPS and g.nactive == c.nactive
    return g


def _values(pattern, nsamps, nchans, nbits, seed):
    top = (1 << nbits) - 1
    rng = np.random.default_rng(seed)
    if pattern == "random":
        return rng.integers(0, top + 1, size=(nsamps, nchans), dtype=np.uint8)
    v = np.full((nsamps, nchans), top, dtype=np.uint8)
    if pattern == "near":
        idx = rng.integers(0, v.size, int(0.03 * v.size))
        v.reshape(-1)[idx] = rng.integers(0, top + 1, idx.size, dtype=np.uint8)
    else:
        assert pattern == "saturated"
    return v


def _oracle(vals, offs, nbits, kill, out_nsamps, chunk=512):
    """ref.dedisperse with int32 sums over chunks of channels (no int64 copy of the input: the 21848-channel case
    stays below 1 GB): vals [nsamps, nchans] raw, offs [ndm, nchans] -> uint8 [ndm, out_nsamps]."""
    nchans = vals.shape[1]
    assert ((1 << nbits) - 1) * nchans < 2 ** 31
    active = np.nonzero(np.asarray(kill))[0]
    sums = np.zeros((offs.shape[0], out_nsamps), dtype=np.int32)
    for c0 in range(0, len(active), chunk):
        chans = active[c0:c0 + chunk]
        x = np.ascontiguousarray(vals[:, chans].T)
        for d in range(offs.shape[0]):
            s = sums[d]
            for i, ch in enumerate(chans):
                o = int(offs[d, ch])
                s += x[i, o:o + out_nsamps]
    scale = np.float32(192.0 / (((1 << nbits) - 1) * nchans))
    return np.clip(sums.astype(np.float32) * scale, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=12)
def _data(c):
    """(geometry, raw values, expected rows) of a case's input; computed once per case, never modified."""
    c = c._replace(kinds=(), ranges=(), tag=None)
    g = _geometry(c)
    vals = _values(c.pattern, g.nsamps, c.nchans, c.nbits, _seed("vals", _id(c)))
    offs = np.array(g.offsets(0, c.ndm), dtype=np.int32).reshape(c.ndm, c.nchans)
    exp = _oracle(vals, offs, c.nbits, g.killmask, OUT_NSAMPS)
    vals.setflags(write=False)
    exp.setflags(write=False)
    return g, vals, exp


def _key(c):
    return c._replace(kinds=(), ranges=(), tag=None)


# ---------------------------------------------------- the dispatch, modelled --
Measure = collections.namedtuple("Measure", "window window2 mfma_lds_fits")


def _measure(g, d0, d1):
    """The host quantities the dispatch decides on, for the 32-DM tiles of [d0, d1), from g.offsets: the largest
    byte window, the 2-bit kernel's window (dwords) and whether every tile fits the LDS-fed MFMA kernel."""
    ndm, nch = len(g.dm_list), g.nchans
    offs = np.array(g.offsets(0, ndm), dtype=np.int64).reshape(ndm, nch)[:, np.asarray(g.killmask) != 0]
    window, fits = 0, True
    for T in range(d0 // 32, (d1 - 1) // 32 + 1):
        tile = offs[32 * T:32 * T + 32]  # (a short last tile is padded with its last DM: the same extremes)
        lo, hi = tile.min(axis=0), tile.max(axis=0)
        reach = int((hi - (lo & ~15)).max())
        window = max(window, 1024 + reach + 32)
        fits = fits and reach + 1044 <= 1280
    spread = window - 1056
    return Measure(window, ((2048 + spread + 48 + 63) // 64 + 1) * 4, fits)


def _regime(m):
    return ("one" if m.window <= 4096 else "two" if m.window <= 8192 else "global", m.window2 <= 384,
            m.mfma_lds_fits)


def _expected(kind, g, d0, d1, dd=None):
    """The set of tags Dedisperser::run(d0, d1, kind) must launch.  Auto asks the dedisperser for its split and
    choice (both weigh measured step counts) and then has to launch what they say."""
    m = _measure(g, d0, d1)
    top, na, n = (1 << g.nbits) - 1, g.nactive, d1 - d0
    p2 = g.nbits <= 2 and na <= 21845 and m.window2 <= 384
    if kind == "Auto":
        split = dd.mfma_lds_split(d0, d1)
        if split > d0:
            rest = _expected("Auto2", g, split, d1) if split < d1 else set()
            return {"mfma_lds"} | rest
        if not p2 and dd.choose(d0, d1) == C.DedispKernel.Mfma:
            return {"mfma"}
        kind = "Auto2"
    if kind == "Auto2":
        kind = "Packed2" if p2 else "Valu"
    if kind == "Direct":
        return {"direct"}
    if kind == "Mfma":
        return {"mfma_lds"} if m.mfma_lds_fits else {"mfma"}
    if kind == "Packed2" and p2:
        return {"2bit<dpw=%d>" % (2 if n <= 8 and d0 % 8 + n <= 8 else 4)}
    assert kind in ("Valu", "Packed2")
    xor = int(g.nbits == 8)
    if top * na <= 65535 and m.window <= 8192:
        two = m.window > 4096
        dpt = 2 if n <= 8 and not two else 4
        return {"lds<xor=%d,passes=%d,dpt=%d,bytes=%d>" % (xor, 2 if two else 1, dpt, int(g.nbits <= 4 and not two))}
    wide = top * na > 65535
    return {"valu<dpt=%d,wide=%d,xor=%d>" % (4 if wide else 8, int(wide), xor)}


# --------------------------------------------------------------- CPU tests --
def test_conditions_hold_for_every_case():
    """Each case lies in the regime its DM list is named for, in every range it runs; the limit cases sit on their
    limits; the compact coverage set's model covers every variant but the staging kernel."""
    for c in EVERY_CASE:
        g = _geometry(_key(c))
        top = (1 << c.nbits) - 1
        for d0, d1 in tuple(c.ranges) + ((0, c.ndm),):
            m = _measure(g, d0, d1)
            assert _regime(m) == REGIME[c.dm], (_id(c), d0, d1, m)
        if c.tag:
            assert all(_expected(c.kinds[0], g, d0, d1) == {c.tag} for d0, d1 in c.ranges), _id(c)
        if c in LIMIT2:
            assert top * c.nactive == 65535 and c.nchans % 4 == 0 and c.nchans - c.nactive < 4
        if c in LIMIT16:
            assert top * c.nactive in (65535, 65535 + top)
    # the windows of the issue's table, 64 and 1024 channels
    for dm, w64, w1024 in ((LOW, (1139, 144), (1145, 144)), (MID, (1790, 184), (1816, 184)),
                           (TWO, (4686, 364), (4828, 372)), (TWO_NO2, (6494, 476), (6708, 492)),
                           (GLOBAL, (11917, 816), (12346, 844))):
        for nch, w in ((64, w64), (1024, w1024)):
            g = _geometry(Case(4, nch, nch, dm, 64, "random", (), ()))
            assert _measure(g, 0, 64)[:2] == w, (dm, nch)
    want = set()
    for c in COVER:
        g = _geometry(c)
        for k in c.kinds:
            for d0, d1 in c.ranges:
                want |= _expected(k, g, d0, d1)
    assert want | {"pack2"} == ALL_TAGS, sorted(ALL_TAGS - want)


def _lane_pair_sums(x, lane_bits, flush):
    """Model of one packed accumulator word with the kernels' spill cadence: two adjacent lanes of lane_bits each
    take the samples 2k and 2k + 1 of x [nsamps, nchans] channel by channel and are spilled to wide sums (masked
    apart, then cleared) every `flush` channels.  A lane that overflows loses the carry and corrupts its
    neighbour, as in the kernels."""
    mask = (1 << lane_bits) - 1
    x = x.astype(np.int64)
    lo, hi = x[0::2], x[1::2]
    out = np.zeros((2,) + lo.shape[:1], dtype=np.int64)
    for c0 in range(0, x.shape[1], flush):
        word = lo[:, c0:c0 + flush].sum(axis=1) + (hi[:, c0:c0 + flush].sum(axis=1) << lane_bits)
        out[0] += word & mask
        out[1] += (word >> lane_bits) & mask
    return out, np.stack([lo.sum(axis=1), hi.sum(axis=1)])


def test_why_saturated_inputs():
    """A spill cadence one channel too long is invisible on the uniform random input of the older tests (their
    seed, 7) and visible on the saturated and near-saturated inputs of this file.  Byte lanes of 4-bit data are
    spilled every 17 channels (17 x 15 = 255); the 2-bit kernel's byte lanes take 64 channels (16 nibble spills of
    at most 12) and would hold 85 (85 x 3 = 255).  Its nibble lanes (4 x 3 = 12) have one channel of slack, 5 x 3 =
    15: the first cadence they overflow at is 6, and that one uniform random data does notice."""
    nsamps, nchans = 5000, 1024
    for nbits, lane_bits, good, bad, random_sees_it in ((4, 8, 17, 18, False), (2, 8, 85, 86, False),
                                                        (2, 4, 5, 6, True), (1, 8, 255, 256, False)):
        inputs = {"random": np.random.default_rng(7).integers(0, 1 << nbits, size=(nsamps, nchans), dtype=np.uint8),
                  "saturated": _values("saturated", nsamps, nchans, nbits, 0),
                  "near": _values("near", nsamps, nchans, nbits, _seed("why", nbits))}
        for name, x in inputs.items():
            got, true = _lane_pair_sums(x, lane_bits, good)
            assert np.array_equal(got, true), (nbits, lane_bits, name)
            got, true = _lane_pair_sums(x, lane_bits, bad)
            wrong = not np.array_equal(got, true)
            assert wrong == (name != "random" or random_sees_it), (nbits, lane_bits, name)


@pytest.mark.parametrize("nbits", [2, 8])
def test_oracle_equals_reference(nbits):
    rng = np.random.default_rng(nbits)
    c = Case(nbits, 64, 51, MID, 9, "near", (), ())
    g = _geometry(c)
    for pattern in ("near", "random"):
        vals = _values(pattern, g.nsamps, 64, nbits, int(rng.integers(1 << 30)))
        offs = np.array(g.offsets(0, 9), dtype=np.int32).reshape(9, 64)
        exp = ref.dedisperse(vals, offs, nbits, g.killmask, OUT_NSAMPS)
        assert exp.min() < exp.max()
        for chunk in (7, 512):  # several chunks with a ragged last one, and one chunk
            assert np.array_equal(_oracle(vals, offs, nbits, g.killmask, OUT_NSAMPS, chunk), exp)


# --------------------------------------------------------------- GPU tests --
class _Loaded:
    """A case's filterbank on the device and its dedisperser."""

    def __init__(self, c, trace_load=False):
        self.g, vals, self.exp = _data(_key(c))
        self.stream = torch.cuda.current_stream().cuda_stream
        self.stride = C.Dedisperser.row_stride(OUT_NSAMPS)
        assert self.stride > OUT_NSAMPS  # there are pad bytes to watch
        packed = torch.from_numpy(sigproc.pack_samples(vals, c.nbits)).to(dev)
        self.load_tags = _traced(lambda: self._load(packed)) if trace_load else self._load(packed)
        self.dd = C.Dedisperser(self.dfb, self.stream)

    def _load(self, packed):
        self.dfb = C.DeviceFilterbank(self.g, self.stream)
        self.dfb.load_packed_device(packed.data_ptr())
        torch.cuda.synchronize()

    def rows(self, launch, n):
        """Run launch(out pointer, stride) into n rows of a 0xA5-filled buffer with a guard row on each side, under
        the trace: (rows [n, out_nsamps], tags); nothing outside the rows' samples may have been written."""
        o = torch.full(((n + 2) * self.stride,), FILL, dtype=torch.uint8, device=dev)
        tags = _traced(lambda: (launch(o.data_ptr() + self.stride, self.stride), torch.cuda.synchronize()))
        got = o.view(n + 2, self.stride).cpu().numpy()
        assert (got[0] == FILL).all() and (got[n + 1] == FILL).all(), "a guard row was written"
        assert (got[1:n + 1, OUT_NSAMPS:] == FILL).all(), "bytes past out_nsamps were written"
        return got[1:n + 1, :OUT_NSAMPS], tags


def _traced(fn):
    C.kernels.dedisp_trace_take()
    C.kernels.dedisp_trace(True)
    try:
        fn()
    finally:
        C.kernels.dedisp_trace(False)
    return C.kernels.dedisp_trace_take()


def _check(c, trace_load=False):
    ld = _Loaded(c, trace_load)
    seen = set(ld.load_tags or ())
    for d0, d1 in c.ranges:
        for kind in c.kinds:
            got, tags = ld.rows(lambda p, st: ld.dd.run(d0, d1, p, st, getattr(C.DedispKernel, kind)), d1 - d0)
            assert set(tags) == _expected(kind, ld.g, d0, d1, ld.dd), (kind, d0, d1, tags)
            if c.tag and kind == c.kinds[0]:  # the variant the case exists for, named literally
                assert set(tags) == {c.tag}, (kind, d0, d1, tags)
            assert np.array_equal(got, ld.exp[d0:d1]), (kind, d0, d1)
            seen |= set(tags)
    return seen


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c", LANE2, ids=_id)
def test_lane_limits_2bit(c):
    seen = _check(c)
    assert "2bit<dpw=4>" in seen and ("2bit<dpw=2>" in seen or (8, 16) not in c.ranges)


@gpu
@pytest.mark.parametrize("c", LIMIT2, ids=_id)
def test_channel_limit_2bit(c):
    _check(c)


@gpu
@pytest.mark.parametrize("c", BYTES4, ids=_id)
def test_byte_lanes_4bit(c):
    seen = _check(c)
    assert {"lds<xor=0,passes=1,dpt=4,bytes=1>", "lds<xor=0,passes=1,dpt=2,bytes=1>"} <= seen


@gpu
@pytest.mark.parametrize("c", LIMIT16, ids=_id)
def test_16bit_limit_of_the_narrow_kernels(c):
    _check(c)


@gpu
@pytest.mark.parametrize("c", WIDE8, ids=_id)
def test_wide_flush_8bit(c):
    seen = _check(c)
    assert "valu<dpt=4,wide=1,xor=1>" in seen and "mfma" in seen


@gpu
@pytest.mark.parametrize("c", TWOPASS, ids=_id)
def test_two_pass_lds_and_fallbacks(c):
    _check(c)


@gpu
@pytest.mark.parametrize("c", KILLED1024, ids=_id)
def test_1024_channels_killed_against_numpy(c):
    _check(c)


@gpu
@pytest.mark.parametrize("c,tag", LISTS, ids=[_id(c) for c, _ in LISTS])
def test_run_list(c, tag):
    ld = _Loaded(c)
    rng = np.random.default_rng(_seed("list", _id(c)))
    lst = [int(v) for v in rng.permutation(c.ndm)[:35]] + [7, 7, 0]  # unsorted, repeats, more than one 32-DM tile
    got, tags = ld.rows(lambda p, st: ld.dd.run_list(lst, p, st), len(lst))
    assert tags == [tag]
    assert np.array_equal(got, ld.exp[lst])


@gpu
def test_every_variant_is_launched():
    seen = set()
    for c in COVER:
        seen |= _check(c, trace_load=True)
    assert seen == ALL_TAGS, (sorted(ALL_TAGS - seen), sorted(seen - ALL_TAGS))
