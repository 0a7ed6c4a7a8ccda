"""Burst cutouts (csrc/include/psoup/burstcube.hpp; an extension beyond the
reference): the dedispersed waterfall and the DM-time plane per single-pulse
candidate.

CPU: option parsing, both candidate readers, identities of the NumPy oracle, the
cutout file (header and first candidate pinned by explicit offsets, Python and
native writers byte-identical), the panels.  GPU: the kernel's int32 planes must
EQUAL the oracle's (torch.equal) over a sweep of shapes, batching, determinism,
errors, recovery of an injected burst beside a zero-DM impulse, and the entry
points (bin/burstcube, python -m peasoup_amd burst)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.outputs import BurstCubeFile, burst_mean, write_burst_file
from peasoup_amd.utils.plotting import burst_dmtime_panel, burst_profile_panel, burst_waterfall_panel

W = C.burst_window()
TSAMP = 64e-6
GOLDEN_SP = os.path.join(REPO, "tests", "golden", "spsearch_flags_off.output")


# ------------------------------------------------------------------- CPU ----
def test_burst_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_burst_cmdline(["burstcube", "-i", "x.fil", "--spfile", "sp.txt"])
    assert ok and not exit_now and a.infilename == "x.fil" and a.spfilename == "sp.txt" and a.candfilename == ""
    assert (a.ntime, a.nsub, a.ndm, a.tscrunch, a.dm_half_range, a.limit) == (256, 256, 256, 0, 0.0, 100)
    assert not a.verbose and a.killfilename == ""
    assert a.outfilename.endswith("_burstcube.bursts")
    assert len(a.outfilename) == len("2026-01-01-00:00_burstcube.bursts")
    ok, _, a = C.parse_burst_cmdline(["burstcube", "-i", "y.fil", "-o", "out.bursts", "--candfile", "c.txt", "-k",
                                      "kill.txt", "--ntime", "64", "--nsub", "5", "--ndm", "33", "--tscrunch", "12",
                                      "--dm_half_range", "7.5", "--limit", "3", "-v"])
    assert ok and a.outfilename == "out.bursts" and a.candfilename == "c.txt" and a.spfilename == ""
    assert a.killfilename == "kill.txt" and (a.ntime, a.nsub, a.ndm, a.tscrunch) == (64, 5, 33, 12)
    assert a.dm_half_range == 7.5 and a.limit == 3 and a.verbose
    ok, exit_now, _ = C.parse_burst_cmdline(["burstcube", "-h"])
    assert ok and exit_now


@pytest.mark.parametrize("extra", [
    [],                                            # neither --spfile nor --candfile
    ["--spfile", "s.txt", "--candfile", "c.txt"],  # both
    ["--spfile", "s.txt", "--ntime", "0"], ["--spfile", "s.txt", "--ntime", "1025"],
    ["--spfile", "s.txt", "--ndm", "0"], ["--spfile", "s.txt", "--ndm", "1025"],
    ["--spfile", "s.txt", "--nsub", "0"],
    ["--spfile", "s.txt", "--tscrunch", "-1"], ["--spfile", "s.txt", "--tscrunch", "4097"],
])
def test_burst_cmdline_errors(extra):
    assert not C.parse_burst_cmdline(["burstcube", "-i", "x.fil"] + extra)[0]
    assert not C.parse_burst_cmdline(["burstcube", "--spfile", "s.txt"])[0]  # -i is required


def test_candidate_readers(tmp_path):
    f = tmp_path / "cands.txt"
    f.write_text("# sample width dm snr\n1000 16 30.5 12.25\n\n   # indented comment\n7\t1\t0 extra columns 7\n"
                 "123456789012 4096 2.5\n")
    c = C.read_burst_candfile(str(f))
    assert [(x.sample, x.width, x.dm, x.snr) for x in c] == [(1000, 16, 30.5, 12.25), (7, 1, 0.0, 0.0),
                                                             (123456789012, 4096, 2.5, 0.0)]
    assert len(C.read_burst_candfile(str(f), 2)) == 2
    f.write_text("1000 16 30.5\n# c\n2000 abc 1\n")
    with pytest.raises(C.NativeError, match="line 3"):
        C.read_burst_candfile(str(f))
    f.write_text("1000 16\n")
    with pytest.raises(C.NativeError, match="line 1"):
        C.read_burst_candfile(str(f))
    # a real spsearch output: S/N, sample, width and DM as printed
    sp = C.read_sp_output(GOLDEN_SP)
    lines = [ln.split() for ln in open(GOLDEN_SP) if not ln.startswith("#")]
    assert len(sp) == len(lines) > 10
    for x, ln in zip(sp, lines):
        assert (x.sample, x.width) == (int(ln[1]), int(ln[3]))
        assert x.dm == np.float32(ln[5]) and x.snr == np.float32(ln[0])
    assert (sp[0].sample, sp[0].width, sp[0].dm) == (69120, 32, np.float32(49.7063))
    assert len(C.read_sp_output(GOLDEN_SP, 5)) == 5
    f.write_text("# header\n    9.229        69120     22.123520000      32      15\n")
    with pytest.raises(C.NativeError, match="line 2"):
        C.read_sp_output(str(f))


def _header(nchans, nbits, tsamp=TSAMP):
    return synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=tsamp)


def _delays(hdr):
    return ref.delay_table(hdr["nchans"], hdr["tsamp"], hdr["fch1"], hdr["foff"])


def _kill(nchans, idx):
    k = np.ones(nchans, int)
    k[list(idx)] = 0
    return k


def test_burst_dms_and_definition_helpers():
    for dm, ndm, half in ((100.0, 256, 0.0), (33.3, 7, 0.0), (49.7063, 33, 5.0), (2.0, 4, 50.0), (0.0, 5, 0.0),
                          (1234.5, 1, 0.0)):
        d = ref.burst_dms(dm, ndm, half)
        assert d.dtype == np.float32 and d.shape == (ndm,)
        assert d[ndm // 2] == np.float32(dm) and np.all(d >= 0) and np.all(np.diff(d) >= 0)
        assert np.array_equal(d, C.burst_dms(dm, ndm, half))
    assert ref.burst_dms(100.0, 4)[0] == 0.0 and ref.burst_dms(100.0, 4)[3] == 150.0
    assert ref.burst_dms(100.0, 4, 10.0)[0] == 90.0
    for width, ts in ((1, 0), (2, 0), (3, 0), (4, 0), (96, 0), (4096, 0), (5, 7)):
        assert ref.burst_tscrunch(width, ts) == C.burst_tscrunch(width, ts) == (ts or max(1, width // 2))
    assert ref.burst_t0(10, 4, 2, 64) == C.burst_t0(10, 4, 2, 64) == 12 - 64
    assert ref.burst_t0(5000, 33, 16, 37) == C.burst_t0(5000, 33, 16, 37) == 5016 - 18 * 16


def test_oracle_identities():
    nchans, nsub, ndm, ntime = 24, 5, 7, 16
    hdr = _header(nchans, 8)
    delays = _delays(hdr)
    kill = _kill(nchans, [3, 10, 11])
    n = 6000
    # constant filterbank: sums == v * hits, at the edges too
    const = np.full((n, nchans), 7, dtype=np.uint8)
    for sample in (3000, 5, n - 3):
        c = ref.burst_cube(const, sample, 12, 150.0, delays, ntime, nsub, ndm, killmask=kill)
        assert all(c[k].dtype == np.int32 for k in ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits", "nactive"))
        assert np.array_equal(c["ds_sums"], 7 * c["ds_hits"]) and np.array_equal(c["dmt_sums"], 7 * c["dmt_hits"])
        assert c["tscrunch"] == 6 and c["t0"] == sample + 6 - 8 * 6
    assert (c["ds_hits"] == 0).any() and (c["ds_hits"] > 0).any()  # the last: a window past the end
    vals = synthetic.generate(n, hdr, (), seed=3)
    c = ref.burst_cube(vals, 3000, 12, 150.0, delays, ntime, nsub, ndm, killmask=kill)
    # the DM row of the candidate is the waterfall summed over the band
    assert np.array_equal(c["dmt_sums"][ndm // 2], c["ds_sums"].sum(axis=0))
    assert np.array_equal(c["dmt_hits"][ndm // 2], c["ds_hits"].sum(axis=0))
    # an interior candidate: every bin is full
    assert np.array_equal(c["ds_hits"], np.broadcast_to(6 * c["nactive"][:, None], (nsub, ntime)))
    assert list(c["nactive"]) == [np.sum(kill[[ch for ch in range(nchans) if ch * nsub // nchans == s]])
                                  for s in range(nsub)]
    # written from the definition: one bin of one subband and of one DM row by hand
    off = ref.dm_offsets(c["dms"], delays)
    k, j, s = 5, 2, 1
    live = [ch for ch in range(nchans) if kill[ch]]
    exp = sum(int(vals[c["t0"] + k * 6 + i + off[j][ch], ch]) for ch in live for i in range(6))
    assert c["dmt_sums"][j, k] == exp
    off_dm = ref.dm_offsets([150.0], delays)[0]
    exp = sum(int(vals[c["t0"] + k * 6 + i + off_dm[ch], ch]) for ch in live if ch * nsub // nchans == s
              for i in range(6))
    assert c["ds_sums"][s, k] == exp
    # nvalid: samples from nvalid on are not read
    short = ref.burst_cube(vals, 3000, 12, 150.0, delays, ntime, nsub, ndm, killmask=kill, nvalid=3010)
    full = ref.burst_cube(vals[:3010], 3000, 12, 150.0, delays, ntime, nsub, ndm, killmask=kill)
    assert all(np.array_equal(short[k], full[k]) for k in ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits"))


def _hand_cutout(ntime=6, nsub=5, ndm=3, seed=0):
    rng = np.random.default_rng(seed)
    c = {"sample": (1 << 33) + 7, "width": 16, "tscrunch": 8, "t0": -41, "dm": 12.25, "snr": 9.5,
         "dms": np.array([0.0, 12.25, 20.5], dtype=np.float32)[:ndm],
         "nactive": np.array([3, 2, 0, 3, 2], dtype=np.int32)[:nsub]}
    for k, rows in (("ds_sums", nsub), ("ds_hits", nsub), ("dmt_sums", ndm), ("dmt_hits", ndm)):
        c[k] = rng.integers(0, 1 << 30, (rows, ntime)).astype(np.int32)
    return c


def test_burst_file_roundtrip_and_layout(tmp_path):
    hdr = {"ntime": 6, "nsub": 5, "ndm": 3, "nchans": 12, "nbits": 8, "nsamps": (1 << 34) + 5, "tsamp": 64e-6,
           "fch1": 1510.0, "foff": -1.09}
    cands = [_hand_cutout(seed=1), dict(_hand_cutout(seed=2), sample=3, width=1, tscrunch=1, t0=0, dm=0.0, snr=0.0)]
    path = str(tmp_path / "a.bursts")
    write_burst_file(path, hdr, cands)
    assert not os.path.exists(path + ".tmp")
    raw = open(path, "rb").read()
    # the header, by explicit offsets
    assert raw[0:8] == b"PSBRST01"
    assert struct.unpack_from("<6I", raw, 8) == (2, 6, 5, 3, 12, 8)
    assert struct.unpack_from("<Q", raw, 32) == ((1 << 34) + 5,)
    assert struct.unpack_from("<3d", raw, 40) == (64e-6, 1510.0, -1.09)
    # the first candidate
    assert struct.unpack_from("<QIIqff", raw, 64) == ((1 << 33) + 7, 16, 8, -41, 12.25, 9.5)
    assert struct.unpack_from("<3f", raw, 96) == (0.0, 12.25, 20.5)
    assert struct.unpack_from("<5i", raw, 108) == (3, 2, 0, 3, 2)
    assert struct.unpack_from("<i", raw, 128) == (int(cands[0]["ds_sums"][0, 0]),)
    assert struct.unpack_from("<i", raw, 128 + 4 * 30) == (int(cands[0]["ds_hits"][0, 0]),)
    assert struct.unpack_from("<i", raw, 128 + 4 * 60) == (int(cands[0]["dmt_sums"][0, 0]),)
    assert struct.unpack_from("<i", raw, 128 + 4 * 78) == (int(cands[0]["dmt_hits"][0, 0]),)
    rec = 32 + 4 * 3 + 4 * 5 + 8 * (5 + 3) * 6
    assert len(raw) == 64 + 2 * rec
    f = BurstCubeFile(path)
    assert len(f) == 2 and f.header == dict(hdr, ncand=2)
    for i, c in enumerate(cands):
        g = f.candidate(i)
        assert all(g[k] == c[k] for k in ("sample", "width", "tscrunch", "t0", "dm", "snr"))
        for k in ("dms", "nactive", "ds_sums", "ds_hits", "dmt_sums", "dmt_hits"):
            assert g[k].dtype == c[k].dtype and np.array_equal(g[k], c[k])
    with pytest.raises(IndexError):
        f.candidate(2)
    # the native writer gives the same bytes
    h = C.BurstFileHeader()
    h.ncand, h.ntime, h.nsub, h.ndm, h.nchans, h.nbits = 2, 6, 5, 3, 12, 8
    h.nsamps, h.tsamp, h.fch1, h.foff = hdr["nsamps"], hdr["tsamp"], hdr["fch1"], hdr["foff"]
    native = str(tmp_path / "b.bursts")
    C.write_burst_file(native, h, [C.BurstCandidate(c["sample"], c["width"], c["dm"], c["snr"]) for c in cands], cands)
    assert open(native, "rb").read() == raw and not os.path.exists(native + ".tmp")
    open(path, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        BurstCubeFile(path)
    # burst_mean: sums / hits, NaN where nothing was counted
    m = burst_mean(np.array([[6, 0], [5, 9]]), np.array([[3, 0], [2, 3]]))
    assert m.dtype == np.float64 and m[0, 0] == 2.0 and np.isnan(m[0, 1]) and m[1, 0] == 2.5 and m[1, 1] == 3.0


def test_panels_on_a_hand_built_cutout():
    nsub, ndm, ntime = 4, 5, 8
    hits = np.full((nsub, ntime), 10, dtype=np.int32)
    hits[2] = 0      # a killed subband
    hits[:, 0] = 0   # a bin before the start of the file
    level = 100 + 10 * np.arange(nsub)
    mean = np.broadcast_to(level[:, None], (nsub, ntime)).copy()
    mean[:, 5] += 40
    dh = np.full((ndm, ntime), 30, dtype=np.int32)
    dh[:, 0] = 0
    dmean = np.full((ndm, ntime), 50)
    dmean[3, 4] += 9
    c = {"ds_sums": (mean * hits).astype(np.int32), "ds_hits": hits, "dmt_sums": (dmean * dh).astype(np.int32),
         "dmt_hits": dh}
    wf = burst_waterfall_panel(c)
    assert wf.shape == (nsub, ntime) and wf.dtype == np.float64 and np.all(wf[2] == 0) and np.all(wf[:, 0] == 0)
    for s in (0, 1, 3):
        assert int(np.argmax(wf[s])) == 5 and wf[s, 5] == pytest.approx(40.0) and wf[s, 1] == 0
    dt = burst_dmtime_panel(c)
    assert dt.shape == (ndm, ntime) and np.unravel_index(np.argmax(dt), dt.shape) == (3, 4) and dt[3, 4] == 9.0
    assert np.all(dt[:, 0] == 0) and dt[0, 3] == 0
    prof = burst_profile_panel(c)
    assert prof.shape == (ntime,) and int(np.argmax(prof)) == 5 and prof[5] == pytest.approx(40.0) and prof[0] == 0


# ----------------------------------------------------------------- sweep ----
# nbits (bias 128 for 8 bits, else 0), nchans, nsub, ndm, ntime, nsamps N, candidate (sample, width, dm; "big": the
# offsets of adjacent DM rows differ by more than the kernel's window in the last channel), tscrunch, kill.  The
# rows are `pad` samples longer than N, filled with other noise: a read past N would show.
SWEEP = [
    dict(id="f1-2bit-ragged-ntime", nbits=2, nchans=64, nsub=8, ndm=5, ntime=37, n=20000, sample=9001, width=1,
         dm=30.0, tscrunch=0, kill=None),
    dict(id="f2-8bit-before-start-nsub7", nbits=8, nchans=64, nsub=7, ndm=6, ntime=64, n=20000, sample=10, width=4,
         dm=55.5, tscrunch=0, kill=None),
    dict(id="f3-nsub=nchans-odd-ndm-kill", nbits=8, nchans=40, nsub=40, ndm=7, ntime=50, n=20000, sample=7003, width=9,
         dm=40.0, tscrunch=3, kill=[1, 17, 38]),
    dict(id="f48-two-time-tiles-past-end", nbits=2, nchans=64, nsub=8, ndm=3, ntime=199, n=30000, sample=29950,
         width=96, dm=20.0, tscrunch=0, kill=[0, 9, 63]),
    dict(id="f2048-ntime8-nsub1-ndm1", nbits=2, nchans=40, nsub=1, ndm=1, ntime=8, n=30000, sample=15000, width=4096,
         dm=10.0, tscrunch=0, kill=None),
    dict(id="bigdm-one-row-tiles-rows-past-end", nbits=8, nchans=64, nsub=8, ndm=4, ntime=16, n=40000, sample=2001,
         width=16, dm="big", tscrunch=0, kill=None),
    dict(id="killed-subband-ntime1", nbits=8, nchans=64, nsub=8, ndm=6, ntime=1, n=20000, sample=5005, width=33,
         dm=100.0, tscrunch=0, kill=[2, 31] + list(range(40, 48))),
    dict(id="f8-many-rows-shared-window", nbits=8, nchans=24, nsub=5, ndm=65, ntime=32, n=20000, sample=8000, width=16,
         dm=12.0, tscrunch=0, kill=None),
]
PAD = 4000


@functools.lru_cache(maxsize=None)
def _sweep_case(i):
    """(values incl. padding, ds offsets, dmt offsets, t0, f, kill, bias, oracle dict) of SWEEP[i], computed once."""
    c = SWEEP[i]
    hdr = _header(c["nchans"], c["nbits"])
    delays = _delays(hdr)
    dm = float(np.float32(1.1 * W * c["ndm"] / 2 / float(delays[-1]))) if c["dm"] == "big" else c["dm"]
    kill = None if c["kill"] is None else _kill(c["nchans"], c["kill"])
    vals = synthetic.generate(c["n"] + PAD, hdr, (), seed=31 + i)
    vals.setflags(write=False)
    exp = ref.burst_cube(vals, c["sample"], c["width"], dm, delays, c["ntime"], c["nsub"], c["ndm"], c["tscrunch"],
                         killmask=kill, nvalid=c["n"])
    ds = ref.dm_offsets([dm], delays)[0]
    dmt = ref.dm_offsets(exp["dms"], delays)
    return vals, ds, dmt, exp["t0"], exp["tscrunch"], kill, 128 if c["nbits"] == 8 else 0, exp


def test_sweep_covers_what_it_must():
    """The properties the shape sweep has to contain, checked on the CPU from the oracle alone."""
    seen = set()
    for i, c in enumerate(SWEEP):
        vals, ds, dmt, t0, f, kill, bias, exp = _sweep_case(i)
        seen.add(f)
        n, nt = c["n"], c["ntime"]
        full = f * exp["nactive"].sum()
        if t0 < 0:
            seen.add("before-start")
            # leading bins empty (the DM 0 row) and short (rows whose sweep reaches into the file)
            assert exp["dmt_hits"][0, 0] == 0 and (exp["dmt_hits"][c["ndm"] // 2] == full).any()
            assert ((exp["dmt_hits"] > 0) & (exp["dmt_hits"] < full)).any()
        if t0 + nt * f + int(ds.max()) > n and (exp["ds_hits"] > 0).any():
            seen.add("past-end")
            assert (exp["ds_hits"][:, -1] < f * exp["nactive"]).any()
        if (t0 + dmt > n).any():
            seen.add("row-past-end")  # a DM row none of whose samples exist for some channels
            assert (exp["dmt_hits"][-1] < full).all()
        if c["dm"] == "big":
            seen.add("fallback")
            assert np.diff(dmt[:, -1].astype(np.int64)).min() > W
        if any((t0 + int(o)) % 16 for o in ds):
            seen.add("unaligned")
        if c["nchans"] % c["nsub"]:
            seen.add("nsub-ragged")
        if (exp["nactive"] == 0).any():
            seen.add("dead-subband")
            s = int(np.argmin(exp["nactive"]))
            assert not exp["ds_sums"][s].any() and not exp["ds_hits"][s].any()
        if kill is not None:
            seen.add("kill")
        if nt * f > W // 2 and nt > 2 and all(nt % b for b in range(2, nt)):
            seen.add("time-tiles")  # more bins than one workgroup's window holds; a prime count is no multiple
        seen.add(("bits", c["nbits"], bias))
        seen.add(("nsub", "all" if c["nsub"] == c["nchans"] else c["nsub"]))
        seen.add(("ndm", c["ndm"] if c["ndm"] == 1 else ("odd" if c["ndm"] % 2 else "even")))
        seen.add(("ntime", 1 if nt == 1 else "n"))
        assert max(int(exp["dmt_sums"].max()), 255 * f * int(exp["nactive"].sum())) < 2 ** 31
        assert c["n"] <= 40000 and c["nchans"] <= 64
    need = {1, 2, 3, 48, 2048, "before-start", "past-end", "row-past-end", "fallback", "unaligned", "nsub-ragged",
            "dead-subband", "kill", "time-tiles", ("bits", 2, 0), ("bits", 8, 128), ("nsub", "all"), ("nsub", 1),
            ("ndm", 1), ("ndm", "odd"), ("ntime", 1)}
    assert need <= seen, need - seen
    assert SWEEP[4]["ntime"] == 8 and _sweep_case(4)[4] == 2048


# ------------------------------------------------------------------- GPU ----
def _device_rows(values, nbits, bias):
    """values [nsamps, nchans] raw -> int8 [nchans, stride] on the device through unpack_transpose."""
    import torch

    from peasoup_amd import ops
    from peasoup_amd.utils.sigproc import pack_samples

    nsamps, nchans = values.shape
    packed = torch.from_numpy(pack_samples(values, nbits)).cuda()
    stride = (nsamps + 15) // 16 * 16
    return ops.unpack_transpose(packed, nsamps, nchans, nbits, bias, stride)


def _equal(got, exp):
    import torch

    for g, k in zip(got, ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits")):
        assert g.dtype == torch.int32 and tuple(g.shape[1:]) == exp[k].shape
        assert torch.equal(g.cpu()[0], torch.from_numpy(exp[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c["id"] for c in SWEEP])
def test_burst_cube_equals_oracle(i):
    import torch

    from peasoup_amd import ops

    c = SWEEP[i]
    vals, ds, dmt, t0, f, kill, bias, exp = _sweep_case(i)
    rows = _device_rows(vals, c["nbits"], bias)
    args = (rows, torch.from_numpy(ds[None].astype(np.int32)), torch.from_numpy(dmt[None].astype(np.int32)), [t0], f)
    kw = dict(ntime=c["ntime"], nsub=c["nsub"], bias=bias, killmask=kill, nsamps=c["n"])
    got = ops.burst_cube(*args, **kw)
    _equal(got, exp)
    # determinism: a second call gives identical tensors
    again = ops.burst_cube(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def _batch_setup():
    nchans, n = 64, 30000
    hdr = _header(nchans, 8)
    delays = _delays(hdr)
    cands = [(9000, 1, 0.0), (12000, 64, 120.5), (200, 8, 300.0), (29990, 512, 33.0), (15000, 3, 500.0)]
    vals = synthetic.generate(n, hdr, (), seed=5)
    return hdr, delays, cands, vals, n


def _cutter(rows, n, delays, kill, params, **kw):
    import torch

    return C.BurstCutter(rows.data_ptr(), rows.shape[1], n, rows.shape[0], 128, [float(d) for d in delays],
                         [] if kill is None else [int(k) for k in kill], params,
                         torch.cuda.current_stream().cuda_stream, **kw)


PLANES = ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits")


@pytest.mark.gpu
def test_batch_equals_one_at_a_time_and_keeps_order():
    hdr, delays, cands, vals, n = _batch_setup()
    kill = _kill(64, [7, 8, 50])
    rows = _device_rows(vals, 8, 128)
    ntime, nsub, ndm = 48, 8, 9
    p = C.BurstParams(ntime, nsub, ndm)
    both = _cutter(rows, n, delays, kill, p)
    res = both.cut([C.BurstCandidate(*c) for c in cands])
    assert both.batches == 1 and len(res) == len(cands)
    assert len({r["tscrunch"] for r in res}) >= 4
    for i, c in enumerate(cands):
        exp = ref.burst_cube(vals, c[0], c[1], c[2], delays, ntime, nsub, ndm, killmask=kill)
        one = _cutter(rows, n, delays, kill, p).cut([C.BurstCandidate(*c)])[0]
        for k in PLANES + ("nactive", "dms"):
            assert np.array_equal(res[i][k], exp[k]), (i, k)
            assert np.array_equal(one[k], exp[k]), (i, k)
        assert (res[i]["tscrunch"], res[i]["t0"]) == (exp["tscrunch"], exp["t0"])
        assert list(res[i]["nactive"]) == [7, 7, 8, 8, 8, 8, 7, 8]
    # a budget of two candidates: three launches, input order kept
    small = _cutter(rows, n, delays, kill, p, batch_bytes=2 * both.bytes_per_candidate + 8)
    assert small.batch_size == 2
    res2 = small.cut([C.BurstCandidate(*c) for c in cands])
    assert small.batches == 3
    for a, b in zip(res, res2):
        assert all(np.array_equal(a[k], b[k]) for k in PLANES) and a["t0"] == b["t0"]


@pytest.mark.gpu
def test_big_dm_takes_the_one_row_path():
    c = SWEEP[5]
    vals, ds, dmt, t0, f, kill, bias, exp = _sweep_case(5)
    rows = _device_rows(vals, 8, 128)
    delays = _delays(_header(c["nchans"], 8))
    dm = float(np.float32(1.1 * W * c["ndm"] / 2 / float(delays[-1])))
    cutter = _cutter(rows, c["n"], delays, None, C.BurstParams(c["ntime"], c["nsub"], c["ndm"]))
    res = cutter.cut([C.BurstCandidate(c["sample"], c["width"], dm)])[0]
    assert cutter.single_row_tiles == c["ndm"] and cutter.tiles == c["nsub"] + c["ndm"]
    assert all(np.array_equal(res[k], exp[k]) for k in PLANES)
    # a low DM shares windows between rows
    shared = _cutter(rows, c["n"], delays, None, C.BurstParams(c["ntime"], c["nsub"], c["ndm"]))
    shared.cut([C.BurstCandidate(c["sample"], c["width"], 10.0)])
    assert shared.single_row_tiles == 0 and shared.tiles < c["nsub"] + c["ndm"]


@pytest.mark.gpu
def test_bad_candidates_are_named_and_nothing_is_launched():
    hdr, delays, cands, vals, n = _batch_setup()
    rows = _device_rows(vals, 8, 128)
    cutter = _cutter(rows, n, delays, None, C.BurstParams(48, 8, 9))
    good = C.BurstCandidate(*cands[0])
    # the 32-bit bound from the definition: 255 f (unkilled channels) < 2^31, f = width // 2
    f_bad = -(-2 ** 31 // (255 * 64))
    assert 255 * f_bad * 64 >= 2 ** 31 > 255 * (f_bad - 1) * 64
    for bad in (C.BurstCandidate(n, 4, 10.0), C.BurstCandidate(n + 5000, 4, 10.0), C.BurstCandidate(100, 0, 10.0),
                C.BurstCandidate(100, 4, -1.0), C.BurstCandidate(100, 2 * f_bad, 10.0),
                C.BurstCandidate(100, 2 * C.burst_max_f() + 2, 10.0)):
        with pytest.raises(C.NativeError, match="candidate 2[ :]"):
            cutter.cut([good, good, bad])
    with pytest.raises(C.NativeError, match="candidate 2: 255 x"):
        cutter.cut([good, good, C.BurstCandidate(100, 2 * f_bad, 10.0)])
    assert cutter.batches == 0
    # candidates at the very edges are not refused
    res = cutter.cut([C.BurstCandidate(n - 1, 1, 10.0), C.BurstCandidate(0, 1, 10.0)])
    assert cutter.batches == 1 and res[0]["ds_hits"].any() and res[1]["ds_hits"].any()


# An injected burst (DM 100: a sweep of 277 samples over the band) and, 0.6 s
# later, a zero-DM impulse, in 64 channels of 8 bits; the search runs at DMs 50
# .. 150, so the impulse is found smeared at the lowest trial.
R_N = 1 << 15
R_DM = 100.0
R_BURST = synthetic.BurstSpec(time=0.8, dm=R_DM, width=16 * TSAMP, amplitude=1.0)
R_IMPULSE = synthetic.RfiSpec(kind="impulse", time=1.4, duration=16 * TSAMP, amplitude=1.5)
R_DMS = [50.0, 75.0, 100.0, 125.0, 150.0]
R_NTIME, R_NSUB, R_NDM = 64, 8, 33
R_BASELINE = 4096


@functools.lru_cache(maxsize=None)
def _recovery():
    """values, delays, the search's offsets, and the float64 oracle's best (sample, width, dm) near each event."""
    hdr = _header(64, 8)
    delays = _delays(hdr)
    sweep = int(ref.dm_offsets([R_DM], delays).max())
    assert 200 < sweep < 400
    vals = synthetic.generate(R_N, hdr, (), seed=41, bursts=[R_BURST], rfi=[R_IMPULSE])
    offs = ref.dm_offsets(R_DMS, delays)
    out_n = R_N - int(offs.max())
    trials = ref.dedisperse(vals, offs, 8, out_nsamps=out_n)
    widths = ref.sp_widths(out_n, 256)
    best = {}
    for name, t in (("burst", R_BURST.time / TSAMP), ("impulse", R_IMPULSE.time / TSAMP)):
        lo, hi = int(t) - 600, int(t) + 200
        top = (-1.0, 0, 0, 0.0)
        for d, dm in enumerate(R_DMS):
            for w, snr in zip(widths, ref.sp_boxcar_snr(trials[d], R_BASELINE, widths)):
                k = lo + int(np.argmax(snr[lo:hi]))
                if snr[k] > top[0]:
                    top = (float(snr[k]), k, int(w), dm)
        best[name] = top
    return vals, delays, offs, out_n, best


def _assert_burst(c):
    nt, nd = R_NTIME, R_NDM
    prof = burst_profile_panel(c)
    assert abs(int(np.argmax(prof)) - nt // 2) <= 1
    dt = burst_dmtime_panel(c)
    assert abs(int(np.unravel_index(np.argmax(dt), dt.shape)[0]) - nd // 2) <= 2
    wf = burst_waterfall_panel(c)
    peaks = [int(np.argmax(wf[s])) for s in range(wf.shape[0])]
    assert max(peaks) - min(peaks) <= 1, peaks


def _lowest_rows(c, delays):
    """The DM rows that a time bin cannot tell from DM 0: their sweep over the band is at most one bin of
    tscrunch samples plus the impulse's own 16.  They end well below the candidate's row."""
    low = int(np.sum(c["dms"].astype(np.float64) * float(delays[-1]) <= c["tscrunch"] + 16))
    assert 1 <= low <= R_NDM // 2 - 4
    return low


def _assert_impulse(c, delays):
    dt = burst_dmtime_panel(c)
    assert int(np.unravel_index(np.argmax(dt), dt.shape)[0]) < _lowest_rows(c, delays)


def test_recovery_seed_on_the_oracle():
    vals, delays, _, _, best = _recovery()
    snr, sample, width, dm = best["burst"]
    assert snr > 15 and dm == R_DM and abs(sample + width / 2 - R_BURST.time / TSAMP) <= width
    c = ref.burst_cube(vals, sample, width, dm, delays, R_NTIME, R_NSUB, R_NDM)
    _assert_burst(c)
    # with margin: the profile's peak stands 10 sigma of its other bins above them, the DM-time plane's best
    # row beats every row more than two away by a tenth of its height
    prof = burst_profile_panel(c)
    rest = np.delete(prof, np.arange(R_NTIME // 2 - 2, R_NTIME // 2 + 3))
    assert prof.max() > rest.max() + 10 * rest.std()
    dt = burst_dmtime_panel(c).max(axis=1)
    far = np.abs(np.arange(R_NDM) - R_NDM // 2) > 2
    assert dt[~far].max() > 1.1 * dt[far].max()
    snr, sample, width, dm = best["impulse"]
    assert snr > 8 and dm == R_DMS[0]
    ci = ref.burst_cube(vals, sample, width, dm, delays, R_NTIME, R_NSUB, R_NDM)
    _assert_impulse(ci, delays)
    dt = burst_dmtime_panel(ci).max(axis=1)
    assert dt[:_lowest_rows(ci, delays)].max() > 1.5 * dt[R_NDM // 2:].max()


@pytest.mark.gpu
def test_recovers_a_burst_and_tells_a_zero_dm_impulse():
    import torch

    from peasoup_amd import ops

    vals, delays, offs, out_n, best = _recovery()
    rows = _device_rows(vals, 8, 128)
    scale = 192.0 / (255 * 64)
    trials = ops.dedisperse(rows, torch.from_numpy(offs), out_n, scale, bias=128)
    p = C.SpParams()
    p.tsamp, p.min_snr, p.boxcar_max, p.baseline_samples, p.capacity = TSAMP, 8.0, 256, R_BASELINE, 1 << 16
    events = ops.single_pulse_search(trials, out_n, p)
    band_delay = 4.15e3 * (1.0 / (1510.0 - 1.09 * 63) ** 2 - 1.0 / 1510.0 ** 2)
    found = sorted(C.sp_cluster(events, R_DMS, band_delay, TSAMP), key=lambda c: -c.snr)[:4]
    assert len(found) >= 2
    cutter = _cutter(rows, R_N, delays, None, C.BurstParams(R_NTIME, R_NSUB, R_NDM))
    res = cutter.cut([C.BurstCandidate(c.sample, c.width, c.dm, c.snr) for c in found])
    for c, r in zip(found, res):
        exp = ref.burst_cube(vals, c.sample, c.width, c.dm, delays, R_NTIME, R_NSUB, R_NDM)
        assert all(np.array_equal(r[k], exp[k]) for k in PLANES)
    near = lambda t: min(range(len(found)), key=lambda i: abs(found[i].sample + found[i].width / 2 - t))  # noqa: E731
    b, i = near(R_BURST.time / TSAMP), near(R_IMPULSE.time / TSAMP)
    assert b != i and found[b].dm == R_DM and found[i].dm == R_DMS[0]
    _assert_burst(res[b])
    _assert_impulse(res[i], delays)


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.mark.gpu
def test_cli_and_module_write_identical_files(tmp_path):
    import torch

    from peasoup_amd import ops

    nchans, nsamps = 40, 20000
    hdr = _header(nchans, 8)
    fil = str(tmp_path / "a.fil")
    hdr = synthetic.write(fil, nsamps, hdr, (), seed=9)
    vals = synthetic.generate(nsamps, hdr, (), seed=9)
    killf = tmp_path / "kill.txt"
    kill = _kill(nchans, [4, 5, 30])
    killf.write_text("".join(f"{k}\n" for k in kill))
    cands = [(9.229, 6912, 32, 49.7063), (8.564, 19990, 1, 32.9407), (8.527, 3, 64, 36.2595)]
    spf = tmp_path / "sp.txt"
    spf.write_text("# peasoup_amd single-pulse search (spsearch)\n#     snr       sample           time_s   width  dm_idx"
                   "         dm  members first_sample  last_sample   dm_lo   dm_hi\n" +
                   "".join(f"{s:9.3f} {t:12d} {t * TSAMP:16.9f} {w:7d} {3:7d} {dm:10.4f} {5:8d} {t:12d} {t + w:12d} "
                           f"{0:7d} {18:7d}\n" for s, t, w, dm in cands) +
                   "    8.000         5000      0.320000000       8       1     3.0000        1         5000         "
                   "5008       0       2\n")  # beyond --limit
    flags = ["-i", fil, "--spfile", str(spf), "--ntime", "24", "--nsub", "7", "--ndm", "5", "--limit", "3"]
    a, b, k = str(tmp_path / "native.bursts"), str(tmp_path / "module.bursts"), str(tmp_path / "kill.bursts")
    _run([os.path.join(REPO, "bin", "burstcube")] + flags + ["-o", a])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "burst"] + flags + ["-o", b], env=env, cwd=REPO)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = BurstCubeFile(a)
    assert f.header == {"ncand": 3, "ntime": 24, "nsub": 7, "ndm": 5, "nchans": nchans, "nbits": 8, "nsamps": nsamps,
                        "tsamp": hdr["tsamp"], "fch1": hdr["fch1"], "foff": hdr["foff"]}
    delays = _delays(hdr)
    rows = _device_rows(vals, 8, 128)
    for i, (snr, t, w, dm) in enumerate(cands):
        g = f.candidate(i)
        exp = ref.burst_cube(vals, t, w, float(np.float32(dm)), delays, 24, 7, 5)
        assert (g["sample"], g["width"], g["dm"], g["snr"]) == (t, w, np.float32(dm), np.float32(snr))
        assert (g["tscrunch"], g["t0"]) == (exp["tscrunch"], exp["t0"])
        for key in PLANES + ("dms", "nactive"):
            assert np.array_equal(g[key], exp[key]), (i, key)
        got = ops.burst_cube(rows, torch.from_numpy(ref.dm_offsets([np.float32(dm)], delays)),
                             torch.from_numpy(ref.dm_offsets(exp["dms"], delays)[None]), [exp["t0"]], exp["tscrunch"],
                             ntime=24, nsub=7, bias=128, nsamps=nsamps)
        assert all(np.array_equal(t_.cpu().numpy()[0], g[key]) for t_, key in zip(got, PLANES))
    # -k changes nactive (and the sums), a nsub above nchans is capped
    _run([os.path.join(REPO, "bin", "burstcube")] + flags + ["-o", k, "-k", str(killf), "--nsub", "64"])
    fk = BurstCubeFile(k)
    assert fk.header["nsub"] == nchans
    assert np.array_equal(fk.candidate(0)["nactive"], kill.astype(np.int32))
    exp = ref.burst_cube(vals, cands[0][1], cands[0][2], float(np.float32(cands[0][3])), delays, 24, nchans, 5,
                         killmask=kill)
    assert all(np.array_equal(fk.candidate(0)[key], exp[key]) for key in PLANES)
    # giving both candidate sources is an error
    r = subprocess.run([os.path.join(REPO, "bin", "burstcube"), "-i", fil, "--spfile", str(spf), "--candfile", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
