"""Filterbank fold cubes (csrc/include/psoup/foldcube.hpp; an extension beyond
the reference): subint x subband x phase cubes per periodicity candidate.

CPU: option parsing, the candidate file, identities of the NumPy oracle, the
cube file (header layout pinned by explicit offsets, Python and native writers
byte-identical), the two plot panels and the plot tool.  GPU: the kernel's
integer cubes must EQUAL the oracle's (torch.equal) over a sweep of shapes,
batching, determinism, recovery of an injected dispersed pulsar, errors, and
the entry points (bin/foldcube, python -m peasoup_amd cube, --overview)."""
import functools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_CANDS, GOLDEN_XML, REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.outputs import FoldCubeFile, OverviewFile, cube_mean, write_cube_file
from peasoup_amd.utils.plotting import CandidatePlotter, freq_phase_panel, time_phase_panel

T = C.cube_tile()
TSAMP = 64e-6


# ------------------------------------------------------------------- CPU ----
def test_cube_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_cube_cmdline(["foldcube", "-i", "x.fil", "--candfile", "c.txt"])
    assert ok and not exit_now and a.infilename == "x.fil" and a.candfilename == "c.txt"
    assert (a.nints, a.nsub, a.nbins, a.fold_nsamps, a.limit, a.top) == (16, 32, 64, 0, 1000, 16)
    assert not a.verbose and a.killfilename == "" and a.overviewfilename == ""
    assert a.outfilename.endswith("_foldcube.cubes")
    assert len(a.outfilename) == len("2026-01-01-00:00_foldcube.cubes")
    ok, _, a = C.parse_cube_cmdline(["foldcube", "-i", "y.fil", "-o", "out.cubes", "--overview", "ov.xml", "--top", "3",
                                     "-k", "kill.txt", "--nints", "8", "--nsub", "5", "--nbins", "128",
                                     "--fold_nsamps", "4096", "--limit", "7", "-v"])
    assert ok and a.outfilename == "out.cubes" and a.overviewfilename == "ov.xml" and a.top == 3
    assert a.killfilename == "kill.txt" and (a.nints, a.nsub, a.nbins) == (8, 5, 128)
    assert a.fold_nsamps == 4096 and a.limit == 7 and a.verbose and a.candfilename == ""
    ok, exit_now, _ = C.parse_cube_cmdline(["foldcube", "-h"])
    assert ok and exit_now


@pytest.mark.parametrize("extra", [
    [],                                               # neither --candfile nor --overview
    ["--candfile", "c.txt", "--overview", "o.xml"],   # both
    ["--candfile", "c.txt", "--nbins", "1"], ["--candfile", "c.txt", "--nbins", "257"],
    ["--candfile", "c.txt", "--nints", "0"], ["--candfile", "c.txt", "--nints", "257"],
    ["--candfile", "c.txt", "--nsub", "0"],
])
def test_cube_cmdline_errors(extra):
    assert not C.parse_cube_cmdline(["foldcube", "-i", "x.fil"] + extra)[0]
    assert not C.parse_cube_cmdline(["foldcube", "--candfile", "c.txt"])[0]  # -i is required


def test_cube_candfile(tmp_path):
    f = tmp_path / "cands.txt"
    f.write_text("# period dm acc\n0.25 30.5 -1.5\n\n   # indented comment\n1e-3\t0\t0 extra columns 7\n0.5 2 3\n")
    c = C.read_cube_candfile(str(f))
    assert [(x.period, x.dm, x.acc) for x in c] == [(0.25, 30.5, -1.5), (1e-3, 0.0, 0.0), (0.5, 2.0, 3.0)]
    assert len(C.read_cube_candfile(str(f), 2)) == 2
    f.write_text("0.25 30.5 -1.5\n# c\n0.5 abc 1\n")
    with pytest.raises(C.NativeError, match="line 3"):
        C.read_cube_candfile(str(f))
    f.write_text("0.25 30.5\n")
    with pytest.raises(C.NativeError, match="line 1"):
        C.read_cube_candfile(str(f))


def _header(nchans, nbits, tsamp=TSAMP):
    return synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=tsamp)


def _offsets(hdr, dm):
    delays = ref.delay_table(hdr["nchans"], hdr["tsamp"], hdr["fch1"], hdr["foff"])
    return delays, ref.dm_offsets([dm], delays)[0]


def _dedispersed_sum(values, off, src, kill):
    """The oracle's unscaled dedispersed series summed over the fold's source samples."""
    series = sum(values[off[c]:off[c] + int(src.max()) + 1, c].astype(np.int64) for c in np.nonzero(kill)[0])
    return int(series[src].sum())


def test_oracle_identities():
    nchans, nsub, nints, nbins, n = 24, 5, 3, 16, 1000
    hdr = _header(nchans, 8)
    _, off = _offsets(hdr, 150.0)
    nsamps = n + int(off.max())
    kill = np.ones(nchans, int)
    kill[[3, 10, 11]] = 0
    period, af = 37.3 * TSAMP, 2.5e-6
    # constant filterbank: sums == v * hits x nactive
    const = np.full((nsamps, nchans), 7, dtype=np.uint8)
    sums, hits, nact = ref.fold_cube(const, off, period, af, TSAMP, n, nints, nsub, nbins, kill)
    assert sums.dtype == np.int64 and hits.dtype == np.int32 and nact.dtype == np.int32
    assert np.array_equal(sums, 7 * hits[:, None, :].astype(np.int64) * nact[None, :, None])
    assert hits.sum() == nints * (n // nints) and nact.sum() == nchans - 3
    assert list(nact) == [np.sum(kill[[c for c in range(nchans) if c * nsub // nchans == s]]) for s in range(nsub)]
    # noise: the cube's total is the dedispersed series summed over src
    vals = synthetic.generate(nsamps, hdr, (), seed=3)
    sums, hits, _ = ref.fold_cube(vals, off, period, af, TSAMP, n, nints, nsub, nbins, kill)
    nps, h = n // nints, n / 2.0
    d = np.arange(nints * nps, dtype=np.float64)
    src = np.clip(np.rint(d + af * ((d - h) ** 2 - h * h)), 0, n - 1).astype(np.int64)
    assert sums.sum() == _dedispersed_sum(vals, off, src, kill)
    assert hits.sum() == nints * nps
    with pytest.raises(ValueError):
        ref.fold_cube(vals[:-1], off, period, af, TSAMP, n, nints, nsub, nbins, kill)


def _hand_cube(nints=3, nsub=5, nbins=8, seed=0):
    rng = np.random.default_rng(seed)
    nact = np.array([3, 2, 0, 3, 2], dtype=np.int32)[:nsub]
    hits = rng.integers(0, 50, (nints, nbins)).astype(np.int32)
    sums = rng.integers(0, 1 << 40, (nints, nsub, nbins)).astype(np.int64) * (nact[None, :, None] > 0)
    return {"period": 0.123456789012345, "dm": 12.25, "acc": -3.5, "nactive": nact, "hits": hits, "sums": sums}


def test_cube_file_roundtrip_and_layout(tmp_path):
    hdr = {"nints": 3, "nsub": 5, "nbins": 8, "nchans": 12, "nbits": 8, "fold_nsamps": (1 << 33) + 5,
           "tsamp": 64e-6, "fch1": 1510.0, "foff": -1.09}  # nsub does not divide nchans
    cands = [_hand_cube(seed=1), dict(_hand_cube(seed=2), period=1.5, dm=0.0, acc=0.0)]
    path = str(tmp_path / "a.cubes")
    write_cube_file(path, hdr, cands)
    assert not os.path.exists(path + ".tmp")
    raw = open(path, "rb").read()
    # the header, by explicit offsets
    assert raw[0:8] == b"PSCUBE01"
    assert struct.unpack_from("<6I", raw, 8) == (2, 3, 5, 8, 12, 8)
    assert struct.unpack_from("<Q", raw, 32) == ((1 << 33) + 5,)
    assert struct.unpack_from("<3d", raw, 40) == (64e-6, 1510.0, -1.09)
    # the first candidate
    assert struct.unpack_from("<dff", raw, 64) == (0.123456789012345, 12.25, -3.5)
    assert struct.unpack_from("<5i", raw, 80) == tuple(int(x) for x in cands[0]["nactive"])
    assert struct.unpack_from("<i", raw, 100) == (int(cands[0]["hits"][0, 0]),)
    assert struct.unpack_from("<q", raw, 100 + 4 * 24) == (int(cands[0]["sums"][0, 0, 0]),)
    rec = 16 + 4 * 5 + 4 * 24 + 8 * 120
    assert len(raw) == 64 + 2 * rec
    f = FoldCubeFile(path)
    assert len(f) == 2 and f.header == dict(hdr, ncand=2)
    for i, c in enumerate(cands):
        g = f.candidate(i)
        assert (g["period"], g["dm"], g["acc"]) == (c["period"], c["dm"], c["acc"])
        for k in ("nactive", "hits", "sums"):
            assert g[k].dtype == c[k].dtype and np.array_equal(g[k], c[k])
        m = f.mean(i)
        den = c["hits"][:, None, :].astype(np.float64) * c["nactive"][None, :, None]
        assert m.dtype == np.float64 and np.all(m[den == 0] == 0)
        assert np.array_equal(m[den != 0], (c["sums"] / np.where(den == 0, 1, den))[den != 0])
    with pytest.raises(IndexError):
        f.candidate(2)
    # the native writer gives the same bytes
    h = C.CubeFileHeader()
    h.ncand, h.nints, h.nsub, h.nbins, h.nchans, h.nbits = 2, 3, 5, 8, 12, 8
    h.fold_nsamps, h.tsamp, h.fch1, h.foff = hdr["fold_nsamps"], hdr["tsamp"], hdr["fch1"], hdr["foff"]
    native = str(tmp_path / "b.cubes")
    C.write_cube_file(native, h, [C.CubeCandidate(c["period"], c["dm"], c["acc"]) for c in cands],
                      [c["nactive"] for c in cands], [c["hits"] for c in cands], [c["sums"] for c in cands])
    assert open(native, "rb").read() == raw and not os.path.exists(native + ".tmp")
    open(path, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        FoldCubeFile(path)


def _panel_cube():
    """5 subbands (subband 2 killed) x 4 subints x 16 bins: a pulse at bin 11 on a sloping baseline."""
    nints, nsub, nbins = 4, 5, 16
    nact = np.array([3, 2, 0, 3, 2], dtype=np.int32)
    hits = np.full((nints, nbins), 10, dtype=np.int32)
    hits[:, 5] = 0  # a bin that is never hit
    level = 100 + 10 * np.arange(nsub)  # per-subband baseline, removed by the median
    mean = np.broadcast_to(level[None, :, None], (nints, nsub, nbins)).astype(np.int64).copy()
    mean[:, :, 11] += 40
    mean[2, :, 3] += 25  # one subint brighter at bin 3
    sums = mean * hits[:, None, :] * nact[None, :, None]
    return {"period": 1.0, "dm": 0.0, "acc": 0.0, "nactive": nact, "hits": hits, "sums": sums}


def test_panels_on_a_hand_built_cube():
    cube = _panel_cube()
    fp = freq_phase_panel(cube)
    assert fp.shape == (5, 16) and fp.dtype == np.float64
    assert np.all(fp[2] == 0)  # the killed subband
    for s in (0, 1, 3, 4):
        assert int(np.argmax(fp[s])) == 11 and fp[s, 11] == pytest.approx(40.0)
        assert fp[s, 0] == 0 and fp[s, 5] == 0  # baseline removed; the unhit bin stays 0
    tp = time_phase_panel(cube)
    assert tp.shape == (4, 16) and tp.dtype == np.float64
    assert all(int(np.argmax(tp[i])) == 11 for i in range(4))
    assert int(np.argmax(tp[:, 3])) == 2 and np.all(tp[:, 5] == 0)
    w = cube["nactive"] / cube["nactive"].sum()
    assert tp[0, 0] == pytest.approx(float((w * (100 + 10 * np.arange(5))).sum()))
    assert np.array_equal(cube_mean(cube)[:, 2], np.zeros((4, 16)))


def test_plot_tool_with_cubes(tmp_path):
    shutil.copy(GOLDEN_XML, tmp_path / "overview.xml")
    shutil.copy(GOLDEN_CANDS, tmp_path / "candidates.peasoup")
    cube = _panel_cube()
    hdr = {"nints": 4, "nsub": 5, "nbins": 16, "nchans": 12, "nbits": 8, "fold_nsamps": 4096, "tsamp": 64e-6,
           "fch1": 1510.0, "foff": -1.09}
    cubes = str(tmp_path / "c.cubes")
    write_cube_file(cubes, hdr, [cube, cube])
    # the panel data (the .npz fallback's path), with and without --cubes
    pl = CandidatePlotter(str(tmp_path), cubes=cubes)
    pl._plt = None
    with np.load(pl.plot_cand(1, str(tmp_path / "with.npz"))) as z:
        assert np.array_equal(z["freq_phase"], freq_phase_panel(cube))
        assert np.array_equal(z["time_phase"], time_phase_panel(cube))
        with_keys = set(z.files)
    plain = CandidatePlotter(str(tmp_path))
    plain._plt = None
    with np.load(plain.plot_cand(1, str(tmp_path / "without.npz"))) as z:
        assert with_keys - set(z.files) == {"freq_phase", "time_phase"}
    # the tool
    out = str(tmp_path / "cand1.png")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "peasoup_plot_cand.py"), str(tmp_path), "1",
                        "--cubes", cubes, "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    written = r.stdout.strip().splitlines()[-1]
    assert os.path.getsize(written) > 0
    if written.endswith(".npz"):
        with np.load(written) as z:
            assert "freq_phase" in z.files and "time_phase" in z.files


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


def _acc_for_shift(shift, n, tsamp):
    """float32 acceleration whose largest resampling shift |af| h^2 is about `shift` samples (signed)."""
    h = n / 2.0
    return float(np.float32(shift / (h * h) * 2 * ref.C_LIGHT / float(np.float32(tsamp))))


def _kill(nchans, idx):
    k = np.ones(nchans, int)
    k[list(idx)] = 0
    return k


# nbits/bias, nchans/nsub, nints, nbins, n, period in samples, resampling shift, dm ("big": largest offset > T), kill
SWEEP = [
    dict(id="2bit-64ch-8sub-ragged", nbits=2, nchans=64, nsub=8, nints=16, nbins=64, n=3 * T + 37, psamp=100.3,
         shift=0.0, dm=0.0, kill=None),
    dict(id="8bit-40ch-7sub-bigdm-acc+", nbits=8, nchans=40, nsub=7, nints=3, nbins=256, n=3 * T + 37, psamp=700.7,
         shift=5.0, dm="big", kill=None),
    dict(id="nsub=nchans-short-acc-", nbits=8, nchans=40, nsub=40, nints=1, nbins=2, n=T - 5, psamp=33.3,
         shift=-4.0, dm=40.0, kill=[1, 17, 38]),
    dict(id="nsub=1-bins-skipped", nbits=2, nchans=64, nsub=1, nints=16, nbins=64, n=3 * T + 37, psamp=20.5,
         shift=-3.5, dm=30.0, kill=[0, 9, 63]),
    dict(id="killed-subband-long-period", nbits=8, nchans=64, nsub=8, nints=3, nbins=64, n=3 * T + 37, psamp=5000.0,
         shift=0.0, dm=100.0, kill=[2, 31] + list(range(40, 48))),
    dict(id="short-16ints-256bins", nbits=2, nchans=40, nsub=7, nints=16, nbins=256, n=T - 300, psamp=411.1,
         shift=3.0, dm=0.0, kill=None),
]


@functools.lru_cache(maxsize=None)
def _sweep_case(i):
    """(values, offsets, period, acc, af, kill, oracle sums, oracle hits) of SWEEP[i], computed once."""
    c = SWEEP[i]
    hdr = _header(c["nchans"], c["nbits"])
    delays = ref.delay_table(c["nchans"], TSAMP, hdr["fch1"], hdr["foff"])
    dm = float(np.float32(1.1 * T / float(delays[-1]))) if c["dm"] == "big" else c["dm"]
    off = ref.dm_offsets([dm], delays)[0]
    n = c["n"]
    acc = _acc_for_shift(c["shift"], n, TSAMP) if c["shift"] else 0.0
    af = ref.accel_factor(acc, TSAMP)
    period = c["psamp"] * TSAMP
    kill = None if c["kill"] is None else _kill(c["nchans"], c["kill"])
    vals = synthetic.generate(n + int(off.max()) + 3, hdr, (), seed=11 + i)
    sums, hits, _ = ref.fold_cube(vals, off, period, af, TSAMP, n, c["nints"], c["nsub"], c["nbins"], kill)
    return vals, off, period, acc, af, kill, sums, hits


def test_sweep_covers_what_it_must():
    """The properties the shape sweep has to contain, checked on the CPU."""
    for i, c in enumerate(SWEEP):
        _, off, period, _, af, _, _, hits = _sweep_case(i)
        h = c["n"] / 2.0
        if c["shift"]:
            assert abs(af) * h * h >= 3 and np.sign(af) == np.sign(c["shift"])
        if c["dm"] == "big":
            assert off.max() > T
        if c["id"] == "nsub=1-bins-skipped":
            assert c["psamp"] < c["nbins"]
        if c["id"] == "killed-subband-long-period":
            assert c["psamp"] > c["n"] // c["nints"] and (hits == 0).any()
            assert all(cc * c["nsub"] // c["nchans"] == 5 for cc in range(40, 48))
    assert {c["shift"] > 0 for c in SWEEP if c["shift"]} == {True, False}
    assert any(c["n"] < T for c in SWEEP) and any(c["n"] == 3 * T + 37 for c in SWEEP)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c["id"] for c in SWEEP])
def test_fold_cube_equals_oracle(i):
    import torch

    from peasoup_amd import ops

    c = SWEEP[i]
    vals, off, period, acc, _, kill, exp_sums, exp_hits = _sweep_case(i)
    bias = 128 if c["nbits"] == 8 else 0
    rows = _device_rows(vals, c["nbits"], bias)
    sums, hits = ops.fold_cube(rows, torch.from_numpy(off[None, :].astype(np.int32)), [period], [acc], TSAMP, c["n"],
                               c["nints"], c["nsub"], c["nbins"], bias=bias, killmask=kill)
    assert sums.dtype == torch.int64 and hits.dtype == torch.int32
    assert tuple(sums.shape) == (1, c["nints"], c["nsub"], c["nbins"])
    assert torch.equal(hits.cpu()[0], torch.from_numpy(exp_hits))
    assert torch.equal(sums.cpu()[0], torch.from_numpy(exp_sums))
    # determinism: a second call gives identical tensors
    sums2, hits2 = ops.fold_cube(rows, torch.from_numpy(off[None, :].astype(np.int32)), [period], [acc], TSAMP,
                                 c["n"], c["nints"], c["nsub"], c["nbins"], bias=bias, killmask=kill)
    assert torch.equal(sums, sums2) and torch.equal(hits, hits2)


def _batch_setup():
    nchans, n = 64, 3 * T + 37
    hdr = _header(nchans, 8)
    delays = ref.delay_table(nchans, TSAMP, hdr["fch1"], hdr["foff"])
    cands = [(100.3 * TSAMP, 0.0, 0.0), (57.9 * TSAMP, 120.5, _acc_for_shift(4.0, n, TSAMP)),
             (1234.5 * TSAMP, 300.0, _acc_for_shift(-6.0, n, TSAMP)), (20.5 * TSAMP, 33.0, 0.0),
             (411.1 * TSAMP, 500.0, _acc_for_shift(3.0, n, TSAMP))]
    offs = ref.dm_offsets([c[1] for c in cands], delays)
    vals = synthetic.generate(n + int(offs.max()) + 1, hdr, (), seed=5)
    return hdr, delays, cands, offs, vals, n


@pytest.mark.gpu
def test_batch_equals_one_at_a_time_and_keeps_order():
    import torch

    from peasoup_amd import ops

    hdr, delays, cands, offs, vals, n = _batch_setup()
    kill = _kill(64, [7, 8, 50])
    rows = _device_rows(vals, 8, 128)
    kw = dict(nints=3, nsub=8, nbins=64, bias=128, killmask=kill)
    per, acc = [c[0] for c in cands], [c[2] for c in cands]
    sums, hits = ops.fold_cube(rows, torch.from_numpy(offs), per, acc, TSAMP, n, **kw)
    for i in range(len(cands)):
        s1, h1 = ops.fold_cube(rows, torch.from_numpy(offs[i:i + 1]), per[i:i + 1], acc[i:i + 1], TSAMP, n, **kw)
        assert torch.equal(s1[0], sums[i]) and torch.equal(h1[0], hits[i])
        es, eh, _ = ref.fold_cube(vals, offs[i], per[i], ref.accel_factor(acc[i], TSAMP), TSAMP, n, 3, 8, 64, kill)
        assert torch.equal(sums[i].cpu(), torch.from_numpy(es)) and torch.equal(hits[i].cpu(), torch.from_numpy(eh))
    # a budget of two candidates' outputs: three launches, input order kept
    per_cand = 3 * 64 * (8 * 8 + 4) + 64 * 4 + 16
    folder = C.CubeFolder(rows.data_ptr(), rows.shape[1], vals.shape[0], 64, 128, TSAMP, [float(d) for d in delays],
                          [int(k) for k in kill], C.CubeParams(3, 8, 64, n),
                          torch.cuda.current_stream().cuda_stream, batch_bytes=2 * per_cand + 8)
    assert folder.batch_size == 2
    res = folder.fold([C.CubeCandidate(*c) for c in cands])
    assert folder.batches == 3 and len(res) == len(cands)
    for i, r in enumerate(res):
        assert np.array_equal(r["sums"], sums[i].cpu().numpy()) and np.array_equal(r["hits"], hits[i].cpu().numpy())
        assert list(r["nactive"]) == [7, 7, 8, 8, 8, 8, 7, 8]


@pytest.mark.gpu
def test_bad_candidates_are_named_and_nothing_is_launched():
    import torch

    hdr, delays, cands, offs, vals, n = _batch_setup()
    rows = _device_rows(vals, 8, 128)
    folder = C.CubeFolder(rows.data_ptr(), rows.shape[1], vals.shape[0], 64, 128, TSAMP, [float(d) for d in delays],
                          [], C.CubeParams(3, 8, 64, n), torch.cuda.current_stream().cuda_stream)
    good = C.CubeCandidate(*cands[0])
    for bad in (C.CubeCandidate(0.0, 10.0, 0.0), C.CubeCandidate(-0.1, 10.0, 0.0), C.CubeCandidate(0.01, -1.0, 0.0),
                C.CubeCandidate(0.01, 5000.0, 0.0)):  # the last: offsets that do not fit
        with pytest.raises(C.NativeError, match="candidate 2 "):
            folder.fold([good, good, bad])
    assert folder.batches == 0


# An injected pulsar whose dispersive delay across the band is 0.355 periods:
# 64 channels of 8 bits, n = 2^16, the period on a Fourier bin of the search.
R_TSAMP = 320e-6
R_N = 1 << 16
R_PERIOD = R_N * R_TSAMP / 210.0
R_DM = 200.0
R_NSUB, R_NBINS = 8, 64


@functools.lru_cache(maxsize=None)
def _recovery():
    hdr = _header(64, 8, R_TSAMP)
    delays = ref.delay_table(64, R_TSAMP, hdr["fch1"], hdr["foff"])
    band_delay = 4.15e3 * R_DM * (1.0 / (hdr["fch1"] + 63 * hdr["foff"]) ** 2 - 1.0 / hdr["fch1"] ** 2)
    assert 0.25 * R_PERIOD < band_delay < 0.5 * R_PERIOD
    off = ref.dm_offsets([R_DM], delays)[0]
    nsamps = R_N + int(ref.dm_offsets([260.0], delays).max()) + 8  # room for the search's DM trials up to 260
    psr = [synthetic.PulsarSpec(period=R_PERIOD, dm=R_DM, duty=0.05, amplitude=1.0)]
    vals = synthetic.generate(nsamps, hdr, psr, seed=21)
    at_dm = ref.fold_cube(vals, off, R_PERIOD, 0.0, R_TSAMP, R_N, 16, R_NSUB, R_NBINS)
    at_zero = ref.fold_cube(vals, np.zeros(64, np.int32), R_PERIOD, 0.0, R_TSAMP, R_N, 16, R_NSUB, R_NBINS)
    return hdr, delays, off, vals, psr, at_dm, at_zero


def _circ(a, b, nbins):
    d = abs(int(a) - int(b)) % nbins
    return min(d, nbins - d)


def _assert_aligned(cube, nbins=R_NBINS):
    """Every subband's frequency-phase row peaks within +-1 bin (circular) of the band-collapsed peak."""
    fp = freq_phase_panel(cube)
    peak = int(np.argmax(time_phase_panel(cube).sum(axis=0)))
    for s in range(fp.shape[0]):
        assert _circ(np.argmax(fp[s]), peak, nbins) <= 1, (s, int(np.argmax(fp[s])), peak)


def _assert_swept(cube, nbins=R_NBINS):
    """Folded at DM 0 the first and last subbands' peaks are at least nbins / 4 bins apart."""
    fp = freq_phase_panel(cube)
    assert _circ(np.argmax(fp[0]), np.argmax(fp[-1]), nbins) >= nbins // 4


def _as_cube(sums, hits, nact):
    return {"sums": np.asarray(sums), "hits": np.asarray(hits), "nactive": np.asarray(nact)}


def test_recovery_seed_on_the_oracle():
    _, _, _, _, _, at_dm, at_zero = _recovery()
    _assert_aligned(_as_cube(*at_dm))
    _assert_swept(_as_cube(*at_zero))


@pytest.mark.gpu
def test_recovers_a_dispersed_pulsar():
    import torch

    from peasoup_amd import ops

    hdr, delays, off, vals, _, at_dm, at_zero = _recovery()
    rows = _device_rows(vals, 8, 128)
    offs = np.stack([off, np.zeros(64, np.int32)]).astype(np.int32)
    sums, hits = ops.fold_cube(rows, torch.from_numpy(offs), [R_PERIOD, R_PERIOD], [0.0, 0.0], R_TSAMP, R_N, 16,
                               R_NSUB, R_NBINS, bias=128)
    for i, exp in enumerate((at_dm, at_zero)):
        assert torch.equal(sums[i].cpu(), torch.from_numpy(exp[0]))
        assert torch.equal(hits[i].cpu(), torch.from_numpy(exp[1]))
    nact = np.full(R_NSUB, 8, np.int32)
    _assert_aligned(_as_cube(sums[0].cpu().numpy(), hits[0].cpu().numpy(), nact))
    _assert_swept(_as_cube(sums[1].cpu().numpy(), hits[1].cpu().numpy(), nact))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def _module(args):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return _run([sys.executable, "-m", "peasoup_amd", "cube"] + args, env=env, cwd=REPO)


@pytest.mark.gpu
def test_cli_and_module_write_identical_files(tmp_path):
    nchans, nsamps = 40, 3 * T + 500
    hdr = _header(nchans, 8)
    fil = str(tmp_path / "a.fil")
    hdr = synthetic.write(fil, nsamps, hdr, (), seed=9)
    vals = synthetic.generate(nsamps, hdr, (), seed=9)
    killf = tmp_path / "kill.txt"
    kill = _kill(nchans, [4, 5, 30])
    killf.write_text("".join(f"{k}\n" for k in kill))
    candf = tmp_path / "cands.txt"
    cands = [(100.3 * TSAMP, 50.0, 0.0), (33.3 * TSAMP, 0.0, -150.0), (700.7 * TSAMP, 120.0, 90.0)]
    candf.write_text("# period dm acc snr\n" + "".join(f"{p!r} {d} {a} 12.5\n" for p, d, a in cands) +
                     "0.5 10 0\n")  # beyond --limit
    flags = ["-i", fil, "--candfile", str(candf), "-k", str(killf), "--nints", "3", "--nsub", "7", "--nbins", "32",
             "--limit", "3"]
    a, b = str(tmp_path / "native.cubes"), str(tmp_path / "module.cubes")
    _run([os.path.join(REPO, "bin", "foldcube")] + flags + ["-o", a])
    _module(flags + ["-o", b])
    assert open(a, "rb").read() == open(b, "rb").read()
    f = FoldCubeFile(a)
    delays = ref.delay_table(nchans, TSAMP, hdr["fch1"], hdr["foff"])
    n = 1 << int(np.floor(np.log2(nsamps - int(ref.dm_offsets([120.0], delays).max()))))
    assert f.header == {"ncand": 3, "nints": 3, "nsub": 7, "nbins": 32, "nchans": nchans, "nbits": 8,
                        "fold_nsamps": n, "tsamp": hdr["tsamp"], "fch1": hdr["fch1"], "foff": hdr["foff"]}
    for i, (p, d, acc) in enumerate(cands):
        g = f.candidate(i)
        assert (g["period"], g["dm"], g["acc"]) == (p, np.float32(d), np.float32(acc))
        es, eh, ena = ref.fold_cube(vals, ref.dm_offsets([d], delays)[0], p, ref.accel_factor(acc, TSAMP), TSAMP, n,
                                    3, 7, 32, kill)
        assert np.array_equal(g["sums"], es) and np.array_equal(g["hits"], eh) and np.array_equal(g["nactive"], ena)
    # a nsub above nchans is capped
    _run([os.path.join(REPO, "bin", "foldcube")] + flags + ["-o", a, "--nsub", "64"])
    assert FoldCubeFile(a).header["nsub"] == nchans


@pytest.mark.gpu
def test_overview_path(tmp_path):
    hdr, delays, off, vals, psr, _, _ = _recovery()
    from peasoup_amd.utils.sigproc import write_filterbank

    fil = str(tmp_path / "psr.fil")
    write_filterbank(fil, dict(hdr, nsamples=vals.shape[0]), vals)
    outdir = tmp_path / "search"
    _run([os.path.join(REPO, "bin", "peasoup"), "-i", fil, "-o", str(outdir), "--dm_start", "200", "--dm_end", "204",
          "--acc_start", "0", "--acc_end", "0", "-n", "2", "--npdmp", "4", "-m", "8", "-t", "1"])
    ov = OverviewFile(str(outdir / "overview.xml"))
    assert len(ov) >= 2 and len(ov.dm_list) >= 1
    cubes = str(tmp_path / "top.cubes")
    _module(["-i", fil, "--overview", str(outdir / "overview.xml"), "--top", "2", "-o", cubes, "--nsub", str(R_NSUB)])
    f = FoldCubeFile(cubes)
    assert len(f) == 2 and f.header["fold_nsamps"] == R_N
    for i in range(2):
        c, g = ov.get_candidate(i), f.candidate(i)
        period = c["opt_period"] if c["opt_period"] > 0 else c["period"]
        assert (g["period"], g["dm"], g["acc"]) == (period, np.float32(c["dm"]), np.float32(c["acc"]))
    top = ov.get_candidate(0)
    # the list starts on the pulsar's DM and steps by about 6 (a third of a phase bin across a subband's
    # neighbours): whichever of its trials the search ranks first, the subbands still line up
    assert 2 <= len(ov.dm_list) <= 4 and abs(top["dm"] - R_DM) <= 12
    assert abs(f.candidate(0)["period"] / R_PERIOD - 1) < 2e-3
    _assert_aligned(f.candidate(0))
    # the plot tool draws the two panels from this pair of files
    r = _run([sys.executable, os.path.join(REPO, "tools", "peasoup_plot_cand.py"), str(outdir), "0", "--cubes", cubes,
              "-o", str(tmp_path / "cand0.png")])
    assert os.path.getsize(r.stdout.strip().splitlines()[-1]) > 0
    # giving both sources is an error
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "cube", "-i", fil, "--overview",
                        str(outdir / "overview.xml"), "--candfile", "x.txt"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert r.returncode != 0
