"""filscrunch (csrc/include/psoup/scrunch.hpp; an extension beyond the
reference): subband and time-scrunch a filterbank into an 8-bit SIGPROC file.

CPU: option parsing, identities of the NumPy oracle, the host scale step and the
plan through the bindings against the oracle, the header rewrite, the native host
unit tests with their sanitizer builds.  GPU: the kernels' integer outputs must
EQUAL the oracle's (torch.equal) over a sweep of shapes with sentinel-filled row
padding, the requantisation with explicit tables, chunking, refusals, the entry
points (bin/filscrunch, python -m peasoup_amd scrunch) and the recovery of an
injected burst from the scrunched file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, TUTORIAL
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import read_filterbank, read_header, write_filterbank

L = C.scrunch_stat_block()
TSAMP = 64e-6


def _header(nchans, nbits, tsamp=TSAMP, **kw):
    return synthetic.make_header(nchans=nchans, nbits=nbits, tsamp=tsamp, **kw)


def _delays(hdr):
    return ref.delay_table(hdr["nchans"], hdr["tsamp"], hdr["fch1"], hdr["foff"])


def _kill(nchans, idx):
    k = np.ones(nchans, int)
    k[list(idx)] = 0
    return k


# ------------------------------------------------------------------- CPU ----
def test_scrunch_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_scrunch_cmdline(["filscrunch", "-i", "x.fil"])
    assert ok and not exit_now and a.infilename == "x.fil"
    assert (a.dm, a.nsub, a.tscrunch, a.sigma_out) == (0.0, 0, 1, 16.0)  # nsub 0: nchans
    assert not a.plan and not a.verbose and a.killfilename == "" and a.killoutfilename == ""
    assert a.outfilename.endswith("_filscrunch.fil") and len(a.outfilename) == len("2026-01-01-00:00_filscrunch.fil")
    ok, _, a = C.parse_scrunch_cmdline(["filscrunch", "-i", "y.fil", "-o", "o.fil", "-k", "kill.txt", "--dm", "56.5",
                                        "--nsub", "16", "--tscrunch", "4", "--sigma_out", "12.5", "--kill_out",
                                        "ko.txt", "-v"])
    assert ok and (a.outfilename, a.killfilename, a.killoutfilename) == ("o.fil", "kill.txt", "ko.txt")
    assert (a.dm, a.nsub, a.tscrunch, a.sigma_out, a.verbose) == (56.5, 16, 4, 12.5, True)
    ok, _, a = C.parse_scrunch_cmdline(["filscrunch", "-i", "y.fil", "--plan", "--dm_end", "3000"])
    assert ok and a.plan and a.dm_end == 3000.0
    ok, exit_now, _ = C.parse_scrunch_cmdline(["filscrunch", "-h"])
    assert ok and exit_now
    p = C.scrunch_check_params(C.scrunch_params_from(a), 64)
    assert (p.nsub, p.tscrunch, p.dm, p.sigma_out) == (64, 1, 0.0, 16.0)


@pytest.mark.parametrize("extra", [["--tscrunch", "0"], ["--tscrunch", "257"], ["--sigma_out", "0"],
                                   ["--sigma_out", "-2"], ["--plan"], ["--dm", "-1"], ["--nsub", "-4"]])
def test_scrunch_cmdline_errors(extra):
    assert not C.parse_scrunch_cmdline(["filscrunch", "-i", "x.fil"] + extra)[0]
    assert not C.parse_scrunch_cmdline(["filscrunch", "--dm", "3"])[0]  # -i is required


def test_scrunch_params_errors_are_named():
    # nsub is checked against the file's channel count, once that is known
    for nsub in (24, 65, 128):
        with pytest.raises(C.NativeError, match="nsub must divide nchans"):
            C.scrunch_check_params(C.ScrunchParams(10.0, nsub, 1, 16.0), 64)
    for f in (0, 257):
        with pytest.raises(C.NativeError, match="tscrunch must be in 1..256"):
            C.scrunch_check_params(C.ScrunchParams(10.0, 8, f, 16.0), 64)
    with pytest.raises(C.NativeError, match="sigma_out must be positive"):
        C.scrunch_check_params(C.ScrunchParams(10.0, 8, 1, 0.0), 64)
    assert C.scrunch_check_params(C.ScrunchParams(10.0, 8, 256, 0.5), 64).nsub == 8


def test_offsets_equal_the_oracle():
    hdr = _header(64, 8)
    delays = _delays(hdr)
    for dm, nsub in ((0.0, 8), (100.0, 8), (100.0, 64), (33.3, 1), (700.0, 32)):
        rel, R = ref.scrunch_offsets(dm, delays, nsub)
        got, gR = C.scrunch_offsets(dm, [float(d) for d in delays], nsub)
        assert np.array_equal(rel, got) and R == gR and rel.dtype == np.int32
        assert (rel[::64 // nsub] == 0).all() and (rel >= 0).all()
    assert ref.scrunch_offsets(100.0, delays, 1)[1] == ref.dm_offsets([100.0], delays).max()


def _direct(vals, off, kill, n):
    """Plain integer dedispersion sum at offsets off over n samples."""
    s = np.zeros(n, dtype=np.int64)
    for c in np.nonzero(kill)[0]:
        s += vals[off[c]:off[c] + n, c].astype(np.int64)
    return s


def test_band_sum_identity_on_the_oracle():
    nchans, n, dm = 64, 6000, 100.0
    hdr = _header(nchans, 8)
    delays = _delays(hdr)
    vals = synthetic.generate(n, hdr, (), seed=2)
    kill = _kill(nchans, [3, 8, 40])
    off = ref.dm_offsets([dm], delays)[0].astype(np.int64)
    common = n - int(off.max())
    direct = _direct(vals, off, kill, common)
    # f = 1: the subbands' sums, each read at its first channel's offset, add up to the dedispersed series
    for nsub in (8, 32):
        rel, R = ref.scrunch_offsets(dm, delays, nsub)
        A, nactive, _, _ = ref.scrunch_sums(vals, rel, 1, nsub, kill)
        w = nchans // nsub
        assert A.shape == (nsub, n - R) and A.dtype == np.int64 and nactive.sum() == 61
        both = min(common, n - R - int(off[(nsub - 1) * w]))  # the range every subband's row covers
        assert both > 5000
        band = sum(A[s, off[s * w]:off[s * w] + both] for s in range(nsub))
        assert np.array_equal(band, direct[:both])
    # nsub = 1: A is that sum
    rel, R = ref.scrunch_offsets(dm, delays, 1)
    A, _, S1, S2 = ref.scrunch_sums(vals, rel, 1, 1, kill)
    assert R == off.max() and np.array_equal(A[0], direct)
    assert int(S1.sum()) == int(A.sum()) and int(S2[0, 0]) == int((A[0, :L] ** 2).sum())
    assert S1.shape == (1, -(-common // L))
    # dm = 0, nsub = nchans: A is the time-scrunched input
    for f in (1, 3, 4):
        rel, R = ref.scrunch_offsets(0.0, delays, nchans)
        A, nactive, _, _ = ref.scrunch_sums(vals, rel, f, nchans)
        nout = n // f
        assert R == 0 and A.shape == (nchans, nout) and (nactive == 1).all()
        assert np.array_equal(A, vals[:nout * f].astype(np.int64).reshape(nout, f, nchans).sum(axis=1).T)
    # nvalid: samples from nvalid on are not read
    a = ref.scrunch_sums(vals, rel, 4, nchans, nvalid=4001)[0]
    assert np.array_equal(a, ref.scrunch_sums(vals[:4001], rel, 4, nchans)[0])


def _scale_tables():
    """(name, A int64 [nsub, nout], nactive) whose block sums exercise the host step."""
    rng = np.random.default_rng(7)
    out = []
    nout = 5 * L + 777  # six blocks (an even count), the last short
    A = rng.integers(900, 1100, (5, nout)).astype(np.int64)
    A[1] = 1000                      # a dead subband: zero variance
    A[3] *= 3                        # another level and sigma
    A[4, 2 * L:3 * L] += rng.integers(0, 50000, L)  # an outlier block that must not move the medians
    out.append(("even-count-dead-killed-outlier", A, np.array([4, 4, 0, 4, 4], np.int32)))  # subband 2 killed
    out.append(("odd-count", A[:, :4 * L + 5].copy(), np.array([4, 4, 0, 4, 4], np.int32)))
    out.append(("one-short-block", rng.integers(0, 40, (3, 321)).astype(np.int64), np.array([1, 2, 3], np.int32)))
    out.append(("near-the-bound", (1 << 26) - 1 - rng.integers(0, 3, (2, L + 9)).astype(np.int64),
                np.array([9, 9], np.int32)))
    return out


@pytest.mark.parametrize("i", range(4), ids=[t[0] for t in _scale_tables()])
def test_scale_through_the_bindings_equals_the_oracle(i):
    name, A, nactive = _scale_tables()[i]
    S1, S2 = ref.scrunch_block_sums(A)
    nout = A.shape[1]
    for sigma_out in (16.0, 3.7, 1e-7, 1e8):
        exp = ref.scrunch_scale(S1, S2, nout, nactive, sigma_out)
        got = C.scrunch_scale(S1, S2, nout, nactive, sigma_out)
        assert np.array_equal(got["M"], exp["M"]) and np.array_equal(got["live"], exp["live"])
        assert got["mul"] == exp["mul"] and got["sigma_ref"] == exp["sigma_ref"] and got["nlive"] == exp["nlive"]
        assert 1 <= got["mul"] <= 2 ** 31 - 1
    if i == 0:
        assert list(exp["live"]) == [1, 0, 0, 1, 1]
        clean = A[4].copy()
        clean[2 * L:3 * L] = A[4, :L]
        s1, s2 = ref.scrunch_block_sums(np.stack([A[0], A[1], A[2], A[3], clean]))
        assert abs(int(ref.scrunch_scale(s1, s2, nout, nactive)["M"][4]) - int(exp["M"][4])) <= 1
        assert ref.scrunch_scale(S1, S2, nout, nactive, 1e-7)["mul"] == 1
        assert ref.scrunch_scale(S1, S2, nout, nactive, 1e8)["mul"] == 2 ** 31 - 1
    with pytest.raises(C.NativeError, match="no live subband"):
        C.scrunch_scale(S1, S2, nout, np.zeros(len(nactive), np.int32), 16.0)
    with pytest.raises(ValueError, match="no live subband"):
        ref.scrunch_scale(S1, S2, nout, np.zeros(len(nactive), np.int32), 16.0)


def test_plan_equals_the_oracle_and_tiers_are_contiguous():
    t = read_header(TUTORIAL)
    big = dict(tsamp=64e-6, fch1=1500.0, foff=-400.0 / 4096, nchans=4096)
    for h in (t, big):
        for dm_end in (0.0, 10.0, 300.0, 3000.0, 1e6):
            args = (float(h["tsamp"]), float(h["fch1"]), float(h["foff"]), int(h["nchans"]), dm_end)
            exp = ref.scrunch_plan(*args)
            got = [tuple(x) for x in C.scrunch_plan(*args)]
            assert got == exp and exp[0][0] == 0.0 and exp[-1][1] == dm_end
            assert [f for _, _, f in exp] == [1 << k for k in range(len(exp))] and exp[-1][2] <= 64
            assert all(a[1] == b[0] for a, b in zip(exp, exp[1:]))
    exp = ref.scrunch_plan(big["tsamp"], big["fch1"], big["foff"], big["nchans"], 1e6)
    assert len(exp) == 7 and exp[-1][2] == 64
    # the boundary of tier 2^k is where the smearing inside the lowest channel is 2^k samples
    nu = (1500.0 - 400.0 * 4095 / 4096) / 1000.0
    for lo, _, f in exp[1:]:
        assert 8.3e-6 * lo * (400.0 / 4096) / nu ** 3 == pytest.approx(f * 64e-6, rel=1e-12)


def test_header_rewrite_keeps_every_key(tmp_path):
    hdr = _header(64, 2)
    hdr.update(ibeam=3, nbeams=13, az_start=12.5, src_raj=123456.7, machine_id=9, telescope_id=4)
    vals = synthetic.generate(9000, hdr, (), seed=4)
    src, dst = str(tmp_path / "in.fil"), str(tmp_path / "out.fil")
    write_filterbank(src, hdr, vals)
    res = ref.scrunch_filterbank(src, dst, dm=56.5, nsub=16, f=4, sigma_out=16.0)
    assert not os.path.exists(dst + ".tmp")
    a, b = read_header(src), read_header(dst)
    assert set(a["_present"]) | {"refdm"} == set(b["_present"])
    changed = {"nchans": 16, "foff": 4 * a["foff"], "tsamp": 4 * a["tsamp"], "nbits": 8, "nsamples": res["nout"],
               "refdm": 56.5}
    for k in b["_present"]:
        assert b[k] == changed.get(k, a[k]), k
    assert b["fch1"] == a["fch1"] and res["nout"] == (9000 - res["R"]) // 4
    out = read_filterbank(dst)
    assert out.data.shape == (res["nout"], 16) and np.array_equal(out.data, res["y"].T)
    # the native reader agrees
    n = C.read_header(dst)
    assert (n["nchans"], n["nbits"], n["nsamples"], n["refdm"], n["foff"]) == (16, 8, res["nout"], 56.5, 4 * a["foff"])
    # without nsamples in the input the output has none either
    raw = open(src, "rb").read()
    from peasoup_amd.utils.sigproc import header_bytes
    h2 = {k: v for k, v in a.items() if k != "nsamples"}
    open(src, "wb").write(header_bytes(h2) + raw[a["size"]:])
    ref.scrunch_filterbank(src, dst, dm=56.5, nsub=16, f=4)
    assert "nsamples" not in read_header(dst)["_present"]
    write_filterbank(src, dict(hdr, foff=1.09), vals)
    with pytest.raises(ValueError, match="foff must be negative"):
        ref.scrunch_filterbank(src, dst)


def _run_native(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    return r


def test_native_unit_tests():
    _run_native(os.path.join(REPO, "bin", "psoup_scrunch_unit_tests"))


@pytest.mark.parametrize("san", ["address", "undefined"])
def test_native_unit_tests_under_host_sanitizers(san):
    """A stand-alone host binary built with the sanitizer, run in the inherited environment."""
    from peasoup_amd import _build

    _build.build(sanitize=san, sanitize_target="psoup_scrunch_unit_tests")
    r = _run_native(os.path.join(REPO, "bin", f"psoup_scrunch_unit_tests_{san}"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ----------------------------------------------------------------- sweep ----
# nbits (bias 128 for 8 bits, else 0), nchans, nsub, f, valid samples n, dm, killed channels.  "hdr": header
# overrides; "full": every sample is V.  Each case states what it guards.
LOW = dict(fch1=400.0, foff=-1.0)  # 8 channels at 400 MHz: 14.6 samples of delay per DM unit across them
SWEEP = [
    dict(id="f1-8bit-odd-rel-kill-ref-channel-ragged-blocks", nbits=8, nchans=64, nsub=8, f=1, n=20000, dm=100.0,
         kill=[8, 9, 33]),       # rel 0 / odd / not multiples of 16; c_s of subband 1 killed; nout = 4 L + a part
    dict(id="f2-2bit-nsub16", nbits=2, nchans=64, nsub=16, f=2, n=20001, dm=60.0, kill=None),
    dict(id="f3-nsub=nchans", nbits=8, nchans=64, nsub=64, f=3, n=20000, dm=50.0, kill=[5]),  # 3 does not divide a tile
    dict(id="f4-4bit-nsub1", nbits=4, nchans=64, nsub=1, f=4, n=20000, dm=75.0, kill=None),
    dict(id="f5-w2-killed-subband", nbits=8, nchans=64, nsub=32, f=5, n=20003, dm=200.0, kill=[10, 11, 40]),
    dict(id="f16-1bit-nout-below-L", nbits=1, nchans=64, nsub=8, f=16, n=20000, dm=30.0, kill=None),
    dict(id="f64-lane-groups", nbits=8, nchans=64, nsub=4, f=64, n=20011, dm=120.0, kill=[0]),
    dict(id="f256-whole-wave-halves", nbits=8, nchans=64, nsub=8, f=256, n=20000, dm=10.0, kill=None),
    dict(id="nout1", nbits=8, nchans=64, nsub=8, f=5, n="R+7", dm=100.0, kill=None),
    dict(id="nchans8-rel-above-16384", nbits=8, nchans=8, nsub=1, f=1, n=40000, dm=1500.0, kill=None, hdr=LOW),
    dict(id="nchans4096-2048-samples", nbits=2, nchans=4096, nsub=256, f=2, n=2048, dm=10.0, kill=[0, 17, 4095],
         hdr=dict(fch1=1500.0, foff=-400.0 / 4096)),
    dict(id="all-V-at-the-2^26-bound", nbits=8, nchans=1028, nsub=1, f=256, n=1000, dm=0.0, kill=None, full=True,
         hdr=dict(fch1=1500.0, foff=-0.1)),
]
PAD = 48  # samples of row padding past n, filled with a sentinel


@functools.lru_cache(maxsize=None)
def _sweep_case(i):
    """(values, rel, n, kill, bias, A, nactive, S1, S2) of SWEEP[i], computed once."""
    c = SWEEP[i]
    hdr = _header(c["nchans"], c["nbits"], **c.get("hdr", {}))
    delays = _delays(hdr)
    rel, R = ref.scrunch_offsets(c["dm"], delays, c["nsub"])
    n = R + 7 if c["n"] == "R+7" else c["n"]
    kill = None if c["kill"] is None else _kill(c["nchans"], c["kill"])
    if c.get("full"):
        vals = np.full((n, c["nchans"]), (1 << c["nbits"]) - 1, dtype=np.uint8)
    else:
        vals = synthetic.generate(n, hdr, (), seed=51 + i)
    vals.setflags(write=False)
    A, nactive, S1, S2 = ref.scrunch_sums(vals, rel, c["f"], c["nsub"], kill)
    return vals, rel, n, kill, 128 if c["nbits"] == 8 else 0, A, nactive, S1, S2


def test_sweep_covers_what_it_must():
    """The properties the shape sweep has to contain, checked on the CPU from the oracle alone."""
    seen = set()
    for i, c in enumerate(SWEEP):
        vals, rel, n, kill, bias, A, nactive, S1, S2 = _sweep_case(i)
        f, nout, w = c["f"], A.shape[1], c["nchans"] // c["nsub"]
        V = (1 << c["nbits"]) - 1
        assert V * f * int(nactive.max()) < 2 ** 26 and A.max() < 2 ** 26
        seen.add(("f", f))
        seen.add(("bits", c["nbits"]))
        tile = C.scrunch_tile_at(f)
        if nout % tile and nout % L and nout > L:
            seen.add("ragged")
        if nout < L:
            seen.add("below-L")
        if nout == 1:
            seen.add("nout1")
        if C.scrunch_tile() % f:
            seen.add("f-not-dividing-tile")
        if (rel % 2 == 1).any() and (rel % 16 != 0).any() and (rel == 0).sum() >= c["nsub"]:
            seen.add("odd-rel")
        if rel.max() > 16384:
            seen.add("big-rel")
        seen.add(("nsub", "all" if c["nsub"] == c["nchans"] else c["nsub"]))
        if w == 2:
            seen.add("w2")
        seen.add(("nchans", c["nchans"]))
        if kill is not None and (kill[::w] == 0).any() and nactive.min() > 0:
            seen.add("ref-channel-killed")
        if (nactive == 0).any():
            seen.add("dead-subband")
            assert not A[int(np.argmin(nactive))].any()
        if c.get("full") and V * f * int(nactive.max()) + V * f >= 2 ** 26:
            seen.add("at-the-bound")  # one more channel would break it
            assert (A == V * f * nactive.max()).all()
    need = {("f", f) for f in (1, 2, 3, 4, 5, 16, 64, 256)} | {("bits", b) for b in (1, 2, 4, 8)} | {
        "ragged", "below-L", "nout1", "f-not-dividing-tile", "odd-rel", "big-rel", ("nsub", "all"), ("nsub", 1), "w2",
        ("nchans", 8), ("nchans", 4096), "ref-channel-killed", "dead-subband", "at-the-bound"}
    assert need <= seen, need - seen
    assert SWEEP[10]["n"] == 2048


# ------------------------------------------------------------------- GPU ----
def _device_rows(values, nbits, bias, sentinel=127):
    """values [n, nchans] raw -> int8 [nchans, stride] on the device through unpack_transpose, the padding
    [n, stride) of every row filled with `sentinel`."""
    import torch

    from peasoup_amd import ops
    from peasoup_amd.utils.sigproc import pack_samples

    n, nchans = values.shape
    packed = torch.from_numpy(pack_samples(values, nbits)).cuda()
    stride = (n + PAD + 15) // 16 * 16
    rows = ops.unpack_transpose(packed, n, nchans, nbits, bias, stride)
    rows[:, n:] = sentinel
    return rows


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c["id"] for c in SWEEP])
def test_scrunch_sums_equal_oracle(i):
    import torch

    from peasoup_amd import ops

    c = SWEEP[i]
    vals, rel, n, kill, bias, A, nactive, S1, S2 = _sweep_case(i)
    first = None
    for sentinel in (127, -128):
        rows = _device_rows(vals, c["nbits"], bias, sentinel)
        gA, g1, g2 = ops.scrunch_sums(rows, n, rel, c["f"], c["nsub"], A.shape[1], bias=bias, killmask=kill)
        assert gA.dtype == torch.int32 and tuple(gA.shape) == A.shape
        assert torch.equal(gA.cpu().to(torch.int64), torch.from_numpy(A))
        assert np.array_equal(_u64(g1), S1) and np.array_equal(_u64(g2), S2)
        if first is None:
            first = (gA.clone(), g1.clone(), g2.clone())
    # determinism, and independence of the padding
    assert all(torch.equal(a, b) for a, b in zip(first, (gA, g1, g2)))


@pytest.mark.gpu
def test_scrunch_quant_equals_oracle_with_explicit_tables():
    import torch

    from peasoup_amd import ops

    rng = np.random.default_rng(3)
    nsub, nout = 5, 4133  # more than one workgroup per row, a ragged tail
    M = np.array([1000, 0, 70000, 5, 12345], np.int32)
    A = (M[:, None] + rng.integers(-400, 400, (nsub, nout))).astype(np.int64)
    A[0, :8] = M[0] + np.array([1, -1, 3, -3, 255, -255, 257, -257])  # x mul 32768: exactly .5 on both signs
    A[1, :4] = [0, 1, 2 ** 26 - 1, 3]
    A[2, :4] = [0, 2 ** 26 - 1, 70000, 69999]   # saturation at 0 and at 255
    live = np.array([1, 1, 1, 0, 1], np.uint8)  # subband 3 is not live
    for mul in (32768, 1, 2 ** 31 - 1, 65536, 41234567):
        exp = ref.scrunch_quant(A, M, mul, live)
        got = ops.scrunch_quant(torch.from_numpy(A.astype(np.int32)).cuda(), M, mul, live)
        assert got.dtype == torch.int8 and got.shape[1] % 16 == 0 and got.data_ptr() % 16 == 0
        y = (got[:, :nout].cpu().numpy().astype(np.int16) + 128).astype(np.uint8)
        assert np.array_equal(y, exp), mul
        assert (y[3] == 128).all()
    exp = ref.scrunch_quant(A, M, 32768, live)
    assert list(exp[0, :8]) == [129, 128, 130, 127, 255, 1, 255, 0]  # .5 rounds up on both signs
    exp = ref.scrunch_quant(A, M, 2 ** 31 - 1, live)
    assert exp[2, 0] == 0 and exp[2, 1] == 255 and exp[2, 2] == 128
    assert (ref.scrunch_quant(A, M, 1, live) == 128).sum() > nsub * nout * 0.9
    # the rows feed pack_transpose as they are
    packed = ops.pack_transpose(got, nout, 8, 128)
    assert np.array_equal(packed.cpu().numpy().reshape(nout, nsub), ref.scrunch_quant(A, M, 41234567, live).T)


def _oracle_run(vals, hdr, dm, nsub, f, kill, sigma_out=16.0):
    rel, R = ref.scrunch_offsets(dm, _delays(hdr), nsub)
    A, nactive, S1, S2 = ref.scrunch_sums(vals, rel, f, nsub, kill)
    sc = ref.scrunch_scale(S1, S2, A.shape[1], nactive, sigma_out)
    return A, S1, S2, sc, ref.scrunch_quant(A, sc["M"], sc["mul"], sc["live"])


@pytest.mark.gpu
def test_chunked_run_equals_one_chunk_and_the_oracle():
    from peasoup_amd import ops

    nchans, n, nsub, f, dm = 64, 20000, 8, 1, 100.0
    hdr = _header(nchans, 8)
    vals = synthetic.generate(n, hdr, (), seed=12)
    kill = _kill(nchans, [2, 16, 17, 18, 19, 20, 21, 22, 23])  # subband 2 entirely killed
    A, S1, S2, sc, y = _oracle_run(vals, hdr, dm, nsub, f, kill)
    rows = _device_rows(vals, 8, 128)
    args = (rows, n, 8, _delays(hdr), dm, nsub, f, 16.0, 128, kill, hdr["foff"])
    y1, r1 = ops.scrunch(*args)
    yc, rc = ops.scrunch(*args, budget_bytes=4 * nsub * L)  # one statistics block per chunk
    nout = A.shape[1]
    assert r1["chunks"] == 1 and rc["chunks"] == -(-nout // L) >= 3 and r1["nout"] == rc["nout"] == nout
    assert r1["launches"] == 2 and rc["launches"] == 3 * rc["chunks"]  # one chunk keeps its sums
    for r in (r1, rc):
        assert np.array_equal(r["S1"], S1) and np.array_equal(r["S2"], S2)
        assert np.array_equal(r["M"], sc["M"]) and r["mul"] == sc["mul"] and np.array_equal(r["live"], sc["live"])
        assert list(r["killmask"]) == [1, 1, 0, 1, 1, 1, 1, 1] and r["sigma_ref"] == sc["sigma_ref"]
    for got in (y1, yc):
        assert np.array_equal((got[:, :nout].cpu().numpy().astype(np.int16) + 128).astype(np.uint8), y)
    assert (y[2] == 128).all() and abs(float(y[0].std()) - 16.0) < 2.0


@pytest.mark.gpu
def test_refusals_are_named_and_nothing_is_launched():
    import torch

    from peasoup_amd import ops

    nchans, n = 64, 6000
    hdr = _header(nchans, 8)
    delays = [float(d) for d in _delays(hdr)]
    vals = synthetic.generate(n, hdr, (), seed=13)
    rows = _device_rows(vals, 8, 128)
    s = torch.cuda.current_stream().cuda_stream

    def make(nsamps=n, nbits=8, foff=hdr["foff"], kill=(), p=C.ScrunchParams(100.0, 8, 1, 16.0), r=rows, nch=nchans,
             dl=delays):
        return C.Scruncher(r.data_ptr(), r.shape[1], nsamps, nch, nbits, 128 if nbits == 8 else 0, foff, dl,
                           list(kill), p, s)

    # the constructor validates and launches nothing; a refused one leaves no object to launch from
    with pytest.raises(C.NativeError, match="foff must be negative"):
        make(foff=1.09)
    R = ref.scrunch_offsets(100.0, _delays(hdr), 1)[1]
    with pytest.raises(C.NativeError, match="nout < 1"):
        make(nsamps=R + 3, p=C.ScrunchParams(100.0, 1, 4, 16.0))
    assert make(nsamps=R + 4, p=C.ScrunchParams(100.0, 1, 4, 16.0)).nout == 1
    with pytest.raises(C.NativeError, match="2\\^26 bound"):
        make(p=C.ScrunchParams(0.0, 1, 256, 16.0), nch=1029, dl=[0.0] * 1029)  # 255 x 256 x 1029 >= 2^26
    with pytest.raises(C.NativeError, match="no live subband"):
        make(kill=[0] * nchans)
    with pytest.raises(C.NativeError, match="nsub must divide nchans"):
        make(p=C.ScrunchParams(100.0, 24, 1, 16.0))
    ok = make()
    assert ok.launches == 0 and ok.nout == n - ref.scrunch_offsets(100.0, _delays(hdr), 8)[1]
    # constant data: no subband has variance; refused by name after the sums, nothing is requantised
    flat = _device_rows(np.full((n, nchans), 9, np.uint8), 8, 128)
    scr = make(r=flat)
    y = torch.full((8, (scr.nout + 255) // 256 * 256), 77, dtype=torch.int8, device="cuda")
    with pytest.raises(C.NativeError, match="no live subband"):
        scr.run(y.data_ptr(), y.shape[1])
    assert scr.launches == 1 and bool((y == 77).all())
    # the raw kernels refuse reads past the rows
    with pytest.raises(C.NativeError, match="read past the rows"):
        ops.scrunch_sums(rows, n, np.zeros(nchans, np.int32), 4, 8, n // 4 + 1, bias=128)


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("nbits", [2, 8])
def test_cli_module_and_oracle_write_identical_files(tmp_path, nbits):
    nchans, nsamps = 64, 20000
    hdr = _header(nchans, nbits)
    hdr["ibeam"] = 2
    fil = str(tmp_path / "a.fil")
    synthetic.write(fil, nsamps, hdr, (), seed=21)
    kill = _kill(nchans, [4, 5, 6, 7, 30])  # subband 1 entirely killed
    killf = tmp_path / "kill.txt"
    killf.write_text("".join(f"{k}\n" for k in kill))
    flags = ["-i", fil, "-k", str(killf), "--dm", "56.5", "--nsub", "16", "--tscrunch", "4"]
    out = {k: (str(tmp_path / f"{k}.fil"), str(tmp_path / f"{k}.kill")) for k in ("native", "module", "oracle")}
    r = _run([os.path.join(REPO, "bin", "filscrunch")] + flags + ["-o", out["native"][0], "--kill_out",
                                                                  out["native"][1], "-v"])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "scrunch"] + flags + ["-o", out["module"][0], "--kill_out",
                                                                     out["module"][1]], env=env, cwd=REPO)
    res = ref.scrunch_filterbank(fil, out["oracle"][0], dm=56.5, nsub=16, f=4, killmask=kill,
                                 kill_out=out["oracle"][1])
    a = open(out["native"][0], "rb").read()
    assert a == open(out["module"][0], "rb").read()
    assert a == open(out["oracle"][0], "rb").read()
    k = open(out["native"][1]).read()
    assert k == open(out["module"][1]).read() == open(out["oracle"][1]).read()
    assert k.split() == ["1", "0"] + ["1"] * 14
    assert f"mul {res['mul']}," in r.stdout and "15 of 16 subbands live" in r.stdout
    assert "M: " + " ".join(str(int(m)) for m in res["M"]) in r.stdout
    h = read_header(out["native"][0])
    assert (h["nchans"], h["nbits"], h["nsamples"], h["refdm"], h["ibeam"]) == (16, 8, res["nout"], 56.5, 2)
    # --plan reads no data and prints the oracle's tiers
    p = _run([os.path.join(REPO, "bin", "filscrunch"), "-i", fil, "--plan", "--dm_end", "3000"])
    exp = ref.scrunch_plan(hdr["tsamp"], hdr["fch1"], hdr["foff"], nchans, 3000.0)
    assert p.stdout == "".join(f"{lo:.6f} {hi:.6f} {f}\n" for lo, hi, f in exp)
    pm = _run([sys.executable, "-m", "peasoup_amd", "scrunch", "-i", fil, "--plan", "--dm_end", "3000"], env=env,
              cwd=REPO)
    assert pm.stdout == p.stdout
    # a refusal reaches the command line by name
    bad = subprocess.run([os.path.join(REPO, "bin", "filscrunch"), "-i", fil, "--nsub", "24", "-o",
                          str(tmp_path / "bad.fil")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "nsub must divide nchans" in bad.stderr
    assert not os.path.exists(str(tmp_path / "bad.fil"))


# An injected burst at DM 100 in 64 channels of 8 bits; scrunched at that DM to 16 subbands and a quarter of the
# sample rate, it must come out of a plain dedispersion of the scrunched file at the same DM.
R_N = 1 << 15
R_DM = 100.0
R_NSUB, R_F = 16, 4
R_BURST = synthetic.BurstSpec(time=0.8, dm=R_DM, width=16 * TSAMP, amplitude=1.0)


@functools.lru_cache(maxsize=None)
def _recovery_values():
    hdr = _header(64, 8)
    return hdr, synthetic.generate(R_N, hdr, (), seed=41, bursts=[R_BURST])


def _recovered_peak(y):
    """y uint8 [nsub, nout]: the scrunched values dedispersed at R_DM with the output's own delay table
    (the direct dedispersion oracle): (index of the maximum, the series)."""
    hdr, _ = _recovery_values()
    w = 64 // R_NSUB
    delays = ref.delay_table(R_NSUB, R_F * hdr["tsamp"], hdr["fch1"], w * hdr["foff"])
    series = ref.dedisperse(np.ascontiguousarray(y.T), ref.dm_offsets([R_DM], delays), 8)[0]
    return int(np.argmax(series)), series.astype(np.float64)


def test_recovery_seed_on_the_oracle():
    hdr, vals = _recovery_values()
    _, _, _, sc, y = _oracle_run(vals, hdr, R_DM, R_NSUB, R_F, None)
    k, series = _recovered_peak(y)
    assert abs(k - R_BURST.time / TSAMP / R_F) <= 1
    rest = np.delete(series, np.arange(k - 8, k + 9))
    assert series[k] > rest.max() + 5 * rest.std()  # with margin
    assert sc["nlive"] == R_NSUB and abs(float(y[0].std()) - 16.0) < 2.0


@pytest.mark.gpu
def test_recovers_a_burst_from_the_scrunched_file():
    from peasoup_amd import ops

    hdr, vals = _recovery_values()
    rows = _device_rows(vals, 8, 128)
    got, res = ops.scrunch(rows, R_N, 8, _delays(hdr), R_DM, R_NSUB, R_F, 16.0, 128, None, hdr["foff"])
    nout = int(res["nout"])
    y = (got[:, :nout].cpu().numpy().astype(np.int16) + 128).astype(np.uint8)
    assert np.array_equal(y, _oracle_run(vals, hdr, R_DM, R_NSUB, R_F, None)[4])
    k, _ = _recovered_peak(y)
    assert abs(k - R_BURST.time / TSAMP / R_F) <= 1
