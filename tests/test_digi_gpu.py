"""fildigi on the GPU (see test_digi.py): every comparison is exact equality
with the NumPy oracle of peasoup_amd.utils.reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import read_header, write_raw_filterbank
from test_digi import (E_BURST, E_N, L, SP_THRESHOLD, SWEEP_CHANS, SWEEP_SAMPS, SWEEP_TYPES, _digi_oracle, _e2e_values,
                       _float_case, _header, _int_case, _sweep_case)

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()   # a copy: the shared cases are read-only


@pytest.mark.parametrize("kind", SWEEP_TYPES)
def test_digi_block_sums_equal_oracle(kind):
    from peasoup_amd import ops

    for nchans in SWEEP_CHANS:
        for nsamps in SWEEP_SAMPS:
            x, exp = _sweep_case(kind, nsamps, nchans)
            got = ops.digi_block_sums(_dev(x))
            where = (kind, nchans, nsamps)
            assert np.array_equal(got["N"].cpu().numpy(), exp["N"].astype(np.int64)), where
            assert np.array_equal(got["S1"].cpu().numpy(), exp["S1"]), where
            assert np.array_equal(got["S2"].cpu().numpy().view(np.uint64), exp["S2"]), where
            assert np.array_equal(got["E"].cpu().numpy(), exp["E"]), where
            assert np.array_equal(got["nbad"].cpu().numpy().astype(np.uint64), exp["nbad"]), where


def _quant_case(kind, nchans):
    """Samples [2 L + 37, nchans] and tables for J = 2 (intervals of 2 and 1 blocks) that put exact .5 ties,
    both clamps, a dead channel, a killed channel and non-finite samples in front of the kernel."""
    rng = np.random.default_rng(nchans)
    nsamps = 2 * L + 37
    dt = np.dtype(kind)
    if kind == "float32":
        x = rng.integers(-300, 300, (nsamps, nchans)).astype(np.float32)
        x[rng.integers(0, nsamps, 40), rng.integers(0, nchans, 40)] = np.nan
        x[rng.integers(0, nsamps, 40), rng.integers(0, nchans, 40)] = np.inf
        x[rng.integers(0, nsamps, 40), rng.integers(0, nchans, 40)] = -np.inf
    else:
        info = np.iinfo(dt)
        x = rng.integers(max(info.min, -300), min(info.max, 600) + 1, (nsamps, nchans)).astype(dt)
    mean = rng.integers(-5, 50, (2, nchans)).astype(np.float64)
    gain = np.full((2, nchans), 0.5)              # (x - mean) / 2: n + 0.5 for every odd difference
    gain[:, 1 % nchans] = 1000.0                  # both clamps
    gain[1, 2 % nchans] = 0.25
    if nchans > 4:
        gain[:, 3] = 0.0                          # dead or killed: not live anywhere
        gain[1, 4] = 0.0                          # not live in the last interval
        mean[:, 4] += 0.5                         # no ties here: the differences are n + 0.5 before the gain
    return x, mean, gain


@pytest.mark.parametrize("kind", SWEEP_TYPES)
def test_digi_quant_equals_oracle_with_explicit_tables(kind):
    from peasoup_amd import ops

    for nchans in (1, 7, 64, 130):   # scalar gathers (odd rows) and 16-byte groups; more than one workgroup
        x, mean, gain = _quant_case(kind, nchans)
        d = _dev(x)
        j = np.arange(x.shape[0]) // L // 2
        with np.errstate(invalid="ignore"):
            p = (x.astype(np.float64) - mean[j]) * gain[j]
            assert (np.isfinite(p) & (p % 1 == 0.5)).sum() > 0   # exact .5 ties, from the tables
        for flip in (False, True):
            exp, nclip = ref.digi_quant(x, mean, gain, 2, flip)
            got, gclip = ops.digi_quant(d, mean, gain, 2, flip)
            assert tuple(got.shape) == x.shape and np.array_equal(got.cpu().numpy(), exp), (kind, nchans, flip)
            assert gclip == nclip and nclip > 0
            assert {0, 255} <= set(np.unique(exp[:, (nchans - 1 - 1 % nchans) if flip else 1 % nchans]))
        if nchans > 4:
            assert (exp[:, nchans - 1 - 3] == 128).all() and (exp[2 * L:, nchans - 1 - 4] == 128).all()
            assert not (exp[:2 * L, nchans - 1 - 4] == 128).all()
    # half to even on both signs, from the tables
    x = np.array([[11], [13], [15], [7], [5], [3]], dtype=np.float32 if kind == "float32" else np.int8).astype(kind)
    y, _ = ops.digi_quant(_dev(x), np.array([[10.0]]), np.array([[0.5]]))
    assert y.cpu().numpy()[:, 0].tolist() == [128, 130, 130, 126, 126, 124] == ref.digi_quant(x, [[10.0]], [[0.5]])[0][:, 0].tolist()


@pytest.mark.parametrize("kind", ["float32", "uint16"])
def test_chunked_run_equals_one_chunk_and_the_oracle(kind):
    from peasoup_amd import ops

    nsamps, nchans = 3 * L + 100, 65
    x = _float_case(nsamps, nchans, seed=9) if kind == "float32" else _int_case(np.uint16, nsamps, nchans, 9)
    if kind == "uint16":
        x = (x // 16 + np.arange(nchans, dtype=np.uint16) * 50).astype(np.uint16)
        x[:, 2] = (x[:, 2] % 40)
    kill = [1] * nchans
    kill[10] = 0
    for foff, mode, J in ((+0.5, "channel", 2), (-0.5, "file", 0)):
        s, sc, y, nclip = _digi_oracle(x, foff, kill, 12.0, mode, J)
        y1, r1 = ops.digitise(x, foff, 12.0, mode, J, kill)
        yc, rc = ops.digitise(x, foff, 12.0, mode, J, kill, budget_bytes=1)   # one statistics block per chunk
        assert r1["chunks"] == 1 and rc["chunks"] == 4 and rc["chunk_samples"] == L
        assert r1["launches"] == 2 and rc["launches"] == 8
        for yy, r in ((y1, r1), (yc, rc)):
            for k in ("N", "S1", "S2", "E", "nbad"):
                assert np.array_equal(r[k], s[k]), k
            for k in ("mean", "gain", "live"):
                assert np.array_equal(r[k], sc[k]), k
            assert r["nclip"] == nclip and r["flip"] == (foff > 0) and r["nlive"] == sc["nlive"]
            alive = list(sc["alive"][::-1] if foff > 0 else sc["alive"])
            assert list(r["killmask"]) == alive and alive[(nchans - 1 - 10) if foff > 0 else 10] == 0
            assert yy.dtype == np.uint8 and np.array_equal(yy, y)


def test_refusals_are_named_and_nothing_is_launched():
    import torch

    s = torch.cuda.current_stream().cuda_stream
    x = _float_case(L + 5, 7, seed=4)
    raw = x.reshape(-1).view(np.uint8)

    def make(data=raw, nbits=32, nsamps=L + 5, nchans=7, foff=-1.0, kill=(), p=None):
        return C.Digitiser(data, nbits, False, nsamps, nchans, foff, list(kill), p or C.DigiParams(), s)

    with pytest.raises(C.NativeError, match="nbits must be 8, 16 or 32"):
        make(nbits=4)
    with pytest.raises(C.NativeError, match="foff must not be zero"):
        make(foff=0.0)
    with pytest.raises(C.NativeError, match="sigma_out must be positive"):
        make(p=C.DigiParams(0.0, "channel", 0))
    with pytest.raises(C.NativeError, match="rescale_blocks must be non-negative"):
        make(p=C.DigiParams(16.0, "channel", -2))
    with pytest.raises(C.NativeError, match="shorter than one sample"):
        make(nsamps=0)
    with pytest.raises(C.NativeError, match="no live channel"):
        make(kill=[0] * 7)
    with pytest.raises(C.NativeError, match="killmask size"):
        make(kill=[1] * 6)
    with pytest.raises(C.NativeError, match="smaller than nsamps x nchans"):
        make(nsamps=L + 6)
    with pytest.raises(C.NativeError, match="nifs must be 1"):
        C.digi_check_header(32, 0, 4, -1.0, 7)
    ok = make()
    assert ok.launches == 0 and ok.chunk_samples >= L
    # constant data: no channel has variance; refused by name after the sums, nothing is requantised
    flat = C.Digitiser(np.full(3 * 5000, 9, np.uint8), 8, False, 5000, 3, 1.0, [], C.DigiParams(), s)
    with pytest.raises(C.NativeError, match="no live channel"):
        flat.run()
    assert flat.launches == 1


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


CLI_CASES = [
    dict(id="float32-ascending", kind="float32", ascending=True, flags=[]),
    dict(id="uint16-descending", kind="uint16", ascending=False, flags=[]),
    dict(id="scale-file", kind="float32", ascending=False, flags=["--scale", "file", "--sigma_out", "9.5"]),
    dict(id="rescale-blocks-2", kind="uint16", ascending=True, flags=["--rescale_blocks", "2"]),
]


@pytest.mark.parametrize("case", CLI_CASES, ids=[c["id"] for c in CLI_CASES])
def test_cli_module_and_oracle_write_identical_files(tmp_path, case):
    nchans, nsamps = 64, 3 * L + 500
    hdr = _header(nchans)
    hdr["ibeam"] = 2
    vals = synthetic.generate(nsamps, hdr, (), seed=31)
    h, x = synthetic.as_raw(vals, hdr, case["kind"], decades=3.0, drift=0.3, ascending=case["ascending"], seed=5)
    if case["kind"] == "float32":
        x[100:140, 7] = np.nan
    x[:, 20] = 3                      # a dead channel
    fil = str(tmp_path / "a.fil")
    write_raw_filterbank(fil, h, x)
    kill = [1] * nchans
    kill[5] = kill[6] = 0
    killf = tmp_path / "kill.txt"
    killf.write_text("".join(f"{k}\n" for k in kill))
    flags = ["-i", fil, "-k", str(killf)] + case["flags"]
    out = {k: (str(tmp_path / f"{k}.fil"), str(tmp_path / f"{k}.kill")) for k in ("native", "module", "oracle")}
    r = _run([os.path.join(REPO, "bin", "fildigi")] + flags + ["-o", out["native"][0], "--kill_out", out["native"][1],
                                                               "-v"])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "digi"] + flags + ["-o", out["module"][0], "--kill_out",
                                                                  out["module"][1]], env=env, cwd=REPO)
    f = case["flags"]
    res = ref.digi_filterbank(fil, out["oracle"][0], sigma_out=float(f[f.index("--sigma_out") + 1]) if "--sigma_out" in f
                              else 16.0, scale="file" if "file" in f else "channel",
                              J=2 if "--rescale_blocks" in f else 0, killmask=kill, kill_out=out["oracle"][1])
    a = open(out["native"][0], "rb").read()
    assert a == open(out["module"][0], "rb").read()
    assert a == open(out["oracle"][0], "rb").read()
    k = open(out["native"][1]).read()
    assert k == open(out["module"][1]).read() == open(out["oracle"][1]).read()
    dead = sorted((nchans - 1 - c) if case["ascending"] else c for c in (5, 6, 20))
    assert [i for i, v in enumerate(k.split()) if v == "0"] == dead
    nbad = 40 if case["kind"] == "float32" else 0
    assert f"nbad {nbad}, nclip {res['nclip']}, 61 of 64 channels live" in r.stdout
    o = read_header(out["native"][0])
    assert (o["nchans"], o["nbits"], o["nsamples"], o["ibeam"], o["foff"]) == (nchans, 8, nsamps, 2, hdr["foff"])
    assert o["fch1"] == pytest.approx(hdr["fch1"], abs=1e-9)   # flipped twice: 1510 + 63 foff - 63 foff
    assert C.Filterbank.from_file(out["native"][0]).nsamps == nsamps
    if case["id"] == "float32-ascending":
        # a refusal reaches the command line by name and writes nothing
        write_raw_filterbank(fil, dict(h, nifs=2), x)
        bad = subprocess.run([os.path.join(REPO, "bin", "fildigi"), "-i", fil, "-o", str(tmp_path / "bad2.fil")],
                             capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "nifs must be 1" in bad.stderr and not os.path.exists(str(tmp_path / "bad2.fil"))


def test_spsearch_recovers_a_burst_after_fildigi(tmp_path):
    """64 channels x 2^16 samples at 1 ms with one burst (DM 25, FWHM 8 ms, 1.5 sigma per channel) as a float32
    ascending-band file with gains over four decades, offsets and a drifting baseline: Filterbank refuses it;
    after fildigi, spsearch's strongest candidate is the burst."""
    hdr, h, x = _e2e_values()
    src, dst, out = str(tmp_path / "f32.fil"), str(tmp_path / "u8.fil"), str(tmp_path / "sp.txt")
    write_raw_filterbank(src, h, x)
    with pytest.raises(C.NativeError, match=r"unsupported nbits=32 \(1/2/4/8 supported\)"):
        C.Filterbank.from_file(src)
    _run([os.path.join(REPO, "bin", "fildigi"), "-i", src, "-o", dst, "--rescale_blocks", "4"])
    _, _, y, _ = _digi_oracle(x, h["foff"], None, J=4)
    assert open(dst, "rb").read()[read_header(dst)["size"]:] == y.tobytes()
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", dst, "--dm_start", "0", "--dm_end", "50", "-t", "1", "-o", out])
    assert ok
    res = C.run_sp_pipeline(a)
    assert res.candidates, "no single-pulse candidates"
    best = res.candidates[0]
    dms = np.asarray(res.dm_list)
    assert best.dm_idx == int(np.argmin(np.abs(dms - E_BURST.dm)))
    assert abs(best.time_s - E_BURST.time) / hdr["tsamp"] <= best.width
    assert best.snr > SP_THRESHOLD and E_N == x.shape[0]
