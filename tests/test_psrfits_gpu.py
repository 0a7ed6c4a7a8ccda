"""fits2fil on the GPU (see test_psrfits.py): every comparison is exact equality
with the NumPy oracle of peasoup_amd.utils.reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import psrfits as pf
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import synthetic
from peasoup_amd.utils.sigproc import read_header
from test_digi import E_BURST, E_N, E_SEED, SP_THRESHOLD, _header
from test_psrfits import (KINDS, L, NAN, SLOT_ROW, TOOL_NSAMPS, Z, bits, contraction_case, decode_case, decode_shapes,
                          tool_case)

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()   # a copy: the shared cases are read-only


def _decode_both(raw, scl, offs, wts, nbits, signed, pols, z, ranges):
    from peasoup_amd import ops

    nrows, nsblk, npol, nchan = raw.shape
    data = _dev(pf.pack_samples(raw, nbits).reshape(nrows, -1))
    d_scl, d_offs, d_wts = _dev(scl), _dev(offs), _dev(wts)
    exp = ref.fits_decode(raw, scl, offs, wts, SLOT_ROW, pols, z)
    for t0, count in ranges:
        got = ops.fits_decode(data, d_scl, d_offs, d_wts, SLOT_ROW, nsblk, nbits, signed, pols, z, t0, count)
        assert tuple(got.shape) == (count, nchan)
        yield t0, count, bits(got.cpu().numpy()), bits(exp[t0:t0 + count])


@pytest.mark.parametrize("kind", KINDS, ids=[f"{b}{'s' if s else 'u'}" for b, s in KINDS])
def test_fits_decode_equals_oracle(kind):
    nbits, signed = kind
    for nchan, npol, ptype, pol, nsblk in decode_shapes(nbits):
        raw, scl, offs, wts = decode_case(nbits, signed, nchan, npol, nsblk)
        pols = ref.fits_pols(npol, ptype, pol)
        assert tuple(C.fits_pols(npol, ptype, pol)) == pols
        nsamps = len(SLOT_ROW) * nsblk
        ranges = [(0, nsamps)]
        if nsamps > 12:
            ranges.append((10, nsamps - 10 - max(1, nsblk // 3)))     # starts and ends inside a row
        for t0, count, got, exp in _decode_both(raw, scl, offs, wts, nbits, signed, pols, Z, ranges):
            where = (kind, nchan, npol, ptype, pol, nsblk, t0, count)
            assert np.array_equal(got, exp), (where, int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
        assert (exp[-1:, :] != NAN).any()


def test_fits_decode_is_not_contracted():
    """The input of test_psrfits.test_contraction_guard, on which a fused multiply-add gives other bits."""
    raw, scl, offs, wts, z = contraction_case()
    nsamps = len(SLOT_ROW) * raw.shape[1]
    for pols in ((0, -1), (0, 1)):
        for t0, count, got, exp in _decode_both(raw, scl, offs, wts, 8, False, pols, z, [(0, nsamps)]):
            assert np.array_equal(got, exp), (pols, int((got != exp).sum()))


@pytest.mark.parametrize("mode", [("channel", 1), ("file", 0)], ids=["channel-J1", "file-J0"])
def test_fits_digitise_equals_oracle_in_one_chunk_and_block_by_block(mode):
    from peasoup_amd import ops

    scale, J = mode
    b, raw, kw = tool_case()
    kill = [1] * 72
    kill[40] = 0
    exp = ref.fits_filterbank(b, sigma_out=12.0, scale=scale, J=J, killmask=kill, rawdatafile="t.sf")
    nblk = -(-TOOL_NSAMPS // L)
    for budget, chunks, launches in ((None, 1, 3), (1, nblk, 4 * nblk)):
        y, r = ops.fits_digitise(b, 12.0, scale, J, kill, rawdatafile="t.sf", budget_bytes=budget)
        assert (r["chunks"], r["launches"]) == (chunks, launches) and (budget is None or r["chunk_samples"] == L)
        assert y.dtype == np.uint8 and y.shape == (TOOL_NSAMPS, 72) and np.array_equal(y, exp["y"])
        for k in ("N", "S1", "S2", "E", "nbad", "mean", "gain", "live"):
            assert np.array_equal(r[k], exp[k]), k
        assert r["nclip"] == exp["nclip"] and r["flip"] and list(r["killmask"]) == exp["killmask"]
        assert r["killmask"][71 - 40] == 0 and r["killmask"][71 - 9] == 0 and sum(r["killmask"]) == 70
        assert int(r["nbad"].sum()) == int(exp["nbad"].sum()) > 0
        assert (r["rows"], r["ndropped"], tuple(r["pols"]), r["z"]) == (8, 1, (0, 1), 0.0)
        assert r["header"]["bytes"] == exp["header_bytes"]


def test_refusals_before_anything_is_launched():
    import torch

    s = torch.cuda.current_stream().cuda_stream
    b, _, _ = tool_case()
    arr = np.frombuffer(b, np.uint8)

    def make(data=arr, opt=None, kill=(), p=None):
        return C.FitsDigitiser(data, opt or C.FitsOptions(), list(kill), p or C.DigiParams(), "", s)

    with pytest.raises(C.NativeError, match="not below NPOL"):
        make(opt=C.FitsOptions(pol=2))
    with pytest.raises(C.NativeError, match="sigma_out must be positive"):
        make(p=C.DigiParams(0.0, "channel", 0))
    with pytest.raises(C.NativeError, match="killmask size"):
        make(kill=[1] * 71)
    only9 = [0] * 72
    only9[9] = 1                                   # the one unkilled channel has zero weight everywhere
    with pytest.raises(C.NativeError, match="no live channel"):
        make(kill=only9)
    assert make(kill=only9, opt=C.FitsOptions(no_weights=True)).launches == 0
    with pytest.raises(C.NativeError, match="runs past the end of the file"):
        make(data=arr[:len(arr) // 2])
    ok = make()
    assert ok.launches == 0 and ok.chunk_samples >= L and (ok.nsamps, ok.nchan) == (TOOL_NSAMPS, 72)


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_cli_module_and_oracle_write_identical_files(tmp_path):
    b, _, _ = tool_case()
    src = str(tmp_path / "obs.sf")
    open(src, "wb").write(b)
    kill = [1] * 72
    kill[5] = 0
    killf = tmp_path / "kill.txt"
    killf.write_text("".join(f"{k}\n" for k in kill))
    flags = ["-i", src, "-k", str(killf), "--rescale_blocks", "1", "--sigma_out", "10", "--machine_id", "3"]
    out = {k: (str(tmp_path / f"{k}.fil"), str(tmp_path / f"{k}.kill")) for k in ("native", "module", "oracle")}
    r = _run([os.path.join(REPO, "bin", "fits2fil")] + flags + ["-o", out["native"][0], "--kill_out", out["native"][1],
                                                                "-v"])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    _run([sys.executable, "-m", "peasoup_amd", "fits"] + flags + ["-o", out["module"][0], "--kill_out",
                                                                  out["module"][1]], env=env, cwd=REPO)
    res = ref.fits_filterbank(src, out["oracle"][0], sigma_out=10.0, J=1, killmask=kill, kill_out=out["oracle"][1],
                              machine_id=3)
    a = open(out["native"][0], "rb").read()
    assert a == open(out["module"][0], "rb").read()
    assert a == open(out["oracle"][0], "rb").read()
    k = open(out["native"][1]).read()
    assert k == open(out["module"][1]).read() == open(out["oracle"][1]).read()
    assert [i for i, v in enumerate(k.split()) if v == "0"] == sorted([71 - 5, 71 - 9])
    assert (f"8 rows, 1 dropped slots, polarisations 0+1, z 0, {TOOL_NSAMPS} samples x 72 channels, nbad "
            f"{int(res['nbad'].sum())}, nclip {res['nclip']}, 70 of 72 channels live") in r.stdout
    o = read_header(out["native"][0])
    assert (o["nchans"], o["nbits"], o["nsamples"], o["nifs"], o["ibeam"]) == (72, 8, TOOL_NSAMPS, 1, 2)
    assert (o["fch1"], o["foff"], o["tsamp"], o["telescope_id"], o["machine_id"]) == (1235.5, -0.5, 1e-3, 6, 3)
    assert (o["source_name"], o["rawdatafile"], o["data_type"]) == ("J1234+56", "obs.sf", 1)
    assert o["tstart"] == res["header"]["tstart"] and abs(o["tstart"] - (58000 + 3603.125 / 86400)) < 1e-12
    assert C.Filterbank.from_file(out["native"][0]).nsamps == TOOL_NSAMPS
    # a refusal reaches the command line by name and writes nothing
    open(src, "wb").write(b[:len(b) // 2])
    bad = subprocess.run([os.path.join(REPO, "bin", "fits2fil"), "-i", src, "-o", str(tmp_path / "bad.fil")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "runs past the end of the file" in bad.stderr
    assert not os.path.exists(str(tmp_path / "bad.fil"))


def test_spsearch_recovers_the_burst_after_fits2fil(tmp_path):
    """The burst case of test_digi_gpu.py (64 channels x 2^16 samples at 1 ms, DM 25, FWHM 8 ms) as 8-bit
    two-polarisation PSRFITS with an ascending band: after fits2fil, spsearch's strongest candidate is the burst."""
    hdr = _header(64)
    vals = synthetic.generate(E_N, hdr, (), seed=E_SEED, bursts=[E_BURST]).astype(np.int32)
    asc = vals[:, ::-1]
    nsblk = 4096
    raw = np.stack([asc // 2, asc - asc // 2], axis=1).reshape(E_N // nsblk, nsblk, 2, 64)
    freq = (hdr["fch1"] + 63 * hdr["foff"]) - hdr["foff"] * np.arange(64)
    src, dst, out = str(tmp_path / "b.sf"), str(tmp_path / "u8.fil"), str(tmp_path / "sp.txt")
    pf.write_psrfits(src, raw, 8, hdr["tsamp"], freq, freq_form="D")
    _run([os.path.join(REPO, "bin", "fits2fil"), "-i", src, "-o", dst])
    o = read_header(dst)
    assert (o["nsamples"], o["nchans"]) == (E_N, 64)
    assert abs(o["foff"] - hdr["foff"]) < 1e-12 and abs(o["fch1"] - hdr["fch1"]) < 1e-9
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", dst, "--dm_start", "0", "--dm_end", "50", "-t", "1", "-o", out])
    assert ok
    res = C.run_sp_pipeline(a)
    assert res.candidates, "no single-pulse candidates"
    best = res.candidates[0]
    dms = np.asarray(res.dm_list)
    assert best.dm_idx == int(np.argmin(np.abs(dms - E_BURST.dm)))
    assert abs(best.time_s - E_BURST.time) / hdr["tsamp"] <= best.width
    assert best.snr >= SP_THRESHOLD
