"""burstopt on the GPU (csrc/kernels/burstopt.hip): the kernel's integer outputs
must EQUAL the NumPy oracle's (reference.burst_opt_search) over a sweep of
shapes at the int32 bound of the definition, with shifts at their limits, on
all-negative and all-equal rows, in batches, and through the whole chain
filterbank -> BurstCutter -> BurstOptimiser and the two entry points."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_burstopt as tb
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils.outputs import BurstOptFile, write_burst_file

pytestmark = pytest.mark.gpu
KEYS = tb.SEARCH_KEYS

# ntime, nsub, ndm, nfine: every ntime of {8, 9, 63, 64, 65, 256, 1000, 1024} (below, at and above a wave's 64 bins
# and a workgroup's 256; not a multiple of either), nsub of {1, 3, 256} (256 at ntime 256 and 1024: several staging
# steps), ndm of {1, 2, 1024} and nfine of {1, 65, 257} (one, a partial last and a full last group of eight rows)
SHAPES = [(8, 1, 1, 1), (9, 3, 2, 65), (63, 3, 2, 1), (64, 1, 2, 257), (65, 3, 1, 65), (256, 256, 2, 65),
          (1000, 3, 1024, 1), (1024, 256, 2, 257)]


def bounds(ntime, nsub):
    """The largest |d_ds| and |d_dmt| that step 1 lets through."""
    return (2 ** 31 - 1) // (nsub * (ntime // 2)), (2 ** 31 - 1) // (ntime // 2)


def shifts(rng, nfine, nsub, ntime):
    """Small random shifts of both signs, and every limit: 0, +-1, +-(ntime - 1), +-ntime."""
    sf = rng.integers(-min(ntime, 40), min(ntime, 40) + 1, (nfine, nsub)).astype(np.int32)
    special = np.array([0, 1, -1, ntime - 1, 1 - ntime, ntime, -ntime], np.int32)
    flat = sf.reshape(-1)
    pos = rng.permutation(flat.size)[:special.size]
    flat[pos] = special[:pos.size]
    if nfine > 2:
        sf[1] = np.where(np.arange(nsub) % 2 == 0, ntime - 1, 1 - ntime)  # mixed signs across subbands, at the limit
        sf[2] = ntime * np.where(np.arange(nsub) % 2 == 0, 1, -1)        # every term outside the window
    return sf


@functools.lru_cache(maxsize=None)
def shape_case(i):
    ntime, nsub, ndm, nfine = SHAPES[i]
    rng = np.random.default_rng(70 + i)
    a_ds, a_dmt = bounds(ntime, nsub)
    d_ds = rng.integers(-a_ds, a_ds + 1, (nsub, ntime)).astype(np.int32)
    d_dmt = rng.integers(-a_dmt, a_dmt + 1, (ndm, ntime)).astype(np.int32)
    d_ds.flat[0], d_ds.flat[-1] = -a_ds, a_ds      # the bound itself, both signs
    d_dmt.flat[0], d_dmt.flat[-1] = a_dmt, -a_dmt
    sf = shifts(rng, nfine, nsub, ntime)
    return d_ds, d_dmt, sf, ref.burst_opt_search(d_ds, d_dmt, sf)


def gpu_search(d_ds, d_dmt, sf, **kw):
    import torch

    from peasoup_amd import ops

    out = ops.burst_search(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (d_ds, d_dmt, sf)), **kw)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in out)
    return dict(zip(KEYS, out))


def assert_gpu_equals(got, exp, cand=0):
    for k in KEYS:
        g = got[k][cand].cpu().numpy()
        assert g.shape == exp[k].shape and np.array_equal(g, exp[k]), k


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_burst_search_equals_oracle(i):
    import torch

    d_ds, d_dmt, sf, exp = shape_case(i)
    got = gpu_search(d_ds[None], d_dmt[None], sf[None])
    assert_gpu_equals(got, exp)
    again = gpu_search(d_ds[None], d_dmt[None], sf[None])
    assert all(torch.equal(got[k], again[k]) for k in KEYS)


def test_negative_rows_and_ties():
    ntime, nsub, ndm, nfine = 65, 3, 10, 17
    rng = np.random.default_rng(5)
    sf = shifts(rng, nfine, nsub, ntime)
    zero = sf * 0
    # entirely negative planes: the maxima are the least negative boxes (with shifts a row's edge loses terms
    # and is less negative still)
    d_ds = rng.integers(-900, -1, (nsub, ntime)).astype(np.int32)
    d_dmt = rng.integers(-900, -1, (ndm, ntime)).astype(np.int32)
    exp = ref.burst_opt_search(d_ds, d_dmt, zero)
    assert exp["best_val"].max() < 0 and exp["curve"].max() < 0
    assert_gpu_equals(gpu_search(d_ds[None], d_dmt[None], zero[None]), exp)
    exp = ref.burst_opt_search(d_ds, d_dmt, sf)
    assert exp["best_val"][0].max() < 0
    assert_gpu_equals(gpu_search(d_ds[None], d_dmt[None], sf[None]), exp)
    # rows of equal values: within a row and across rows (of more than one workgroup) the smallest index wins
    eq_ds, eq_dmt = np.full((nsub, ntime), -4, np.int32), np.full((ndm, ntime), 6, np.int32)
    exp = ref.burst_opt_search(eq_ds, eq_dmt, zero)
    assert not exp["best_idx"].any() and not exp["curve_bin"].any()
    assert_gpu_equals(gpu_search(eq_ds[None], eq_dmt[None], zero[None]), exp)
    # the same maximum planted in two rows of two workgroups and twice within a row
    two = np.zeros((ndm, ntime), np.int32)
    two[9, 3] = two[2, 40] = two[2, 50] = 7
    exp = ref.burst_opt_search(eq_ds, two, sf)
    assert exp["best_idx"][0, 0] == 2 * ntime + 40 and exp["curve_bin"][0, 2] == 40
    assert_gpu_equals(gpu_search(eq_ds[None], two[None], sf[None]), exp)
    # fine rows that tie: with shifts that are equal in two rows the first wins
    sf2 = sf.copy()
    sf2[12] = sf2[4]
    exp = ref.burst_opt_search(d_ds, d_dmt, sf2)
    assert np.array_equal(exp["curve"][:, ndm + 12], exp["curve"][:, ndm + 4])
    assert_gpu_equals(gpu_search(d_ds[None], d_dmt[None], sf2[None]), exp)


def test_batch_equals_one_at_a_time_and_keeps_order():
    ntime, nsub, ndm, nfine = 63, 5, 9, 9
    rng = np.random.default_rng(9)
    d_ds = rng.integers(-3000, 3000, (5, nsub, ntime)).astype(np.int32)
    d_dmt = rng.integers(-3000, 3000, (5, ndm, ntime)).astype(np.int32)
    sf = np.stack([shifts(rng, nfine, nsub, ntime) for _ in range(5)])
    exp = [ref.burst_opt_search(d_ds[c], d_dmt[c], sf[c]) for c in range(5)]
    both = gpu_search(d_ds, d_dmt, sf)
    for c in range(5):
        assert_gpu_equals(both, exp[c], c)
        assert_gpu_equals(gpu_search(d_ds[c:c + 1], d_dmt[c:c + 1], sf[c:c + 1]), exp[c])
    # a budget of two candidates: three launches, input order kept
    g, grid = C.BurstOptGeom(ntime, nsub, ndm), C.BurstOptGrid(nfine, 0.0)
    per = C.BurstOptimiser(g, grid).bytes_per_candidate
    opt = C.BurstOptimiser(g, grid, 0, 2 * per + 8)
    assert opt.batch_size == 2
    res = opt.search(d_ds, d_dmt, sf)
    assert opt.batches == 3 and len(res) == 5
    for c in range(5):
        for k in KEYS:
            assert res[c][k].dtype == np.int32 and np.array_equal(res[c][k], exp[c][k]), (c, k)


def test_a_bad_candidate_is_named_and_nothing_is_launched():
    import torch

    from peasoup_amd import ops

    _, header, delays, out = tb.recovery()
    good = out["burst"][0]
    opt = C.BurstOptimiser(tb._geom(64, 8, 32), C.BurstOptGrid(9, 0.0))
    no_hits = dict(good, ds_hits=np.zeros_like(good["ds_hits"]))
    too_big = dict(good, dmt_sums=good["dmt_sums"].copy())
    too_big["dmt_sums"][3, 30] = 2 ** 31 - 1
    for bad in (no_hits, too_big, dict(good, dm=-1.0)):
        with pytest.raises(C.NativeError, match="candidate 1 "):
            opt.optimise([good, bad, good], [float(x) for x in delays])
    assert opt.batches == 0
    # a shift out of range in the middle of a batch: named, and the output buffers stay as they were
    d_ds = np.zeros((3, 8, 64), np.int32)
    d_dmt = np.zeros((3, 32, 64), np.int32)
    sf = np.zeros((3, 9, 8), np.int32)
    sf[1, 4, 2] = 65
    with pytest.raises(C.NativeError, match="candidate 1 "):
        opt.search(d_ds, d_dmt, sf)
    assert opt.batches == 0
    nw = opt.nwidths
    bufs = [torch.full(s, -77, dtype=torch.int32, device="cuda") for s in ((3, 2, nw), (3, 2, nw), (3, nw, 41), (3, nw, 41))]
    with pytest.raises(ValueError, match="candidate 1 "):
        ops.burst_search(torch.from_numpy(d_ds), torch.from_numpy(d_dmt), torch.from_numpy(sf), out=bufs)
    torch.cuda.synchronize()
    assert all(bool((b == -77).all()) for b in bufs)
    sf[1, 4, 2] = 64  # the limit itself is served, into the same buffers
    got = ops.burst_search(torch.from_numpy(d_ds), torch.from_numpy(d_dmt), torch.from_numpy(sf), out=bufs)
    assert all(g.data_ptr() == b.data_ptr() for g, b in zip(got, bufs)) and not bool(bufs[0].any())


def device_rows(values, nbits, bias):
    import torch

    from peasoup_amd import ops
    from peasoup_amd.utils.sigproc import pack_samples

    nsamps, nchans = values.shape
    packed = torch.from_numpy(pack_samples(values, nbits)).cuda()
    stride = (nsamps + 15) // 16 * 16
    return ops.unpack_transpose(packed, nsamps, nchans, nbits, bias, stride)


def test_end_to_end_equals_the_oracle_chain_and_recovers_the_dm():
    import torch

    from peasoup_amd import ops

    vals, header, delays, out = tb.recovery()
    cut0, rec0 = out["burst"]
    rows = device_rows(vals, 8, 128)
    # the candidate as spsearch reports it: sample, width, dm, snr
    cand = C.BurstCandidate(cut0["sample"], cut0["width"], cut0["dm"], 12.5)
    cutter = C.BurstCutter(rows.data_ptr(), rows.shape[1], tb.R_N, 64, 128, [float(d) for d in delays], [],
                           C.BurstParams(64, 8, 32, 4, 0.0), torch.cuda.current_stream().cuda_stream)
    cut = cutter.cut([cand])[0]
    for k in ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits", "dms", "nactive"):
        assert np.array_equal(cut[k], cut0[k]), k
    cut.update(sample=cand.sample, width=cand.width, dm=cand.dm, snr=cand.snr)
    got = ops.burst_optimise([cut, cut], header, nfine=65, delays=delays)
    assert len(got) == 2
    exp = dict(rec0, cand_snr=12.5)
    tb.assert_same_record(got[0], exp)
    tb.assert_same_record(got[1], exp)
    bin_dm = 4 / float(delays[-1])
    assert abs(got[0]["opt_dm"] - tb.R_DM) <= float(got[0]["dmf"][1] - got[0]["dmf"][0]) + bin_dm < abs(cand.dm - tb.R_DM)


def test_cli_and_module_write_identical_files(tmp_path):
    _, header, delays, out = tb.recovery()
    cuts = [out["burst"][0], out["impulse"][0]]  # both 64 x 8 x 32
    src = str(tmp_path / "t.bursts")
    write_burst_file(src, dict(header, ntime=64, nsub=8, ndm=32, nbits=8, nsamps=tb.R_N), cuts)
    flags = ["-i", src, "--nfine", "33", "--fine_half_range", "5"]
    a, b, c = str(tmp_path / "native.bopt"), str(tmp_path / "module.bopt"), str(tmp_path / "one.bopt")
    r = tb.run([os.path.join(REPO, "bin", "burstopt")] + flags + ["-o", a, "-v"])
    lines = [ln for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(lines) == 2 and len(lines[0].split()) == 11
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    m = tb.run([sys.executable, "-m", "peasoup_amd", "bopt"] + flags + ["-o", b, "-v"], env=env, cwd=REPO)
    assert [ln for ln in m.stdout.splitlines() if ln and ln[0].isdigit()] == lines
    assert open(a, "rb").read() == open(b, "rb").read()
    f = BurstOptFile(a)
    assert len(f) == 2 and (f.header["nfine"], f.header["fine_half_range"], f.header["nw"]) == (33, 5.0, 6)
    assert f.header["nsamps"] == tb.R_N and f.header["nchans"] == 64
    for i, cut in enumerate(cuts):
        tb.assert_same_record(f.candidate(i), ref.burst_optimise(cut, header, delays, 33, 5.0))
    native = C.read_burst_file(src)
    assert len(native["candidates"]) == 2 and native["geom"].ntime == 64 and native["nsamps"] == tb.R_N
    for k in ("ds_sums", "dmt_hits", "dms", "nactive"):
        assert np.array_equal(native["candidates"][1][k], cuts[1][k]), k
    tb.run([os.path.join(REPO, "bin", "burstopt"), "-i", src, "--limit", "1", "-o", c])
    assert len(BurstOptFile(c)) == 1 and BurstOptFile(c).header["nfine"] == 65
    bad = subprocess.run([os.path.join(REPO, "bin", "burstopt"), "-i", a], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "not a burst-cutout file" in bad.stderr
