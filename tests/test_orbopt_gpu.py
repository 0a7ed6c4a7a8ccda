"""orbopt on the GPU: both kernels must EQUAL the NumPy oracle at the smallest
shapes that reach each path, with every output between poisoned guards;
OrbitOptimiser must equal reference.orbit_optimise field by field; the binary
and the module write identical bytes; an injected orbit is recovered from an
off-grid candidate; every refusal reaches the user of the binary by name."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orbopt_cases as cc
from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import outputs
from peasoup_amd.utils import reference as ref
from test_orbopt import cc_compare

pytestmark = pytest.mark.gpu

GUARD = 64          # int32 cells on both sides of every output
POISON = 0x5A5A5A5A
TS = cc.TS


def _guarded(shape, dtype):
    """A device tensor of `shape` inside a poisoned buffer: (buffer, view)."""
    import torch

    total = int(np.prod(shape))
    buf = torch.full((GUARD + total + GUARD,), POISON if dtype == torch.int32 else 0x5A5A5A5A5A5A5A5A, dtype=dtype,
                     device="cuda")
    return buf, buf[GUARD:GUARD + total].view(*shape)


def _guards_intact(buf, total):
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == h[0]).all() and (h[GUARD + total:] == h[0]).all() and h[0] != 0)


def _fold(x, nrow, n, Gs, quant, nints, nbins, in_offset=0, row_of=None):
    """The op on host rows x [nrows, row_stride]: int32 [ncand, K, nints, nbins], the output between poisoned guards
    that must come back unchanged.  ``in_offset`` shifts the first input byte off its 4-byte alignment."""
    import torch

    from peasoup_amd import ops

    raw = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
    d = raw[in_offset:in_offset + x.size].view(x.shape).copy_(torch.from_numpy(np.array(x)).cuda())
    assert d.data_ptr() % 4 == in_offset % 4
    shape = (len(Gs), len(quant[0]), nints, nbins)
    buf, out = _guarded(shape, torch.int32)
    ops.orbopt_fold(d[:, :nrow], n, Gs, quant, nints, nbins, row_of=row_of, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf, int(np.prod(shape))), "wrote outside the output"
    return out.cpu().numpy()


# -------------------------------------------------------------------- fold ----
@pytest.mark.parametrize("n,pad", cc.SHAPES)
def test_fold_equals_oracle(n, pad):
    """3 rows; K of 1, 5 and 13 (and the rest of the 60 templates: amplitudes of 0 to 1000 samples, both clamps, the
    turning points) per launch; every nints with every nbins; the three periods dealt to the three rows."""
    x, tpl, y = cc.shape_case(n, pad)
    nrow = n + pad
    for nints, nbins, Gs in cc.combos(n):
        for k0, k1 in cc.group_bounds(len(tpl)):
            got = _fold(x, nrow, n, Gs, [tpl[k0:k1]] * 3, nints, nbins)
            np.testing.assert_array_equal(got, cc.want_fold(y, k0, k1, n, Gs, nints, nbins),
                                          err_msg=f"nints {nints} nbins {nbins} templates {k0}:{k1}")


@pytest.mark.parametrize("n,pad", [(17, 0), (4101, 37), (65539, 0)])
def test_fold_rows_off_alignment_and_odd_strides(n, pad):
    """Row bases off 4-byte alignment (the kernel then reads by bytes) and strides that are no multiple of 16 (source
    windows of every alignment); candidates that share a row and come in another order than the rows."""
    import orbit_cases as oc

    nrow = n + pad
    x0, tpl, y = cc.shape_case(n, pad)
    sel = list(range(25, 60, 7))                           # 3, 40 and 1000 samples over every orbit and phase
    x = np.ascontiguousarray(np.concatenate([x0[:, :nrow], oc.rows(3, 3, 1)], axis=1))   # row_stride = nrow + 3
    nints, nbins, Gs = cc.combos(n)[6]
    want = np.stack([cc.want_fold(y, k, k + 1, n, Gs, nints, nbins)[:, 0] for k in sel], axis=1)
    for off in (0, 1, 2, 3):
        got = _fold(x, nrow, n, Gs, [[tpl[k] for k in sel]] * 3, nints, nbins, in_offset=off)
        np.testing.assert_array_equal(got, want, err_msg=f"input offset {off}")
    # candidates 0..3 on rows 2, 0, 2, 1, each with its own templates
    rows = [2, 0, 2, 1]
    G4 = [Gs[1]] * 4
    quant = [[tpl[sel[(c + j) % 5]] for j in range(2)] for c in range(4)]
    got = _fold(x, nrow, n, G4, quant, nints, nbins, row_of=rows)
    for c, r in enumerate(rows):
        for j in range(2):
            k = sel[(c + j) % 5]
            np.testing.assert_array_equal(got[c, j], ref.orbopt_fold_plain(y[r, k], n, G4[c], nints, nbins))


def test_fold_equals_the_resample_kernel_then_the_plain_fold():
    """The cross-check: ops.orbit_resample writes the rows, the oracle folds them plainly."""
    import torch

    from peasoup_amd import ops

    n, pad = 4101, 37
    x, tpl, _ = cc.shape_case(n, pad)
    nints, nbins, Gs = cc.combos(n)[10]
    sel = tpl[20:33]
    rows = ops.orbit_resample(torch.from_numpy(np.array(x)).cuda(), n, (), 0.0, nrow=n + pad, quant=sel)
    rows = rows.cpu().numpy()
    got = _fold(x, n + pad, n, Gs, [sel] * 3, nints, nbins)
    for c in range(3):
        for k in range(len(sel)):
            np.testing.assert_array_equal(got[c, k], ref.orbopt_fold_plain(rows[c, k], n, Gs[c], nints, nbins))


def test_fold_many_slices_and_a_slow_pulsar():
    """A subint longer than one workgroup's tiles (the second slice starts mid-subint) and a period of 40 n samples:
    every sample of the row in one bin, one wave-wide add per wave."""
    n = C.OOPT_TILE * C.OOPT_TILES_PER_GROUP * 2 + 4101
    import orbit_cases as oc

    x = oc.rows(2, n + 11, 31)
    quant = [oc.quant(n / 3.0, 40.0, 0.37), oc.quant(5000.0, 300.0, 0.25), oc.quant(100.0, 0.0, 0.0)]
    Gs = [cc.phase_step(700.3), cc.phase_step(40.0 * n)]
    for nints, nbins in ((1, 64), (3, 7)):
        got = _fold(x, n + 11, n, Gs, [quant] * 2, nints, nbins)
        for c in range(2):
            np.testing.assert_array_equal(got[c], ref.orbopt_fold(x[c], n, Gs[c], quant, nints, nbins))
    assert np.count_nonzero(got[1, 2]) == 3 and got[1, 2].astype(np.int64).sum() == x[1, :n].astype(np.int64).sum()


def test_fold_refusals():
    import torch

    from peasoup_amd import ops

    import orbit_cases as oc

    d = torch.zeros((2, 256), dtype=torch.uint8, device="cuda")
    q = oc.quant(100.0, 3.0, 0.0)
    G = cc.phase_step(10.0)
    with pytest.raises(ValueError, match="n <= the row length"):
        ops.orbopt_fold(d, 300, [G, G], [[q], [q]], 4, 16)
    with pytest.raises(ValueError, match="row in"):
        ops.orbopt_fold(d, 256, [G, G], [[q], [q]], 4, 16, row_of=[0, 2])
    with pytest.raises(RuntimeError, match="Aq >= 2\\^30"):
        ops.orbopt_fold(d, 256, [G, G], [[(q[0], q[1], 1 << 30)], [q]], 4, 16)
    with pytest.raises(RuntimeError, match="nbins in 2..256"):
        ops.orbopt_fold(d, 256, [G, G], [[q], [q]], 4, 257)
    with pytest.raises(RuntimeError, match="templates per launch"):
        ops.orbopt_fold(d, 256, [G], [[q] * 4097], 1, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ search ----
def _search(folds, hits, ms, st):
    """The op on host planes of ncand candidates; every output between poisoned guards."""
    import torch

    from peasoup_amd import ops

    out = ops.orbopt_search(torch.from_numpy(np.ascontiguousarray(folds)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(hits)).cuda(),
                            torch.tensor(ms, dtype=torch.int32, device="cuda"), st)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _search_guarded(folds, hits, ms, st):
    """As _search through the raw entry, with the five outputs inside poisoned buffers."""
    import torch

    ncand, K, nints, nbins = folds.shape
    nw, np_ = C.oopt_nwidths(nbins), st.shape[0]
    dev = dict(device="cuda")
    f = torch.from_numpy(np.ascontiguousarray(folds)).cuda()
    h = torch.from_numpy(np.ascontiguousarray(hits)).cuda()
    m = torch.tensor(ms, dtype=torch.int32, **dev)
    d_st = torch.from_numpy(np.ascontiguousarray(st, dtype=np.int32)).cuda()
    keys = torch.empty((ncand, nw), dtype=torch.int64, **dev)
    bufs, outs = {}, {}
    for name, shape, dt in (("best_val", (ncand, nw), torch.int32), ("best_idx", (ncand, nw), torch.int32),
                            ("centre", (ncand, nw), torch.int32), ("tcurve", (ncand, nw, K), torch.int32),
                            ("msum", (ncand, K), torch.int64)):
        bufs[name], outs[name] = _guarded(shape, dt)
    C.orbopt_search_raw(f.data_ptr(), h.data_ptr(), m.data_ptr(), [int(v) for v in st.ravel()], d_st.data_ptr(), ncand, K,
                        nints, nbins, np_, keys.data_ptr(), outs["best_val"].data_ptr(), outs["best_idx"].data_ptr(),
                        outs["tcurve"].data_ptr(), outs["centre"].data_ptr(), outs["msum"].data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name in bufs:
        assert _guards_intact(bufs[name], outs[name].numel()), f"wrote outside {name}"
    return {k: v.cpu().numpy() for k, v in outs.items()}


SEARCH_CASES = [("bound", 3, 4, 16, 5), ("equal", 3, 4, 16, 5), ("bound", 5, 3, 7, 9), ("equal", 2, 1, 2, 1),
                ("bound", 13, 16, 64, 33), ("equal", 5, 3, 200, 3), ("bound", 2, 64, 256, 1), ("bound", 2, 64, 256, 257),
                ("equal", 2, 64, 256, 257), ("bound", 3, 5, 130, 7)]


@pytest.mark.parametrize("kind,K,nints,nbins,np_", SEARCH_CASES)
def test_search_equals_oracle(kind, K, nints, nbins, np_):
    """Random planes at the int32 bound, all-equal planes (ties go to the smallest index) and nints * nbins = 16384
    with np of 1 and 257; two candidates per launch with their own m and hits."""
    st = ref.orbopt_drift_table(nints, nbins, np_, 1.0)
    cases = [cc.search_planes(kind, K, nints, nbins, seed=s) for s in (K + nbins, 7 * K + np_)]
    got = _search_guarded(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases], st)
    for i, (fold, hits, m) in enumerate(cases):
        want = ref.orbopt_search(fold, hits, m, st)
        for key in ("best_val", "best_idx", "centre", "tcurve", "msum"):
            assert got[key].dtype == want[key].dtype
            np.testing.assert_array_equal(got[key][i], want[key], err_msg=f"{key} of candidate {i}")
        if kind == "equal":
            assert not got["best_idx"][i].any()
    again = _search(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases], st)
    for key in got:
        np.testing.assert_array_equal(again[key], got[key])


# --------------------------------------------------------------- optimiser ----
def _resident(fil, dms):
    """A DeviceFilterbank of `fil` for the DM list, with what keeps it alive."""
    import torch

    fb = C.Filterbank.from_file(fil)
    packed = torch.from_numpy(fb.data().copy()).cuda()
    stream = C.GpuStream()
    torch.cuda.synchronize()
    geom = C.DedispGeometry.make(fb.header, fb.nsamps, dms, [1] * int(fb.header["nchans"]))
    dfb = C.DeviceFilterbank(geom, stream.handle)
    dfb.load_packed_device(packed.data_ptr())
    stream.synchronize()
    return dfb, stream, fb


def test_optimiser_equals_oracle_and_both_drivers_write_the_same_bytes(tmp_path):
    """Two candidates at two DMs (the second with a1 = 0: 3 templates against 27, so two batches): every field of
    OrbitOptimiser's records equals reference.orbit_optimise on the device's own dedispersed rows; bin/orbopt and
    python -m peasoup_amd oopt write the bytes of outputs.write_orbopt_file of those records."""
    fil, candfile = cc.small_file(tmp_path)
    cands = C.oopt_parse_candidates(cc.CAND_TEXT)
    dms = C.oopt_dm_list(cands)
    assert dms == [3.0, 12.5]
    dfb, stream, fb = _resident(fil, dms)
    fft = int(C.prev_power_of_two(fb.nsamps))
    p = C.OrbOptParams(nbins=16, nints=4, npb=3, na1=3, nphase=3, np=5)
    opt = C.OrbitOptimiser(p, dfb, fft, stream.handle)
    recs = opt.optimise(cands)
    n = int(opt.span)
    assert n == min(int(opt.nrow), fft) and opt.batches == 2 and len(recs) == 2
    for k, (c, r) in enumerate(zip(cands, recs)):
        row = opt.row(dms.index(c[1]))
        assert row.shape == (opt.nrow,)
        cc_compare(r, ref.orbit_optimise(row, c, n, TS, k=k, **cc.SMALL_PARAMS))
    assert (recs[0]["npb"], recs[1]["npb"], recs[1]["na1"]) == (3, 1, 3)
    # a budget of one candidate per batch changes nothing
    one = C.OrbitOptimiser(p, dfb, fft, stream.handle, batch_bytes=1).optimise(cands[:1] * 3 + cands)
    for r, w in zip(one, [recs[0]] * 3 + recs):
        cc_compare(r, w)
    del opt, dfb
    header = dict(nints=4, nbins=16, npb=3, na1=3, nphase=3, np=5, nw=C.oopt_nwidths(16), n=n, tsamp=TS, p_step=1.0)
    want = str(tmp_path / "want.oopt")
    outputs.write_orbopt_file(want, header, recs)
    opts = [str(o) for o in cc.SMALL_OPTS]
    o1, o2 = str(tmp_path / "native.oopt"), str(tmp_path / "module.oopt")
    r = subprocess.run([os.path.join(REPO, "bin", "orbopt"), "-i", fil, "-c", candfile, "-o", o1, "-v"] + opts,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith(("#", "orbopt:"))]
    assert lines == [C.oopt_verbose_line(rec) for rec in recs]
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "oopt", "-i", fil, "-c", candfile, "-o", o2] + opts,
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(want, "rb") as f, open(o1, "rb") as g, open(o2, "rb") as h:
        bw, b1, b2 = f.read(), g.read(), h.read()
    assert b1 == bw and b2 == bw and not os.path.exists(o1 + ".tmp") and not os.path.exists(o2 + ".tmp")
    assert len(outputs.OrbOptFile(o1)) == 2


# ---------------------------------------------------------------- recovery ----
def test_recovery_from_an_off_grid_candidate(tmp_path):
    """The orbsearch test's pulsar (2^17 samples at 320 us, P = 10.1 ms, DM 20, pb 60 s, a1 0.0096 ls, phase 0.75)
    from the off-grid candidate (63, 0.0088, 0.72).  The CPU oracle gives S/N 46.305 at the injected template and
    13.939 at the starting one (1 x 1 x 1 grids); the midpoint is 30.122.  The truth lies 22, 10 and 21 default steps
    from the start: the default 9 x 9 x 9 grid reaches 16.189 on the oracle with flag bit 0 set, and counts that hold
    the truth inside at the default steps (47 x 23 x 45) exceed the 4096 templates of a launch.  So the test widens the
    counts to 19 x 11 x 19 AND triples the three steps (1.5 phase bins a step); the oracle then gives 46.004 with flag
    bit 0 clear.  The rule is unchanged: above the midpoint, flag bit 0 clear.  A second pass, the default grid at the
    default steps around the first pass's optimum (oracle: 47.102), must be above the midpoint and above the first."""
    fil, candfile = cc.recovery_file(tmp_path)
    cands = C.oopt_parse_candidates(open(candfile).read())
    dfb, stream, fb = _resident(fil, C.oopt_dm_list(cands))
    n = min(cc.NS, int(C.DedispGeometry.make(fb.header, fb.nsamps, [cc.DM0], [1] * 64).out_nsamps))
    g = ref.orbopt_grid(cands[0], n, TS)
    p = C.OrbOptParams(npb=19, na1=11, nphase=19, pb_step=3.0 * g["dpb"], a1_step=3.0 * g["da1"], phase_step=3.0 * g["dph"])
    r = C.OrbitOptimiser(p, dfb, cc.NS, stream.handle).optimise(cands)[0]
    print(f"S/N {r['snr']:.3f} (in {r['snr_in']:.3f}) at pb {r['opt_pb']:.4f} a1 {r['opt_a1']:.6f} phase {r['opt_phase']:.4f} "
          f"period {r['opt_period']:.9g} width {r['opt_width']} flags {r['flags']}; oracle: truth {cc.SNR_TRUTH:.3f} "
          f"start {cc.SNR_START:.3f}")
    mid = 0.5 * (cc.SNR_TRUTH + cc.SNR_START)
    assert r["snr"] > mid
    assert r["flags"] & 1 == 0
    assert abs(r["opt_pb"] - cc.TRUTH[0]) < 1.0 and abs(r["opt_period"] / cc.P0 - 1) < 1e-4
    # the second pass the README advises: the default 9 x 9 x 9 grid at the default steps around that optimum (the
    # oracle gives 47.102 there).  Its centre is the first pass's optimum folded at the refined period.
    c2 = (r["opt_period"], cc.DM0, 0.0, r["opt_pb"], r["opt_a1"], r["opt_phase"])
    r2 = C.OrbitOptimiser(C.OrbOptParams(), dfb, cc.NS, stream.handle).optimise([c2])[0]
    print(f"second pass: S/N {r2['snr']:.3f} (in {r2['snr_in']:.3f}) at pb {r2['opt_pb']:.4f} a1 {r2['opt_a1']:.6f} "
          f"phase {r2['opt_phase']:.4f} flags {r2['flags']}")
    assert r2["snr"] > mid and r2["snr"] >= r2["snr_in"] > mid and r2["snr"] > r["snr"]
    assert (r2["npb"], r2["na1"], r2["nphase"]) == (9, 9, 9)


def test_the_int32_bound_is_refused_by_both_drivers_and_leaves_no_file(tmp_path):
    """max(m, 255 - m) * n >= 2^31 holds for every row of 2^24 samples (max(m, 255 - m) >= 128).  It is raised inside
    optimise, after the rows have been dedispersed for their moments and before any fold: an 8-channel 8-bit file of
    2^24 samples, every byte 170 (the dedispersed row is 127 or 128 throughout), through bin/orbopt and through the
    module, by name, with no output left; one sample fewer (128 * (2^24 - 1) < 2^31) is accepted."""
    from peasoup_amd.models.orbopt import run_orbit_optimise
    from peasoup_amd.utils import synthetic
    from peasoup_amd.utils.sigproc import write_filterbank

    n = 1 << 24
    fil = str(tmp_path / "long.fil")
    hdr = dict(synthetic.make_header(nchans=8, nbits=8, tsamp=320e-6))
    hdr["nsamples"] = n
    write_filterbank(fil, hdr, np.zeros((0, 8), dtype=np.uint8))
    with open(fil, "ab") as f:
        f.write(np.full(8 * n, 170, dtype=np.uint8).tobytes())
    cand = str(tmp_path / "c.txt")
    with open(cand, "w") as f:
        f.write("0.0123 0 0 40 0.004 0.3\n")
    what = "max(m, 255 - m) * n >= 2^31"
    opts = ["--fft_size", str(n), "--npb", "1", "--na1", "1", "--nphase", "1", "--np", "1"]
    o1, o2 = str(tmp_path / "native.oopt"), str(tmp_path / "module.oopt")
    r = subprocess.run([os.path.join(REPO, "bin", "orbopt"), "-i", fil, "-c", cand, "-o", o1] + opts, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr and "candidate 0" in r.stderr, (r.returncode, r.stderr)
    ok, _, a = C.parse_oopt_cmdline(["orbopt", "-i", fil, "-c", cand, "-o", o2] + opts)
    assert ok
    with pytest.raises(RuntimeError, match="candidate 0: max\\(m, 255 - m\\) \\* n >= 2\\^31"):
        run_orbit_optimise(a)
    for o in (o1, o2):
        assert not os.path.exists(o) and not os.path.exists(o + ".tmp")
    # one sample fewer is accepted
    ok, _, a = C.parse_oopt_cmdline(["orbopt", "-i", fil, "-c", cand, "-o", o2] + opts[2:] + ["--fft_size", str(n - 1)])
    assert ok
    rec = run_orbit_optimise(a).records[0]
    assert rec["m"] in (127, 128) and rec["v1"] == 0 and rec["snr"] == 0.0 and os.path.exists(o2)


# ---------------------------------------------------------------- refusals ----
def test_every_refusal_reaches_the_user_by_name(tmp_path):
    import orbit_cases as oc

    fil, _ = cc.small_file(tmp_path)
    out = str(tmp_path / "refused.oopt")
    cases = [(t, e, w) for t, e, w in cc.refusal_cases(tmp_path)]
    for i, (text, extra, what) in enumerate(cases):
        cand = str(tmp_path / f"c{i}.txt")
        if text is not None:
            with open(cand, "w") as f:
                f.write(text)
        r = subprocess.run([os.path.join(REPO, "bin", "orbopt"), "-i", fil, "-c", cand, "-o", out] + [str(e) for e in extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, (r.returncode, r.stderr)
        assert what in r.stderr, r.stderr
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    r = subprocess.run([os.path.join(REPO, "bin", "orbopt"), "-i", fil, "-c", str(tmp_path / "c0.txt"), "-o", out, "-t", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "one device" in r.stderr
    with open(str(tmp_path / "good.txt"), "w") as f:
        f.write("0.0123 0 0 40 0.004 0.3\n")
    r = subprocess.run([os.path.join(REPO, "bin", "orbopt"), "-i", oc.big_file(tmp_path), "-c", str(tmp_path / "good.txt"),
                        "-o", out, "--fft_size", str(1 << 27)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "longer than 2^26" in r.stderr and not os.path.exists(out)
