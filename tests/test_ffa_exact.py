"""FFA search against exact oracles (kernels in csrc/kernels/ffa.hip, engine
in csrc/src/ffa.cpp).

The FFA only adds.  On integer-valued input of small magnitude every float32
partial sum is an exact integer below 2^24, so the planes must equal an int64
oracle bit for bit, and so must the boxcar sums (differences of exact prefix
sums).  What is left of the S/N is w * var (exact), rsqrtf (at most 2 ulp on
gfx950), one multiply and the conversion: the best S/N is held to 4 ulp of
float32 (4 * 2^-24 relative) against the float64 oracle.

Width rule: a reported width is accepted if the oracle's S/N at that width is
within the same 4 ulp of the oracle's best; where it equals the best exactly
(a tie in float64) it must be the narrowest such width.

CPU: the oracles themselves, the threshold gaps, the exactness of the engine
input.  GPU: planes, dense S/N, threshold records, capacity, ladder cut,
detrend, downsample, and FfaEngine.search against ffa_search_oracle."""
import functools

import numpy as np
import pytest
import torch

from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref

ULP = 2.0 ** -24
TOL = 4 * ULP

# name -> (periods, nds, explicit width ladder or None)
CASES = {
    # m = 70000, 46666, 20000 -> m2 = 2^17, 2^16, 2^15: 13, 12 and 11 global stages in one chunk (results in
    # different arenas), two rounds of the LDS block loop, grid-stride fill and pass loops, shifts up to 2^16
    "deep": ([2, 3, 7], 140000, None),
    # m2 = 1, 2, 4, 8, 16, 32 with the LDS kernel on: fewer than four LDS stages, no global pass but for the last
    "shallow": ([1000, 500, 300, 130, 64, 40], 1000, None),
    # the last period that uses LDS (fills both 64 KiB buffers)
    "p1024": ([1024, 700], 40960, None),
    # the first period without LDS up to kMaxProfile; m2 = 32, 16, 16: three passes against two
    "nolds": ([1025, 1500, 2048], 18432, None),
    # P = 5 may only use widths below 5, P = 40 all of them; m = m2 = 256 and 32 (no padding rows)
    "ladder": ([5, 40], 1283, [1, 2, 3, 5, 8, 12, 18]),
    # several hundred profiles of ordinary depth for the threshold tests
    "mid": ([37, 38, 50, 64], 5000, None),
}


def _series(name):
    periods, nds, _ = CASES[name]
    rng = np.random.default_rng(sum(periods) + nds)
    return rng.integers(-3, 4, nds).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Per period: (P, m, m2, int64 plane, used widths, snr[width, drift]); computed once, never modified."""
    periods, nds, widths = CASES[name]
    ds = _series(name).astype(np.int64)
    if widths is None:
        widths = C.ffa_widths(min(periods))
    out = []
    for P in periods:
        plane = ref.ffa_transform_exact(ref.ffa_fold_matrix_exact(ds, P))
        m = nds // P
        used, snr = ref.ffa_boxcar_snr(plane, widths, float(m))
        plane.setflags(write=False)
        snr.setflags(write=False)
        out.append((P, m, plane.shape[0], plane, used, snr))
    return tuple(out)


def _oracle_best(name):
    return np.concatenate([snr.max(axis=0) for (_, _, _, _, _, snr) in _oracle(name)])


def _gap_threshold(vals):
    """Midpoint (as float32) of the widest gap between consecutive sorted oracle S/N values near the 99th
    percentile.  The gap must exceed 100 ulp, so that a 4 ulp error cannot move a value across."""
    v = np.sort(np.asarray(vals, dtype=np.float64))
    n = len(v)
    win = v[int(0.98 * n): min(n, int(0.998 * n) + 1)]
    assert len(win) >= 2
    gaps = np.diff(win)
    i = int(np.argmax(gaps))
    thr = float(np.float32(0.5 * (win[i] + win[i + 1])))
    assert gaps[i] > 100 * ULP * abs(thr), (gaps[i], thr)
    assert thr - win[i] > 40 * ULP * abs(thr) and win[i + 1] - thr > 40 * ULP * abs(thr)
    return thr


def _assert_snr(got, exp64, what):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - exp64)
    bound = TOL * np.abs(exp64)
    worst = float((err / np.maximum(np.abs(exp64), 1e-300)).max() / ULP) if len(err) else 0.0
    print(f"{what}: worst S/N error {worst:.3f} ulp")
    assert (err <= bound).all(), f"{what}: worst S/N error {worst:.3f} ulp"


def _assert_widths(reported, used, snr, what):
    """Width rule (module docstring); reported[i] belongs to profile i of snr[width, profile]."""
    reported = np.asarray(reported)
    used = np.asarray(used)
    assert np.isin(reported, used).all(), f"{what}: a width outside the ladder cut {used} was reported"
    k = np.searchsorted(used, reported)
    best = snr.max(axis=0)
    at = snr[k, np.arange(snr.shape[1])]
    assert (np.abs(at - best) <= TOL * np.abs(best)).all(), f"{what}: reported width is not a best width"
    tie = at == best
    assert (k[tie] == snr.argmax(axis=0)[tie]).all(), f"{what}: tie not resolved to the narrowest width"


def _run(name, thresh, capacity=None):
    periods, nds, widths = CASES[name]
    kw = dict(records=True)
    if widths is not None:
        kw["widths"] = widths
    if capacity is not None:
        kw["capacity"] = capacity
    return C.ffa_fold_planes(_series(name), periods, 1.0, thresh, **kw)


# ------------------------------------------------------------------ CPU ------
@pytest.mark.parametrize("m2", [1, 2, 8, 64])
@pytest.mark.parametrize("P", [2, 3, 37])
def test_ffa_transform_exact_matches_recursive(m2, P):
    X = np.random.default_rng(100 * m2 + P).integers(-50, 51, (m2, P))
    got = ref.ffa_transform_exact(X)
    assert got.dtype == np.int64 and got.shape == (m2, P)
    np.testing.assert_array_equal(got.astype(np.float64), ref.ffa_transform(X))


def test_ffa_boxcar_snr_matches_scalar_oracle():
    X = np.random.default_rng(5).integers(-9, 10, (8, 13))
    widths = [1, 2, 3, 5, 8, 12, 18]
    used, snr = ref.ffa_boxcar_snr(X, widths, 7.0)
    assert used == [1, 2, 3, 5, 8, 12]
    for s in range(8):
        assert snr[:, s].max() == ref.boxcar_best_snr(X[s], widths, 7.0)
        for k, w in enumerate(used):
            ext = np.concatenate([X[s], X[s]])
            assert snr[k, s] == max(ext[ph: ph + w].sum() for ph in range(13)) / np.sqrt(w * 7.0)


def test_ffa_case_shapes_and_exactness():
    """The row counts the cases are meant to have, and every sum small enough to be exact in float32."""
    shapes = {n: [(m, m2) for (_, m, m2, _, _, _) in _oracle(n)] for n in CASES}
    assert shapes["deep"] == [(70000, 131072), (46666, 65536), (20000, 32768)]
    assert [m2 for (_, m2) in shapes["shallow"]] == [1, 2, 4, 8, 16, 32]
    assert shapes["p1024"] == [(40, 64), (58, 64)]
    assert [m2 for (_, m2) in shapes["nolds"]] == [32, 16, 16]
    assert shapes["ladder"] == [(256, 256), (32, 32)]
    for n in CASES:
        for (P, m, m2, plane, used, snr) in _oracle(n):
            assert 3 * m * P < 1 << 24  # bound of any prefix sum
    (_, _, _, _, used5, _), (_, _, _, _, used40, _) = _oracle("ladder")
    assert used5 == [1, 2, 3] and used40 == [1, 2, 3, 5, 8, 12, 18]


@pytest.mark.parametrize("name", ["deep", "mid"])
def test_ffa_threshold_gap(name):
    best = _oracle_best(name)
    thr = _gap_threshold(best)
    ncross = int((best > thr).sum())
    assert 6 <= ncross < len(best) // 20


# ------------------------------------------------------------------ GPU ------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_ffa_planes_and_dense_records_exact(name):
    planes, widths, count, r_pidx, r_drift, r_snr, r_width = _run(name, float("-inf"), capacity=1 << 18)
    oracle = _oracle(name)
    assert len(planes) == len(oracle)
    nprof = sum(m2 for (_, _, m2, _, _, _) in oracle)
    # every profile crosses -inf: one record each
    assert count == nprof == len(r_pidx)
    offs = np.concatenate([[0], np.cumsum([m2 for (_, _, m2, _, _, _) in oracle])])
    assert ((r_pidx >= 0) & (r_pidx < len(oracle))).all()
    assert ((r_drift >= 0) & (r_drift < np.array([o[2] for o in oracle])[r_pidx])).all()
    flat = offs[r_pidx] + r_drift
    assert len(np.unique(flat)) == nprof
    best_all = np.concatenate([b for (_, _, _, _, b) in planes])
    assert best_all.dtype == np.float32 and r_snr.dtype == np.float32
    np.testing.assert_array_equal(r_snr, best_all[flat])
    width_of = np.empty(nprof, dtype=np.int64)
    width_of[flat] = r_width
    for i, ((P, m, m2, plane, best), (eP, em, em2, eplane, used, snr)) in enumerate(zip(planes, oracle)):
        assert (P, m, m2) == (eP, em, em2) and plane.shape == (m2, P)
        np.testing.assert_array_equal(plane, eplane.astype(np.float32), err_msg=f"{name} P={P}")
        _assert_snr(best, snr.max(axis=0), f"{name} P={P}")
        _assert_widths(width_of[offs[i]: offs[i + 1]], used, snr, f"{name} P={P}")


def _crossings(name, thr):
    oracle = _oracle(name)
    exp = {}
    for i, (_, _, _, _, _, snr) in enumerate(oracle):
        best = snr.max(axis=0)
        for s in np.nonzero(best > thr)[0]:
            exp[(i, int(s))] = best[s]
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep", "mid"])
def test_ffa_threshold_records_equal_oracle_crossings(name):
    thr = _gap_threshold(_oracle_best(name))
    exp = _crossings(name, thr)
    _, _, count, r_pidx, r_drift, r_snr, r_width = _run(name, thr, capacity=1 << 16)
    got = list(zip(r_pidx.tolist(), r_drift.tolist()))
    assert count == len(exp) == len(got)
    assert len(set(got)) == len(got) and set(got) == set(exp)
    _assert_snr(r_snr, np.array([exp[k] for k in got]), f"{name} records")
    oracle = _oracle(name)
    for (i, s), w in zip(got, r_width.tolist()):
        _assert_widths([w], oracle[i][4], oracle[i][5][:, s: s + 1], f"{name} record {(i, s)}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep", "mid"])
def test_ffa_counter_exceeds_capacity(name):
    thr = _gap_threshold(_oracle_best(name))
    exp = _crossings(name, thr)
    cap = len(exp) // 3
    assert cap >= 2
    _, _, count, r_pidx, r_drift, r_snr, _ = _run(name, thr, capacity=cap)
    assert count == len(exp)
    got = list(zip(r_pidx.tolist(), r_drift.tolist()))
    assert len(got) == cap and len(set(got)) == cap and set(got) <= set(exp)
    _assert_snr(r_snr, np.array([exp[k] for k in got]), f"{name} stored records")


@pytest.mark.gpu
def test_ffa_fold_planes_default_call_unchanged():
    """The driver's earlier signature and two-element result still work."""
    periods, _, _ = CASES["mid"]
    planes, widths = C.ffa_fold_planes(_series("mid"), periods, 1.0)
    assert widths == C.ffa_widths(min(periods)) and len(planes) == len(periods)
    for (P, m, m2, plane, best), (_, _, _, eplane, _, _) in zip(planes, _oracle("mid")):
        np.testing.assert_array_equal(plane, eplane.astype(np.float32))


# ------------------------------------------------- detrend and downsample ----
@pytest.mark.gpu
@pytest.mark.parametrize("n,w", [(50000, 4096), (50000, 20000), (193, 64), (4096, 4096)])
def test_ffa_detrend_matches_oracle(n, w):
    """(50000, 20000): a window above 4096 splits each block sum over several workgroups and an atomic;
    (193, 64): the last block is one sample; (4096, 4096): a single block.
    atol 1e-4 is about 6 ulp at magnitude 256: two rounded float means, the float interpolation (three
    roundings) and the final subtraction."""
    t = np.arange(n)
    u8 = np.clip(np.rint(60 + 120 * t / n + np.random.default_rng(n + w).normal(0, 6, n)), 0, 255).astype(np.uint8)
    nblk = (n + w - 1) // w
    xt = torch.from_numpy(u8).cuda()
    out = torch.empty(n, device="cuda")
    means = torch.empty(nblk, device="cuda")
    sums = torch.empty(nblk, dtype=torch.int64, device="cuda")
    C.kernels.ffa_detrend(xt.data_ptr(), n, w, sums.data_ptr(), means.data_ptr(), out.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    blocks = [u8[i:i + w].astype(np.int64) for i in range(0, n, w)]
    np.testing.assert_array_equal(sums.cpu().numpy(), np.array([b.sum() for b in blocks]))
    exp_means = np.array([np.float32(b.sum() / len(b)) for b in blocks], dtype=np.float32)
    np.testing.assert_array_equal(means.cpu().numpy(), exp_means)
    exp = u8.astype(np.float64) - ref.sp_trend(u8, w)
    got = out.cpu().numpy().astype(np.float64)
    print(f"detrend ({n}, {w}): worst error {np.abs(got - exp).max():.3e}")
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("f", [1, 2, 8])
def test_ffa_downsample_integer_factor_exact_and_in_bounds(f):
    """Integer factors put every bin edge on a sample edge: the last output's right edge is i1 == n, where a
    read of x[n] (NaN here) would be multiplied by zero and poison the output."""
    n = 4096
    xi = np.random.default_rng(f).integers(-100, 101, n)
    buf = torch.full((n + 16,), float("nan"), device="cuda")
    buf[:n] = torch.from_numpy(xi.astype(np.float32)).cuda()
    x = buf[:n]
    nout = n // f
    out = torch.full((nout + 16,), -7.0, device="cuda")
    C.kernels.ffa_downsample(x.data_ptr(), n, float(f), out.data_ptr(), nout, torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), "the kernel read past the end of x"
    np.testing.assert_array_equal(got[:nout], xi.reshape(nout, f).sum(axis=1).astype(np.float32))
    assert (got[nout:] == -7.0).all()


# ---------------------------------------------------------------- engine -----
ENG_N = 1 << 15
ENG_WINDOW = 1 << 12
ENG_PERIOD = 40.37  # injected period in samples (= bins of octave 0)
# The strongest octave-0 candidate lies within this many drift steps (1 / (m2 - 1) bins each) of the injected
# period.  Two were hoped for; the oracle itself lands 3.51 steps away (drift 375 of 1023 at P = 40, where
# 0.37 * 1023 = 378.5: the rows next to the best one fold the 811 pulses almost as well), so the bound is the
# smallest whole number of steps the oracle meets.
ENG_STEPS = 4


def _engine_params(min_snr):
    p = C.FfaParams()
    p.tsamp = 2.0 ** -10
    p.nbins = 32
    p.p_start, p.p_end = 2.0 ** -5, 2.0 ** -3
    p.detrend_s = ENG_WINDOW * p.tsamp
    p.min_snr = min_snr
    return p


@functools.lru_cache(maxsize=None)
def _engine_series():
    """98 / 102 only; 102 forced at floor(k * 40.37 + 5), the rest of each 4096-sample trend window balanced
    around them to 2048 samples of each value: trend exactly 100, mean 0, standard deviation exactly 2."""
    rng = np.random.default_rng(4037)
    u = np.full(ENG_N, 98, dtype=np.uint8)
    forced = np.floor(np.arange(int(ENG_N / ENG_PERIOD) + 2) * ENG_PERIOD + 5).astype(np.int64)
    forced = np.unique(forced[forced < ENG_N])
    for b0 in range(0, ENG_N, ENG_WINDOW):
        f = forced[(forced >= b0) & (forced < b0 + ENG_WINDOW)]
        rest = np.setdiff1d(np.arange(b0, b0 + ENG_WINDOW), f)
        u[f] = 102
        u[rng.choice(rest, ENG_WINDOW // 2 - len(f), replace=False)] = 102
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _engine_dense():
    dense, _, _ = ref.ffa_search_oracle(_engine_series(), _engine_params(0.0))
    return dense


@functools.lru_cache(maxsize=None)
def _engine_threshold():
    return _gap_threshold(np.concatenate([d["snr"].max(axis=0) for d in _engine_dense()]))


@functools.lru_cache(maxsize=None)
def _engine_oracle(min_snr):
    _, raw, cands = ref.ffa_search_oracle(_engine_series(), _engine_params(min_snr), min_snr, dense=_engine_dense())
    return raw, cands


def test_ffa_engine_input_is_exact():
    u = _engine_series()
    assert set(np.unique(u).tolist()) == {98, 102}
    assert (u.astype(np.int64).reshape(-1, ENG_WINDOW).sum(axis=1) == 100 * ENG_WINDOW).all()
    x = u.astype(np.float64) - ref.sp_trend(u, ENG_WINDOW)
    assert (x * x == 4.0).all() and x.sum() == 0.0
    p = _engine_params(0.0)
    plan = C.ffa_plan(p, ENG_N)
    assert [o["factor"] for o in plan] == [1.0, 2.0]
    assert [(o["pa"], o["pb"], len(o["chunks"])) for o in plan] == [(32, 64, 1), (32, 64, 1)]
    assert {per[2] for per in plan[0]["chunks"][0]["periods"]} == {1024}
    assert plan[0]["chunks"][0]["nprof"] == 32768 and plan[1]["chunks"][0]["nprof"] == 16384
    assert C.ffa_widths(C.ffa_base_bins(p)) == [1, 2, 3, 5, 8, 11]
    # the normalised series is +-1: every downsampled value, plane entry and boxcar sum is a small integer
    for d in _engine_dense():
        assert d["m"] * d["P"] * d["factor"] < 1 << 24


def test_ffa_engine_oracle_finds_injected_period():
    """The oracle alone puts the strongest octave-0 candidate within ENG_STEPS drift steps of the injected
    period (and not within one step fewer), and with min_snr = 0 every profile crosses."""
    p = _engine_params(0.0)
    raw, cands = _engine_oracle(_engine_threshold())
    top = next(c for c in cands if c.octave == 0)
    assert (ENG_STEPS - 1) / 1023 < abs(top.period / p.tsamp - ENG_PERIOD) <= ENG_STEPS / 1023
    raw0, _ = _engine_oracle(0.0)
    assert len(raw0) == 32768 + 16384


def _cand_key(c):
    return (c.period, c.snr, c.width, c.nbins, c.octave, c.dm, c.dm_idx)


def test_ffa_engine_oracle_is_stable_under_snr_error():
    """The engine's S/N may differ from the oracle's by 4 ulp.  Equal oracle values stay equal on the GPU
    (same arithmetic on the same numbers), so perturb every distinct S/N value by its own random error of up
    to 4 ulp: the clustered periods must not depend on it, or the comparison below would test luck."""
    for min_snr in (_engine_threshold(), 0.0):
        raw, cands = _engine_oracle(min_snr)
        vals = np.array([r["snr"] for r in raw])
        uniq, inv = np.unique(vals, return_inverse=True)
        tol = _engine_params(min_snr).cluster_tol / (ENG_N * 2.0 ** -10)
        for trial in range(3):
            eps = np.random.default_rng(trial).uniform(-TOL, TOL, len(uniq))
            pert = (uniq * (1 + eps))[inv]
            lst = []
            for r, s in zip(raw, pert):
                c = C.FfaCandidate()
                c.period, c.snr, c.width, c.nbins, c.octave = r["period"], s, r["width"], r["nbins"], r["octave"]
                lst.append(c)
            out = C.ffa_cluster(lst, tol)
            assert [(c.period, c.nbins, c.octave) for c in out] == [(c.period, c.nbins, c.octave) for c in cands]


def _search(eng):
    xt = torch.from_numpy(np.array(_engine_series())).cuda()
    torch.cuda.synchronize()
    return eng.search(xt.data_ptr(), 0.0, 0)


def _assert_candidates(got, min_snr):
    raw, exp = _engine_oracle(min_snr)
    by_key = {(r["octave"], r["nbins"], r["period"]): r for r in raw}
    assert len(got) == len(exp)
    assert [c.period for c in got] == [c.period for c in exp]
    assert [(c.nbins, c.octave) for c in got] == [(c.nbins, c.octave) for c in exp]
    rec = [by_key[(c.octave, c.nbins, c.period)] for c in got]
    _assert_snr([c.snr for c in got], np.array([r["snr"] for r in rec]), "engine candidates")
    for c, r in zip(got, rec):
        _assert_widths([c.width], r["widths"], r["snr_by_width"][:, None], f"candidate P={c.period}")


@pytest.mark.gpu
def test_ffa_engine_equals_oracle_at_gap_threshold():
    thr = _engine_threshold()
    eng = C.FfaEngine(_engine_params(thr), ENG_N)
    got = _search(eng)
    raw, _ = _engine_oracle(thr)
    assert eng.peaks == len(raw) and eng.profiles == 32768 + 16384
    _assert_candidates(got, thr)
    top = next(c for c in got if c.octave == 0)
    assert abs(top.period * 2.0 ** 10 - ENG_PERIOD) <= ENG_STEPS / 1023


@pytest.mark.gpu
def test_ffa_engine_overflow_rerun_and_repeat_calls():
    """min_snr = 0: every profile crosses, 32768 records in octave 0's chunk against a record buffer of 16384,
    so the search grows the buffer and runs again.  Thousands of records share an S/N value: two calls agree
    only if the result does not depend on the order in which the atomics landed."""
    eng = C.FfaEngine(_engine_params(0.0), ENG_N)
    first = _search(eng)
    assert eng.peaks == eng.profiles == 32768 + 16384
    _assert_candidates(first, 0.0)
    second = _search(eng)
    assert eng.peaks == eng.profiles == 2 * (32768 + 16384)
    assert [_cand_key(c) for c in first] == [_cand_key(c) for c in second]
