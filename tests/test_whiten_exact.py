"""The whitener against a float64 oracle, bin by bin, in all three median regions.

Under test: the whole whitening chain of SearchEngine / Whitener (engine.cpp
Whitener::whiten and Whitener::whiten_batch): 8-bit trial -> float32 with the
mean pad (timeseries.hip u8_sum_kernel, u8_to_f32_pad_kernel, or pass A's own
8-bit / strip / f32 sources) -> real FFT (four-step passes, mixed radix or
rocFFT) -> running median, dereddening, zapping and the interbin statistics
(spectrum.hip deredden_zap_kernel, deredden_zap_moments_kernel) -> inverse
real FFT (fft4_c2r_pre or pass A's on-the-fly pre-processing, fft4_c2r_post or
fft4_c2r_post_pad).  The oracle (utils/reference.py whiten64) is the
definition in float64 with the algorithm's integer decisions taken in float32
as the code takes them.

Metric: the whitened float32 series w of the GPU is taken back to the
spectrum on the host, D_gpu = rfft(float64(w)) / n, and compared with the
oracle's dereddened half spectrum D in every one of the n/2 + 1 bins:
max and rms of |D_gpu - D|.  |D| is O(1) (its median is 1), so this is an
absolute error at unit scale; bins 0..4 must come back as 0 and zapped bins
as 1 within the same bound (no bin is skipped).  {mean, std} of copy_stats are
compared with the oracle's float64 statistics, relative.

Inputs: clip(rint(normal(128, 12))) as uint8, one seed per row (a stride
error reads another row's data).  tsamp = 8000 / n puts the region switches
at pos5 = 400 and pos25 = 3999 at every length, so that the medians of 5, of
25 and of 125 each divide hundreds of bins (asserted: >= 100 bins per region,
and a zapped bin in each).  The production value tsamp = 64e-6 has pos5 <= 3:
its m5 region is empty by construction (asserted), which is why no earlier
test ever ran the m5 branch.  The zap list (in bins: _zap_bins) has a range
crossing bits 31 / 32 of a mask word, one covering bins 3..9 (zap wins over
the zeroing of bins 0..4), one with f - w < 0, one beyond Nyquist (ignored),
one clamped at nbins - 1 (the Nyquist bin itself stays unzapped) and two
overlapping ones; every one of these facts is asserted on the oracle's mask
and on build_zap_mask's bits in every case that uses the list.

Lengths.  fft4_geometry needs both factors of n / 2 in 128..4096, so the
smallest four-step whitener is n = 2^15 (128 x 128): at 2^14 n / 2 = 128 x 64
is refused and Whitener and SearchEngine run rocFFT (fft_mode falls to 1),
whatever fft_mode or allow_fft4 say.  2^14 is therefore the rocFFT length, and
every axis is given its full range at 2^14 AND at 2^15; 2^17, 2^20 (1024 x
512) and the mixed-radix 3 * 2^14 and 17 * 2^16 take a thinned set.  The
mixed-radix lengths go through Whitener.whiten only (no zap list, no stats:
the engine's search at these lengths would need rocFFT transforms with odd
factors); their float32 input is ops.convert_pad's.

Measured error of the GPU against the oracle (MI355X, the kernels as of this
module's first commit, noise input, worst over every case of this module):

    n          max        rms        mean (rel)  std (rel)   worst case (max)
    2^14       4.54e-06   3.04e-07   6.71e-08    6.99e-07    search_trial, no zap list (rocFFT), bin 85
    2^15       3.38e-06   3.94e-07   9.90e-08    6.41e-07    search_trial, fft_mode = 1, bin 270
    2^17       2.99e-06   4.10e-07   6.52e-08    6.15e-07    batched count 3, nsamps = n, slot 0, bin 3728
    2^20       6.26e-06   4.39e-07   5.76e-08    4.85e-07    batched count 3, nsamps = n/2 + 5, slot 1, bin 2775
    3 * 2^14   2.11e-06   3.41e-07   -           -           Whitener.whiten, tsamp = 64e-6, bin 9580
    17 * 2^16  2.70e-06   3.60e-07   -           -           Whitener.whiten, tsamp = 64e-6, bin 396272

The forward sources (padded f32, strips, 8-bit rows, unpadded f32), the
environment switches and both halves of the prepared slots give the same
figures to every printed digit; no source or inverse path is worse than
another.  tol = 4 x measured per length (seed-to-seed spread of a maximum),
under the caps 2e-5 (max), 2e-6 (rms), 1e-4 (mean), 1e-3 (std); no length comes
near a cap.  The float32 NumPy reference ref.whiten lies within 7.3e-7 max /
8.8e-8 rms / 5e-7 stats of the oracle; every figure above is within 10 x that.

Two bugs found by this module and fixed with it (before: max 4.6e-5 .. 4.7e-4,
rms up to 1.0e-5, on every path alike):
  * The DC term.  The transform's input carried the trial's mean: a DC term
    of 128 n, 10 sqrt(n) times the noise amplitude, so a float32 FFT rounded
    its partial sums at ulp(128 n) relative to |X_k| ~ 12 sqrt(n / 2), and the
    roundings added up where the twiddles are 1, -1, +-i (bins n/2, n/4, n/8:
    5e-5 at 2^14, 1.8e-4 at 2^15, 4.7e-4 at 2^20, on rocFFT and the four-step
    passes alike; rows with nsamps >= n were spared while their partial sums
    stayed exact integers, 128 n < 2^24).  A single-precision pocketfft of the
    same input reproduces it without a GPU.  The whitener now transforms the
    series less rint(mean) -- exact for 8-bit samples and, by Sterbenz' lemma,
    for the pad -- and adds n rint(mean) back to X_0 (which only the first
    median of 5 reads).
  * The stretch.  stretch_at's x = float(i) * step was contracted into
    frac = x - float(j) as fma(i, step, -j), so frac came from the unrounded
    product while j came from the rounded one: off by up to half an ulp of x,
    which at bin 5e5 of a 2^20 spectrum is 2.4e-4 in frac and 3.1e-4 of the
    median in D (2.2e-5 at 2^17; rms 8.8e-6 at 2^20: every high bin is
    touched).  The reference's functor rounds the product; so does the kernel
    now (contraction off in stretch_at).  An oracle with the contracted frac
    reproduced the GPU's figure to three digits, in the same bin.

Bright lines (test_pulse_train; measured 4.6e-6 / 7.8e-6 / 9.3e-6 at 2^14 /
2^15 / 2^17, in line bins): a float32 D cannot be nearer to its float64
value than half an ulp, so bins with |D| > 8 get 2^-22 (|D_k| - 8) on top of
tol_max (the rule of test_search_spectrum_exact (b)); the C2R pre-processing
forms z_m from D_m and D_{n/2 - m}, so bin k also gets the allowance of its
mirror n/2 - k; and a float32 butterfly that adds a line to a noise value
rounds at the line's ulp, so every bin gets the allowance of the largest bin.
The whitener has no interbin coupling (k - 1) in its series.  The rms bound is
unchanged.

Kernel level (test_deredden_kernel): deredden_zap_kernel on ops.running_median's
medians against the oracle's stretch for nbins in {126, 130, 629, 3127, 8193}
(every residue mod 5) with pos5 / pos25 on, one before and one after a bin at
which the stretch's node index advances.  Bound per bin: 2^-19 max(|D|, 1),
i.e. 32 float32 half-ulps for the amplitude (two products, a sum, rsqrt, a
product), the interpolation (three operations on values of the median's size)
and cdiv_real (two reciprocals, six products); a switch off by one bin is an
error of 0.08 .. 0.25.

CPU tests: ref.whiten (float32 NumPy) lies inside the tolerances at every
length, zap list and nsamps; ten defective oracles must exceed tol_max by
100 x at 2^14 and 2^17 (their figures are printed; DEFECT_NOTES says which do
not reach the margin and why).
"""
import functools

import numpy as np
import pytest

from peasoup_amd.utils import reference as ref

dev = "cuda"
TSAMP_PROD = 64e-6
N14, N15, N17, N20, N3, N17M = 1 << 14, 1 << 15, 1 << 17, 1 << 20, 3 << 14, 17 << 16
POW2 = [N14, N15, N17, N20]
FULL = [N14, N15]  # every axis in full: the rocFFT length and the smallest four-step length

# max, rms of |D_gpu - D|; relative error of mean, std -- per length, worst case of this module
TOL_CAP = (2e-5, 2e-6, 1e-4, 1e-3)
# (None: Whitener.whiten's statistics are not exposed at the mixed-radix lengths; the cap alone holds there)
MEASURED = {N14: (4.539e-6, 3.044e-7, 6.711e-8, 6.992e-7), N15: (3.375e-6, 3.937e-7, 9.897e-8, 6.409e-7),
            N17: (2.988e-6, 4.102e-7, 6.522e-8, 6.153e-7), N20: (6.260e-6, 4.394e-7, 5.759e-8, 4.851e-7),
            N3: (2.106e-6, 3.410e-7, None, None), N17M: (2.698e-6, 3.595e-7, None, None)}
TOL = {n: tuple(c if m is None else min(4 * m, c) for m, c in zip(v, TOL_CAP)) for n, v in MEASURED.items()}


def _zap_bins(nb):
    """(centre, half width) of every zap entry in bins; see the module docstring"""
    return [(32.0, 2.5), (6.25, 3.0), (1.0, 2.5), (nb + 10.5, 2.0), (nb - 3.5, 10.0), (1000.5, 3.0), (1003.5, 2.0)]


def _tsamp(n, kind):
    return 8000.0 / n if kind == "regions" else TSAMP_PROD


def _zap_list(n, tsamp):
    """(freqs, widths) of _zap_bins at this length, as the float32 values the engine is given"""
    bw = float(ref.whiten_positions(n, tsamp)[0])
    zb = _zap_bins(n // 2 + 1)
    return [float(np.float32(c * bw)) for c, _ in zb], [float(np.float32(w * bw)) for _, w in zb]


def _assert_zap_edges(mask):
    nb = len(mask)
    z = np.flatnonzero(mask)
    assert mask[29:35].all() and not mask[28] and not mask[35], "the range over bits 31 / 32 of word 0"
    assert mask[0:10].all() and not mask[10], "bins 0..9: f - w < 0 and the range over the zeroed bins"
    assert mask[nb - 14:nb - 1].all() and not mask[nb - 1] and not mask[nb - 15], "the range clamped at nbins - 1"
    assert mask[997:1006].all() and not mask[996] and not mask[1006], "the two overlapping ranges"
    assert len(z) == 6 + 10 + 13 + 9, "the entry beyond Nyquist adds nothing"


@functools.lru_cache(maxsize=None)
def _row(n, seed, length, pulse=False):
    x = np.random.default_rng(seed).normal(128.0, 12.0, length)
    if pulse:  # a pulse train of period 512 samples, 8 wide: lines at multiples of n / 512 with |D| >> 8
        x = x + 60.0 * ((np.arange(length) % 512) < 8)
    r = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=32)
def _oracle(n, seed, length, nsamps, kind="regions", zap=True, pulse=False):
    """(D, stats, pos5, pos25, zap mask or None) of row (seed, length)'s first nsamps samples"""
    tsamp = _tsamp(n, kind)
    zf, zw = _zap_list(n, tsamp) if zap else ((), ())
    D, st, pos5, pos25 = ref.whiten64(_row(n, seed, length, pulse)[:nsamps], n, tsamp, zf, zw)
    nb = n // 2 + 1
    mask = ref.zap_mask(zf, zw, float(ref.whiten_positions(n, tsamp)[0]), nb) if zap else None
    if kind == "regions":
        assert pos5 - 5 >= 100 and pos25 - pos5 >= 100 and nb - pos25 >= 100, (pos5, pos25, nb)
        if zap:
            z = np.flatnonzero(mask)
            assert (z < pos5).any() and ((z >= pos5) & (z < pos25)).any() and (z >= pos25).any()
    else:
        assert pos5 <= 3, "tsamp = 64e-6: bins below 5 are zeroed, so no bin takes the medians of 5"
    if zap:
        _assert_zap_edges(mask)
        assert np.all(D[mask] == 1) and not D[:5][~mask[:5]].any()
    else:
        assert not D[:5].any()
    D.setflags(write=False)
    return D, st, pos5, pos25, mask


def _figures(w, stats, D, st):
    """(err per bin, max, rms, relative error of mean, of std)"""
    n = len(w)
    err = np.abs(np.fft.rfft(w.astype(np.float64)) / n - D)
    rel = (abs(stats[0] - st[0]) / st[0], abs(stats[2] - st[2]) / st[2]) if stats is not None else (0.0, 0.0)
    return err, float(err.max()), float(np.sqrt((err ** 2).mean())), rel[0], rel[1]


def _judge(label, w, stats, D, st, bound=None):
    n = len(w)
    err, emax, erms, emean, estd = _figures(w, stats, D, st)
    tol = TOL[n]
    print(f"WHITEN_EXACT n={n} max={emax:.3e} rms={erms:.3e} mean={emean:.3e} std={estd:.3e} "
          f"bin={int(np.argmax(err))} case={label}")
    assert np.isfinite(w).all() and np.abs(w).max() > 0, label
    if bound is None:
        assert emax < tol[0], (label, int(np.argmax(err)), emax)
    else:
        worst = int(np.argmax(err / bound))
        assert (err < bound).all(), (label, worst, err[worst], bound[worst])
    assert erms < tol[1], (label, erms)
    assert emean < tol[2] and estd < tol[3], (label, emean, estd)


# ------------------------------------------------------------- GPU helpers --
def _engine(n, tsamp, zap=True, fft_mode=2):
    import torch

    import peasoup_amd._C as C

    p = C.SearchParams()
    p.fft_size, p.tsamp, p.nharmonics, p.accel_batch, p.fft_mode = n, tsamp, 1, 16, fft_mode
    if zap:
        p.zap_freqs, p.zap_widths = _zap_list(n, tsamp)
        bits = np.array(C.build_zap_mask(p.zap_freqs, p.zap_widths, float(ref.whiten_positions(n, tsamp)[0]),
                                         n // 2 + 1), dtype=np.uint32)
        mask = ref.zap_mask(p.zap_freqs, p.zap_widths, float(ref.whiten_positions(n, tsamp)[0]), n // 2 + 1)
        assert np.array_equal(np.unpackbits(bits.view(np.uint8), bitorder="little")[:n // 2 + 1].astype(bool), mask)
    return C.SearchEngine(p, torch.cuda.current_stream().cuda_stream)


def _device_rows(rows, rs, offset):
    """the rows at byte `offset` of a 16-byte aligned device buffer, rs bytes apart; (tensor, address of row 0)"""
    import torch

    buf = np.full(offset + len(rows) * rs + 256, 255, dtype=np.uint8)
    for b, r in enumerate(rows):
        buf[offset + b * rs:offset + b * rs + len(r)] = r
    t = torch.from_numpy(buf).to(dev)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset


def _read_slot(e, n):
    import torch

    w = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.empty(3, dtype=torch.float32, device=dev)
    e.copy_whitened(w.data_ptr())
    e.copy_stats(st.data_ptr())
    torch.cuda.synchronize()
    return w.cpu().numpy(), st.cpu().numpy().astype(np.float64)


def _batched(label, n, count, nsamps=None, kind="regions", zap=True, fft_mode=2, rs=None, offset=0, second=False,
             seed0=None):
    """prepare(count rows) -> search_prepared(b, [0.0]) -> every slot against its own row's oracle"""
    nsamps = n - 1003 if nsamps is None else nsamps
    length = max(nsamps, n) + 13  # the row is longer than what is read: samples past nsamps must not matter
    rs = (length + 79) // 16 * 16 if rs is None else rs
    assert rs >= length
    seed0 = 100 * n.bit_length() + 7 * count if seed0 is None else seed0
    rows = [_row(n, seed0 + b, length) for b in range(count)]
    t, ptr = _device_rows(rows, rs, offset)
    e = _engine(n, _tsamp(n, kind), zap, fft_mode)
    first = 0
    if second:
        other = [_row(n, seed0 + 50 + b, length) for b in range(count)]
        t0, ptr0 = _device_rows(other, rs, 0)
        first = e.max_prepare
        e.reserve(count, 1, True)
        e.prepare(ptr0, rs, nsamps, count)
    assert e.max_prepare >= count
    e.prepare(ptr, rs, nsamps, count, first)
    for b in range(count):
        e.search_prepared(first + b, 0.0, b, [0.0])
        w, st = _read_slot(e, n)
        D, st64, _, _, _ = _oracle(n, seed0 + b, length, nsamps, kind, zap)
        _judge(f"{label} slot {b}/{count}", w, st, D, st64)


# --------------------------------------------------------------- GPU tests --
TRIAL_CASES = ([(n, k) for n in POW2 for k in ("regions", "production")] +
               [(n, k) for n in FULL for k in ("no zap", "rocfft")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", TRIAL_CASES)
def test_search_trial(n, kind):
    """Single path: search_trial on one aligned row; tsamp = 64e-6; a null zap mask; fft_mode = 1."""
    nsamps, length = n - 1003, n + 13
    seed = 11 * n.bit_length()
    tk = "production" if kind == "production" else "regions"
    zap = kind != "no zap"
    e = _engine(n, _tsamp(n, tk), zap, 1 if kind == "rocfft" else 2)
    assert e.fft_mode == (2 if n >= N15 and kind != "rocfft" else 1)
    t, ptr = _device_rows([_row(n, seed, length)], length, 0)
    e.search_trial(ptr, nsamps, 0.0, 0, [0.0])
    w, st = _read_slot(e, n)
    D, st64, _, _, _ = _oracle(n, seed, length, nsamps, tk, zap)
    _judge(f"search_trial {kind}", w, st, D, st64)


# tsamp = 64e-6: one single-path case per length (search_trial's for the powers of two)
WHITENER_CASES = ([(n, True, "regions") for n in POW2 + [N3, N17M]] + [(n, False, "regions") for n in FULL] +
                  [(N3, True, "production"), (N17M, True, "production")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,allow_fft4,kind", WHITENER_CASES)
def test_whitener_whiten(n, allow_fft4, kind):
    """Single path: Whitener.whiten in place on ops.convert_pad's series (no zap list; its stats are not exposed):
    four-step, mixed radix, and rocFFT (allow_fft4 = False; odd factors excepted)."""
    import torch

    import peasoup_amd._C as C
    from peasoup_amd import ops

    nsamps = n - 1003
    seed = 13 * n.bit_length() + (n % 7)
    wh = C.Whitener(n, _tsamp(n, kind), torch.cuda.current_stream().cuda_stream, allow_fft4)
    assert wh.uses_fft4 == (allow_fft4 and n != N14) and wh.mixed_radix == (n in (N3, N17M))
    x = ops.convert_pad(torch.from_numpy(np.array(_row(n, seed, nsamps))).to(dev), n)
    wh.whiten(x.data_ptr(), True)
    torch.cuda.synchronize()
    D, st64, _, _, _ = _oracle(n, seed, nsamps, nsamps, kind, False)
    _judge(f"Whitener.whiten fft4={allow_fft4} {kind}", x.cpu().numpy(), None, D, st64)


BATCH_CASES = ([(n, c, s) for n in FULL for c in (1, 3, 5) for s in (False, True)] +
               [(N17, 3, False), (N17, 3, True), (N20, 3, False), (N20, 3, True)])


@pytest.mark.gpu
@pytest.mark.parametrize("n,count,second", BATCH_CASES)
def test_batched_slots(n, count, second):
    """prepare / search_prepared / copy_whitened / copy_stats, every slot, and the second half of the prepared
    slots (reserve(two = True), first = max_prepare) with other rows prepared into the first half."""
    _batched(f"batched second={second}", n, count, second=second)


@pytest.fixture
def fft4_flags():
    import peasoup_amd._C as C

    old = C.kernels.fft4_flags()
    try:
        yield old
    finally:
        C.kernels.fft4_set_flags(old)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["padded f32", "strips", "u8", "f32"])
@pytest.mark.parametrize("n", POW2)
def test_forward_sources(n, source, fft4_flags):
    """The four forward sources of whiten_batch (test_whitening_direct_sources_equal_padded_path's settings)."""
    import peasoup_amd._C as C

    WS, U8, F32 = 16777216, 33554432, 67108864
    f0 = fft4_flags
    assert f0 & WS
    C.kernels.fft4_set_flags({"padded f32": f0 & ~WS, "strips": f0 & ~(U8 | F32), "u8": (f0 & ~F32) | U8,
                              "f32": (f0 & ~U8) | F32}[source])
    _batched(f"source {source}", n, 3)


ENV_CASES = ([(n, d, m) for n in FULL for d in ("00", "10", "11") for m in (1, 2)] +
             [(n, d, 2) for n in (N17, N20) for d in ("00", "10", "11")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,direct,fft_mode", ENV_CASES)
def test_environment(monkeypatch, n, direct, fft_mode):
    """PSOUP_WHITEN_PAD_DIRECT x PSOUP_WHITEN_FUSED_STATS: the inverse into pass A's padded input and the fused
    deredden_zap_moments_kernel against the two-kernel sequences, each against the oracle."""
    monkeypatch.setenv("PSOUP_WHITEN_PAD_DIRECT", direct[0])
    monkeypatch.setenv("PSOUP_WHITEN_FUSED_STATS", direct[1])
    _batched(f"env {direct} fft_mode={fft_mode}", n, 3, fft_mode=fft_mode)


def _nsamps(n, which):
    return {"n": n, "n-1": n - 1, "n-3": n - 3, "n-1003": n - 1003, "n+77": n + 77, "n/2+5": n // 2 + 5}[which]


NSAMPS_CASES = ([(n, w) for n in FULL for w in ("n", "n-1", "n-3", "n-1003", "n+77", "n/2+5")] +
                [(N17, "n"), (N17, "n-3"), (N17, "n+77"), (N20, "n-1"), (N20, "n/2+5")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,which", NSAMPS_CASES)
def test_nsamps(n, which):
    """No padding, truncation (the row is longer than n), lengths that are no multiple of 4 or 16."""
    _batched(f"nsamps {which}", n, 3, nsamps=_nsamps(n, which))


ALIGN_CASES = ([(n, a) for n in FULL for a in ("aligned", "+1", "+4", "odd stride", "+1 single")] +
               [(N17, "+1"), (N17, "odd stride"), (N20, "+4"), (N20, "odd stride")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,align", ALIGN_CASES)
def test_alignment(n, align):
    """Row pointers and strides that make u8_aligned false (asserted through the result only)."""
    if align == "odd stride":
        _batched("align odd stride", n, 3, nsamps=n - 3, rs=n + 67)
    elif align == "+1 single":
        _batched("align +1 single", n, 1, nsamps=n - 3, offset=1)
    else:
        _batched(f"align {align}", n, 3, nsamps=n - 3, offset={"aligned": 0, "+1": 1, "+4": 4}[align])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N14, N15, N17])
def test_pulse_train(n):
    """Lines with |D| >> 8: the float32-ulp allowance of the module docstring, nothing else."""
    nsamps, length = n - 1003, n + 13
    seed = 17 * n.bit_length()
    D, st64, _, _, _ = _oracle(n, seed, length, nsamps, "regions", True, True)
    big = np.maximum(np.abs(D) - 8.0, 0.0)
    assert big.max() > 8.0 and (big > 0).sum() >= 4, "the pulse train gives too few bright lines"
    M = n // 2
    assert len(big) == M + 1
    bound = TOL[n][0] + 2.0 ** -22 * (big + big[::-1] + big.max())  # [::-1]: bin n/2 - k
    e = _engine(n, _tsamp(n, "regions"))
    t, ptr = _device_rows([_row(n, seed, length, True)], length, 0)
    e.search_trial(ptr, nsamps, 0.0, 0, [0.0])
    w, st = _read_slot(e, n)
    _judge("pulse train", w, st, D, st64, bound)


def _node_bin(in_count, out_count, lo):
    """the first bin k > lo at which the stretch's node index advances"""
    j = ref.stretch_nodes(in_count, out_count)[0]
    return int(lo + 1 + np.flatnonzero(j[lo + 1:] != j[lo:-1])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("place", [-1, 0, 1])
@pytest.mark.parametrize("nbins", [126, 130, 629, 3127, 8193])
def test_deredden_kernel(nbins, place):
    import torch

    import peasoup_amd._C as C
    from peasoup_amd import ops

    rng = np.random.default_rng(nbins)
    Xn = (rng.standard_normal(nbins) + 1j * rng.standard_normal(nbins)).astype(np.complex64)
    Xn *= np.linspace(3.0, 1.0, nbins).astype(np.float32)  # a red slope: neighbouring medians differ
    X = torch.from_numpy(Xn).to(dev)
    n5, n25, n125 = nbins // 5, max(1, nbins // 25), max(1, nbins // 125)
    pos5 = _node_bin(n5, nbins, 8) + place
    pos25 = _node_bin(n25, nbins, max(pos5 + 10, nbins // 2)) + place
    assert 5 < pos5 < pos25 < nbins - 5
    m5, m25, m125 = ops.running_median(X)
    amp = np.abs(Xn.astype(np.complex128))
    e5 = ref.median_scrunch5_64(amp)
    e25 = ref.median_scrunch5_64(e5)
    e125 = ref.median_scrunch5_64(e25)
    for got, exp in ((m5, e5), (m25, e25), (m125, e125)):
        g = got.cpu().numpy()[:len(exp)]
        # a median selects an amplitude; its rounding: |x|^2 (1 ulp), rsqrt (2 ulp), a product
        assert (np.abs(g - exp) <= 2.0 ** -21 * exp).all()
    zm = np.zeros(nbins, bool)
    zm[[3, 31, 32, nbins - 2]] = True
    bits = np.packbits(zm, bitorder="little")
    bits = np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.int32)
    zt = torch.from_numpy(bits.copy()).to(dev)
    C.kernels.deredden_zap(X.data_ptr(), nbins, m5.data_ptr(), n5, m25.data_ptr(), n25, m125.data_ptr(), n125,
                           pos5, pos25, zt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    D = Xn.astype(np.complex128) / ref.running_median64(amp, pos5, pos25)
    D[:5] = 0
    D[zm] = 1
    err = np.abs(X.cpu().numpy().astype(np.complex128) - D)
    bound = 2.0 ** -19 * np.maximum(np.abs(D), 1.0)
    k = int(np.argmax(err / bound))
    print(f"WHITEN_KERNEL nbins={nbins} pos5={pos5} pos25={pos25} max={err.max():.3e} bin={k}")
    assert (err <= bound).all(), (k, err[k], bound[k])
    # each switch bin differs between its two regions by far more than the bound, so either switch off by one fails
    X64 = Xn.astype(np.complex128)
    r5 = np.abs(X64 / ref.running_median64(amp, pos5 + 1, pos25) - D)[pos5] / bound[pos5]
    r25 = np.abs(X64 / ref.running_median64(amp, pos5, pos25 - 1) - D)[pos25 - 1] / bound[pos25 - 1]
    print(f"WHITEN_KERNEL nbins={nbins} place={place}: pos5 + 1 is {r5:.3g} x the bound, pos25 - 1 is {r25:.3g} x")
    assert r5 > 100
    if (nbins, place) == (130, 0):
        # the stretched m25 passes within 1.3e-4 of the single m125 value at bin 96: 64 x the bound, not 100 x
        assert r25 > 1
    else:
        assert r25 > 100


# --------------------------------------------------------------- CPU tests --
SELF_CASES = ([(N14, w, z) for w in ("n", "n-1", "n-3", "n-1003", "n+77", "n/2+5") for z in (True, False)] +
              [(n, "n-1003", True) for n in (N15, N17, N20)] + [(n, "n-1003", False) for n in (N3, N17M)])


@pytest.mark.parametrize("n,which,zap", SELF_CASES)
def test_float32_reference_lies_inside_the_tolerances(n, which, zap):
    nsamps = _nsamps(n, which)
    length = max(nsamps, n) + 13
    seed = 19 * n.bit_length()
    for kind in ("regions", "production"):
        D, st64, _, _, mask = _oracle(n, seed, length, nsamps, kind, zap)
        w, st = ref.whiten(_row(n, seed, length)[:nsamps], n, _tsamp(n, kind), mask)
        _judge(f"ref.whiten {which} zap={zap} {kind}", w, np.array(st), D, st64)


DEFECTS = ["pos5 + 1", "pos25 - 1", "m5 node j + 1", "frac guard dropped", "zap range one longer",
           "zap range one shorter", "zap before zeroing", "bin 4 not zeroed", "pad mean over n",
           "neighbour's medians"]
# defects that do not reach 100 x tol_max, with the reason (their figures are printed and nothing is asserted)
DEFECT_NOTES = {
    "frac guard dropped": "frac = float32(k * step) - j is either exactly 0 or far above 1e-5 at these lengths "
                          "(step = (in - 1) / (out - 1) ~ 0.2, 0.04, 0.008: the smallest non-zero frac is ~1e-4), so "
                          "interpolating at frac <= 1e-5 adds frac * (next - a) = 0: max 0.0 / rms 0.0 at 2^14 and "
                          "2^17.  The guard cannot be tested through the values at any length used here.",
}


def _defective(name, n, seed, length, nsamps, zap=True):
    """whiten64's D and stats, recomposed from its pieces with one defect (name = "": none)."""
    tsamp = _tsamp(n, "regions")
    u8 = _row(n, seed, length)[:nsamps]
    nvalid = min(nsamps, n)
    x = ref.convert_pad64(u8, n)
    if name == "pad mean over n":
        x[nvalid:] = np.float32(float(u8[:nvalid].astype(np.int64).sum()) / n)
    X = np.fft.rfft(x)
    nb = len(X)
    bw, pos5, pos25 = ref.whiten_positions(n, tsamp)
    pos5 += name == "pos5 + 1"
    pos25 -= name == "pos25 - 1"
    amp = np.abs(X)
    if name == "neighbour's medians":
        amp = np.abs(np.fft.rfft(ref.convert_pad64(_row(n, seed + 1, length)[:nsamps], n)))
    m5 = ref.median_scrunch5_64(amp)
    m25 = ref.median_scrunch5_64(m5)
    m125 = ref.median_scrunch5_64(m25)
    j, frac, use = ref.stretch_nodes(len(m5), nb)
    if name == "m5 node j + 1":
        j = j.copy()
        j[pos5 // 2] += 1
    if name == "frac guard dropped":
        use = j + 1 < len(m5)
        # the guard only matters where 0 < frac <= 1e-5: there must be such bins for the defect to exist
    k = np.arange(nb)
    s25 = ref.linear_stretch64(m25, nb)
    s125 = ref.linear_stretch64(m125, nb)
    if name == "frac guard dropped":
        j25, f25, _ = ref.stretch_nodes(len(m25), nb)
        s25 = ref.linear_stretch64(m25, nb, (j25, f25, j25 + 1 < len(m25)))
        j125, f125, _ = ref.stretch_nodes(len(m125), nb)
        s125 = ref.linear_stretch64(m125, nb, (j125, f125, j125 + 1 < len(m125)))
    med = np.where(k >= pos25, s125, np.where(k >= pos5, s25, ref.linear_stretch64(m5, nb, (j, frac, use))))
    D = X / med
    zf, zw = _zap_list(n, tsamp) if zap else ((), ())
    mask = ref.zap_mask(zf, zw, float(bw), nb)
    if name == "zap range one longer":
        mask = mask.copy()
        mask[1006] = True
    if name == "zap range one shorter":
        mask = mask.copy()
        mask[997] = False
    if name == "zap before zeroing":
        D[mask] = 1
        D[:5] = 0
    else:
        D[:5 - (name == "bin 4 not zeroed")] = 0
        D[mask] = 1
    return D, ref.stats64(ref.interbin64(D))


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("n", [N14, N17])
def test_tolerances_reject_defective_oracles(n, defect):
    nsamps, length = n - 1003, n + 13
    seed = 23 * n.bit_length()
    zap = defect != "bin 4 not zeroed"  # the zap list covers bin 4: that defect shows without it only
    D, st64, _, _, _ = _oracle(n, seed, length, nsamps, "regions", zap)
    D0, st0 = _defective("", n, seed, length, nsamps, zap)
    assert np.array_equal(D0, D) and st0 == st64, "the recomposition reproduces whiten64"
    Dd, std_ = _defective(defect, n, seed, length, nsamps, zap)
    err = np.abs(Dd - D)
    emax, erms = float(err.max()), float(np.sqrt((err ** 2).mean()))
    print(f"n={n} {defect}: max {emax:.3e} rms {erms:.3e} (tol {TOL[n][0]:.1e} / {TOL[n][1]:.1e}) "
          f"at bin {int(np.argmax(err))}")
    if defect in DEFECT_NOTES:  # below the margin (the note says why): figures only
        return
    assert emax > 100 * TOL[n][0]


@pytest.mark.parametrize("n", [N14, N17])
def test_mean_tolerance_rejects_stats_over_nbins_minus_one(n):
    nsamps, length = n - 1003, n + 13
    D, st64, _, _, _ = _oracle(n, 23 * n.bit_length(), length, nsamps)
    nb = n // 2 + 1
    rel = abs(st64[0] * nb / (nb - 1) - st64[0]) / st64[0]
    print(f"n={n} stats / (nbins - 1): mean off by {rel:.3e} (tol {TOL[n][2]:.1e})")
    assert rel > TOL[n][2]


def test_oracle_pieces_agree():
    """whiten64's pieces against the float32 reference's: positions, stretch decisions, medians, series."""
    n, nsamps = N14, N14 - 1003
    tsamp = _tsamp(n, "regions")
    bw, pos5, pos25 = ref.whiten_positions(n, tsamp)
    assert (pos5, pos25) == (400, 3999) and bw.dtype == np.float32
    amp = np.abs(np.fft.rfft(ref.convert_pad64(_row(n, 1, n)[:nsamps], n)))
    assert np.allclose(ref.running_median64(amp, pos5, pos25), ref.running_median(amp.astype(np.float32), float(bw)),
                       rtol=1e-6)
    for cnt in (1, 2, 3, 4, 5, 11):
        v = amp[:cnt]
        assert np.allclose(ref.median_scrunch5_64(v), ref.median_scrunch5(v.astype(np.float32)), rtol=1e-6)
    j, frac, use = ref.stretch_nodes(len(amp) // 5, len(amp))
    assert j.max() == len(amp) // 5 - 1 and (frac[use] > 1e-5).all() and (frac < 1.0 + 1e-6).all()
    D, st64, _, _ = ref.whiten64(_row(n, 1, n)[:nsamps], n, tsamp)
    assert D.dtype == np.complex128 and D.shape == (n // 2 + 1,)
    assert abs(np.median(np.abs(D[5:])) - 1.0) < 0.05 and 0.3 < st64[2] < 1.0
