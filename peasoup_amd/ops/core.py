"""Op implementations (see package docstring)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _C

K = _C.kernels


def _s() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a HIP (cuda) tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _cplx_ptr(t: torch.Tensor) -> int:
    _check(t, torch.complex64, "complex tensor")
    return t.data_ptr()


# ------------------------------------------------------------------ dedisp --
def unpack_transpose(packed: torch.Tensor, nsamps: int, nchans: int, nbits: int, bias: int = 0,
                     stride: Optional[int] = None) -> torch.Tensor:
    """Packed SIGPROC bytes -> int8 [nchans, stride] (value - bias)."""
    _check(packed, torch.uint8, "packed")
    stride = stride or nsamps
    out = torch.zeros((nchans, stride), dtype=torch.int8, device=packed.device)
    K.unpack_transpose(packed.data_ptr(), nsamps, nchans, nbits, out.data_ptr(), stride, bias, _s())
    return out


def dedisperse(chan_major: torch.Tensor, offsets: torch.Tensor, out_nsamps: int, scale: float, bias: int = 0,
               killmask: Optional[torch.Tensor] = None, kernel: str = "direct") -> torch.Tensor:
    """Brute-force dedispersion of an int8 [nchans, stride] block.

    offsets: int32 [ndm, nchans] sample delays.  Returns uint8 [ndm, out_nsamps].
    kernel: "direct" (VALU) or "mfma" (v_mfma_i32_32x32x32_i8 one-hot GEMM).
    """
    _check(chan_major, torch.int8, "chan_major")
    nchans, stride = chan_major.shape
    ndm = offsets.shape[0]
    dev = chan_major.device
    kill = killmask if killmask is not None else torch.ones(nchans, dtype=torch.int32, device=dev)
    nactive = int(kill.ne(0).sum())
    out = torch.empty((ndm, out_nsamps), dtype=torch.uint8, device=dev)
    if kernel == "direct":
        offs = offsets.to(dev, torch.int32).contiguous()
        K.dedisperse_direct(chan_major.data_ptr(), stride, nchans, offs.data_ptr(), kill.to(dev, torch.int32).contiguous().data_ptr(),
                            ndm, out_nsamps, out.data_ptr(), out_nsamps, float(scale), int(bias), nactive, _s())
        return out
    raise ValueError("mfma dedispersion is driven through _C.Dedisperser (needs padded rows)")


# ------------------------------------------------------------ time series --
def convert_pad(trial: torch.Tensor, n: int) -> torch.Tensor:
    """uint8 trial -> float32[n]: copy (truncate) or pad with the trial mean."""
    _check(trial, torch.uint8, "trial")
    out = torch.empty(n, dtype=torch.float32, device=trial.device)
    tmp = torch.zeros(1, dtype=torch.int64, device=trial.device)
    K.u8_to_f32_pad(trial.data_ptr(), min(trial.numel(), n), out.data_ptr(), n, tmp.data_ptr(), _s())
    return out


# ------------------------------------------------------------------ FFT -----
class FFTPlanCache:
    """rocFFT plan cache keyed by (type, n, batch)."""

    _plans: Dict[Tuple, object] = {}

    @classmethod
    def get(cls, kind: str, n: int, batch: int = 1):
        key = (kind, n, batch, torch.cuda.current_device())
        p = cls._plans.get(key)
        if p is None:
            t = {"r2c": _C.FftType.R2C, "c2r": _C.FftType.C2R, "c2c_fwd": _C.FftType.C2C_FWD,
                 "c2c_inv": _C.FftType.C2C_INV}[kind]
            p = _C.FftPlan(t, n, batch)
            cls._plans[key] = p
        return p


def rfft(x: torch.Tensor) -> torch.Tensor:
    """Unnormalised real-to-complex FFT over the last dim (rocFFT)."""
    _check(x, torch.float32, "x")
    n = x.shape[-1]
    batch = x.numel() // n
    out = torch.empty(x.shape[:-1] + (n // 2 + 1,), dtype=torch.complex64, device=x.device)
    FFTPlanCache.get("r2c", n, batch).execute(x.data_ptr(), out.data_ptr(), _s())
    return out


def irfft(X: torch.Tensor, n: int) -> torch.Tensor:
    """Unnormalised complex-to-real inverse FFT (cuFFT/rocFFT convention: x*n)."""
    Xc = X.contiguous().clone()  # C2R may overwrite its input
    batch = Xc.numel() // (n // 2 + 1)
    out = torch.empty(X.shape[:-1] + (n,), dtype=torch.float32, device=X.device)
    FFTPlanCache.get("c2r", n, batch).execute(_cplx_ptr(Xc), out.data_ptr(), _s())
    return out


# --------------------------------------------------------------- spectra ----
def form_amplitude(X: torch.Tensor) -> torch.Tensor:
    out = torch.empty(X.numel(), dtype=torch.float32, device=X.device)
    K.form_amplitude(_cplx_ptr(X), X.numel(), out.data_ptr(), _s())
    return out


def form_interbin(X: torch.Tensor) -> torch.Tensor:
    out = torch.empty(X.numel(), dtype=torch.float32, device=X.device)
    K.form_interbin(_cplx_ptr(X), X.numel(), out.data_ptr(), _s())
    return out


def normalise(x: torch.Tensor, mean: float, sigma: float) -> torch.Tensor:
    _check(x, torch.float32, "x")
    K.normalise(x.data_ptr(), x.numel(), float(mean), float(sigma), _s())
    return x


def median_scrunch5(x: torch.Tensor, from_complex: bool = False) -> torch.Tensor:
    n = x.numel()
    out = torch.empty(max(1, n // 5), dtype=torch.float32, device=x.device)
    if from_complex:
        K.median5_amp(_cplx_ptr(x), n, out.data_ptr(), _s())
    else:
        _check(x, torch.float32, "x")
        K.median5(x.data_ptr(), n, out.data_ptr(), _s())
    return out


def running_median(X: torch.Tensor):
    """The three median scrunches of Dereddener::calculate_median."""
    m5 = median_scrunch5(X, from_complex=True)
    m25 = median_scrunch5(m5)
    m125 = median_scrunch5(m25)
    return m5, m25, m125


def deredden(X: torch.Tensor, bin_width: float, zapmask: Optional[torch.Tensor] = None,
             boundary5: float = 0.05, boundary25: float = 0.5) -> torch.Tensor:
    """In place: X /= running median (bins < 5 -> 0), zapped bins -> 1+0i."""
    nb = X.numel()
    m5, m25, m125 = running_median(X)
    pos5 = int(float(torch.tensor(boundary5, dtype=torch.float32) / torch.tensor(bin_width, dtype=torch.float32)))
    pos25 = int(float(torch.tensor(boundary25, dtype=torch.float32) / torch.tensor(bin_width, dtype=torch.float32)))
    zp = 0
    if zapmask is not None:
        _check(zapmask, torch.int32, "zapmask")
        zp = zapmask.data_ptr()
    K.deredden_zap(_cplx_ptr(X), nb, m5.data_ptr(), nb // 5, m25.data_ptr(), max(1, nb // 25), m125.data_ptr(),
                   max(1, nb // 125), pos5, pos25, zp, _s())
    return X


def interbin_stats(X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Interbinned spectrum + device stats {mean, rms, std}."""
    P = torch.empty(X.numel(), dtype=torch.float32, device=X.device)
    partials = torch.empty(2048, dtype=torch.float64, device=X.device)
    st = torch.empty(4, dtype=torch.float32, device=X.device)
    K.interbin_stats(_cplx_ptr(X), X.numel(), P.data_ptr(), partials.data_ptr(), 1024, st.data_ptr(), _s())
    return P, st


def interbin_normalise(X: torch.Tensor, stats: torch.Tensor, nscale: float, nbins_out: Optional[int] = None):
    """Batched: X complex [K, B] -> (interbin(X) - mean*nscale)/(std*nscale)."""
    Kb, nb = X.shape
    nbo = nbins_out or nb
    P = torch.empty((Kb, nbo), dtype=torch.float32, device=X.device)
    K.interbin_normalise_batch(_cplx_ptr(X), nb, nb, P.data_ptr(), nbo, Kb, nbo, stats.data_ptr(), float(nscale), _s())
    return P


def r2c_interbin_normalise(x: torch.Tensor, stats: torch.Tensor, nscale: float,
                           nbins_out: Optional[int] = None) -> torch.Tensor:
    """Batched real series x [K, N] (N even) -> same output as
    ``interbin_normalise(rfft(x))`` but via an N/2-point complex FFT of the
    packed series with the real-FFT post-processing fused into the kernel."""
    _check(x, torch.float32, "x")
    Kb, n = x.shape
    assert n % 2 == 0
    M = n // 2
    Z = torch.fft.fft(torch.view_as_complex(x.contiguous().view(Kb, M, 2)), dim=-1).contiguous()
    nbo = nbins_out or (M + 1)
    P = torch.empty((Kb, nbo), dtype=torch.float32, device=x.device)
    K.r2c_interbin_normalise_batch(_cplx_ptr(Z), M, M, M.bit_length() - 1, M, 8, 3, P.data_ptr(), nbo, Kb, nbo,
                                   stats.data_ptr(), float(nscale), _s())
    return P


# ---------------------------------------------------------- acceleration ---
def resample(x: torch.Tensor, accels: Sequence[float], tsamp: float) -> torch.Tensor:
    """Batched time-domain acceleration resampling (resampleII semantics)."""
    _check(x, torch.float32, "x")
    n = x.numel()
    af = torch.tensor([(float(torch.tensor(a, dtype=torch.float32)) * float(torch.tensor(tsamp, dtype=torch.float32)))
                       / (2 * 299792458.0) for a in accels], dtype=torch.float64, device=x.device)
    stride = (n + 3) // 4 * 4
    out = torch.empty((len(accels), stride), dtype=torch.float32, device=x.device)
    K.resample_batch(x.data_ptr(), n, out.data_ptr(), stride, af.data_ptr(), len(accels), _s())
    return out[:, :n]


def _accel_factors(accels: Sequence[float], tsamp: float, device) -> torch.Tensor:
    return torch.tensor([(float(torch.tensor(a, dtype=torch.float32)) * float(torch.tensor(tsamp, dtype=torch.float32)))
                         / (2 * 299792458.0) for a in accels], dtype=torch.float64, device=device)


def _fft4_padded(x: torch.Tensor, accels: Sequence[float], tsamp: float, nbins_out: int = 0):
    _check(x, torch.float32, "x")
    n = x.numel()
    g = K.fft4_geometry(n // 2)
    if not g.ok or n % 2:
        raise ValueError(f"fft4: unsupported length {n}")
    tab = torch.from_numpy(K.fft4_tables(g)).to(x.device)
    af = _accel_factors(accels, tsamp, x.device)
    Kb = len(accels)
    xp = torch.empty(g.insize, dtype=torch.float32, device=x.device)
    Y = torch.empty((Kb, g.ystride, 2), dtype=torch.float32, device=x.device)
    X = torch.empty((Kb, g.xstride, 2), dtype=torch.float32, device=x.device)
    K.fft4_pad_input(x.data_ptr(), n, xp.data_ptr(), g, _s())
    K.fft4_resample_colpass(x.data_ptr(), xp.data_ptr(), n, af.data_ptr(), Kb, Y.data_ptr(), g, tab.data_ptr(), _s())
    K.fft4_rowpass(Y.data_ptr(), X.data_ptr(), Kb, g, tab.data_ptr(), _s(), nbins_out)
    return g, X


def fft4_x_layout(g):
    """(log2_row, row_pitch, blk_pitch, log2_blk, tiled) of the fused FFT's
    spectrum layout under the current kernel flags."""
    return K.fft4_x_layout(g)


def fft4_resample_spectrum(x: torch.Tensor, accels: Sequence[float], tsamp: float) -> torch.Tensor:
    """Fused resample + four-step FFT: returns Z [K, N/2] complex64 with
    Z[k] = FFT_{N/2}(z_k), z_k[m] = r_k[2m] + i r_k[2m+1], r_k = resample(x, accels[k])."""
    g, X = _fft4_padded(x, accels, tsamp)
    Kb = X.shape[0]
    M = g.n1 * g.n2
    log2_row, row, blk, lw, tiled = fft4_x_layout(g)
    k = torch.arange(M, device=x.device, dtype=torch.int64)
    k2 = k & (g.n2 - 1)
    k1 = k >> log2_row
    if tiled:
        addr = (k2 >> 3) * (8 * g.n1) + (k1 >> 3) * 64 + (k2 & 7) * 8 + (k1 & 7)
    else:
        addr = (k2 >> lw) * blk + k1 * row + (k2 & ((1 << lw) - 1))
    Xc = torch.view_as_complex(X)  # [K, xstride]
    return Xc[:, addr].contiguous()


def fft4_resample_interbin(x: torch.Tensor, accels: Sequence[float], tsamp: float, stats: torch.Tensor,
                           nscale: float, nbins_out: int | None = None, screen: bool = False):
    """The search hot path of fft_mode 2: fused resample + four-step FFT, then
    the paired real-FFT post-processing + interbin + normalise on the fused
    FFT's spectrum layout.  Returns P [K, N/2 + 1]; with ``nbins_out`` only
    bins below it are formed (pass B then stores only the spectrum rows the
    r2c step reads, as the search engine does) and the rest stay zero.  With
    ``screen`` (tiled layout only) returns (P, Q): Q [K, qstride] uint8 the
    screening bytes the r2c kernel writes for the harmonic sum."""
    M = (x.numel()) // 2
    nbo = M + 1 if nbins_out is None else int(nbins_out)
    g, X = _fft4_padded(x, accels, tsamp, nbins_out=0 if nbins_out is None else nbo)
    Kb = X.shape[0]
    log2_row, row, blk, lw, tiled = fft4_x_layout(g)
    P = torch.zeros((Kb, M + 1), dtype=torch.float32, device=x.device)
    if screen and not tiled:
        raise ValueError("screening bytes come from the tiled r2c kernel only")
    if tiled:
        qst = (M + 1 + 63) // 64 * 64
        Q = torch.zeros((Kb, qst), dtype=torch.uint8, device=x.device) if screen else None
        K.r2c_interbin_normalise_tiled(X.data_ptr(), g.n1, g.n2, g.xstride, P.data_ptr(), M + 1, Kb, nbo,
                                       stats.data_ptr(), float(nscale), _s(), Q.data_ptr() if screen else 0,
                                       qst if screen else 0)
        if screen:
            return P, Q
    else:
        K.r2c_interbin_normalise_batch(X.data_ptr(), M, g.xstride, log2_row, row, blk, lw, P.data_ptr(), M + 1, Kb,
                                       nbo, stats.data_ptr(), float(nscale), _s())
    return P


def fft4_spectrum_pass(x: torch.Tensor, accels: Sequence[float], tsamp: float, stats: torch.Tensor,
                       nscale: float, pair_y: bool | None = None, nbins: int = 0):
    """The search hot path with the fused spectrum pass (the default engine
    path): fused resample + pass A, then pass B forming the normalised
    interbinned spectrum and its screening bytes directly
    (kernels.hpp fft4_rowpass_spectrum).  Returns (Pb, Q, g): Pb [K, pstride]
    in the blocked layout (``spec_unblock`` gives natural order), Q [K,
    qstride] uint8 with bin b at column ``spec_q_shift`` + b.  ``pair_y``:
    pass A hands over Y in row pairs (default: where ``fft4_pair_y`` allows,
    as the search engine does).  ``nbins`` > 0: only bins below it are
    written (whole 4-bin groups; the rest of Pb / Q keeps its zeros)."""
    _check(x, torch.float32, "x")
    n = x.numel()
    g = K.fft4_geometry(n // 2)
    if not g.ok or n % 2:
        raise ValueError(f"fft4: unsupported length {n}")
    M = g.n1 * g.n2
    g.ypair = K.fft4_pair_y(g) if pair_y is None else bool(pair_y)
    tab = torch.from_numpy(K.fft4_tables(g)).to(x.device)
    af = _accel_factors(accels, tsamp, x.device)
    Kb = len(accels)
    xp = torch.empty(g.insize, dtype=torch.float32, device=x.device)
    Y = torch.empty((Kb, g.ystride, 2), dtype=torch.float32, device=x.device)
    K.fft4_pad_input(x.data_ptr(), n, xp.data_ptr(), g, _s())
    K.fft4_resample_colpass(x.data_ptr(), xp.data_ptr(), n, af.data_ptr(), Kb, Y.data_ptr(), g, tab.data_ptr(), _s())
    pst = (M + 1 + 63) // 64 * 64
    qst = (M + 1 + K.spec_q_shift + 63) // 64 * 64
    Pb = torch.zeros((Kb, pst), dtype=torch.float32, device=x.device)
    Q = torch.zeros((Kb, qst), dtype=torch.uint8, device=x.device)
    K.fft4_rowpass_spectrum(Y.data_ptr(), Kb, g, tab.data_ptr(), Pb.data_ptr(), pst, Q.data_ptr(), qst,
                            stats.data_ptr(), float(nscale), _s(), 0, int(nbins))
    return Pb, Q, g


def spec_pblk_index(b: torch.Tensor, log2_n2: int, n1: int) -> torch.Tensor:
    """kernels.hpp spec_pblk_index, vectorised: position of bins b (int64,
    0..M) in the blocked spectrum of ``fft4_spectrum_pass``."""
    n2 = 1 << log2_n2
    M = n1 * n2
    r = b & (n2 - 1)
    prim = (r >= 1) & (r <= n2 // 2)
    ip = (((r - 1) >> 2) * 2 * n1 + (b >> log2_n2)) * 4 + ((r - 1) & 3)
    bm = M - b
    rm = bm & (n2 - 1)
    im = (((rm >> 2) * 2 + 1) * n1 + (bm >> log2_n2)) * 4 + (rm & 3)
    out = torch.where(prim, ip, im)
    return torch.where(b == 0, torch.full_like(b, M), out)


def spec_unblock(Pb: torch.Tensor, g) -> torch.Tensor:
    """Natural-order P [K, M + 1] from the blocked spectrum of ``fft4_spectrum_pass``."""
    M = g.n1 * g.n2
    b = torch.arange(M + 1, device=Pb.device, dtype=torch.int64)
    return Pb[:, spec_pblk_index(b, g.log2_xrow, g.n1)]


def resample_v1(x: torch.Tensor, accel: float, tsamp: float) -> torch.Tensor:
    _check(x, torch.float32, "x")
    af = (float(torch.tensor(accel, dtype=torch.float32)) * float(torch.tensor(tsamp, dtype=torch.float32))) / (2 * 299792458.0)
    out = torch.empty_like(x)
    K.resample_v1(x.data_ptr(), x.numel(), out.data_ptr(), af, _s())
    return out


def harmonic_sums(P: torch.Tensor, nlevels: int) -> torch.Tensor:
    """Materialised harmonic sums [nlevels, n] (debug/test path)."""
    _check(P, torch.float32, "P")
    out = torch.empty((max(1, nlevels), P.numel()), dtype=torch.float32, device=P.device)
    K.harmonic_sums(P.data_ptr(), P.numel(), nlevels, out.data_ptr(), _s())
    return out[:nlevels]


def quantize_q8(P: torch.Tensor) -> torch.Tensor:
    """Screening bytes (device_common.hpp dev::q8) of spectra P [K, n]:
    [K, qstride] uint8, qstride = n rounded up to 64."""
    _check(P, torch.float32, "P")
    Kb, n = P.shape
    qst = (n + 63) // 64 * 64
    Q = torch.zeros((Kb, qst), dtype=torch.uint8, device=P.device)
    K.quantize_q8(P.data_ptr(), n, n, Kb, Q.data_ptr(), qst, _s())
    return Q


def harmonic_peaks(P: torch.Tensor, nlevels: int, starts: Sequence[int], ends: Sequence[int], thresh: float,
                   capacity: int = 1 << 20, nbins: int | None = None, Q: torch.Tensor | None = None,
                   pblk=None):
    """Fused harmonic sum + threshold: P [K, n] -> records (trial, level, idx, snr)
    as int64/float32 tensors sorted by (trial, level, idx) (the kernel's chunk
    descriptors, kernels.hpp kPeakChunk, are dropped).  ``nbins``: bins per
    spectrum when the rows are padded (default n).  ``Q``: screening bytes of
    P ([K, qstride] uint8, ``quantize_q8``) -- the screened kernel, same
    records.  ``pblk`` = the geometry ``g`` of ``fft4_spectrum_pass``: P is
    its blocked spectrum and Q its screening rows (bins shifted by
    ``spec_q_shift``)."""
    _check(P, torch.float32, "P")
    Kb, n = P.shape
    rec = torch.empty((capacity, 3), dtype=torch.int32, device=P.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=P.device)
    nb = n if nbins is None else int(nbins)
    if Q is not None:
        if Q.dtype != torch.uint8 or Q.shape[0] != Kb or not Q.is_contiguous():
            raise ValueError("Q must be a contiguous [K, qstride] uint8 tensor")
    extra = {}
    if pblk is not None:
        extra = dict(pblk_log2_n2=pblk.log2_xrow, pblk_n1=pblk.n1, qshift=K.spec_q_shift)
    K.harmonic_peaks_batch(P.data_ptr(), nb, n, Kb, nlevels, list(starts), list(ends), float(thresh), capacity,
                           rec.data_ptr(), cnt.data_ptr(), _s(), 0 if Q is None else Q.data_ptr(),
                           0 if Q is None else Q.shape[1], **extra)
    c = int(cnt.item())
    if c > capacity:
        return harmonic_peaks(P, nlevels, starts, ends, thresh, capacity=c + 1024, nbins=nbins, Q=Q, pblk=pblk)
    r = rec[:c]
    r = r[r[:, 0] >= 0]  # drop the chunk descriptors (seg field with kPeakChunk, bit 31, set)
    seg = r[:, 0].to(torch.int64)
    idx = r[:, 1].to(torch.int64)
    snr = r[:, 2].view(torch.float32)
    order = torch.argsort(seg * (1 << 32) + idx)
    return seg[order] // 8, seg[order] % 8, idx[order], snr[order]


# --------------------------------------------------------------- folding ----
def fold_series(series: torch.Tensor, periods: Sequence[float], accels: Sequence[float], tsamp: float):
    """Fold + optimise a whitened series for several (period, accel) pairs.
    Returns native FoldResult objects (folded_snr, opt_period, fold[16*64], ...)."""
    _check(series, torch.float32, "series")
    fe = _C.FoldEngine(series.numel(), float(tsamp), _s())
    return fe.fold_series(series.data_ptr(), [float(p) for p in periods], [float(a) for a in accels])


FOLD_JOB_DTYPE = [("tsamp_by_period", "<f8"), ("af", "<f8"), ("series", "<u8")]  # kern::FoldJob
_POISON = 0x7FC0DEAD  # a NaN as float32: an element the kernel skipped compares unequal to everything


def _guarded(rows: int, shape: tuple, device) -> torch.Tensor:
    """int32 [rows + 2, *shape] filled with _POISON: rows 1..rows are the
    payload, rows 0 and rows + 1 the guards."""
    return torch.full((rows + 2,) + tuple(shape), _POISON, dtype=torch.int32, device=device)


def _check_guards(buf: torch.Tensor, name: str) -> None:
    if not (bool((buf[0] == _POISON).all()) and bool((buf[-1] == _POISON).all())):
        raise RuntimeError(f"{name}: a guard row was overwritten")


def fold_raw(series: torch.Tensor, jobs, nbins: int = 64, nints: int = 16, chunk: Optional[int] = None):
    """The raw fold (fold_accumulate + fold_reduce) of a batch of series
    [nseries, n] for ``jobs``: (tsamp_by_period, af, series) records
    (FOLD_JOB_DTYPE, or a sequence of such triples).  Returns (psum float32
    [nj, nints, nchunk, nbins], pcount int32 likewise, fold float32 [nj, nints,
    nbins]).  chunk None is FoldEngine's min(4096, n // nints).  Each output
    lies between two poisoned guard rows; a changed guard raises."""
    _check(series, torch.float32, "series")
    if series.dim() != 2:
        raise ValueError("series must be [nseries, n]")
    nseries, n = int(series.shape[0]), int(series.shape[1])
    jobs = np.ascontiguousarray(np.asarray([tuple(j) for j in jobs], dtype=FOLD_JOB_DTYPE)
                                if not isinstance(jobs, np.ndarray) else jobs.astype(FOLD_JOB_DTYPE))
    if jobs.dtype.itemsize != K.fold_job_size:
        raise RuntimeError("FOLD_JOB_DTYPE does not match kern::FoldJob")
    nj = int(jobs.shape[0])
    if nj == 0:
        raise ValueError("fold_raw: no jobs")
    if int(jobs["series"].max()) >= nseries:
        raise ValueError("fold_raw: a job indexes a series past the batch")
    if nints < 1 or n < nints:
        raise ValueError("fold_raw: series shorter than nints")
    if chunk is None:
        chunk = min(4096, n // nints)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("fold_raw: chunk must be positive")
    if nbins < 1:
        raise ValueError("fold_raw: nbins must be positive")  # the launcher refuses nbins > 64
    nps = n // nints
    nchunk = (nps + chunk - 1) // chunk
    dev = series.device
    d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(nj, -1).copy()).to(dev)
    psum = _guarded(nj, (nints, nchunk, nbins), dev)
    pcount = _guarded(nj, (nints, nchunk, nbins), dev)
    fold = _guarded(nj, (nints, nbins), dev)
    K.fold_accumulate(series.data_ptr(), n, d_jobs.data_ptr(), nj, nbins, nints, chunk, psum[1].data_ptr(),
                      pcount[1].data_ptr(), _s())
    K.fold_reduce(psum[1].data_ptr(), pcount[1].data_ptr(), nj, nbins, nints, nchunk, fold[1].data_ptr(), _s())
    for buf, name in ((psum, "psum"), (pcount, "pcount"), (fold, "fold")):
        _check_guards(buf, "fold_raw " + name)
    return psum[1:-1].view(torch.float32), pcount[1:-1], fold[1:-1].view(torch.float32)


def fold_optimise(folds: torch.Tensor, return_val: bool = False):
    """Fused fold optimiser on [nfold, 16, 64] folds -> (opt_int[nfold,3], opt_fold, opt_prof), with
    ``return_val`` also opt_val[nfold] (the winning |S| / sqrt(width)).  Every
    output lies between two poisoned guard rows; a changed guard raises."""
    _check(folds, torch.float32, "folds")
    if folds.dim() != 3 or tuple(folds.shape[1:]) != (16, 64):
        raise ValueError("folds must be [nfold, 16, 64]")
    nf = folds.shape[0]
    dev = folds.device
    table = torch.empty((64, 16, 64), dtype=torch.complex64, device=dev)
    K.fold_shift_table(table.data_ptr(), 64, 16, _s())
    of = _guarded(nf, (16, 64), dev)
    op = _guarded(nf, (64,), dev)
    oi = _guarded(nf, (3,), dev)
    ov = _guarded(nf, (), dev)
    K.fold_optimise(folds.data_ptr(), nf, table.data_ptr(), of[1].data_ptr(), op[1].data_ptr(), oi[1].data_ptr(),
                    ov[1:].data_ptr(), _s())
    for buf, name in ((of, "opt_fold"), (op, "opt_prof"), (oi, "opt_int"), (ov, "opt_val")):
        _check_guards(buf, "fold_optimise " + name)
    out = (oi[1:-1], of[1:-1].view(torch.float32), op[1:-1].view(torch.float32))
    return out + (ov[1:-1].view(torch.float32),) if return_val else out


# ----------------------------------------------------------- coincidence ----
def coincidence_counts(x: torch.Tensor, thresh: float, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check(x, torch.float32, "x")
    if counts is None:
        counts = torch.zeros(x.numel(), dtype=torch.uint8, device=x.device)
    K.count_above(x.data_ptr(), x.numel(), float(thresh), counts.data_ptr(), _s())
    return counts


def coincidence_mask(counts: torch.Tensor, beam_thresh: int) -> torch.Tensor:
    _check(counts, torch.uint8, "counts")
    mask = torch.empty(counts.numel(), dtype=torch.float32, device=counts.device)
    K.coincidence_mask(counts.data_ptr(), counts.numel(), int(beam_thresh), mask.data_ptr(), _s())
    return mask


# ----------------------------------------------------------- correlation ----
def conjugate(x: torch.Tensor) -> torch.Tensor:
    K.conjugate(_cplx_ptr(x), x.numel(), _s())
    return x


def cmul_(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y <- x * y (complex, in place)."""
    K.cmul_inplace(_cplx_ptr(x), _cplx_ptr(y), y.numel(), _s())
    return y


# ----------------------------------------------------------- single pulses --
def single_pulse_search(trials: torch.Tensor, nsamps: int, params, dm_idx0: int = 0, dense: bool = False):
    """Boxcar single-pulse search of uint8 trials [ndm, row_stride] (the first
    ``nsamps`` samples of each row; row_stride a multiple of 4) with a
    ``_C.SpParams``.  Returns the ``_C.SpEvent`` list sorted by (dm_idx,
    width_log2, sample); with ``dense`` also the per-block maximum S/N
    (float32) and its sample (int64, -1 where a block has no valid start),
    each [ndm, K + 1, ceil(nsamps / 64)]."""
    _check(trials, torch.uint8, "trials")
    if trials.dim() != 2:
        raise ValueError("trials must be [ndm, row_stride]")
    ndm, stride = int(trials.shape[0]), int(trials.shape[1])
    eng = _C.SinglePulseEngine(params, int(nsamps), _s())
    if not dense:
        return eng.search_block(trials.data_ptr(), stride, ndm, int(dm_idx0))
    shape = (ndm, len(eng.widths), (int(nsamps) + _C.SP_BLOCK - 1) // _C.SP_BLOCK)
    snr = torch.empty(shape, dtype=torch.float32, device=trials.device)
    arg = torch.empty(shape, dtype=torch.int32, device=trials.device)  # the kernel's uint32, 0xffffffff = -1
    ev = eng.search_block(trials.data_ptr(), stride, ndm, int(dm_idx0), snr.data_ptr(), arg.data_ptr())
    arg = arg.to(torch.int64) & 0xFFFFFFFF
    return ev, snr, torch.where(arg == 0xFFFFFFFF, torch.full_like(arg, -1), arg)


# -------------------------------------------------------------- fold cubes --
def fold_cube(chan_major: torch.Tensor, offsets: torch.Tensor, periods, accels, tsamp: float, fold_nsamps: int,
              nints: int = 16, nsub: int = 32, nbins: int = 64, bias: int = 0, killmask=None,
              batch_bytes: int = None):
    """Folds the channel-major int8 filterbank ``chan_major`` [nchans, stride]
    (raw sample = stored value + ``bias``; stride a multiple of 16) into one
    subint x subband x phase cube per candidate: ``offsets`` int32 [ncand,
    nchans] sample offsets, ``periods`` (s) and ``accels`` (m/s^2) of length
    ncand.  Returns (sums int64 [ncand, nints, nsub, nbins], hits int32
    [ncand, nints, nbins]); integer sums, exactly the NumPy oracle's
    (utils.reference.fold_cube).  Every candidate is validated before
    anything is launched (``NativeError`` naming the candidate)."""
    _check(chan_major, torch.int8, "chan_major")
    if chan_major.dim() != 2:
        raise ValueError("chan_major must be [nchans, stride]")
    nchans, stride = int(chan_major.shape[0]), int(chan_major.shape[1])
    off = offsets.detach().to("cpu", torch.int32).contiguous()
    periods = [float(p) for p in periods]
    accels = [float(a) for a in accels]
    ncand = len(periods)
    if off.dim() != 2 or tuple(off.shape) != (ncand, nchans) or len(accels) != ncand:
        raise ValueError("offsets must be [ncand, nchans]; periods and accels of length ncand")
    kill = [] if killmask is None else [int(k) for k in killmask]
    params = _C.CubeParams(int(nints), int(nsub), int(nbins), int(fold_nsamps))
    kw = {} if batch_bytes is None else {"batch_bytes": int(batch_bytes)}
    folder = _C.CubeFolder(chan_major.data_ptr(), stride, stride, nchans, int(bias), float(tsamp), [], kill, params,
                           _s(), **kw)
    sums = torch.empty((ncand, int(nints), int(nsub), int(nbins)), dtype=torch.int64, device=chan_major.device)
    hits = torch.empty((ncand, int(nints), int(nbins)), dtype=torch.int32, device=chan_major.device)
    if ncand:
        folder.fold_offsets(off.numpy(), periods, accels, sums.data_ptr(), hits.data_ptr())
    return sums, hits


# ---------------------------------------------------------------- cubeopt --
def cube_search(d: torch.Tensor, sdm: torch.Tensor, st: torch.Tensor):
    """The search of cubeopt alone (csrc/include/psoup/cubeopt.hpp, step 3),
    with explicit shift tables and a leading candidate axis: ``d`` int32
    [ncand, nints, nsub, nbins], ``sdm`` int32 [ncand, ndm, nsub], ``st`` int32
    [ncand, np, npd, nints], every shift in [0, nbins).  Returns (best_val
    [ncand, nw], best_idx [ncand, nw], dmcurve [ncand, nw, ndm], ppd [ncand,
    nw, np, npd], centre [ncand, nw]), int32 tensors on the current device;
    exactly the NumPy oracle's (utils.reference.cube_opt_search).  Tensors
    given on the host are uploaded; the kernels read and write device memory
    through raw addresses and the results stay on the device.  The shift
    tables are checked before anything is launched (the kernel indexes with
    them): ``ValueError`` naming the candidate."""
    for t, name in ((d, "d"), (sdm, "sdm"), (st, "st")):
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    if d.dim() != 4 or sdm.dim() != 3 or st.dim() != 4:
        raise ValueError("d [ncand, nints, nsub, nbins], sdm [ncand, ndm, nsub], st [ncand, np, npd, nints]")
    ncand, nints, nsub, nbins = (int(x) for x in d.shape)
    ndm, np_, npd = int(sdm.shape[1]), int(st.shape[1]), int(st.shape[2])
    if tuple(sdm.shape) != (ncand, ndm, nsub) or tuple(st.shape) != (ncand, np_, npd, nints):
        raise ValueError("sdm must be [ncand, ndm, nsub] and st [ncand, np, npd, nints] for d's ncand, nsub and nints")
    if nints * nbins > 16384 or ndm * np_ * npd * nbins >= 2 ** 31:
        raise ValueError("nints * nbins must be at most 16384 and ndm * np * npd * nbins below 2^31")
    dev = torch.device("cuda", torch.cuda.current_device())
    d, sdm, st = (t.detach().to(dev).contiguous() for t in (d, sdm, st))
    for t, name in ((sdm, "DM"), (st, "subint")):
        bad = ((t < 0) | (t >= nbins)).reshape(ncand, -1).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"cube search: candidate {int(torch.nonzero(bad)[0])} has a {name} shift outside [0, nbins)")
    opt = _C.CubeOptimiser(_C.CubeOptGeom(nints, nsub, nbins), _C.CubeOptGrid(ndm, 0.0, np_, 1.0, npd, 1.0), _s())
    nw = opt.nwidths
    out = [torch.empty((ncand,) + shape, dtype=torch.int32, device=dev)
           for shape in ((nw,), (nw,), (nw, ndm), (nw, np_, npd), (nw,))]
    if ncand:
        opt.search_device(d.data_ptr(), sdm.data_ptr(), st.data_ptr(), ncand, *(t.data_ptr() for t in out))
    return tuple(out)


def cube_optimise(candidates, header: Dict, ndm: int = 64, np_: int = 65, npd: int = 33, dm_half_range: float = 0.0,
                  p_step: float = 1.0, pd_step: float = 1.0, delays=None, batch_bytes: int = None) -> List[Dict]:
    """cubeopt on candidate dicts (period, dm, acc, nactive, hits, sums) of a
    fold-cube file with ``header``: one record per candidate, exactly
    utils.reference.cube_optimise's.  ``delays``: the float32 delay table
    (default: the header's).  Every candidate is validated before anything is
    launched."""
    cands = list(candidates)
    if not cands:
        return []
    nints, nsub, nbins = (int(x) for x in np.asarray(cands[0]["sums"]).shape)
    geom = _C.CubeOptGeom(nints, nsub, nbins, int(header["nchans"]), int(header["fold_nsamps"]),
                          float(header["tsamp"]), float(header["fch1"]), float(header["foff"]))
    grid = _C.CubeOptGrid(int(ndm), float(dm_half_range), int(np_), float(p_step), int(npd), float(pd_step))
    if delays is None:
        delays = _C.generate_delay_table(geom.nchans, geom.tsamp, geom.fch1, geom.foff)
    kw = {} if batch_bytes is None else {"batch_bytes": int(batch_bytes)}
    opt = _C.CubeOptimiser(geom, grid, _s(), **kw)
    recs = opt.optimise([dict(c) for c in cands], [float(x) for x in delays])
    for r, c in zip(recs, cands):
        r.update(period=float(c["period"]), dm=float(np.float32(c["dm"])), acc=float(np.float32(c["acc"])))
    return recs


# --------------------------------------------------------------- burstopt --
def burst_search(d_ds: torch.Tensor, d_dmt: torch.Tensor, sf: torch.Tensor, out=None):
    """The search of burstopt alone (csrc/include/psoup/burstopt.hpp, step 3),
    with explicit shifts and a leading candidate axis: ``d_ds`` int32 [ncand,
    nsub, ntime], ``d_dmt`` int32 [ncand, ndm, ntime], ``sf`` int32 [ncand,
    nfine, nsub], every shift in [-ntime, ntime].  Returns (best_val [ncand, 2,
    nw], best_idx [ncand, 2, nw], curve [ncand, nw, ndm + nfine], curve_bin
    [ncand, nw, ndm + nfine]), int32 tensors on the current device; exactly the
    NumPy oracle's (utils.reference.burst_opt_search).  Tensors given on the
    host are uploaded; the kernels read and write device memory through raw
    addresses and the results stay on the device (in ``out``, four such
    tensors, where given).  The shifts are checked before anything is launched
    or written: ``ValueError`` naming the candidate."""
    for t, name in ((d_ds, "d_ds"), (d_dmt, "d_dmt"), (sf, "sf")):
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    if d_ds.dim() != 3 or d_dmt.dim() != 3 or sf.dim() != 3:
        raise ValueError("d_ds [ncand, nsub, ntime], d_dmt [ncand, ndm, ntime], sf [ncand, nfine, nsub]")
    ncand, nsub, ntime = (int(x) for x in d_ds.shape)
    ndm, nfine = int(d_dmt.shape[1]), int(sf.shape[1])
    if tuple(d_dmt.shape) != (ncand, ndm, ntime) or tuple(sf.shape) != (ncand, nfine, nsub):
        raise ValueError("d_dmt must be [ncand, ndm, ntime] and sf [ncand, nfine, nsub] for d_ds's ncand, nsub and ntime")
    dev = torch.device("cuda", torch.cuda.current_device())
    d_ds, d_dmt, sf = (t.detach().to(dev).contiguous() for t in (d_ds, d_dmt, sf))
    bad = ((sf < -ntime) | (sf > ntime)).reshape(ncand, -1).any(dim=1)
    if bool(bad.any()):
        raise ValueError(f"burst search: candidate {int(torch.nonzero(bad)[0])} has a shift outside [-ntime, ntime]")
    opt = _C.BurstOptimiser(_C.BurstOptGeom(ntime, nsub, ndm), _C.BurstOptGrid(nfine, 0.0), _s())
    nw = opt.nwidths
    shapes = [(ncand,) + shape for shape in ((2, nw), (2, nw), (nw, ndm + nfine), (nw, ndm + nfine))]
    if out is None:
        out = [torch.empty(shape, dtype=torch.int32, device=dev) for shape in shapes]
    else:
        out = list(out)
        if len(out) != 4 or any(t.dtype != torch.int32 or t.device != dev or tuple(t.shape) != s or not t.is_contiguous()
                                for t, s in zip(out, shapes)):
            raise ValueError("out must be four contiguous int32 device tensors: best_val, best_idx [ncand, 2, nw], "
                             "curve, curve_bin [ncand, nw, ndm + nfine]")
    if ncand:
        opt.search_device(d_ds.data_ptr(), d_dmt.data_ptr(), sf.data_ptr(), ncand, *(t.data_ptr() for t in out))
    return tuple(out)


def burst_optimise(candidates, header: Dict, nfine: int = 65, fine_half_range: float = 0.0, delays=None,
                   batch_bytes: int = None) -> List[Dict]:
    """burstopt on cutout dicts (``BurstCubeFile.candidate``'s keys) of a
    burst-cutout file with ``header`` (nchans, tsamp, fch1, foff): one record
    per candidate, exactly utils.reference.burst_optimise's.  ``delays``: the
    float32 delay table (default: the header's).  Every candidate is validated
    before anything is launched (``NativeError`` naming the candidate)."""
    cands = list(candidates)
    if not cands:
        return []
    nsub, ntime = (int(x) for x in np.asarray(cands[0]["ds_sums"]).shape)
    ndm = int(np.asarray(cands[0]["dmt_sums"]).shape[0])
    geom = _C.BurstOptGeom(ntime, nsub, ndm, int(header["nchans"]), float(header["tsamp"]), float(header["fch1"]),
                           float(header["foff"]))
    grid = _C.BurstOptGrid(int(nfine), float(fine_half_range))
    if delays is None:
        delays = _C.generate_delay_table(geom.nchans, geom.tsamp, geom.fch1, geom.foff)
    kw = {} if batch_bytes is None else {"batch_bytes": int(batch_bytes)}
    opt = _C.BurstOptimiser(geom, grid, _s(), **kw)
    return opt.optimise([dict(c) for c in cands], [float(x) for x in delays])


# ----------------------------------------------------------- burst cutouts --
def burst_cube(chan_major: torch.Tensor, ds_offsets: torch.Tensor, dmt_offsets: torch.Tensor, samples, tscrunch,
               ntime: int = 256, nsub: int = 256, bias: int = 0, killmask=None, nsamps: int = None,
               batch_bytes: int = None):
    """Cuts time-scrunched, dedispersed sums out of the channel-major int8
    filterbank ``chan_major`` [nchans, stride] (raw sample = stored value +
    ``bias``; stride a multiple of 16; the first ``nsamps`` samples of a row
    are valid, default all).  Per candidate: ``ds_offsets`` int32 [ncand,
    nchans] (the waterfall's offsets), ``dmt_offsets`` int32 [ncand, ndm,
    nchans] (one row of offsets per DM row), ``samples`` the first sample t0
    of time bin 0 (may be negative) and ``tscrunch`` the samples f per time
    bin (one int for all, or one per candidate).  Returns (ds_sums, ds_hits)
    int32 [ncand, nsub, ntime] and (dmt_sums, dmt_hits) int32 [ncand, ndm,
    ntime] as four tensors: exactly the NumPy oracle's
    (utils.reference.burst_cube_offsets).  Every candidate is validated before
    anything is launched (``NativeError`` naming the candidate)."""
    _check(chan_major, torch.int8, "chan_major")
    if chan_major.dim() != 2:
        raise ValueError("chan_major must be [nchans, stride]")
    nchans, stride = int(chan_major.shape[0]), int(chan_major.shape[1])
    ds = ds_offsets.detach().to("cpu", torch.int32).contiguous()
    dmt = dmt_offsets.detach().to("cpu", torch.int32).contiguous()
    t0 = [int(t) for t in samples]
    ncand = len(t0)
    fs = [int(tscrunch)] * ncand if isinstance(tscrunch, int) else [int(f) for f in tscrunch]
    if ds.dim() != 2 or tuple(ds.shape) != (ncand, nchans) or dmt.dim() != 3 or dmt.shape[0] != ncand or \
            dmt.shape[2] != nchans or len(fs) != ncand:
        raise ValueError("ds_offsets must be [ncand, nchans], dmt_offsets [ncand, ndm, nchans]; samples and tscrunch "
                         "of length ncand")
    ndm = int(dmt.shape[1])
    kill = [] if killmask is None else [int(k) for k in killmask]
    params = _C.BurstParams(int(ntime), int(nsub), ndm)
    kw = {} if batch_bytes is None else {"batch_bytes": int(batch_bytes)}
    cutter = _C.BurstCutter(chan_major.data_ptr(), stride, stride if nsamps is None else int(nsamps), nchans,
                            int(bias), [], kill, params, _s(), **kw)
    rows = int(nsub) + ndm
    sums = torch.empty((ncand, rows, int(ntime)), dtype=torch.int32, device=chan_major.device)
    hits = torch.empty_like(sums)
    if ncand:
        cutter.cut_offsets(ds.numpy(), dmt.numpy(), t0, fs, sums.data_ptr(), hits.data_ptr())
    ns = int(nsub)
    return (sums[:, :ns].contiguous(), hits[:, :ns].contiguous(), sums[:, ns:].contiguous(),
            hits[:, ns:].contiguous())


# ------------------------------------------------------------ RFI excision --
def _check_rows(t: torch.Tensor, name: str) -> Tuple[int, int]:
    _check(t, torch.int8, name)
    if t.dim() != 2 or t.shape[1] % 16 or t.data_ptr() % 16:
        raise ValueError(f"{name} must be int8 [nchans, stride], 16-byte aligned, stride a multiple of 16")
    return int(t.shape[0]), int(t.shape[1])


def rfi_tile() -> int:
    """Samples per workgroup of the rfi_apply kernel."""
    return int(_C.rfi_tile())


def pack_transpose(chan_major: torch.Tensor, nsamps: int, nbits: int, bias: int = 0) -> torch.Tensor:
    """int8 [nchans, stride] (value - bias) -> packed SIGPROC bytes (time-major,
    LSB-first), the inverse of ``unpack_transpose``."""
    _check(chan_major, torch.int8, "chan_major")
    nchans, stride = int(chan_major.shape[0]), int(chan_major.shape[1])
    out = torch.empty(int(nsamps) * nchans * int(nbits) // 8, dtype=torch.uint8, device=chan_major.device)
    _C.pack_transpose_raw(chan_major.data_ptr(), stride, int(nsamps), nchans, int(nbits), int(bias), out.data_ptr(),
                          _s())
    return out


def rfi_block_sums(chan_major: torch.Tensor, nsamps: int, block: int, bias: int = 0):
    """Exact block sums of the raw samples (stored value + ``bias``) of int8
    rows [nchans, stride]: (S1, S2), each int64 [nchans, ceil(nsamps / block)]
    (the kernel's uint64; the values are below 2^63)."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    nblk = -(-int(nsamps) // int(block))
    S1 = torch.empty((nchans, nblk), dtype=torch.int64, device=chan_major.device)
    S2 = torch.empty_like(S1)
    _C.rfi_block_sums_raw(chan_major.data_ptr(), stride, nchans, int(nsamps), int(block), int(bias), S1.data_ptr(),
                          S2.data_ptr(), _s())
    return S1, S2


def _rfi_params(block, thresh, chan_frac, block_frac, zero_dm):
    return _C.RfiParams(int(block), float(thresh), float(chan_frac), float(block_frac), bool(zero_dm))


def rfi_apply(chan_major: torch.Tensor, nsamps: int, nbits: int, mask, block: int, bias: int = 0,
              zero_dm: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Applies a mask (a ``_C.RfiMask``, or a dict with cell, chan_flag,
    block_flag, fill, G, nb and killmask as ``utils.reference.rfi_flag``
    returns) to int8 rows [nchans, stride]: in place, or into ``out`` (same
    layout rules, own stride).  Returns the tensor written."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    dst = chan_major if out is None else out
    _, dst_stride = _check_rows(dst, "out")
    if isinstance(mask, dict):
        mask = _C.RfiMask(int(nsamps), int(block), mask["chan_flag"], mask["block_flag"], mask["cell"], mask["fill"],
                          mask["G"], mask["nb"], [int(k) for k in mask["killmask"]])
    cleaner = _C.RfiCleaner(_rfi_params(block, 0.0, 0.0, 0.0, zero_dm), _s())
    cleaner.apply(chan_major.data_ptr(), stride, dst.data_ptr(), dst_stride, nchans, int(nsamps), int(nbits),
                  int(bias), mask)
    return dst


def rfi_clean(chan_major: torch.Tensor, nsamps: int, nbits: int, bias: int = 0, killmask=None, block: int = 4096,
              thresh: float = 5.0, chan_frac: float = 0.3, block_frac: float = 0.3, zero_dm: bool = False,
              out: Optional[torch.Tensor] = None):
    """RFI excision of int8 rows [nchans, stride] (raw sample = stored value +
    ``bias``): block sums on the device, flags on the host, mask / zero-DM
    apply on the device, in place or into ``out``.  Integer-exact: equals
    ``utils.reference.rfi_clean``.  Returns (cleaned tensor, ``_C.RfiMask``)."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    dst_ptr, dst_stride = 0, 0
    if out is not None:
        _, dst_stride = _check_rows(out, "out")
        dst_ptr = out.data_ptr()
    kill = [] if killmask is None else [int(k) for k in killmask]
    cleaner = _C.RfiCleaner(_rfi_params(block, thresh, chan_frac, block_frac, zero_dm), _s())
    mask = cleaner.clean(chan_major.data_ptr(), stride, nchans, int(nsamps), int(nbits), int(bias), kill, dst_ptr,
                         dst_stride)
    return (chan_major if out is None else out), mask


# -------------------------------------------------------------- filscrunch --
def scrunch_tile() -> int:
    """Most output samples per workgroup of the scrunch_sums kernel (the tile
    at scrunch factor f is ``_C.scrunch_tile_at(f)``; the statistics block is
    ``_C.scrunch_stat_block()``)."""
    return int(_C.scrunch_tile())


def scrunch_sums(chan_major: torch.Tensor, nsamps: int, rel, tscrunch: int, nsub: int, nout: int, bias: int = 0,
                 killmask=None):
    """Subbanded, time-scrunched sums of int8 rows [nchans, stride] (raw sample
    = stored value + ``bias``; the first ``nsamps`` samples of a row are
    valid): ``A[s, u]`` = sum over the unkilled channels c of subband s and i
    < tscrunch of ``x[c, tscrunch u + i + rel[c]]``.  Returns (A int32 [nsub,
    nout], S1, S2 int64 [nsub, ceil(nout / 4096)], the exact block sums of A
    and A^2; the kernel's uint64): exactly ``utils.reference.scrunch_sums``."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    nout, nsub = int(nout), int(nsub)
    a_stride = (nout + 15) // 16 * 16
    A = torch.empty((nsub, a_stride), dtype=torch.int32, device=chan_major.device)
    nblk = -(-nout // int(_C.scrunch_stat_block()))
    S1 = torch.empty((nsub, nblk), dtype=torch.int64, device=chan_major.device)
    S2 = torch.empty_like(S1)
    kill = [] if killmask is None else [int(k) for k in killmask]
    _C.scrunch_sums_raw(chan_major.data_ptr(), stride, int(nsamps), nchans, int(bias), int(tscrunch), nsub,
                        np.asarray(rel, dtype=np.int32), kill, nout, A.data_ptr(), a_stride, S1.data_ptr(),
                        S2.data_ptr(), _s())
    return A[:, :nout], S1, S2


def scrunch_quant(A: torch.Tensor, M, mul: int, live) -> torch.Tensor:
    """Requantises int32 sums [nsub, nout] with one offset ``M[s]`` per subband
    and one multiplier: ``clamp((((A - M) * mul + 32768) >> 16) + 128, 0,
    255)``, 128 where ``live[s]`` is 0.  Returns int8 rows [nsub, stride]
    holding y - 128 in ``pack_transpose``'s layout (stride a multiple of 16;
    the first nout samples of a row are valid)."""
    if not A.is_cuda or A.dtype != torch.int32 or A.dim() != 2:
        raise ValueError("A must be an int32 HIP tensor [nsub, nout]")
    nsub, nout = int(A.shape[0]), int(A.shape[1])
    a_stride = (nout + 15) // 16 * 16
    a = torch.zeros((nsub, a_stride), dtype=torch.int32, device=A.device)
    a[:, :nout] = A
    y = torch.empty((nsub, a_stride), dtype=torch.int8, device=A.device)
    _C.scrunch_quant_raw(a.data_ptr(), a_stride, nsub, nout, np.asarray(M, dtype=np.int32),
                         np.asarray(live, dtype=np.uint8), int(mul), y.data_ptr(), a_stride, _s())
    return y


def scrunch(chan_major: torch.Tensor, nsamps: int, nbits: int, delays, dm: float = 0.0, nsub: int = 0,
            tscrunch: int = 1, sigma_out: float = 16.0, bias: int = 0, killmask=None, foff: float = -1.0,
            budget_bytes: Optional[int] = None):
    """filscrunch on int8 rows [nchans, stride]: sums, host scale, requantise
    (``_C.Scruncher``).  Returns (y int8 [nsub, stride'] holding y - 128 in
    ``pack_transpose``'s layout, the result dict: nout, M, mul, live, S1, S2,
    nactive, rel, killmask, chunks, ...).  Integer-exact: equals
    ``utils.reference``'s scrunch_sums / scrunch_scale / scrunch_quant.
    Everything is validated before anything is launched (``NativeError``)."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    kill = [] if killmask is None else [int(k) for k in killmask]
    kw = {} if budget_bytes is None else {"budget_bytes": int(budget_bytes)}
    scr = _C.Scruncher(chan_major.data_ptr(), stride, int(nsamps), nchans, int(nbits), int(bias), float(foff),
                       [float(d) for d in delays], kill,
                       _C.ScrunchParams(float(dm), int(nsub), int(tscrunch), float(sigma_out)), _s(), **kw)
    y_stride = (int(scr.nout) + 255) // 256 * 256
    y = torch.zeros((int(scr.nsub), y_stride), dtype=torch.int8, device=chan_major.device)
    res = scr.run(y.data_ptr(), y_stride)
    res["launches"] = int(scr.launches)
    return y, res


# ----------------------------------------------------------------- fildigi --
_DIGI_DTYPES = {torch.uint8: (8, False), torch.int8: (8, True), torch.uint16: (16, False), torch.float32: (32, False)}


def _check_digi(x: torch.Tensor):
    if not x.is_cuda or x.dim() != 2 or x.dtype not in _DIGI_DTYPES or not x.is_contiguous():
        raise ValueError("x must be a contiguous HIP tensor [nsamps, nchans] of uint8, int8, uint16 or float32")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("x must hold at least one sample")
    return (int(x.shape[0]), int(x.shape[1])) + _DIGI_DTYPES[x.dtype]


def digi_block_sums(x: torch.Tensor):
    """Exact block statistics of time-major samples [nsamps, nchans] (uint8,
    int8, uint16 or float32) per channel and block of 4096 samples: a dict of
    N (finite samples; the kernel's uint32 as int64), S1 int64, S2 (the
    kernel's uint64 bits as int64), E int32 (the block quantum's exponent; 0
    for integer input), all [nchans, nblk], and nbad int64 [nchans]: exactly
    ``utils.reference.digi_block_sums``."""
    nsamps, nchans, nbits, signed = _check_digi(x)
    nblk = -(-nsamps // int(_C.digi_stat_block()))
    N = torch.empty((nchans, nblk), dtype=torch.int32, device=x.device)
    S1 = torch.empty((nchans, nblk), dtype=torch.int64, device=x.device)
    S2 = torch.empty_like(S1)
    E = torch.empty_like(N)
    _C.digi_block_sums_raw(x.data_ptr(), nbits, signed, nsamps, nchans, N.data_ptr(), S1.data_ptr(), S2.data_ptr(),
                           E.data_ptr(), _s())
    N = N.to(torch.int64) & 0xFFFFFFFF
    return {"N": N, "S1": S1, "S2": S2, "E": E, "nbad": nsamps - N.sum(dim=1)}


def digi_quant(x: torch.Tensor, mean, gain, J: int = 0, flip: bool = False):
    """Requantises time-major samples [nsamps, nchans] to 8 bits with explicit
    tables ``mean`` and ``gain`` (float64 [nint, nchans], input channel order,
    gain 0 = not live; interval of sample t: ``t // 4096 // J``, 0 for J = 0):
    ``clamp(rint((x - mean) * gain) + 128, 0, 255)``, 128 for a non-finite
    sample or a cell that is not live, the band reversed when ``flip``.
    Returns (y uint8 [nsamps, nchans], nclip)."""
    nsamps, nchans, nbits, signed = _check_digi(x)
    total = nsamps * nchans
    buf = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=x.device)
    nclip = _C.digi_quant_raw(x.data_ptr(), nbits, signed, nsamps, nchans, int(J),
                              np.ascontiguousarray(mean, dtype=np.float64).reshape(-1),
                              np.ascontiguousarray(gain, dtype=np.float64).reshape(-1), bool(flip), buf.data_ptr(),
                              _s())
    return buf[:total].view(nsamps, nchans), int(nclip)


def digitise(data: np.ndarray, foff: float, sigma_out: float = 16.0, scale: str = "channel", rescale_blocks: int = 0,
             killmask=None, budget_bytes: Optional[int] = None):
    """fildigi on host samples ``data`` [nsamps, nchans] (a NumPy array of
    uint8, int8, uint16 or float32: the file, possibly larger than the device
    budget): block sums, host scale, requantise (``_C.Digitiser``), in time
    chunks of whole blocks.  Returns (y uint8 NumPy [nsamps, nchans] in output
    channel order, the result dict: N, S1, S2, E, nbad, mean, gain, live,
    killmask, nclip, chunks, launches, ...).  Equals ``utils.reference``'s
    digi_block_sums / digi_scale / digi_quant.  Everything is validated before
    anything is launched (``NativeError``)."""
    kinds = {np.dtype(np.uint8): (8, False), np.dtype(np.int8): (8, True), np.dtype(np.uint16): (16, False),
             np.dtype(np.float32): (32, False)}
    data = np.ascontiguousarray(data)
    if data.dtype not in kinds or data.ndim != 2:
        raise ValueError("data must be [nsamps, nchans] of uint8, int8, uint16 or float32")
    nbits, signed = kinds[data.dtype]
    nsamps, nchans = data.shape
    kill = [] if killmask is None else [int(k) for k in killmask]
    kw = {} if budget_bytes is None else {"budget_bytes": int(budget_bytes)}
    dig = _C.Digitiser(data.reshape(-1).view(np.uint8), nbits, signed, int(nsamps), int(nchans), float(foff), kill,
                       _C.DigiParams(float(sigma_out), str(scale), int(rescale_blocks)), _s(), **kw)
    y, res = dig.run()
    res["launches"] = int(dig.launches)
    res["chunk_samples"] = int(dig.chunk_samples)
    return y, res


# ---------------------------------------------------------------- fits2fil --
def fits_decode(data: torch.Tensor, scl: torch.Tensor, offs: torch.Tensor, wts: torch.Tensor, slot_row, nsblk: int,
                nbits: int, signed: bool = False, pols: Tuple[int, int] = (0, -1), z: float = 0.0, t0: int = 0,
                count: Optional[int] = None) -> torch.Tensor:
    """Decodes PSRFITS rows on the device (csrc/kernels/psrfits.hip).  data:
    uint8 [nrows, nsblk * npol * nchan * nbits / 8], the DATA fields as in the
    file; scl, offs float32 [nrows, npol, nchan]; wts float32 [nrows, nchan];
    slot_row: the file row of every output slot of nsblk samples, -1 for a
    dropped one.  Returns x float32 [count, nchan], samples [t0, t0 + count):
    bit for bit ``utils.reference.fits_decode``."""
    _check(data, torch.uint8, "data")
    for t, name in ((scl, "scl"), (offs, "offs"), (wts, "wts")):
        _check(t, torch.float32, name)
    if scl.dim() != 3 or offs.shape != scl.shape or wts.dim() != 2 or data.dim() != 2:
        raise ValueError("scl and offs must be [nrows, npol, nchan], wts [nrows, nchan], data [nrows, bytes]")
    nrows, npol, nchan = (int(v) for v in scl.shape)
    if tuple(wts.shape) != (nrows, nchan) or data.shape[0] != nrows:
        raise ValueError("data, scl, offs and wts must hold the same rows and channels")
    if nbits not in (1, 2, 4, 8, 16) or (nchan * nbits) % 8 or nsblk < 1:
        raise ValueError("nbits must be 1, 2, 4, 8 or 16 with nchan * nbits a multiple of 8")
    if data.shape[1] != nsblk * npol * nchan * nbits // 8:
        raise ValueError("data must hold nsblk * npol * nchan * nbits / 8 bytes per row")
    slot_row = [int(r) for r in slot_row]
    nsamps = len(slot_row) * nsblk
    count = nsamps - t0 if count is None else int(count)
    if t0 < 0 or count < 1 or t0 + count > nsamps:
        raise ValueError("[t0, t0 + count) must lie within the slots")
    a, b = int(pols[0]), int(pols[1])
    if not 0 <= a < npol or not -1 <= b < npol:
        raise ValueError("polarisation out of range")
    k0, k1 = t0 // nsblk, (t0 + count - 1) // nsblk
    out = torch.empty((count, nchan), dtype=torch.float32, device=data.device)
    _C.fits_decode_raw(data.data_ptr(), scl.data_ptr(), offs.data_ptr(), wts.data_ptr(), nrows, slot_row[k0:k1 + 1],
                       int(nsblk), npol, nchan, int(nbits), bool(signed), a, b, float(np.float32(z)), int(t0), count,
                       out.data_ptr(), _s())
    return out


def fits_digitise(file_bytes, sigma_out: float = 16.0, scale: str = "channel", rescale_blocks: int = 0, killmask=None,
                  pol: int = -1, no_scales: bool = False, no_offsets: bool = False, no_weights: bool = False,
                  telescope_id: int = -1, machine_id: int = 0, rawdatafile: str = "",
                  budget_bytes: Optional[int] = None):
    """fits2fil on a search-mode PSRFITS file held in host memory (bytes or a
    uint8 NumPy array): decode, block sums, host scale, requantise
    (``_C.FitsDigitiser``), in time chunks of whole blocks.  Returns (y uint8
    NumPy [nsamps, nchan] in output channel order, the result dict: header,
    rows, ndropped, pols, z, N, S1, S2, E, nbad, mean, gain, live, killmask,
    nclip, chunks, launches, ...).  Equals ``utils.reference.fits_filterbank``.
    Everything is validated before anything is launched (``NativeError``)."""
    buf = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(file_bytes, dtype=np.uint8).reshape(-1)
    kill = [] if killmask is None else [int(k) for k in killmask]
    kw = {} if budget_bytes is None else {"budget_bytes": int(budget_bytes)}
    opt = _C.FitsOptions(int(pol), bool(no_scales), bool(no_offsets), bool(no_weights), int(telescope_id),
                         int(machine_id))
    dig = _C.FitsDigitiser(buf, opt, kill, _C.DigiParams(float(sigma_out), str(scale), int(rescale_blocks)),
                           str(rawdatafile), _s(), **kw)
    y, res = dig.run()
    res["launches"] = int(dig.launches)
    res["chunk_samples"] = int(dig.chunk_samples)
    return y, res


# --------------------------------------------------------------- filinject --
# csrc/include/psoup/inject.hpp (definition), csrc/kernels/inject.hip.
def inject_tile() -> int:
    """Samples per workgroup of the inject kernel."""
    return int(_C.inject_tile())


def _inject_signals(signals) -> list:
    """PulsarSpec / BurstSpec (utils.synthetic) or ``_C.InjectSignal`` -> ``_C.InjectSignal``."""
    out = []
    for s in signals:
        if isinstance(s, _C.InjectSignal):
            out.append(s)
        elif hasattr(s, "period"):
            out.append(_C.InjectSignal("pulsar", float(s.period), float(s.dm), float(s.amplitude), float(s.duty),
                                       float(s.accel), float(s.phase), float(getattr(s, "alpha", 0.0))))
        else:
            out.append(_C.InjectSignal("burst", float(s.time), float(s.dm), float(s.amplitude), float(s.width), 0.0,
                                       0.0, float(getattr(s, "alpha", 0.0))))
    return out


def inject_tables(signals, header: Dict, nsamps: int, unit, smear: bool = True) -> Dict:
    """The host tables of the definition (no GPU): sigc, delay, inv_w, w, A_q,
    T, tsamp, nlive for ``signals`` in the filterbank ``header`` describes;
    ``unit`` [nchans] is each channel's sigma (or 1), 0 where untouched.
    Equals ``utils.reference.inject_tables``."""
    return _C.inject_tables(_inject_signals(signals), int(header["nchans"]), int(header["nbits"]), int(nsamps),
                            float(header["tsamp"]), float(header["fch1"]), float(header["foff"]),
                            np.asarray(unit, dtype=np.float64), bool(smear))


def inject(chan_major: torch.Tensor, nsamps: int, nbits: int, tables: Dict, seed: int = 0, t0: int = 0,
           bias: int = 0):
    """The inject kernel alone, in place on int8 rows [nchans, stride] (raw
    sample = stored value + ``bias``) that hold the file's samples from ``t0``
    on, with explicit ``tables`` (as ``inject_tables`` or the oracle's).
    Returns (the tensor, nclip, touched [nsig]); equals
    ``utils.reference.inject_apply``."""
    nchans, stride = _check_rows(chan_major, "chan_major")
    if int(tables["delay"].shape[1]) != nchans:
        raise ValueError("the tables do not fit the rows")
    if int(nsamps) > stride:
        raise ValueError("nsamps exceeds the stride")
    nclip, touched = _C.inject_raw(chan_major.data_ptr(), stride, int(nsamps), int(nbits), int(bias), int(t0),
                                   np.asarray(tables["sigc"], dtype=np.float64), float(tables["tsamp"]),
                                   np.asarray(tables["delay"], dtype=np.float64),
                                   np.asarray(tables["inv_w"], dtype=np.float64),
                                   np.asarray(tables["A_q"], dtype=np.uint32),
                                   np.asarray(tables["T"], dtype=np.uint16), int(seed), _s())
    return chan_major, int(nclip), touched


def inject_filterbank_bytes(packed: np.ndarray, header: Dict, nsamps: int, signals, killmask=None, seed: int = 0,
                            units: str = "sigma", smear: bool = True, budget_bytes: Optional[int] = None):
    """filinject on the packed bytes of a filterbank's data block (a NumPy
    uint8 array on the host): the native ``Injector`` in time chunks
    (statistics pass, host tables, injection pass).  ``signals``: PulsarSpec /
    BurstSpec.  Returns (packed bytes out, result dict with nclip, touched,
    sigma, truth, chunks and the tables).  Everything is validated before the
    first launch."""
    if units not in ("sigma", "level"):
        raise ValueError("inject: units must be sigma or level")
    kill = [] if killmask is None else [int(k) for k in killmask]
    kw = {} if budget_bytes is None else {"budget_bytes": int(budget_bytes)}
    inj = _C.Injector(np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1), int(header["nchans"]),
                      int(header["nbits"]), int(nsamps), float(header["tsamp"]), float(header["fch1"]),
                      float(header["foff"]), _inject_signals(signals), kill, units == "sigma", bool(smear), int(seed),
                      _s(), **kw)
    y, res = inj.run()
    res["chunk_samples"] = int(inj.chunk_samples)
    return y, res


# ------------------------------------------------------------------ jerk ----
def jerk_factors(jerks: Sequence[float], tsamp: float) -> np.ndarray:
    """The definition's jf (float64) of jerk trials in m/s^3 (taken as float32,
    like ``tsamp``): jerk tsamp^2 / (6 c).  Equals ``utils.reference.jerk_factor``."""
    return np.array([_C.jerk_factor(float(np.float32(j)), float(np.float32(tsamp))) for j in jerks], dtype=np.float64)


def jerk_resample(trials: torch.Tensor, n: int, jerks: Sequence[float], tsamp: float, nrow: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, factors=None) -> torch.Tensor:
    """The jerk_resample kernel: uint8 rows ``trials`` [nrows, row_stride], of
    which the first ``nrow`` samples (default: all) are the row and the first
    ``n`` the resampled span, re-indexed at each jerk trial.  Returns ``out``
    [nrows, K, out_stride] (allocated as [nrows, K, nrow] when not given) with
    out[r, k, :nrow] the definition's y; bytes past nrow are not written.
    ``factors`` gives the jerk factors themselves instead of ``jerks`` and
    ``tsamp``.  Equals ``utils.reference.jerk_resample`` byte for byte."""
    _check(trials, torch.uint8, "trials")
    if trials.dim() != 2:
        raise ValueError("trials must be [nrows, row_stride]")
    nrows, row_stride = int(trials.shape[0]), int(trials.shape[1])
    nrow = row_stride if nrow is None else int(nrow)
    jf = jerk_factors(jerks, tsamp) if factors is None else np.asarray(factors, dtype=np.float64).reshape(-1)
    K = int(jf.size)
    if out is None:
        out = torch.empty((nrows, K, nrow), dtype=torch.uint8, device=trials.device)
    _check(out, torch.uint8, "out")
    if out.dim() != 3 or int(out.shape[0]) != nrows or int(out.shape[1]) != K:
        raise ValueError("out must be [nrows, K, out_stride]")
    if not 1 <= int(n) <= nrow <= min(row_stride, int(out.shape[2])):
        raise ValueError("need 1 <= n <= nrow <= the strides")
    jf = np.ascontiguousarray(jf, dtype=np.float64)
    d_jf = torch.from_numpy(jf).to(trials.device)  # freed stream-ordered by torch's allocator
    _C.jerk_resample_raw(trials.data_ptr(), row_stride, nrows, nrow, int(n), jf, d_jf.data_ptr(), out.data_ptr(),
                         int(out.shape[2]), _s())
    return out


# ----------------------------------------------------------------- orbit ----
_ORBIT_TABLES: Dict = {}


def orbit_quantise(templates, tsamp: float):
    """The definition's (W, F, Aq) of circular-orbit templates (pb s, a1
    light-seconds, phase turns) at the float32 ``tsamp``; every refusal of the
    quantisation is raised by name.  Equals ``utils.reference.orbit_quantise``."""
    ts = float(np.float32(tsamp))
    return [tuple(int(v) for v in _C.orbit_quantise(float(pb), float(a1), float(ph), ts)) for pb, a1, ph in templates]


def _orbit_table(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index)
    if key not in _ORBIT_TABLES:
        _ORBIT_TABLES[key] = torch.from_numpy(np.ascontiguousarray(_C.orbit_sine_table(), dtype=np.int32)).to(device)
    return _ORBIT_TABLES[key]


def orbit_resample(trials: torch.Tensor, n: int, templates, tsamp: float, nrow: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, quant=None) -> torch.Tensor:
    """The orbit_resample kernel: uint8 rows ``trials`` [nrows, row_stride], of
    which the first ``nrow`` samples (default: all) are the row and the first
    ``n`` the resampled span, re-indexed at each template.  Returns ``out``
    [nrows, K, out_stride] (allocated as [nrows, K, nrow] when not given) with
    out[r, k, :nrow] the definition's y; bytes past nrow are not written.
    ``quant`` gives the quantised templates (W, F, Aq) themselves instead of
    ``templates`` and ``tsamp``.  Equals ``utils.reference.orbit_resample`` byte
    for byte."""
    _check(trials, torch.uint8, "trials")
    if trials.dim() != 2:
        raise ValueError("trials must be [nrows, row_stride]")
    nrows, row_stride = int(trials.shape[0]), int(trials.shape[1])
    nrow = row_stride if nrow is None else int(nrow)
    q = orbit_quantise(templates, tsamp) if quant is None else [tuple(int(v) for v in t) for t in quant]
    K = len(q)
    if out is None:
        out = torch.empty((nrows, K, nrow), dtype=torch.uint8, device=trials.device)
    _check(out, torch.uint8, "out")
    if out.dim() != 3 or int(out.shape[0]) != nrows or int(out.shape[1]) != K:
        raise ValueError("out must be [nrows, K, out_stride]")
    if not 1 <= int(n) <= nrow <= min(row_stride, int(out.shape[2])):
        raise ValueError("need 1 <= n <= nrow <= the strides")
    packed = np.array([[t[0], t[1], t[2] & 0xFFFFFFFFFFFFFFFF] for t in q], dtype=np.uint64).reshape(-1, 3)
    d_q = torch.from_numpy(packed.view(np.int64)).to(trials.device)  # freed stream-ordered by torch's allocator
    _C.orbit_resample_raw(trials.data_ptr(), row_stride, nrows, nrow, int(n), q, d_q.data_ptr(),
                          _orbit_table(trials.device).data_ptr(), out.data_ptr(), int(out.shape[2]), _s())
    return out


# ---------------------------------------------------------------- orbopt ----
def orbopt_fold(trials: torch.Tensor, n: int, G, quant, nints: int, nbins: int, row_of=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The orbopt_fold kernel (csrc/include/psoup/orbopt.hpp, step 2): uint8
    rows ``trials`` [nrows, row_stride]; candidate c folds the first ``n``
    samples of row ``row_of[c]`` (default: row c) with the phase step ``G[c]``
    at its quantised templates ``quant[c]`` (K triples (W, F, Aq), the same K
    for every candidate).  Returns ``out`` int32 [ncand, K, nints, nbins],
    zeroed and written here.  ``trials`` may be a view whose rows are further
    apart than they are long.  Equals ``utils.reference.orbopt_fold`` exactly."""
    if not trials.is_cuda or trials.dtype != torch.uint8:
        raise ValueError("trials must be a uint8 HIP (cuda) tensor")
    if trials.dim() != 2:
        raise ValueError("trials must be [nrows, row_stride]")
    nrows, row_stride = int(trials.shape[0]), int(trials.stride(0))
    if trials.stride(1) != 1:
        raise ValueError("the samples of a row must be contiguous")
    G = [int(g) for g in G]
    ncand = len(G)
    rows = list(range(ncand)) if row_of is None else [int(r) for r in row_of]
    if ncand < 1 or len(quant) != ncand or len(rows) != ncand or any(not 0 <= r < nrows for r in rows):
        raise ValueError("need one G, one row in [0, nrows) and one template list per candidate")
    K = len(quant[0])
    if K < 1 or any(len(q) != K for q in quant):
        raise ValueError("every candidate needs the same number K >= 1 of templates")
    if not 1 <= int(n) <= int(trials.shape[1]):
        raise ValueError("need 1 <= n <= the row length")
    q = [tuple(int(v) for v in t) for c in quant for t in c]
    if out is None:
        out = torch.empty((ncand, K, nints, nbins), dtype=torch.int32, device=trials.device)
    _check(out, torch.int32, "out")
    if tuple(out.shape) != (ncand, K, nints, nbins) or not out.is_contiguous():
        raise ValueError("out must be contiguous [ncand, K, nints, nbins]")
    dev = trials.device
    packed = np.array([[t[0], t[1], t[2] & 0xFFFFFFFFFFFFFFFF] for t in q], dtype=np.uint64).reshape(-1, 3)
    d_q = torch.from_numpy(packed.view(np.int64)).to(dev)  # freed stream-ordered by torch's allocator
    d_G = torch.from_numpy(np.array(G, dtype=np.uint64).view(np.int64)).to(dev)
    d_rows = torch.tensor(rows, dtype=torch.int32, device=dev)
    in_bytes = (nrows - 1) * row_stride + int(trials.shape[1])
    _C.orbopt_fold_raw(trials.data_ptr(), row_stride, in_bytes, rows, d_rows.data_ptr(), d_G.data_ptr(), q,
                       d_q.data_ptr(), K, int(n), int(nints), int(nbins), _orbit_table(dev).data_ptr(), out.data_ptr(),
                       _s())
    return out


def orbopt_search(fold: torch.Tensor, hits: torch.Tensor, m: torch.Tensor, st) -> Dict[str, torch.Tensor]:
    """The orbopt_search kernel (orbopt.hpp, step 4): ``fold`` int32 [ncand, K,
    nints, nbins], ``hits`` int32 [ncand, nints, nbins], ``m`` int32 [ncand]
    on the device, ``st`` the drift table [np, nints] on the host with every
    shift in [0, nbins).  Returns device tensors best_val, best_idx, centre
    int32 [ncand, nw], tcurve int32 [ncand, nw, K], msum int64 [ncand, K].
    Equals ``utils.reference.orbopt_search`` exactly."""
    for t, name in ((fold, "fold"), (hits, "hits"), (m, "m")):
        _check(t, torch.int32, name)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if fold.dim() != 4:
        raise ValueError("fold must be [ncand, K, nints, nbins]")
    ncand, K, nints, nbins = (int(v) for v in fold.shape)
    st = np.ascontiguousarray(st, dtype=np.int32)
    if tuple(hits.shape) != (ncand, nints, nbins) or tuple(m.shape) != (ncand,) or st.ndim != 2 or st.shape[1] != nints:
        raise ValueError("hits must be [ncand, nints, nbins], m [ncand] and st [np, nints]")
    np_ = int(st.shape[0])
    nw = int(_C.oopt_nwidths(nbins))
    dev = fold.device
    d_st = torch.from_numpy(st).to(dev)
    keys = torch.empty((ncand, nw), dtype=torch.int64, device=dev)
    out = {"best_val": torch.empty((ncand, nw), dtype=torch.int32, device=dev),
           "best_idx": torch.empty((ncand, nw), dtype=torch.int32, device=dev),
           "centre": torch.empty((ncand, nw), dtype=torch.int32, device=dev),
           "tcurve": torch.empty((ncand, nw, K), dtype=torch.int32, device=dev),
           "msum": torch.empty((ncand, K), dtype=torch.int64, device=dev)}
    _C.orbopt_search_raw(fold.data_ptr(), hits.data_ptr(), m.data_ptr(), [int(v) for v in st.ravel()], d_st.data_ptr(),
                         ncand, K, nints, nbins, np_, keys.data_ptr(), out["best_val"].data_ptr(),
                         out["best_idx"].data_ptr(), out["tcurve"].data_ptr(), out["centre"].data_ptr(),
                         out["msum"].data_ptr(), _s())
    return out


def orbit_optimise(fb, candidates, fft_size: int, **params):
    """orbopt on a resident ``_C.DeviceFilterbank`` whose DM list holds every
    candidate's DM: ``candidates`` are (period, dm, acc, pb, a1, phase) tuples,
    ``params`` the fields of ``_C.OrbOptParams`` (nbins, nints, npb, na1, nphase,
    np, p_step, pb_step, a1_step, phase_step) and optionally ``batch_bytes``.
    Returns one record dict per candidate, as ``utils.reference.orbit_optimise``."""
    kw = {}
    if "batch_bytes" in params:
        kw["batch_bytes"] = int(params.pop("batch_bytes"))
    opt = _C.OrbitOptimiser(_C.OrbOptParams(**params), fb, int(fft_size), _s(), **kw)
    return opt.optimise([tuple(float(v) for v in c) for c in candidates])


# -------------------------------------------------------------- sideband ----
_SB_TWIDDLES: Dict = {}
SB_EVENT_DTYPE = [("dm_idx", "<i4"), ("m", "<i4"), ("seg", "<i4"), ("j", "<i4"), ("S", "<f4")]  # SbEvent


def _sb_twiddles(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index)
    if key not in _SB_TWIDDLES:
        _SB_TWIDDLES[key] = torch.from_numpy(np.ascontiguousarray(_C.sb_twiddles(), dtype=np.complex64)).to(device)
    return _SB_TWIDDLES[key]


def _sb_zap_words(zapmask, nbins: int, device) -> Tuple[Optional[torch.Tensor], int]:
    """A boolean mask per bin (True = zapped) -> (build_zap_mask's uint32 words
    on the device as int32, or None; the host copy's bits as a bool array)."""
    if zapmask is None:
        return None, None
    z = np.zeros((nbins + 31) // 32 * 32, dtype=bool)
    z[:nbins] = np.asarray(zapmask, dtype=bool)[:nbins]
    words = np.packbits(z.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.view(np.int32).copy()).to(device), z[:nbins]


def sideband_power(spec: torch.Tensor, k_lo: int, k_hi: int, zapmask=None, out: Optional[torch.Tensor] = None):
    """The sb_power kernels: complex64 spectra ``spec`` [nrows, nbins] ->
    (mu float64 [nrows], P float32 [nrows, stride]) with P written on [k_lo,
    k_hi) only (``out`` given: into it; else a zeroed [nrows, nbins rounded up
    to 4]).  ``zapmask``: a boolean per bin (True = zapped) or None.  Equals
    ``utils.reference.sideband_power`` (mu to 1e-12, P to 4 ulp)."""
    _check(spec, torch.complex64, "spec")
    if spec.dim() != 2:
        raise ValueError("spec must be [nrows, nbins]")
    nrows, nb = int(spec.shape[0]), int(spec.shape[1])
    k_lo, k_hi = int(k_lo), int(k_hi)
    if not 0 <= k_lo < k_hi <= nb:
        raise ValueError("need 0 <= k_lo < k_hi <= nbins")
    dev = spec.device
    if out is None:
        out = torch.zeros((nrows, (nb + 3) // 4 * 4), dtype=torch.float32, device=dev)
    _check(out, torch.float32, "out")
    if out.dim() != 2 or int(out.shape[0]) != nrows or int(out.shape[1]) < k_hi:
        raise ValueError("out must be [nrows, stride >= k_hi]")
    words, bits = _sb_zap_words(zapmask, nb, dev)
    count = (k_hi - k_lo) if bits is None else int((k_hi - k_lo) - np.count_nonzero(bits[k_lo:k_hi]))
    if count < 1:
        raise ValueError("sideband: the band has no unzapped bin")
    nranges = (k_hi - k_lo + _C.SB_RANGE - 1) // _C.SB_RANGE
    partials = torch.empty((nrows, nranges), dtype=torch.float64, device=dev)
    mu = torch.empty(nrows, dtype=torch.float64, device=dev)
    _C.sb_power_raw(spec.data_ptr(), nb, nrows, 0 if words is None else words.data_ptr(), k_lo, k_hi, count,
                    partials.data_ptr(), mu.data_ptr(), out.data_ptr(), int(out.shape[1]), _s())
    return mu, out


def sideband_search(P: torch.Tensor, k_lo: int, k_hi: int, m_lo: int = 5, m_hi: int = 13, j_min: int = 2,
                    clip: float = 32.0, min_power: float = 30.0, dm0: int = 0, capacity: int = 65536,
                    dense: bool = True):
    """The sb_search kernel on float32 rows ``P`` [nrows, stride] (stride a
    multiple of 4; read on [k_lo, k_hi) only).  Returns a dict: ``best_S``
    float32 and ``best_j`` int32 [nrows, m_hi - m_lo + 1, seg_stride] (``dense``;
    entries past a size's segment count keep the poison, a NaN as float32),
    ``nseg`` per size, ``count`` (all events of S >= min_power, which may pass
    ``capacity``) and ``events``, the min(count, capacity) records written, a
    structured array (SB_EVENT_DTYPE).  Every output lies between poisoned
    guards; a changed guard raises.  Equals ``utils.reference.sideband_search``
    within its bound."""
    _check(P, torch.float32, "P")
    if P.dim() != 2:
        raise ValueError("P must be [nrows, stride]")
    nrows, stride = int(P.shape[0]), int(P.shape[1])
    g = _C.sb_band_geometry(int(k_lo), int(k_hi), int(m_lo), int(m_hi))
    if int(k_hi) > stride:
        raise ValueError("the band passes a row")
    dev = P.device
    nm = int(m_hi) - int(m_lo) + 1
    ss = max(int(g.seg_stride), 1)
    capacity = int(capacity)
    ev_words = _C.SB_EVENT_BYTES // 4
    bs = _guarded(nrows, (nm, ss), dev) if dense else None
    bj = _guarded(nrows, (nm, ss), dev) if dense else None
    ev = _guarded(max(capacity, 1), (ev_words,), dev)
    cnt = _guarded(1, (1,), dev)
    cnt[1] = 0
    _C.sb_search_raw(P.data_ptr(), stride, nrows, int(k_lo), int(k_hi), int(m_lo), int(m_hi), int(j_min), float(clip),
                     float(min_power), int(dm0), _sb_twiddles(dev).data_ptr(),
                     bs[1:].data_ptr() if dense else 0, bj[1:].data_ptr() if dense else 0, ss,
                     ev[1:].data_ptr(), capacity, cnt[1:].data_ptr(), _s())
    torch.cuda.current_stream().synchronize()
    for buf, name in ((bs, "best_S"), (bj, "best_j"), (ev, "events"), (cnt, "count")):
        if buf is not None:
            _check_guards(buf, "sideband_search " + name)
    count = int(cnt[1, 0])
    nwritten = min(count, capacity)
    rows = ev[1:1 + max(capacity, 1)].cpu().numpy()
    if capacity == 0 and not bool((ev[1] == _POISON).all()):
        raise RuntimeError("sideband_search events: written at a capacity of 0")
    if not bool((ev[1 + nwritten:1 + max(capacity, 1)] == _POISON).all()) and capacity > 0:
        raise RuntimeError("sideband_search events: a slot past the count was written")
    events = np.ascontiguousarray(rows[:nwritten]).view(SB_EVENT_DTYPE).reshape(-1)
    res = {"count": count, "events": events, "nseg": [int(n) for n in g.nseg], "seg_stride": ss}
    if dense:
        res["best_S"] = bs[1:-1].view(torch.float32)
        res["best_j"] = bj[1:-1]
    return res
