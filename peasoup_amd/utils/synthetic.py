"""Seeded synthetic filterbanks with injected (accelerated) pulsars.

Used by the tests and benchmarks (there is no network access to real data).
The generator produces quantised Gaussian noise plus a dispersed periodic
pulse train whose arrival times follow the same dispersion law the pipeline
searches for (delay_c = 4.15e3 * DM * (1/f_c^2 - 1/f_1^2) s), optionally with
a constant line-of-sight acceleration (phase = (t - a t^2/(2c)) / P, a > 0 away)
and a jerk (a further - j t^3/(6c), ``generate`` only), or on a circular orbit
(``generate`` only).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from .sigproc import pack_samples, write_filterbank

C_LIGHT = 299792458.0


@dataclass
class PulsarSpec:
    period: float = 0.25        # s
    dm: float = 30.0            # pc cm^-3
    duty: float = 0.05          # pulse FWHM as a fraction of the period
    amplitude: float = 1.0      # peak in units of the per-channel noise sigma
    accel: float = 0.0          # m/s^2
    phase: float = 0.0
    alpha: float = 0.0          # spectral index about the band centre (filinject only)
    # (pb s, a1 light-seconds, phase turns) of a circular orbit or None (generate only): a pulse emitted at tau
    # arrives at tau + a1 [sin 2 pi (tau / pb + ph) - sin 2 pi ph] (csrc/include/psoup/orbit.hpp)
    orbit: Optional[Tuple[float, float, float]] = None
    jerk: float = 0.0           # m/s^3 (generate only): phase gains -jerk te^3/(6c)


@dataclass
class BurstSpec:
    """One dispersed Gaussian pulse (a single-pulse search target)."""
    time: float = 1.0           # arrival time in the top channel (s)
    dm: float = 30.0            # pc cm^-3
    width: float = 5e-3         # FWHM (s)
    amplitude: float = 1.0      # peak in units of the per-channel noise sigma
    alpha: float = 0.0          # spectral index about the band centre (filinject only)


@dataclass
class RfiSpec:
    """Interference: ``channel`` multiplies the noise of ``channel`` by
    ``amplitude`` throughout; ``impulse`` adds ``amplitude`` sigma to every
    channel at the same samples (DM 0) from ``time`` for ``duration`` seconds
    (at least one sample); ``cell`` does that to ``channel`` alone."""
    kind: str = "impulse"       # "channel" | "impulse" | "cell"
    channel: int = 0
    time: float = 0.0           # s
    duration: float = 0.0       # s
    amplitude: float = 1.0


def _apply_rfi(x: np.ndarray, rfi, t0: int, tsamp: float, noise_only: bool) -> None:
    """In place on the chunk x [t1 - t0, nchans] of unit-sigma floats."""
    for r in rfi:
        if r.kind == "channel":
            if noise_only:
                x[:, r.channel] *= np.float32(r.amplitude)
            continue
        if noise_only:
            continue
        if r.kind not in ("impulse", "cell"):
            raise ValueError(f"RfiSpec.kind must be channel, impulse or cell, got {r.kind!r}")
        s0 = int(round(r.time / tsamp))
        s1 = max(s0 + 1, int(round((r.time + r.duration) / tsamp)))
        a, b = max(s0 - t0, 0), min(s1 - t0, x.shape[0])
        if a < b:
            if r.kind == "impulse":
                x[a:b, :] += np.float32(r.amplitude)
            else:
                x[a:b, r.channel] += np.float32(r.amplitude)


def make_header(nchans: int = 64, nbits: int = 2, tsamp: float = 320e-6, fch1: float = 1510.0,
                foff: float = -1.09, nsamples: int = 0, source_name: str = "synthetic") -> Dict:
    return {"source_name": source_name, "tsamp": tsamp, "fch1": fch1, "foff": foff, "nchans": nchans,
            "nbits": nbits, "nifs": 1, "data_type": 1, "tstart": 50000.0, "nsamples": nsamples}


def generate(nsamps: int, header: Dict, pulsars=(), seed: int = 0, chunk: int = 1 << 16, bursts=(),
             rfi=()) -> np.ndarray:
    """Return [nsamps, nchans] uint8 quantised samples (values < 2^nbits).
    ``bursts``: :class:`BurstSpec` pulses, dispersed like the pulsars (they
    draw nothing from the generator: the noise is the same with or without).
    ``rfi``: :class:`RfiSpec` interference, likewise without a draw."""
    rng = np.random.default_rng(seed)
    nchans = int(header["nchans"])
    nbits = int(header["nbits"])
    tsamp = float(header["tsamp"])
    fch1 = float(header["fch1"])
    foff = float(header["foff"])
    freqs = fch1 + foff * np.arange(nchans)
    levels = (1 << nbits) - 1
    # Gaussian noise mapped to the quantiser: mean mid-scale, sigma ~ levels/4
    mean = levels / 2.0
    sigma = max(levels / 4.0, 0.5)
    out = np.empty((nsamps, nchans), dtype=np.uint8)
    for t0 in range(0, nsamps, chunk):
        t1 = min(nsamps, t0 + chunk)
        x = rng.standard_normal((t1 - t0, nchans)).astype(np.float32)
        _apply_rfi(x, rfi, t0, tsamp, True)
        t = (np.arange(t0, t1, dtype=np.float64) * tsamp)[:, None]
        for p in pulsars:
            delay = 4.15e3 * p.dm * (1.0 / freqs ** 2 - 1.0 / fch1 ** 2)  # seconds
            te = t - delay[None, :]
            if p.orbit is not None:  # the orbit-frame time tau of te = tau + D(tau), by fixed-point iteration
                pb, a1, oph = (float(v) for v in p.orbit)
                t_arr, te = te, te
                for _ in range(8):
                    te = t_arr - a1 * (np.sin(2 * np.pi * (te / pb + oph)) - np.sin(2 * np.pi * oph))
            # +ve acceleration = away from the observer (distiller.hpp:164):
            # the apparent spin frequency drifts down
            if p.jerk:  # the cubic term of a line-of-sight jerk (csrc/include/psoup/jerk.hpp)
                ph = (te - p.accel * te * te / (2 * C_LIGHT) - p.jerk * te * te * te / (6 * C_LIGHT)) / p.period + p.phase
            else:
                ph = (te - p.accel * te * te / (2 * C_LIGHT)) / p.period + p.phase
            ph = ph - np.floor(ph)
            d = np.minimum(ph, 1.0 - ph)
            w = p.duty / 2.3548
            x += p.amplitude * np.exp(-0.5 * (d / w) ** 2).astype(np.float32)
        for b in bursts:
            delay = 4.15e3 * b.dm * (1.0 / freqs ** 2 - 1.0 / fch1 ** 2)  # seconds
            d = t - delay[None, :] - b.time
            w = b.width / 2.3548
            x += b.amplitude * np.exp(-0.5 * (d / w) ** 2).astype(np.float32)
        _apply_rfi(x, rfi, t0, tsamp, False)
        q = np.rint(mean + sigma * x)
        out[t0:t1] = np.clip(q, 0, levels).astype(np.uint8)
    return out


def write(path: str, nsamps: int, header: Optional[Dict] = None, pulsars=(), seed: int = 0, bursts=(),
          rfi=()) -> Dict:
    hdr = dict(header or make_header())
    hdr["nsamples"] = nsamps
    vals = generate(nsamps, hdr, pulsars, seed, bursts=bursts, rfi=rfi)
    write_filterbank(path, hdr, vals)
    return hdr


def as_raw(values: np.ndarray, header: Dict, dtype="float32", decades: float = 4.0, drift: float = 0.0,
           ascending: bool = False, seed: int = 0) -> Tuple[Dict, np.ndarray]:
    """Turns generated samples ``values`` [nsamps, nchans] (uint8, descending
    band) into the data of a backend that writes float32 or uint16: channel c
    becomes ``gain[c] * (values - mid) * (1 + drift * t / nsamps) + offset[c]``
    with seeded per-channel gains spread log-uniformly over ``decades`` decades
    and offsets of a few sigma, a slow baseline drift, and optionally the band
    stored lowest frequency first.  Returns (header, samples); the header has
    the new nbits, fch1 and foff.  uint16 output is rounded and clipped."""
    rng = np.random.default_rng(seed)
    nsamps, nchans = values.shape
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.uint16)):
        raise ValueError("dtype must be float32 or uint16")
    mid = ((1 << int(header["nbits"])) - 1) / 2.0
    gains = 10.0 ** (rng.uniform(-0.5, 0.5, nchans) * decades)
    offsets = gains * rng.uniform(-3.0, 3.0, nchans) * max(mid / 2.0, 0.5)
    if dt == np.dtype(np.uint16):
        gains = gains / gains.max() * 64.0          # sigma of at most ~4000 counts
        offsets = 20000.0 + offsets / np.abs(offsets).max() * 5000.0
    ramp = 1.0 + drift * np.arange(nsamps, dtype=np.float64)[:, None] / max(nsamps, 1)
    x = (values.astype(np.float64) - mid) * gains[None, :] * ramp + offsets[None, :] * ramp
    x = np.clip(np.rint(x), 0, 65535).astype(np.uint16) if dt == np.dtype(np.uint16) else x.astype(np.float32)
    hdr = dict(header)
    hdr["nbits"] = 8 * dt.itemsize
    if ascending:
        x = np.ascontiguousarray(x[:, ::-1])
        hdr["fch1"] = float(header["fch1"]) + float(nchans - 1) * float(header["foff"])
        hdr["foff"] = -float(header["foff"])
    return hdr, x


def packed(nsamps: int, header: Dict, pulsars=(), seed: int = 0, bursts=(), rfi=()) -> np.ndarray:
    return pack_samples(generate(nsamps, header, pulsars, seed, bursts=bursts, rfi=rfi), int(header["nbits"]))


def generate_packed_torch(nsamps: int, header: Dict, pulsars=(), seed: int = 0, device=None,
                          chunk: int = 1 << 15, birdies=()):
    """GPU form of :func:`packed` (same noise model, quantiser, dispersion and
    acceleration law; torch's generator instead of NumPy's, so not the same
    noise samples): packed SIGPROC bytes as a uint8 tensor on ``device``.
    ``birdies``: (frequency Hz, amplitude) sinusoids added to every channel
    (periodic RFI: strong, undispersed, many harmonics of threshold crossings).
    Minutes-long 2^23-sample, 1024-channel filterbanks take seconds."""
    import torch

    dev = torch.device(device) if device is not None else torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    nchans = int(header["nchans"])
    nbits = int(header["nbits"])
    tsamp = float(header["tsamp"])
    fch1 = float(header["fch1"])
    foff = float(header["foff"])
    levels = (1 << nbits) - 1
    mean = levels / 2.0
    sigma = max(levels / 4.0, 0.5)
    per = 8 // nbits if nbits < 8 else 1
    assert nbits in (1, 2, 4, 8) and nchans % per == 0
    freqs = fch1 + foff * torch.arange(nchans, device=dev, dtype=torch.float64)
    out = torch.empty(nsamps * nchans * nbits // 8, dtype=torch.uint8, device=dev)
    row = nchans * nbits // 8
    for t0 in range(0, nsamps, chunk):
        n = min(chunk, nsamps - t0)
        x = torch.randn((n, nchans), device=dev, generator=g)
        t = (torch.arange(t0, t0 + n, device=dev, dtype=torch.float64) * tsamp)[:, None]
        for p in pulsars:
            delay = 4.15e3 * p.dm * (1.0 / freqs ** 2 - 1.0 / fch1 ** 2)
            te = t - delay[None, :]
            ph = (te - p.accel * te * te / (2 * C_LIGHT)) / p.period + p.phase
            ph = ph - torch.floor(ph)
            d = torch.minimum(ph, 1.0 - ph)
            w = p.duty / 2.3548
            x += (p.amplitude * torch.exp(-0.5 * (d / w) ** 2)).float()
        for f, amp in birdies:
            x += (amp * torch.sin(2 * np.pi * f * t)).float()
        q = torch.clamp(torch.round(mean + sigma * x), 0, levels).to(torch.uint8)
        if nbits == 8:
            packed = q.reshape(-1)
        else:
            q = q.view(n, nchans // per, per).to(torch.int32)
            acc = torch.zeros((n, nchans // per), dtype=torch.int32, device=dev)
            for k in range(per):
                acc |= q[..., k] << (k * nbits)
            packed = acc.to(torch.uint8).reshape(-1)
        out[t0 * row:(t0 + n) * row] = packed
    return out
