"""Candidate diagnostic plots for peasoup outputs (Python 3).

The reference's ``CandidatePlotter`` (tools/peasoup_tools.py:167-383) draws,
per candidate of ``overview.xml`` + ``candidates.peasoup``: the folded
profile, the sub-integration image, per-sub-integration statistics, an info
table, DM / acceleration / S/N scatters of the candidate's associated hits
coloured by harmonic, a DM-acceleration map, and every candidate of the
search in period-DM space with a crosshair on the current one.

Here the panel data are computed first (:func:`candidate_panels`, NumPy
only) and then drawn (:class:`CandidatePlotter`, matplotlib's Agg backend).
Without matplotlib the panels are written as one ``.npz`` instead of a PNG,
so the data path is testable anywhere.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from .outputs import OverviewFile, PeasoupOutput, radec_to_str

HARM_COLOURS = ["darkblue", "lightblue", "green", "orange", "darkred", "purple"]


def candidate_panels(out: PeasoupOutput, idx: int) -> Dict[str, object]:
    """Every panel's data for candidate ``idx`` (NumPy arrays / lists)."""
    cand = out.get_candidate(idx)
    info = cand.info
    hits = np.sort(cand.hits, order="snr")[::-1] if cand.hits.size else cand.hits
    p: Dict[str, object] = {"index": idx}
    fold = None if cand.fold is None else np.array(cand.fold, dtype=np.float64)
    if fold is not None:
        lo, hi = fold.min(), fold.max()
        fold = (fold - lo) / (hi - lo) if hi > lo else fold * 0.0
        p["subints"] = fold                                     # [nints, nbins], normalised to [0, 1]
        p["profile"] = fold.sum(axis=0)
        std = fold.std(axis=1)
        mean = fold.mean(axis=1)
        p["subint_stats"] = np.stack([mean, std, mean - 3 * std, mean + 3 * std, fold.min(axis=1), fold.max(axis=1)])
    # associated hits, grouped by harmonic number (the scatters and the DM-acc map)
    groups: List[Tuple[int, np.ndarray]] = []
    for nh in np.unique(hits["nh"]) if hits.size else []:
        groups.append((int(nh), hits[hits["nh"] == nh]))
    p["hits"] = hits
    p["hit_groups"] = groups
    if hits.size:
        p["dm_acc_limits"] = (float(hits["dm"].min()), float(hits["dm"].max()), float(hits["acc"].min()),
                              float(hits["acc"].max()))
    # every candidate of the search, period vs DM (crosshair on this one)
    allc = out.overview.as_array()
    p["all"] = np.stack([allc["period"], allc["dm"], allc["snr"], allc["nh"]]) if allc.size else np.zeros((4, 0))
    p["crosshair"] = (float(info["period"]), float(info["dm"]))
    hdr = out.overview.header
    ra = radec_to_str(float(hdr.get("src_raj", "0") or 0))
    dec = radec_to_str(float(hdr.get("src_dej", "0") or 0))
    p["table"] = [("R.A.", ra), ("Decl.", dec), ("P0", "%.9f" % info["period"]),
                  ("Opt P0", "%.9f" % info["opt_period"]), ("DM", "%.2f" % info["dm"]), ("Acc", "%.2f" % info["acc"]),
                  ("Harmonic", "%d" % info["nh"]), ("Spec S/N", "%.1f" % info["snr"]),
                  ("Fold S/N", "%.1f" % info["folded_snr"]), ("Adjacent?", str(bool(info["is_adjacent"]))),
                  ("Physical?", str(bool(info["is_physical"]))), ("DDM ratio 1", "%.4f" % info["ddm_count_ratio"]),
                  ("DDM ratio 2", "%.4f" % info["ddm_snr_ratio"]), ("Nassoc", "%d" % info["nassoc"])]
    p["title"] = hdr.get("source_name", "")
    return p


def freq_phase_panel(cand: Dict) -> np.ndarray:
    """Frequency-phase panel of a fold-cube candidate (``FoldCubeFile.candidate``):
    float64 [nsub, nbins], the mean raw sample over all subints (sums over
    subints / (hits over subints x nactive)), each subband's median over its
    filled bins removed, killed subbands (and bins without hits) 0."""
    sums = np.asarray(cand["sums"], dtype=np.float64).sum(axis=0)
    hits = np.asarray(cand["hits"], dtype=np.float64).sum(axis=0)
    nact = np.asarray(cand["nactive"], dtype=np.float64)
    den = nact[:, None] * hits[None, :]
    out = np.zeros(den.shape, dtype=np.float64)
    np.divide(sums, den, out=out, where=den != 0)
    filled = hits > 0
    for s in range(out.shape[0]):
        if nact[s] > 0 and filled.any():
            out[s, filled] -= np.median(out[s, filled])
    return out


def time_phase_panel(cand: Dict) -> np.ndarray:
    """Time-phase panel of a fold-cube candidate: float64 [nints, nbins], the
    mean raw sample over the unkilled channels (0 in bins without hits)."""
    sums = np.asarray(cand["sums"], dtype=np.float64).sum(axis=1)
    den = np.asarray(cand["hits"], dtype=np.float64) * float(np.asarray(cand["nactive"]).sum())
    out = np.zeros(den.shape, dtype=np.float64)
    np.divide(sums, den, out=out, where=den != 0)
    return out


def burst_waterfall_panel(cand: Dict) -> np.ndarray:
    """Dedispersed dynamic spectrum of a burst cutout (``BurstCubeFile.candidate``):
    float64 [nsub, ntime], the mean raw sample with each subband's median over
    its filled bins removed; bins without hits (and killed subbands) 0."""
    from .outputs import burst_mean

    m = burst_mean(cand["ds_sums"], cand["ds_hits"])
    out = np.zeros(m.shape, dtype=np.float64)
    for s in range(m.shape[0]):
        filled = ~np.isnan(m[s])
        if filled.any():
            out[s, filled] = m[s, filled] - np.median(m[s, filled])
    return out


def burst_dmtime_panel(cand: Dict) -> np.ndarray:
    """DM-time plane (the "bow tie") of a burst cutout: float64 [ndm, ntime],
    the mean raw sample with each DM row's median over its filled bins
    removed; bins without hits 0."""
    from .outputs import burst_mean

    m = burst_mean(cand["dmt_sums"], cand["dmt_hits"])
    out = np.zeros(m.shape, dtype=np.float64)
    for j in range(m.shape[0]):
        filled = ~np.isnan(m[j])
        if filled.any():
            out[j, filled] = m[j, filled] - np.median(m[j, filled])
    return out


def burst_profile_panel(cand: Dict) -> np.ndarray:
    """Band-summed profile of a burst cutout at the candidate's DM: float64
    [ntime], the mean raw sample over the unkilled channels with the median
    over the filled bins removed; bins without hits 0."""
    from .outputs import burst_mean

    m = burst_mean(np.asarray(cand["ds_sums"], dtype=np.int64).sum(axis=0),
                   np.asarray(cand["ds_hits"], dtype=np.int64).sum(axis=0))
    out = np.zeros(m.shape, dtype=np.float64)
    filled = ~np.isnan(m)
    if filled.any():
        out[filled] = m[filled] - np.median(m[filled])
    return out


def _opt_snr_plane(rec: Dict, vals: np.ndarray) -> np.ndarray:
    """The S/N (cubeopt.hpp, step 4) of box sums ``vals`` [nw, ...], maximised over the widths."""
    nbins = int(np.asarray(rec["profile"]).shape[0])
    vals = np.asarray(vals, dtype=np.float64)
    if not rec["v"] > 0:
        return np.zeros(vals.shape[1:], dtype=np.float64)
    w = (2.0 ** np.arange(vals.shape[0])).reshape((-1,) + (1,) * (vals.ndim - 1))
    snr = (vals - w * float(rec["mtot"]) / nbins) / np.sqrt(float(rec["v"]) * w * (1.0 - w / nbins))
    return snr.max(axis=0)


def dm_curve_panel(rec: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """(dms float64 [ndm], S/N float64 [ndm]) of a cubeopt record: for every DM
    trial the best S/N over the period and acceleration trials, bins and widths."""
    return np.asarray(rec["dms"], dtype=np.float64), _opt_snr_plane(rec, rec["dmcurve"])


def p_pdot_panel(rec: Dict) -> np.ndarray:
    """float64 [npd, np] of a cubeopt record: for every (acceleration,
    period) trial the best S/N over the DM trials, bins and widths; the
    period trials run along x."""
    return _opt_snr_plane(rec, rec["ppd"]).T.copy()


def orbit_surface_panel(rec: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """Two slices of an orbopt record's S/N surface through the optimum
    template: (float64 [na1, npb] at the optimum's orbital phase, float64 [na1,
    nphase] at the optimum's orbital period), each the S/N (orbopt.hpp, step 5)
    of ``tcurve`` with the template's own ``msum``, maximised over the widths;
    a1 runs along y."""
    npb, na1, nph = int(rec["npb"]), int(rec["na1"]), int(rec["nphase"])
    nbins = int(np.asarray(rec["profile"]).shape[0])
    tc = np.asarray(rec["tcurve"], dtype=np.float64)                       # [nw, K]
    v = float(rec["v1"]) / nbins
    if not v > 0:
        snr = np.zeros(tc.shape[1], dtype=np.float64)
    else:
        w = (2.0 ** np.arange(tc.shape[0]))[:, None]
        snr = ((tc - w * np.asarray(rec["msum"], dtype=np.float64)[None, :] / nbins) /
               np.sqrt(v * w * (1.0 - w / nbins))).max(axis=0)
    cube = snr.reshape(npb, na1, nph)
    k = int(rec["opt_k"])
    kp, kb = k % nph, k // nph // na1
    return cube[:, :, kp].T.copy(), cube[kb].copy()


def burst_dm_curve_panel(rec: Dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(dms float64 [ndm], S/N float64 [ndm], dmf float64 [nfine], S/N float64
    [nfine]) of a burstopt record: for every coarse DM row and every fine DM
    row the best S/N (burstopt.hpp, step 4) over the bins and widths; the
    coarse rows use their own off-pulse mean, the fine rows the waterfall's."""
    dms = np.asarray(rec["dms"], dtype=np.float64)
    dmf = np.asarray(rec["dmf"], dtype=np.float64)
    curve = np.asarray(rec["curve"], dtype=np.float64)
    ndm = dms.shape[0]
    if not rec["v"] > 0:
        return dms, np.zeros(ndm), dmf, np.zeros(dmf.shape[0])
    w = (2.0 ** np.arange(curve.shape[0]))[:, None]
    mbar = np.concatenate([np.asarray(rec["mbar_dmt"], dtype=np.float64), np.full(dmf.shape[0], float(rec["mbar_ds"]))])
    snr = ((curve - w * mbar[None, :]) / np.sqrt(float(rec["v"]) * w)).max(axis=0)
    return dms, snr[:ndm].copy(), dmf, snr[ndm:].copy()


def _sizes(snr: np.ndarray) -> np.ndarray:
    s = np.asarray(snr, dtype=np.float64)
    if s.size == 0:
        return s
    rng = s.max() - s.min()
    return 5.0 + 250.0 * ((s - s.min()) / rng if rng > 0 else np.zeros_like(s))


class CandidatePlotter:
    """Draws :func:`candidate_panels` for any candidate of one search
    output.  ``plot_cand(idx, filename)`` writes ``filename`` (PNG, or
    ``.npz`` panels when matplotlib is missing) and returns its path."""

    def __init__(self, outdir: Optional[str] = None, overview: Optional[str] = None,
                 candidates: Optional[str] = None, cubes: Optional[str] = None, opt: Optional[str] = None):
        # cubes: a fold-cube file whose candidate i belongs to candidate i of
        # the overview (python -m peasoup_amd cube --overview); adds the
        # frequency-phase and time-phase panels
        # opt: the cubeopt result file of those cubes; adds the S/N-DM curve
        # and the P-Pdot plane
        self.opt = None
        if opt:
            from .outputs import FoldOptFile

            self.opt = FoldOptFile(opt)
        self.cubes = None
        if cubes:
            from .outputs import FoldCubeFile

            self.cubes = FoldCubeFile(cubes)
        overview = overview or os.path.join(outdir, "overview.xml")
        candidates = candidates or os.path.join(os.path.dirname(os.path.abspath(overview)), "candidates.peasoup")
        self.out = PeasoupOutput(overview, candidates)
        try:
            import matplotlib

            matplotlib.use("Agg")
            import matplotlib.pyplot as plt

            self._plt = plt
        except ImportError:  # pragma: no cover - matplotlib is in the image
            self._plt = None

    @property
    def overview(self) -> OverviewFile:
        return self.out.overview

    def __len__(self) -> int:
        return len(self.out)

    def plot_cand(self, idx: int, filename: Optional[str] = None) -> str:
        p = candidate_panels(self.out, idx)
        if self.cubes is not None and idx < len(self.cubes):
            cube = self.cubes.candidate(idx)
            p["freq_phase"] = freq_phase_panel(cube)
            p["time_phase"] = time_phase_panel(cube)
        if self.opt is not None and idx < len(self.opt):
            rec = self.opt.candidate(idx)
            p["opt_dms"], p["opt_dm_snr"] = dm_curve_panel(rec)
            p["opt_p_pdot"] = p_pdot_panel(rec)
        if self._plt is None:
            path = (filename or f"cand_{idx:04d}") + ("" if str(filename).endswith(".npz") else ".npz")
            arrays = {k: v for k, v in p.items() if isinstance(v, np.ndarray)}
            arrays["table"] = np.array(p["table"], dtype=object).astype(str)
            np.savez(path, **arrays)
            return path
        path = filename or f"cand_{idx:04d}.png"
        fig = self._draw(p)
        if "freq_phase" in p:
            self._draw_cube(fig, p)
        if "opt_p_pdot" in p:
            self._draw_opt(fig, p)
        fig.savefig(path)
        self._plt.close(fig)
        return path

    # the reference's grid: 5 x 9 cells for the upper panels, the all-candidates strip below
    def _draw(self, p: Dict[str, object]):
        plt = self._plt
        fig = plt.figure(figsize=[14, 12])
        prof_ax = plt.subplot2grid([5, 9], [0, 1], colspan=2, fig=fig)
        fold_ax = plt.subplot2grid([5, 9], [1, 1], colspan=2, rowspan=2, sharex=prof_ax, fig=fig)
        subs_ax = plt.subplot2grid([5, 9], [1, 0], rowspan=2, sharey=fold_ax, fig=fig)
        table_ax = plt.subplot2grid([5, 9], [0, 3], colspan=3, rowspan=3, frameon=False, fig=fig)
        dm_ax = plt.subplot2grid([5, 9], [0, 6], colspan=2, fig=fig)
        acc_ax = plt.subplot2grid([5, 9], [1, 8], rowspan=2, fig=fig)
        dm_acc_ax = plt.subplot2grid([5, 9], [1, 6], colspan=2, rowspan=2, sharex=dm_ax, sharey=acc_ax, fig=fig)
        all_ax = plt.subplot2grid([6, 9], [4, 0], colspan=9, rowspan=2, fig=fig)
        if "subints" in p:
            sub = p["subints"]
            prof_ax.plot(p["profile"])
            prof_ax.set_title("Profile")
            prof_ax.set_ylabel("Flux")
            fold_ax.imshow(sub, aspect="auto", interpolation="nearest", origin="lower")
            fold_ax.set_xlim(-0.5, sub.shape[1] - 0.5)
            fold_ax.set_xlabel("Phase bin")
            mean, _, lo3, hi3, mn, mx = p["subint_stats"]
            y = np.arange(sub.shape[0])
            subs_ax.fill_betweenx(y, lo3, hi3, alpha=0.5, color="lightblue", label="+-3 sigma")
            subs_ax.plot(mean, y, lw=2, alpha=0.8, color="lightblue", label="mean")
            subs_ax.plot(mn, y, lw=2, color="darkblue", label="min")
            subs_ax.plot(mx, y, lw=2, color="darkred", label="max")
            subs_ax.legend(loc="lower left", bbox_to_anchor=(-0.2, 1.0), prop={"size": 8})
            subs_ax.invert_xaxis()
            subs_ax.set_ylim(-0.5, sub.shape[0] - 0.5)
            subs_ax.set_ylabel("Subintegration")
        else:
            fold_ax.text(0.5, 0.5, "not folded", ha="center", va="center", transform=fold_ax.transAxes)
        table_ax.xaxis.set_major_locator(plt.NullLocator())
        table_ax.yaxis.set_major_locator(plt.NullLocator())
        tab = table_ax.table(cellText=[list(r) for r in p["table"]], cellLoc="left", colLoc="left", loc="center")
        for cell in tab.get_celld().values():
            cell.set_linewidth(0)
        tab.scale(1.0, 1.6)
        for ii, (nh, g) in enumerate(p["hit_groups"]):
            col = HARM_COLOURS[ii % len(HARM_COLOURS)]
            dm_ax.scatter(g["dm"], g["snr"], facecolor=col, edgecolor="none", s=10, label="Harm. %d" % nh)
            acc_ax.scatter(g["snr"], g["acc"], facecolor=col, edgecolor="none", s=10)
            dm_acc_ax.scatter(g["dm"], g["acc"], facecolor=col, edgecolor="none", s=_sizes(g["snr"]))
        dm_ax.set_ylabel("S/N")
        dm_ax.yaxis.tick_right()
        if p["hit_groups"]:
            dm_ax.legend(loc="lower left", bbox_to_anchor=(0.0, 1.0), prop={"size": 8}, ncol=3)
        acc_ax.yaxis.tick_right()
        acc_ax.yaxis.set_label_position("right")
        acc_ax.set_ylabel("Acceleration (m/s/s)", rotation=-90, labelpad=12)
        acc_ax.set_xlabel("S/N")
        if "dm_acc_limits" in p:
            d0, d1, a0, a1 = p["dm_acc_limits"]
            dm_acc_ax.set_xlim(d0 - 0.5, d1 + 0.5)
            dm_acc_ax.set_ylim(a0 - 0.5, a1 + 0.5)
        dm_acc_ax.set_xlabel("DM (pc cm^-3)")
        per, dm, snr, nh = p["all"]
        if per.size:
            all_ax.scatter(per, dm, s=_sizes(snr), c=nh, cmap="viridis", edgecolor="none")
            all_ax.set_xscale("log")
            x, y = p["crosshair"]
            all_ax.axvline(x, color="k", lw=0.8)
            all_ax.axhline(y, color="k", lw=0.8)
        all_ax.set_xlabel("Period (s)")
        all_ax.set_ylabel("DM (pc cm^-3)")
        fig.suptitle(f"{p['title']}  candidate {p['index']}")
        return fig

    # the two fold-cube panels, in a strip added to the right of the figure
    def _draw_cube(self, fig, p: Dict[str, object]) -> None:
        w, h = fig.get_size_inches()
        fig.set_size_inches(w + 4.0, h)
        fig.subplots_adjust(right=w / (w + 4.0) * 0.9)
        left = w / (w + 4.0) * 0.9 + 0.05
        fp_ax = fig.add_axes([left, 0.55, 0.98 - left, 0.33])
        tp_ax = fig.add_axes([left, 0.10, 0.98 - left, 0.33])
        fp_ax.imshow(p["freq_phase"], aspect="auto", interpolation="nearest", origin="lower")
        fp_ax.set_title("Frequency-phase (filterbank fold)")
        fp_ax.set_ylabel("Subband")
        tp_ax.imshow(p["time_phase"], aspect="auto", interpolation="nearest", origin="lower")
        tp_ax.set_title("Time-phase (filterbank fold)")
        tp_ax.set_ylabel("Subintegration")
        tp_ax.set_xlabel("Phase bin")

    # the two cubeopt panels, in a further strip on the right
    def _draw_opt(self, fig, p: Dict[str, object]) -> None:
        w, h = fig.get_size_inches()
        for ax in fig.axes:  # squeeze what is there into the old width
            x0, y0, ww, hh = ax.get_position().bounds
            ax.set_position([x0 * w / (w + 4.0), y0, ww * w / (w + 4.0), hh])
        fig.set_size_inches(w + 4.0, h)
        left = w / (w + 4.0) + 0.03
        dm_ax = fig.add_axes([left, 0.55, 0.98 - left, 0.33])
        pp_ax = fig.add_axes([left, 0.10, 0.98 - left, 0.33])
        dm_ax.plot(p["opt_dms"], p["opt_dm_snr"])
        dm_ax.set_title("S/N against DM (cube search)")
        dm_ax.set_xlabel("DM (pc cm^-3)")
        pp_ax.imshow(p["opt_p_pdot"], aspect="auto", interpolation="nearest", origin="lower")
        pp_ax.set_title("P-Pdot plane (cube search)")
        pp_ax.set_xlabel("Period trial")
        pp_ax.set_ylabel("Acceleration trial")


def plot_all(outdir: str, limit: int = 100, dest: Optional[str] = None) -> List[str]:
    """``Cand%04d.png`` for the first ``limit`` candidates (the reference's
    ``main``, peasoup_tools.py:403-412)."""
    pl = CandidatePlotter(outdir)
    dest = dest or outdir
    return [pl.plot_cand(i, os.path.join(dest, "Cand%04d.png" % i)) for i in range(min(limit, len(pl)))]
