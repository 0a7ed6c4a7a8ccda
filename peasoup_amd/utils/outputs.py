"""Python 3 readers for peasoup outputs (overview.xml, candidates.peasoup).

Parity with tools/peasoup_tools.py:14-412 (Python 2: OverviewFile,
CandidateFileParser, PeasoupOutput) -- rewritten on the standard library
(xml.etree) + numpy; lxml and sigpyproc are not required.
"""
from __future__ import annotations

import struct
import xml.etree.ElementTree as ET
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

POD_DTYPE = np.dtype([("dm", "<f4"), ("dm_idx", "<i4"), ("acc", "<f4"), ("nh", "<i4"), ("snr", "<f4"),
                      ("freq", "<f4")])
assert POD_DTYPE.itemsize == 24


def radec_to_str(val: float) -> str:
    """hhmmss.ss-style float -> 'hh:mm:ss.ssss' (peasoup_tools.radec_to_str)."""
    sign = -1 if val < 0 else 1
    frac, integral = np.modf(abs(val))
    xx = (integral - (integral % 10000)) / 10000
    yy = ((integral - (integral % 100)) / 100) - xx * 100
    zz = integral - 100 * yy - 10000 * xx + frac
    return "%02d:%02d:%s" % (sign * xx, yy, "%07.4f" % zz)


class OverviewFile:
    """Parsed overview.xml.  Tolerates an invalid <username> (the reference
    tool strips it on a parse error)."""

    fields = [("period", float), ("opt_period", float), ("dm", float), ("acc", float), ("nh", int), ("snr", float),
              ("folded_snr", float), ("is_adjacent", int), ("is_physical", int), ("ddm_count_ratio", float),
              ("ddm_snr_ratio", float), ("nassoc", int), ("byte_offset", int)]

    def __init__(self, path: str):
        self.path = path
        text = open(path, "r", encoding="latin-1").read()
        try:
            self.root = ET.fromstring(text)
        except ET.ParseError:
            a = text.find("<username>") + len("<username>")
            b = text.find("</username>")
            self.root = ET.fromstring(text[:a] + "pulsar" + text[b:])
        self._cands = self.root.find("candidates").findall("candidate")

    def section(self, name: str) -> Dict[str, str]:
        el = self.root.find(name)
        return {c.tag: (c.text or "") for c in el} if el is not None else {}

    @property
    def dm_list(self) -> List[float]:
        return [float(t.text) for t in self.root.find("dedispersion_trials").findall("trial")]

    @property
    def acc_list(self) -> List[float]:
        return [float(t.text) for t in self.root.find("acceleration_trials").findall("trial")]

    @property
    def execution_times(self) -> Dict[str, float]:
        return {k: float(v) for k, v in self.section("execution_times").items()}

    def __len__(self) -> int:
        return len(self._cands)

    def get_candidate(self, idx: int) -> Dict:
        c = self._cands[idx]
        d = {"cand_num": int(c.attrib["id"])}
        for tag, typ in self.fields:
            el = c.find(tag)
            d[tag] = typ(float(el.text)) if typ is int else typ(el.text)
        return d

    @property
    def header(self) -> Dict[str, str]:
        """The <header_parameters> section (tag -> text)."""
        return self.section("header_parameters")

    def get_candidate_data(self, idx: int) -> "CandidateFileParser":
        """Parser of the candidate file that holds record ``idx`` (the
        reference opens ``candidates.peasoup`` in the working directory,
        peasoup_tools.py:149-151; here the one beside this overview file).
        Read record ``idx`` with ``.cand_from_offset(get_candidate(idx)["byte_offset"])``."""
        import os

        self.get_candidate(idx)  # (IndexError for a missing candidate, as the reference)
        return CandidateFileParser(os.path.join(os.path.dirname(os.path.abspath(self.path)), "candidates.peasoup"))

    def make_predictor(self, idx: int) -> str:
        """Ephemeris-style predictor of candidate ``idx`` (SOURCE, PERIOD, DM,
        ACC, RA, DEC), peasoup_tools.py:153-164.  The reference reads the
        candidate fields as float32 before formatting; so does this."""
        c = self._cands[idx]
        f32 = lambda tag: float(np.float32(c.find(tag).text))  # noqa: E731
        hdr = self.header
        return "\n".join(("SOURCE: %s" % hdr.get("source_name", ""),
                          "PERIOD: %.15f" % f32("period"),
                          "DM: %.3f" % f32("dm"),
                          "ACC: %.3f" % f32("acc"),
                          "RA: %s" % radec_to_str(float(hdr.get("src_raj", "0") or 0)),
                          "DEC: %s" % radec_to_str(float(hdr.get("src_dej", "0") or 0))))

    def as_array(self) -> np.ndarray:
        dt = [("cand_num", "i4")] + [(t, "f8" if ty is float else "i8") for t, ty in self.fields]
        arr = np.zeros(len(self), dtype=dt)
        for i in range(len(self)):
            d = self.get_candidate(i)
            for k in arr.dtype.names:
                arr[i][k] = d[k]
        return arr


class CandidateFileParser:
    """Reads records of candidates.peasoup by byte offset."""

    def __init__(self, path: str):
        self.buf = open(path, "rb").read()

    def cand_from_offset(self, offset: int) -> Tuple[Optional[np.ndarray], np.ndarray]:
        b = self.buf
        fold = None
        if b[offset: offset + 4] == b"FOLD":
            nbins, nints = struct.unpack_from("<ii", b, offset + 4)
            off = offset + 12
            fold = np.frombuffer(b, dtype="<f4", count=nbins * nints, offset=off).reshape(nints, nbins)
            off += 4 * nbins * nints
        else:
            off = offset
        (count,) = struct.unpack_from("<i", b, off)
        hits = np.frombuffer(b, dtype=POD_DTYPE, count=count, offset=off + 4)
        return fold, hits

    def records(self) -> List[Tuple[int, Optional[np.ndarray], np.ndarray]]:
        out = []
        off = 0
        while off < len(self.buf):
            fold, hits = self.cand_from_offset(off)
            out.append((off, fold, hits))
            off += (12 + fold.size * 4 if fold is not None else 0) + 4 + hits.size * 24
        return out


@dataclass
class Candidate:
    info: Dict
    fold: Optional[np.ndarray]
    hits: np.ndarray


class PeasoupOutput:
    def __init__(self, overview_file: str, candidate_file: str):
        self.overview = OverviewFile(overview_file)
        self.cands = CandidateFileParser(candidate_file)

    def __len__(self) -> int:
        return len(self.overview)

    def get_candidate(self, idx: int) -> Candidate:
        d = self.overview.get_candidate(idx)
        fold, hits = self.cands.cand_from_offset(d["byte_offset"])
        return Candidate(d, fold, hits)

    def as_text(self) -> str:
        a = self.overview.as_array()
        lines = ["#cand period opt_period dm acc nh snr folded_snr is_adjacent is_physical ddm_count ddm_snr nassoc"]
        for r in a:
            lines.append(f"{r['cand_num']:d} {r['period']:.12f} {r['opt_period']:.12f} {r['dm']:.3f} {r['acc']:.3f} "
                         f"{r['nh']:d} {r['snr']:.2f} {r['folded_snr']:.2f} {r['is_adjacent']:d} {r['is_physical']:d} "
                         f"{r['ddm_count_ratio']:.4f} {r['ddm_snr_ratio']:.4f} {r['nassoc']:d}")
        return "\n".join(lines)


# ------------------------------------------------------------ fold cubes ----
CUBE_MAGIC = b"PSCUBE01"
_CUBE_HEADER = struct.Struct("<8s6IQ3d")  # magic, ncand nints nsub nbins nchans nbits, fold_nsamps, tsamp fch1 foff
_CUBE_CAND = struct.Struct("<dff")        # period, dm, acc
CUBE_HEADER_FIELDS = ("ncand", "nints", "nsub", "nbins", "nchans", "nbits", "fold_nsamps", "tsamp", "fch1", "foff")


def write_cube_file(path: str, header: Dict, cands: List[Dict]) -> None:
    """Writes a fold-cube file byte for byte as the native ``write_cube_file``
    (csrc/src/foldcube.cpp): little-endian header ``PSCUBE01``, uint32 ncand
    nints nsub nbins nchans nbits, uint64 fold_nsamps, double tsamp fch1 foff;
    per candidate double period, float dm, float acc, int32 nactive[nsub],
    int32 hits[nints][nbins], int64 sums[nints][nsub][nbins].  ``header`` needs
    every field but ncand; each of ``cands`` is a dict(period, dm, acc,
    nactive, hits, sums).  Written to a temporary file, then renamed."""
    import os

    ni, ns, nb = int(header["nints"]), int(header["nsub"]), int(header["nbins"])
    blob = [_CUBE_HEADER.pack(CUBE_MAGIC, len(cands), ni, ns, nb, int(header["nchans"]), int(header["nbits"]),
                              int(header["fold_nsamps"]), float(header["tsamp"]), float(header["fch1"]),
                              float(header["foff"]))]
    for i, c in enumerate(cands):
        na = np.ascontiguousarray(c["nactive"], dtype="<i4")
        hits = np.ascontiguousarray(c["hits"], dtype="<i4")
        sums = np.ascontiguousarray(c["sums"], dtype="<i8")
        if na.shape != (ns,) or hits.shape != (ni, nb) or sums.shape != (ni, ns, nb):
            raise ValueError(f"cube file: candidate {i} has the wrong shape")
        blob += [_CUBE_CAND.pack(float(c["period"]), float(c["dm"]), float(c["acc"])), na.tobytes(), hits.tobytes(),
                 sums.tobytes()]
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class FoldCubeFile:
    """Reader of a fold-cube file (``bin/foldcube`` / ``python -m peasoup_amd
    cube``): ``len``, ``header``, ``candidate(i)``, ``mean(i)``."""

    def __init__(self, path: str):
        self.path = path
        self._buf = open(path, "rb").read()
        if len(self._buf) < _CUBE_HEADER.size or self._buf[:8] != CUBE_MAGIC:
            raise ValueError(f"{path}: not a fold-cube file")
        vals = _CUBE_HEADER.unpack_from(self._buf, 0)[1:]
        self.header: Dict = dict(zip(CUBE_HEADER_FIELDS, vals))
        ni, ns, nb = self.header["nints"], self.header["nsub"], self.header["nbins"]
        self._rec = _CUBE_CAND.size + 4 * ns + 4 * ni * nb + 8 * ni * ns * nb
        if len(self._buf) != _CUBE_HEADER.size + self.header["ncand"] * self._rec:
            raise ValueError(f"{path}: truncated fold-cube file")

    def __len__(self) -> int:
        return int(self.header["ncand"])

    def candidate(self, i: int) -> Dict:
        if not 0 <= i < len(self):
            raise IndexError(i)
        ni, ns, nb = self.header["nints"], self.header["nsub"], self.header["nbins"]
        o = _CUBE_HEADER.size + i * self._rec
        period, dm, acc = _CUBE_CAND.unpack_from(self._buf, o)
        o += _CUBE_CAND.size
        na = np.frombuffer(self._buf, "<i4", ns, o).copy()
        o += 4 * ns
        hits = np.frombuffer(self._buf, "<i4", ni * nb, o).reshape(ni, nb).copy()
        o += 4 * ni * nb
        sums = np.frombuffer(self._buf, "<i8", ni * ns * nb, o).reshape(ni, ns, nb).copy()
        return {"period": period, "dm": dm, "acc": acc, "nactive": na, "hits": hits, "sums": sums}

    def mean(self, i: int) -> np.ndarray:
        """float64 [nints, nsub, nbins]: sums / (hits * nactive), 0 where that product is 0."""
        return cube_mean(self.candidate(i))


def cube_mean(cand: Dict) -> np.ndarray:
    """Mean cube of a candidate dict: sums / (hits * nactive) in float64, 0 where the product is 0."""
    den = (np.asarray(cand["hits"], dtype=np.float64)[:, None, :] *
           np.asarray(cand["nactive"], dtype=np.float64)[None, :, None])
    out = np.zeros(den.shape, dtype=np.float64)
    np.divide(np.asarray(cand["sums"], dtype=np.float64), den, out=out, where=den != 0)
    return out


# --------------------------------------------------------------- cubeopt ----
OPT_MAGIC = b"PSOPT001"
_OPT_HEADER = struct.Struct("<8s10IQ6d")  # magic, ncand nints nsub nbins nchans ndm np npd nw 0, fold_nsamps, 6 doubles
_OPT_CAND = struct.Struct("<dff5df7Iqd")  # period dm acc | snr snr_in snr_dm0 opt_period opt_acc | opt_dm | 7 u32 | mtot v
OPT_HEADER_FIELDS = ("ncand", "nints", "nsub", "nbins", "nchans", "ndm", "np", "npd", "nw", "fold_nsamps", "tsamp",
                     "fch1", "foff", "p_step", "pd_step", "dm_half_range")
_OPT_SCALARS = ("period", "dm", "acc", "snr", "snr_in", "snr_dm0", "opt_period", "opt_acc", "opt_dm", "opt_width",
                "opt_bin", "opt_kd", "opt_kp", "opt_kpd", "flags")


def _opt_arrays(h: Dict):
    nw, ndm, np_, npd, nb = (int(h[k]) for k in ("nw", "ndm", "np", "npd", "nbins"))
    return (("dms", "<f4", (ndm,)), ("best_val", "<i4", (nw,)), ("best_idx", "<i4", (nw,)), ("centre", "<i4", (nw,)),
            ("dmcurve", "<i4", (nw, ndm)), ("ppd", "<i4", (nw, np_, npd)), ("profile", "<i4", (nb,)))


def write_opt_file(path: str, header: Dict, records: List[Dict]) -> None:
    """Writes a cubeopt result file byte for byte as the native
    ``write_opt_file`` (csrc/src/cubeopt.cpp): little-endian ``PSOPT001``,
    uint32 ncand nints nsub nbins nchans ndm np npd nw and a zero, uint64
    fold_nsamps, double tsamp fch1 foff p_step pd_step dm_half_range (104
    bytes); per candidate double period, float dm, float acc, double snr
    snr_in snr_dm0 opt_period opt_acc, float opt_dm, uint32 opt_width opt_bin
    opt_kd opt_kp opt_kpd flags and a zero, int64 mtot, double v (104 bytes),
    then float dms[ndm], int32 best_val[nw], best_idx[nw], centre[nw],
    dmcurve[nw][ndm], ppd[nw][np][npd], profile[nbins].  ``header`` needs
    every field but ncand.  Written to a temporary file, then renamed."""
    import os

    h = dict(header, ncand=len(records))
    blob = [_OPT_HEADER.pack(OPT_MAGIC, *(int(h[k]) for k in OPT_HEADER_FIELDS[:9]), 0, int(h["fold_nsamps"]),
                             *(float(h[k]) for k in OPT_HEADER_FIELDS[10:]))]
    for i, r in enumerate(records):
        blob.append(_OPT_CAND.pack(float(r["period"]), float(r["dm"]), float(r["acc"]), float(r["snr"]),
                                   float(r["snr_in"]), float(r["snr_dm0"]), float(r["opt_period"]),
                                   float(r["opt_acc"]), float(r["opt_dm"]), int(r["opt_width"]), int(r["opt_bin"]),
                                   int(r["opt_kd"]), int(r["opt_kp"]), int(r["opt_kpd"]), int(r["flags"]), 0,
                                   int(r["mtot"]), float(r["v"])))
        for name, dt, shape in _opt_arrays(h):
            a = np.ascontiguousarray(r[name], dtype=dt)
            if a.shape != shape:
                raise ValueError(f"opt file: candidate {i}: {name} has the wrong shape")
            blob.append(a.tobytes())
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class FoldOptFile:
    """Reader of a cubeopt result file (``bin/cubeopt`` / ``python -m
    peasoup_amd opt``): ``len``, ``header``, ``candidate(i)``."""

    def __init__(self, path: str):
        self.path = path
        self._buf = open(path, "rb").read()
        if len(self._buf) < _OPT_HEADER.size or self._buf[:8] != OPT_MAGIC:
            raise ValueError(f"{path}: not a cubeopt result file")
        vals = _OPT_HEADER.unpack_from(self._buf, 0)[1:]
        self.header: Dict = dict(zip(OPT_HEADER_FIELDS, vals[:9] + vals[10:]))
        self._arrays = _opt_arrays(self.header)
        self._rec = _OPT_CAND.size + sum(np.dtype(dt).itemsize * int(np.prod(sh)) for _, dt, sh in self._arrays)
        if len(self._buf) != _OPT_HEADER.size + self.header["ncand"] * self._rec:
            raise ValueError(f"{path}: truncated cubeopt result file")

    def __len__(self) -> int:
        return int(self.header["ncand"])

    def candidate(self, i: int) -> Dict:
        if not 0 <= i < len(self):
            raise IndexError(i)
        o = _OPT_HEADER.size + i * self._rec
        v = _OPT_CAND.unpack_from(self._buf, o)
        out = dict(zip(_OPT_SCALARS, v[:15]))
        out["mtot"], out["v"] = v[16], v[17]
        o += _OPT_CAND.size
        for name, dt, shape in self._arrays:
            n = int(np.prod(shape))
            out[name] = np.frombuffer(self._buf, dt, n, o).reshape(shape).copy()
            o += n * np.dtype(dt).itemsize
        return out


# ---------------------------------------------------------------- orbopt ----
OOPT_MAGIC = b"PSOOPT01"
_OOPT_HEADER = struct.Struct("<8s8IQ2d")   # magic, ncand nints nbins npb na1 nphase np nw, n, tsamp p_step
_OOPT_CAND = struct.Struct("<dff12d8I2q")  # period dm acc | pb a1 phase dpb da1 dph snr snr_in opt_period opt_pb opt_a1
#                                            opt_phase | opt_width opt_bin opt_k opt_l flags npb na1 nphase | m v1
OOPT_HEADER_FIELDS = ("ncand", "nints", "nbins", "npb", "na1", "nphase", "np", "nw", "n", "tsamp", "p_step")
_OOPT_SCALARS = ("period", "dm", "acc", "pb", "a1", "phase", "dpb", "da1", "dph", "snr", "snr_in", "opt_period", "opt_pb",
                 "opt_a1", "opt_phase", "opt_width", "opt_bin", "opt_k", "opt_l", "flags", "npb", "na1", "nphase", "m",
                 "v1")


def _oopt_arrays(h: Dict, K: int):
    nw, ni, nb = (int(h[k]) for k in ("nw", "nints", "nbins"))
    return (("best_val", "<i4", (nw,)), ("best_idx", "<i4", (nw,)), ("centre", "<i4", (nw,)), ("tcurve", "<i4", (nw, K)),
            ("msum", "<i8", (K,)), ("hits", "<i4", (ni, nb)), ("fold", "<i4", (ni, nb)), ("profile", "<i4", (nb,)))


def write_orbopt_file(path: str, header: Dict, records: List[Dict]) -> None:
    """Writes an orbopt result file byte for byte as the native
    ``write_orbopt_file`` (csrc/src/orbopt_host.cpp): little-endian
    ``PSOOPT01``, uint32 ncand nints nbins npb na1 nphase np nw, uint64 n,
    double tsamp p_step (64 bytes); per candidate double period, float dm,
    float acc, double pb a1 phase dpb da1 dph snr snr_in opt_period opt_pb
    opt_a1 opt_phase, uint32 opt_width opt_bin opt_k opt_l flags npb na1 nphase
    (the counts used, K their product), int64 m v1 (160 bytes), then int32
    best_val[nw], best_idx[nw], centre[nw], tcurve[nw][K], int64 msum[K], int32
    hits[nints][nbins], fold[nints][nbins], profile[nbins].  ``header`` needs
    every field but ncand.  Written to a temporary file, then renamed."""
    import os

    h = dict(header, ncand=len(records))
    blob = [_OOPT_HEADER.pack(OOPT_MAGIC, *(int(h[k]) for k in OOPT_HEADER_FIELDS[:9]), float(h["tsamp"]),
                              float(h["p_step"]))]
    for i, r in enumerate(records):
        blob.append(_OOPT_CAND.pack(*(float(r[k]) for k in _OOPT_SCALARS[:15]), *(int(r[k]) for k in _OOPT_SCALARS[15:])))
        K = int(r["npb"]) * int(r["na1"]) * int(r["nphase"])
        for name, dt, shape in _oopt_arrays(h, K):
            a = np.ascontiguousarray(r[name], dtype=dt)
            if a.shape != shape:
                raise ValueError(f"orbopt file: candidate {i}: {name} has the wrong shape")
            blob.append(a.tobytes())
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class OrbOptFile:
    """Reader of an orbopt result file (``bin/orbopt`` / ``python -m
    peasoup_amd oopt``): ``len``, ``header``, ``candidate(i)``."""

    def __init__(self, path: str):
        self.path = path
        self._buf = open(path, "rb").read()
        if len(self._buf) < _OOPT_HEADER.size or self._buf[:8] != OOPT_MAGIC:
            raise ValueError(f"{path}: not an orbopt result file")
        self.header: Dict = dict(zip(OOPT_HEADER_FIELDS, _OOPT_HEADER.unpack_from(self._buf, 0)[1:]))
        # the records differ in size with their template counts: walk them once
        self._offsets = []
        o = _OOPT_HEADER.size
        for _ in range(int(self.header["ncand"])):
            if o + _OOPT_CAND.size > len(self._buf):
                raise ValueError(f"{path}: truncated orbopt result file")
            v = _OOPT_CAND.unpack_from(self._buf, o)
            K = v[20] * v[21] * v[22]
            self._offsets.append(o)
            o += _OOPT_CAND.size + sum(np.dtype(dt).itemsize * int(np.prod(sh)) for _, dt, sh in
                                       _oopt_arrays(self.header, K))
        if o != len(self._buf):
            raise ValueError(f"{path}: truncated orbopt result file")

    def __len__(self) -> int:
        return int(self.header["ncand"])

    def candidate(self, i: int) -> Dict:
        if not 0 <= i < len(self):
            raise IndexError(i)
        o = self._offsets[i]
        out = dict(zip(_OOPT_SCALARS, _OOPT_CAND.unpack_from(self._buf, o)))
        o += _OOPT_CAND.size
        for name, dt, shape in _oopt_arrays(self.header, out["npb"] * out["na1"] * out["nphase"]):
            cnt = int(np.prod(shape))
            out[name] = np.frombuffer(self._buf, dt, cnt, o).reshape(shape).copy()
            o += cnt * np.dtype(dt).itemsize
        return out


# --------------------------------------------------------- burst cutouts ----
BURST_MAGIC = b"PSBRST01"
_BURST_HEADER = struct.Struct("<8s6IQ3d")  # magic, ncand ntime nsub ndm nchans nbits, nsamps, tsamp fch1 foff
_BURST_CAND = struct.Struct("<QIIqff")     # sample, width, tscrunch, t0, dm, snr
BURST_HEADER_FIELDS = ("ncand", "ntime", "nsub", "ndm", "nchans", "nbits", "nsamps", "tsamp", "fch1", "foff")
_BURST_PLANES = ("ds_sums", "ds_hits", "dmt_sums", "dmt_hits")


def write_burst_file(path: str, header: Dict, cands: List[Dict]) -> None:
    """Writes a burst-cutout file byte for byte as the native
    ``write_burst_file`` (csrc/src/burstcube.cpp): little-endian header
    ``PSBRST01``, uint32 ncand ntime nsub ndm nchans nbits, uint64 nsamps,
    double tsamp fch1 foff; per candidate uint64 sample, uint32 width, uint32
    tscrunch, int64 t0, float dm, float snr, float dms[ndm], int32
    nactive[nsub], then int32 ds_sums[nsub][ntime], ds_hits, dmt_sums[ndm][ntime],
    dmt_hits.  ``header`` needs every field but ncand; each of ``cands`` is a
    dict of those fields (snr optional).  Written to a temporary file, then renamed."""
    import os

    nt, ns, nd = int(header["ntime"]), int(header["nsub"]), int(header["ndm"])
    blob = [_BURST_HEADER.pack(BURST_MAGIC, len(cands), nt, ns, nd, int(header["nchans"]), int(header["nbits"]),
                               int(header["nsamps"]), float(header["tsamp"]), float(header["fch1"]),
                               float(header["foff"]))]
    shapes = {"ds_sums": (ns, nt), "ds_hits": (ns, nt), "dmt_sums": (nd, nt), "dmt_hits": (nd, nt)}
    for i, c in enumerate(cands):
        dms = np.ascontiguousarray(c["dms"], dtype="<f4")
        na = np.ascontiguousarray(c["nactive"], dtype="<i4")
        planes = [np.ascontiguousarray(c[k], dtype="<i4") for k in _BURST_PLANES]
        if dms.shape != (nd,) or na.shape != (ns,) or any(p.shape != shapes[k] for p, k in zip(planes, _BURST_PLANES)):
            raise ValueError(f"burst file: candidate {i} has the wrong shape")
        blob += [_BURST_CAND.pack(int(c["sample"]), int(c["width"]), int(c["tscrunch"]), int(c["t0"]),
                                  float(c["dm"]), float(c.get("snr", 0.0))), dms.tobytes(), na.tobytes()]
        blob += [p.tobytes() for p in planes]
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class BurstCubeFile:
    """Reader of a burst-cutout file (``bin/burstcube`` / ``python -m
    peasoup_amd burst``): ``len``, ``header``, ``candidate(i)``."""

    def __init__(self, path: str):
        self.path = path
        self._buf = open(path, "rb").read()
        if len(self._buf) < _BURST_HEADER.size or self._buf[:8] != BURST_MAGIC:
            raise ValueError(f"{path}: not a burst-cutout file")
        vals = _BURST_HEADER.unpack_from(self._buf, 0)[1:]
        self.header: Dict = dict(zip(BURST_HEADER_FIELDS, vals))
        nt, ns, nd = self.header["ntime"], self.header["nsub"], self.header["ndm"]
        self._rec = _BURST_CAND.size + 4 * nd + 4 * ns + 8 * (ns + nd) * nt
        if len(self._buf) != _BURST_HEADER.size + self.header["ncand"] * self._rec:
            raise ValueError(f"{path}: truncated burst-cutout file")

    def __len__(self) -> int:
        return int(self.header["ncand"])

    def candidate(self, i: int) -> Dict:
        if not 0 <= i < len(self):
            raise IndexError(i)
        nt, ns, nd = self.header["ntime"], self.header["nsub"], self.header["ndm"]
        o = _BURST_HEADER.size + i * self._rec
        sample, width, f, t0, dm, snr = _BURST_CAND.unpack_from(self._buf, o)
        o += _BURST_CAND.size
        out = {"sample": sample, "width": width, "tscrunch": f, "t0": t0, "dm": dm, "snr": snr}
        out["dms"] = np.frombuffer(self._buf, "<f4", nd, o).copy()
        o += 4 * nd
        out["nactive"] = np.frombuffer(self._buf, "<i4", ns, o).copy()
        o += 4 * ns
        for k, rows in zip(_BURST_PLANES, (ns, ns, nd, nd)):
            out[k] = np.frombuffer(self._buf, "<i4", rows * nt, o).reshape(rows, nt).copy()
            o += 4 * rows * nt
        return out


def burst_mean(sums, hits) -> np.ndarray:
    """Mean raw sample of a cutout plane: sums / hits in float64, NaN where hits == 0."""
    s = np.asarray(sums, dtype=np.float64)
    h = np.asarray(hits, dtype=np.float64)
    out = np.full(s.shape, np.nan, dtype=np.float64)
    np.divide(s, h, out=out, where=h != 0)
    return out


# ---------------------------------------------------------------- burstopt --
BOPT_MAGIC = b"PSBOPT01"
_BOPT_HEADER = struct.Struct("<8s8IQ4d")  # magic, ncand ntime nsub ndm nchans nbits nfine nw, nsamps, 4 doubles
_BOPT_CAND = struct.Struct("<QIIqff7dqff8I")  # the input's six | 7 doubles | opt_sample | opt_dm coarse_dm | 8 u32
BOPT_HEADER_FIELDS = ("ncand", "ntime", "nsub", "ndm", "nchans", "nbits", "nfine", "nw", "nsamps", "tsamp", "fch1",
                      "foff", "fine_half_range")
_BOPT_SCALARS = ("sample", "width", "tscrunch", "t0", "dm", "cand_snr", "snr", "snr_coarse", "snr_in", "snr_dm0",
                 "frac_pos", "v", "mbar_ds", "opt_sample", "opt_dm", "coarse_dm", "opt_width", "opt_kf", "opt_bin",
                 "coarse_row", "coarse_width", "coarse_bin", "flags")
_BOPT_FLOATS = frozenset(("dm", "cand_snr", "snr", "snr_coarse", "snr_in", "snr_dm0", "frac_pos", "v", "mbar_ds",
                          "opt_dm", "coarse_dm"))


def _bopt_arrays(h: Dict):
    nw, ndm, nf, ns, nt = (int(h[k]) for k in ("nw", "ndm", "nfine", "nsub", "ntime"))
    return (("dms", "<f4", (ndm,)), ("dmf", "<f4", (nf,)), ("mbar_dmt", "<f8", (ndm,)), ("best_val", "<i4", (2, nw)),
            ("best_idx", "<i4", (2, nw)), ("curve", "<i4", (nw, ndm + nf)), ("curve_bin", "<i4", (nw, ndm + nf)),
            ("band", "<i4", (ns,)), ("profile", "<i4", (nt,)))


def write_bopt_file(path: str, header: Dict, records: List[Dict]) -> None:
    """Writes a burstopt result file byte for byte as the native
    ``write_bopt_file`` (csrc/src/burstopt.cpp): little-endian ``PSBOPT01``,
    uint32 ncand ntime nsub ndm nchans nbits nfine nw, uint64 nsamps, double
    tsamp fch1 foff fine_half_range (80 bytes); per candidate uint64 sample,
    uint32 width, uint32 tscrunch, int64 t0, float dm, float cand_snr (the
    input's S/N), double snr snr_coarse snr_in snr_dm0 frac_pos v mbar_ds,
    int64 opt_sample, float opt_dm coarse_dm, uint32 opt_width opt_kf opt_bin
    coarse_row coarse_width coarse_bin flags and a zero (136 bytes), then float
    dms[ndm], float dmf[nfine], double mbar_dmt[ndm], int32 best_val[2][nw],
    best_idx[2][nw], curve[nw][ndm + nfine], curve_bin[nw][ndm + nfine],
    band[nsub], profile[ntime].  ``header`` needs every field but ncand.
    Written to a temporary file, then renamed."""
    import os

    h = dict(header, ncand=len(records))
    blob = [_BOPT_HEADER.pack(BOPT_MAGIC, *(int(h[k]) for k in BOPT_HEADER_FIELDS[:9]),
                              *(float(h[k]) for k in BOPT_HEADER_FIELDS[9:]))]
    for i, r in enumerate(records):
        blob.append(_BOPT_CAND.pack(*((float if k in _BOPT_FLOATS else int)(r[k]) for k in _BOPT_SCALARS), 0))
        for name, dt, shape in _bopt_arrays(h):
            a = np.ascontiguousarray(r[name], dtype=dt)
            if a.shape != shape:
                raise ValueError(f"bopt file: candidate {i}: {name} has the wrong shape")
            blob.append(a.tobytes())
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class BurstOptFile:
    """Reader of a burstopt result file (``bin/burstopt`` / ``python -m
    peasoup_amd bopt``): ``len``, ``header``, ``candidate(i)``."""

    def __init__(self, path: str):
        self.path = path
        self._buf = open(path, "rb").read()
        if len(self._buf) < _BOPT_HEADER.size or self._buf[:8] != BOPT_MAGIC:
            raise ValueError(f"{path}: not a burstopt result file")
        vals = _BOPT_HEADER.unpack_from(self._buf, 0)[1:]
        self.header: Dict = dict(zip(BOPT_HEADER_FIELDS, vals))
        self._arrays = _bopt_arrays(self.header)
        self._rec = _BOPT_CAND.size + sum(np.dtype(dt).itemsize * int(np.prod(sh)) for _, dt, sh in self._arrays)
        if len(self._buf) != _BOPT_HEADER.size + self.header["ncand"] * self._rec:
            raise ValueError(f"{path}: truncated burstopt result file")

    def __len__(self) -> int:
        return int(self.header["ncand"])

    def candidate(self, i: int) -> Dict:
        if not 0 <= i < len(self):
            raise IndexError(i)
        o = _BOPT_HEADER.size + i * self._rec
        out = dict(zip(_BOPT_SCALARS, _BOPT_CAND.unpack_from(self._buf, o)))
        o += _BOPT_CAND.size
        for name, dt, shape in self._arrays:
            n = int(np.prod(shape))
            out[name] = np.frombuffer(self._buf, dt, n, o).reshape(shape).copy()
            o += n * np.dtype(dt).itemsize
        return out


# ---------------------------------------------------------------- RFI mask --
RFI_MASK_MAGIC = b"PSMASK01"
_MASK_HEADER = struct.Struct("<8s4I2Q4d")  # magic, nchans nblk nbits zero_dm, nsamps block, tsamp thresh chan_frac block_frac
MASK_HEADER_FIELDS = ("nchans", "nblk", "nbits", "zero_dm", "nsamps", "block", "tsamp", "thresh", "chan_frac",
                      "block_frac")


def write_rfi_mask(path: str, header: Dict, mask: Dict) -> None:
    """Writes an RFI mask file byte for byte as the native ``write_rfi_mask``
    (csrc/src/rfi.cpp): little-endian header ``PSMASK01``, uint32 nchans nblk
    nbits zero_dm, uint64 nsamps block, double tsamp thresh chan_frac
    block_frac; then uint8 chan_flag[nchans], block_flag[nblk],
    cell[nchans][nblk], int32 fill[nchans], G[nblk].  ``header`` needs every
    field but nchans and nblk; ``mask`` is a dict of those arrays.  Written to
    a temporary file, then renamed."""
    import os

    cell = np.ascontiguousarray(mask["cell"], dtype=np.uint8)
    nchans, nblk = cell.shape
    cf = np.ascontiguousarray(mask["chan_flag"], dtype=np.uint8)
    bf = np.ascontiguousarray(mask["block_flag"], dtype=np.uint8)
    fill = np.ascontiguousarray(mask["fill"], dtype="<i4")
    G = np.ascontiguousarray(mask["G"], dtype="<i4")
    if cf.shape != (nchans,) or bf.shape != (nblk,) or fill.shape != (nchans,) or G.shape != (nblk,):
        raise ValueError("rfi mask: inconsistent shapes")
    blob = [_MASK_HEADER.pack(RFI_MASK_MAGIC, nchans, nblk, int(header["nbits"]), int(bool(header["zero_dm"])),
                              int(header["nsamps"]), int(header["block"]), float(header["tsamp"]),
                              float(header["thresh"]), float(header["chan_frac"]), float(header["block_frac"])),
            cf.tobytes(), bf.tobytes(), cell.tobytes(), fill.tobytes(), G.tobytes()]
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(b"".join(blob))
    os.replace(tmp, path)


class RfiMaskFile:
    """Reader of an RFI mask file (``bin/rficlean`` / ``python -m peasoup_amd
    clean``): ``header`` and the arrays ``chan_flag``, ``block_flag``, ``cell``,
    ``fill``, ``G``; ``killmask`` is 0 for a channel without an unflagged cell."""

    def __init__(self, path: str):
        self.path = path
        buf = open(path, "rb").read()
        if len(buf) < _MASK_HEADER.size or buf[:8] != RFI_MASK_MAGIC:
            raise ValueError(f"{path}: not an RFI mask file")
        self.header: Dict = dict(zip(MASK_HEADER_FIELDS, _MASK_HEADER.unpack_from(buf, 0)[1:]))
        nc, nb = self.header["nchans"], self.header["nblk"]
        if len(buf) != _MASK_HEADER.size + nc + nb + nc * nb + 4 * nc + 4 * nb:
            raise ValueError(f"{path}: truncated RFI mask file")
        o = _MASK_HEADER.size
        self.chan_flag = np.frombuffer(buf, np.uint8, nc, o).copy()
        o += nc
        self.block_flag = np.frombuffer(buf, np.uint8, nb, o).copy()
        o += nb
        self.cell = np.frombuffer(buf, np.uint8, nc * nb, o).reshape(nc, nb).copy()
        o += nc * nb
        self.fill = np.frombuffer(buf, "<i4", nc, o).copy()
        o += 4 * nc
        self.G = np.frombuffer(buf, "<i4", nb, o).copy()

    @property
    def killmask(self) -> List[int]:
        return [int(k) for k in (self.cell == 0).any(axis=1)]

    def as_dict(self) -> Dict:
        return {"chan_flag": self.chan_flag, "block_flag": self.block_flag, "cell": self.cell, "fill": self.fill,
                "G": self.G}
