"""Pure-Python search-mode PSRFITS I/O (NumPy only), written from the PSRFITS
definition as csrc/include/psoup/psrfits.hpp states it and independent of the
native parser, so tests can cross-check the two.

``read_psrfits`` returns the header dicts, the column table and the small
columns as arrays plus the DATA bytes; ``write_psrfits`` writes search-mode
files from arrays (for tests and for users who want to feed ``fits2fil``).
Everything in a FITS file is big-endian; blocks are 2880 bytes, cards 80
characters.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

BLOCK = 2880
CARD = 80
_TFORM_BYTES = {"B": 1, "A": 1, "I": 2, "J": 4, "E": 4, "D": 8}
_NP_TYPE = {"B": ">u1", "A": "S1", "I": ">i2", "J": ">i4", "E": ">f4", "D": ">f8"}


# ------------------------------------------------------------------ cards --
def parse_tform(s: str) -> Tuple[int, str, int]:
    """'rT' -> (repeat, type letter, bytes); the repeat is 1 when absent."""
    s = s.strip()
    i = 0
    while i < len(s) and s[i].isdigit():
        i += 1
    if i + 1 != len(s) or (s[i] not in _TFORM_BYTES and s[i] != "X"):
        raise ValueError(f"fits: unsupported TFORM '{s}'")
    r = int(s[:i]) if i else 1
    t = s[i]
    return r, t, (r + 7) // 8 if t == "X" else r * _TFORM_BYTES[t]


def _card_value(card: str) -> str:
    v = card[10:]
    t = v.lstrip(" ")
    if t.startswith("'"):
        out = []
        i = 1
        while i < len(t):
            if t[i] == "'":
                if i + 1 < len(t) and t[i + 1] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(t[i])
            i += 1
        return "".join(out).rstrip(" ")
    return v.split("/", 1)[0].strip()


def _read_cards(buf: bytes, off: int) -> Tuple[Dict[str, str], int]:
    """The header at ``off``: ({key: value text}, offset of its data area)."""
    cards: Dict[str, str] = {}
    at = off
    while True:
        if at + CARD > len(buf):
            raise ValueError("fits: a header runs past the end of the file (no END card)")
        card = buf[at:at + CARD].decode("latin-1")
        key = card[:8].strip()
        at += CARD
        if key == "END":
            return cards, off + -(-(at - off) // BLOCK) * BLOCK
        if not key or key in ("COMMENT", "HISTORY") or card[8] != "=":
            continue
        cards.setdefault(key, _card_value(card))


def _num(text: str) -> float:
    return float(text.strip().replace("D", "E").replace("d", "E"))


def _data_area(c: Dict[str, str]) -> int:
    if int(c.get("NAXIS", "0")) <= 0:
        return 0
    n = int(c.get("NAXIS1", "0")) * int(c.get("NAXIS2", "1")) + int(c.get("PCOUNT", "0"))
    return -(-n // BLOCK) * BLOCK


def read_psrfits(path_or_bytes) -> Dict:
    """A search-mode PSRFITS file as a dict: ``primary`` and ``subint`` (header
    dicts of value texts), ``columns`` ([(name, type, repeat, offset, bytes)]),
    ``table_off``, ``row_bytes``, ``nrows``, ``npol``, ``nbits``, ``nchan``,
    ``nsblk``, ``signint``, ``tbin``, ``chan_bw``, ``z``, ``pol_type``, and the
    columns OFFS_SUB (float64 [nrows] or None), DAT_FREQ (float64 [nrows,
    nchan]), DAT_WTS (float32 [nrows, nchan]), DAT_OFFS and DAT_SCL (float32
    [nrows, npol, nchan]) in host byte order, DATA (uint8 [nrows, bytes])."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        buf = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            buf = f.read()
    if buf[:9] != b"SIMPLE  =":
        raise ValueError("fits: not a FITS file (no SIMPLE = T)")
    primary, off = _read_cards(buf, 0)
    if primary.get("SIMPLE") != "T":
        raise ValueError("fits: not a FITS file (no SIMPLE = T)")
    if "OBS_MODE" not in primary:
        raise ValueError("fits: missing key OBS_MODE in the primary header")
    if primary["OBS_MODE"].strip().upper() != "SEARCH":
        raise ValueError(f"fits: OBS_MODE is '{primary['OBS_MODE']}', not SEARCH")
    off += _data_area(primary)
    sub = None
    while off < len(buf):
        c, data = _read_cards(buf, off)
        if c.get("XTENSION", "").strip() == "BINTABLE" and c.get("EXTNAME", "").strip() == "SUBINT":
            sub, table_off = c, data
            break
        off = data + _data_area(c)
    if sub is None:
        raise ValueError("fits: no SUBINT table")

    def need(key):
        if key not in sub:
            raise ValueError(f"fits: missing key {key} in the SUBINT header")
        return sub[key]

    out = {"primary": primary, "subint": sub, "table_off": table_off}
    out["row_bytes"], out["nrows"] = int(need("NAXIS1")), int(need("NAXIS2"))
    tfields = int(need("TFIELDS"))
    npol, nbits, nchan, nsblk = (int(need(k)) for k in ("NPOL", "NBITS", "NCHAN", "NSBLK"))
    out.update(npol=npol, nbits=nbits, nchan=nchan, nsblk=nsblk, tbin=_num(need("TBIN")),
               pol_type=need("POL_TYPE").strip())
    if nbits not in (1, 2, 4, 8, 16):
        raise ValueError(f"fits: NBITS must be 1, 2, 4, 8 or 16, got {nbits}")
    if (nchan * nbits) % 8:
        raise ValueError(f"fits: NCHAN x NBITS must be a multiple of 8, got {nchan} x {nbits}")
    try:
        out["signint"] = 1 if int(sub.get("SIGNINT", "0")) == 1 else 0
    except ValueError:
        out["signint"] = 0
    try:
        out["chan_bw"] = _num(sub.get("CHAN_BW", "0"))
    except ValueError:
        out["chan_bw"] = 0.0
    z = 0.0
    try:
        with np.errstate(over="ignore"):
            zf = np.abs(np.float32(_num(sub["ZERO_OFF"])))
        if np.isfinite(zf):
            z = float(zf)
    except (KeyError, ValueError):
        pass
    out["z"] = z
    cols, at = [], 0
    for i in range(1, tfields + 1):
        name = need(f"TTYPE{i}").strip()
        r, t, nb = parse_tform(need(f"TFORM{i}"))
        cols.append((name, t, r, at, nb))
        at += nb
    out["columns"] = cols
    if at != out["row_bytes"]:
        raise ValueError(f"fits: the column sizes add up to {at} bytes, NAXIS1 is {out['row_bytes']}")
    by = {c[0]: c for c in cols}
    for name, kinds, count in (("DAT_FREQ", "ED", nchan), ("DAT_WTS", "E", nchan), ("DAT_OFFS", "E", npol * nchan),
                               ("DAT_SCL", "E", npol * nchan)):
        if name not in by:
            raise ValueError(f"fits: missing column {name}")
        if by[name][1] not in kinds or by[name][2] != count:
            raise ValueError(f"fits: {name} has the wrong length or type")
    if "DATA" not in by:
        raise ValueError("fits: missing column DATA")
    dbytes = nsblk * npol * nchan * nbits // 8
    if by["DATA"][1] not in "BI":
        raise ValueError("fits: DATA must be of type B or I (32-bit float DATA is out of scope)")
    if by["DATA"][4] != dbytes:
        raise ValueError(f"fits: the DATA column holds {by['DATA'][4]} bytes, NSBLK x NPOL x NCHAN x NBITS / 8 is {dbytes}")
    nrows, rb = out["nrows"], out["row_bytes"]
    if nrows < 1:
        raise ValueError("fits: NAXIS2 = 0: the SUBINT table has no rows")
    if table_off + nrows * rb > len(buf):
        raise ValueError("fits: the SUBINT table runs past the end of the file")
    table = np.frombuffer(buf, np.uint8, nrows * rb, table_off).reshape(nrows, rb)

    def column(name, dtype=None):
        _, t, r, o, nb = by[name]
        raw = np.ascontiguousarray(table[:, o:o + nb])
        return raw.view(dtype or _NP_TYPE[t]).reshape(nrows, -1)

    out["OFFS_SUB"] = column("OFFS_SUB").astype(np.float64)[:, 0] if "OFFS_SUB" in by and by["OFFS_SUB"][1:3] == ("D", 1) \
        else None
    out["DAT_FREQ"] = column("DAT_FREQ").astype(np.float64)
    out["DAT_WTS"] = column("DAT_WTS").astype(np.float32)
    out["DAT_OFFS"] = column("DAT_OFFS").astype(np.float32).reshape(nrows, npol, nchan)
    out["DAT_SCL"] = column("DAT_SCL").astype(np.float32).reshape(nrows, npol, nchan)
    out["DATA"] = column("DATA", np.uint8)
    return out


# ---------------------------------------------------------------- samples --
def pack_samples(raw: np.ndarray, nbits: int) -> np.ndarray:
    """Integer samples [..., nchan] -> the DATA bytes: below 8 bits packed
    most-significant bits first, 8 bits one byte (two's complement for negative
    values), 16 bits big-endian."""
    raw = np.asarray(raw)
    if nbits == 16:
        return np.ascontiguousarray(raw.astype(np.int64) & 0xFFFF).astype(">u2").view(np.uint8).reshape(-1)
    if nbits == 8:
        return (raw.astype(np.int64) & 0xFF).astype(np.uint8).reshape(-1)
    per = 8 // nbits
    if raw.shape[-1] % per:
        raise ValueError("NCHAN x NBITS must be a multiple of 8")
    v = (raw.astype(np.int64) & ((1 << nbits) - 1)).reshape(-1, per)
    out = np.zeros(v.shape[0], np.int64)
    for q in range(per):
        out |= v[:, q] << (8 - nbits * (q + 1))
    return out.astype(np.uint8)


def unpack_samples(data: np.ndarray, nbits: int, signed: bool = False) -> np.ndarray:
    """DATA bytes -> int32 samples, flat, in file order."""
    b = np.asarray(data, np.uint8).reshape(-1)
    if nbits == 16:
        v = b.view(">u2").astype(np.int32)
        return np.where(v >= 32768, v - 65536, v) if signed else v
    if nbits == 8:
        return b.view(np.int8).astype(np.int32) if signed else b.astype(np.int32)
    per = 8 // nbits
    out = np.empty((b.size, per), np.int32)
    for q in range(per):
        out[:, q] = (b >> (8 - nbits * (q + 1))) & ((1 << nbits) - 1)
    return out.reshape(-1)


# ----------------------------------------------------------------- writer --
def _card(key: str, value) -> bytes:
    if isinstance(value, bool):
        text = "T" if value else "F"
        text = text.rjust(20)
    elif isinstance(value, str):
        text = "'" + value.replace("'", "''").ljust(8) + "'"
    elif isinstance(value, (int, np.integer)):
        text = str(int(value)).rjust(20)
    else:
        text = repr(float(value)).upper().rjust(20)
    return (key.ljust(8)[:8] + "= " + text).ljust(CARD)[:CARD].encode("latin-1")


def _header(cards: Sequence[Tuple[str, object]]) -> bytes:
    h = b"".join(_card(k, v) for k, v in cards) + b"END".ljust(CARD)
    return h.ljust(-(-len(h) // BLOCK) * BLOCK)


def _pad(b: bytes) -> bytes:
    return b.ljust(-(-len(b) // BLOCK) * BLOCK, b"\0")


def bintable_hdu(extname: str, columns: Sequence[Tuple[str, str, np.ndarray]], extra: Sequence[Tuple[str, object]] = (),
                 heap: bytes = b"") -> bytes:
    """A BINTABLE HDU from (name, TFORM, array [nrows, ...]) columns; ``heap``
    bytes follow the table and are counted in PCOUNT."""
    nrows = len(columns[0][2]) if columns else 0
    fields, row = [], 0
    for name, form, arr in columns:
        r, t, nb = parse_tform(form)
        a = np.asarray(arr)
        if a.dtype == np.uint8:  # the field's bytes as they are
            raw = np.ascontiguousarray(a).reshape(nrows, -1)
        elif t == "A":
            raw = np.array([str(s).encode("latin-1").ljust(r)[:r] for s in a], dtype=f"S{r}").view(np.uint8).reshape(nrows, -1)
        else:
            raw = np.ascontiguousarray(a.reshape(nrows, -1).astype(_NP_TYPE[t])).view(np.uint8).reshape(nrows, -1)
        if raw.shape[1] != nb:
            raise ValueError(f"column {name}: {raw.shape[1]} bytes per row, TFORM {form} holds {nb}")
        fields.append(raw)
        row += nb
    cards: List[Tuple[str, object]] = [("XTENSION", "BINTABLE"), ("BITPIX", 8), ("NAXIS", 2), ("NAXIS1", row),
                                       ("NAXIS2", nrows), ("PCOUNT", len(heap)), ("GCOUNT", 1),
                                       ("TFIELDS", len(columns))]
    for i, (name, form, _) in enumerate(columns, 1):
        cards += [(f"TTYPE{i}", name), (f"TFORM{i}", form)]
    cards.append(("EXTNAME", extname))
    cards += list(extra)
    body = np.concatenate(fields, axis=1).tobytes() if fields and nrows else b""
    return _header(cards) + _pad(body + heap)


def psrfits_bytes(raw: np.ndarray, nbits: int, tbin: float, freq, scl=None, offs=None, wts=None, offs_sub=None,
                  signint: int = 0, zero_off=None, pol_type: Optional[str] = None, primary: Optional[Dict] = None,
                  subint: Optional[Dict] = None, column_order: Optional[Sequence[str]] = None,
                  hdus_before: Sequence[bytes] = (), freq_form: str = "E", extra_columns=(), naxis1_extra: int = 0,
                  data_form: Optional[str] = None) -> bytes:
    """A search-mode PSRFITS file from integer samples ``raw`` [nrows, nsblk,
    npol, nchan].  ``freq`` [nchan] (or [nrows, nchan]) in MHz; ``scl`` and
    ``offs`` [nrows, npol, nchan] (default 1 and 0), ``wts`` [nrows, nchan]
    (default 1), ``offs_sub`` [nrows] seconds (default the rows' centres;
    ``False`` leaves the column out).  ``primary`` / ``subint`` add or override
    header keys (a value of None removes the key); ``column_order`` names the
    columns in the order to write; ``hdus_before`` are whole HDUs put between
    the primary HDU and SUBINT; ``naxis1_extra`` misstates NAXIS1 (for tests)."""
    raw = np.asarray(raw)
    nrows, nsblk, npol, nchan = raw.shape
    freq = np.broadcast_to(np.asarray(freq, np.float64), (nrows, nchan))
    scl = np.ones((nrows, npol, nchan), np.float32) if scl is None else np.asarray(scl, np.float32)
    offs = np.zeros((nrows, npol, nchan), np.float32) if offs is None else np.asarray(offs, np.float32)
    wts = np.ones((nrows, nchan), np.float32) if wts is None else np.asarray(wts, np.float32)
    data = pack_samples(raw, nbits).reshape(nrows, -1)
    cols = {
        "DAT_FREQ": ("DAT_FREQ", f"{nchan}{freq_form}", freq),
        "DAT_WTS": ("DAT_WTS", f"{nchan}E", wts),
        "DAT_OFFS": ("DAT_OFFS", f"{npol * nchan}E", offs),
        "DAT_SCL": ("DAT_SCL", f"{npol * nchan}E", scl),
        "DATA": ("DATA", data_form or f"{data.shape[1]}B", data),
    }
    if offs_sub is not False:
        t = (np.arange(nrows) + 0.5) * (nsblk * tbin) if offs_sub is None else np.asarray(offs_sub, np.float64)
        cols["OFFS_SUB"] = ("OFFS_SUB", "1D", t)
    for c in extra_columns:
        cols[c[0]] = c
    order = list(column_order) if column_order else [k for k in ("OFFS_SUB",) if k in cols] + [
        c[0] for c in extra_columns] + ["DAT_FREQ", "DAT_WTS", "DAT_OFFS", "DAT_SCL", "DATA"]
    if pol_type is None:
        pol_type = {1: "AA+BB", 2: "AABB", 4: "AABBCRCI"}.get(npol, "AABB")
    df = float(freq[0, 1] - freq[0, 0]) if nchan > 1 else 1.0
    sub = {"INT_TYPE": "TIME", "NPOL": npol, "POL_TYPE": pol_type, "TBIN": float(tbin), "NBITS": nbits, "NCHAN": nchan,
           "CHAN_BW": df, "NSBLK": nsblk, "NSUBOFFS": 0, "ZERO_OFF": 0.0 if zero_off is None else zero_off,
           "SIGNINT": int(signint)}
    sub.update(subint or {})
    prim = {"SIMPLE": True, "BITPIX": 8, "NAXIS": 0, "EXTEND": True, "FITSTYPE": "PSRFITS", "TELESCOP": "Parkes",
            "OBS_MODE": "SEARCH", "SRC_NAME": "J0000+0000", "RA": "00:00:00.0", "DEC": "+00:00:00.0",
            "STT_IMJD": 55000, "STT_SMJD": 0, "STT_OFFS": 0.0}
    prim.update(primary or {})
    hdu = bintable_hdu("SUBINT", [cols[k] for k in order], [(k, v) for k, v in sub.items() if v is not None])
    if naxis1_extra:
        row = sum(parse_tform(cols[k][1])[2] for k in order)
        hdu = hdu.replace(_card("NAXIS1", row), _card("NAXIS1", row + naxis1_extra), 1)
    return _header([(k, v) for k, v in prim.items() if v is not None]) + b"".join(hdus_before) + hdu


def write_psrfits(path: str, raw: np.ndarray, nbits: int, tbin: float, freq, **kw) -> None:
    """Writes ``psrfits_bytes(raw, nbits, tbin, freq, **kw)`` to ``path``."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(psrfits_bytes(raw, nbits, tbin, freq, **kw))
    os.replace(tmp, path)
