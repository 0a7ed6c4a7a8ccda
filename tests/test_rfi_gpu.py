"""RFI excision on the device (csrc/kernels/rfi.hip): everything is integer, so
every comparison with the NumPy oracle (utils.reference.rfi_*) is exact.
pack_transpose round trips, rfi_block_sums, the whole cleaner with and without
zero-DM in place and out of place, clamping, blocks without a live channel,
and the two file drivers (bin/rficlean, python -m peasoup_amd clean)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd import ops
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils import sigproc, synthetic
from peasoup_amd.utils.outputs import RfiMaskFile

pytestmark = pytest.mark.gpu
T = C.rfi_tile()


def _bias(nbits):
    return 128 if nbits == 8 else 0


def _rows(x, nbits, pad=16):
    """Raw samples [nchans, nsamps] -> device int8 rows (x - bias) with a padded stride."""
    nchans, nsamps = x.shape
    stride = (nsamps + 15) // 16 * 16 + pad
    rows = torch.zeros((nchans, stride), dtype=torch.int8)
    rows[:, :nsamps] = torch.from_numpy((x - _bias(nbits)).astype(np.int8))
    return rows.cuda()


def _raw(rows, nsamps, nbits):
    return rows[:, :nsamps].cpu().numpy().astype(np.int64) + _bias(nbits)


# -------------------------------------------------------- pack_transpose ----
@pytest.mark.parametrize("nchans", [40, 64])
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_pack_transpose_inverts_unpack(nbits, nchans):
    nsamps = 2 * T + 37
    rng = np.random.default_rng(nbits * 100 + nchans)
    packed = torch.from_numpy(rng.integers(0, 256, nsamps * nchans * nbits // 8, dtype=np.uint8)).cuda()
    rows = ops.unpack_transpose(packed, nsamps, nchans, nbits, _bias(nbits))
    back = ops.pack_transpose(rows, nsamps, nbits, _bias(nbits))
    assert torch.equal(back, packed)
    # a padded stride, and the values agree with the NumPy unpack
    rows2 = ops.unpack_transpose(packed, nsamps, nchans, nbits, _bias(nbits), stride=nsamps + 91)
    assert torch.equal(ops.pack_transpose(rows2, nsamps, nbits, _bias(nbits)), packed)
    vals = sigproc.unpack_samples(packed.cpu().numpy(), nsamps, nchans, nbits)
    assert np.array_equal(_raw(rows, nsamps, nbits), vals.T.astype(np.int64))


# -------------------------------------------------------- rfi_block_sums ----
def _noise(rng, nbits, nchans, nsamps):
    V = (1 << nbits) - 1
    if nbits == 8:
        return np.clip(np.rint(rng.normal(128, 12, (nchans, nsamps))), 0, V).astype(np.int64)
    return rng.choice(4, size=(nchans, nsamps), p=[0.1, 0.4, 0.4, 0.1]).astype(np.int64)


@pytest.mark.parametrize("nchans", [40, 64])
@pytest.mark.parametrize("nbits", [2, 8])
def test_block_sums_equal_oracle(nbits, nchans):
    nsamps, block = 20037, 1024  # a short last block; nsamps is no multiple of 16
    x = _noise(np.random.default_rng(nbits + nchans), nbits, nchans, nsamps)
    x[1] = (1 << nbits) - 1
    x[2] = 0
    S1, S2 = ops.rfi_block_sums(_rows(x, nbits), nsamps, block, _bias(nbits))
    R1, R2 = ref.rfi_block_sums(x, block)
    assert S1.shape == (nchans, 20) and np.array_equal(S1.cpu().numpy().astype(np.uint64), R1)
    assert np.array_equal(S2.cpu().numpy().astype(np.uint64), R2)


def test_block_sums_overflow_corner_and_stride():
    # the longest block, every sample 255: sum x^2 = 65536 * 65025 > 2^31
    nsamps, block = 65536 + 4099, 65536
    x = np.full((1, nsamps), 255, dtype=np.int64)
    S1, S2 = ops.rfi_block_sums(_rows(x, 8), nsamps, block, 128)
    assert S1.cpu().tolist() == [[255 * 65536, 255 * 4099]]
    assert S2.cpu().tolist() == [[65025 * 65536, 65025 * 4099]]
    # and every sample 0 (stored -128: the largest stored squares)
    S1, S2 = ops.rfi_block_sums(_rows(np.zeros((1, nsamps), dtype=np.int64), 8), nsamps, block, 128)
    assert S1.cpu().tolist() == [[0, 0]] and S2.cpu().tolist() == [[0, 0]]
    # a row stride far larger than nsamps, rows after the first non-zero in the padding
    nsamps = 3 * 256 + 5
    x = _noise(np.random.default_rng(9), 8, 5, nsamps)
    rows = _rows(x, 8, pad=1024 + 48)
    rows[:, nsamps:] = 77
    S1, S2 = ops.rfi_block_sums(rows, nsamps, 256, 128)
    R1, R2 = ref.rfi_block_sums(x, 256)
    assert np.array_equal(S1.cpu().numpy().astype(np.uint64), R1)
    assert np.array_equal(S2.cpu().numpy().astype(np.uint64), R2)
    with pytest.raises(ValueError):
        ops.rfi_block_sums(torch.zeros((2, 1000), dtype=torch.int8).cuda(), 1000, 256)  # stride not a multiple of 16


# -------------------------------------------------------------- rfi_clean ---
BLOCK = 512
NSAMPS = 24 * BLOCK + 37
NCHANS = 40
KILL = [1] * NCHANS
KILL[10] = KILL[11] = 0


@functools.lru_cache(maxsize=None)
def _case(nbits):
    """Noise with, all at once: a channel of tripled variance, two adjacent
    blocks of broadband offset, one isolated bad cell, an all-zero channel (and
    two killed channels in KILL)."""
    rng = np.random.default_rng(40 + nbits)
    V = (1 << nbits) - 1
    x = _noise(rng, nbits, NCHANS, NSAMPS)
    if nbits == 8:
        x[20] = np.clip(np.rint(rng.normal(128, 12 * np.sqrt(3.0), NSAMPS)), 0, V)
        x[:, 5 * BLOCK:7 * BLOCK] += 30
        x[7, 2 * BLOCK:3 * BLOCK] += 40
    else:
        x[20] = rng.choice(4, size=NSAMPS, p=[0.425, 0.075, 0.075, 0.425])  # variance 1.95 against 0.65
        x[:, 5 * BLOCK:7 * BLOCK] = np.minimum(x[:, 5 * BLOCK:7 * BLOCK] + 1, V)
        x[7, 2 * BLOCK:3 * BLOCK] = V
    x[3] = 0
    x = np.clip(x, 0, V)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(nbits, zero_dm):
    y, m = ref.rfi_clean(_case(nbits), BLOCK, nbits, KILL, zero_dm=zero_dm)
    y.setflags(write=False)
    return y, m


def _check_mask(mask, m):
    for k in ("chan_flag", "block_flag", "cell", "fill", "G", "nb"):
        assert np.array_equal(np.asarray(getattr(mask, k)), m[k]), k
    assert list(mask.killmask) == m["killmask"]


@pytest.mark.parametrize("nbits", [2, 8])
def test_case_exercises_every_rule(nbits):
    _, m = _oracle(nbits, True)
    # dead and killed channels; the channel that is noisy throughout is no
    # outlier against its own blocks and stays
    assert np.nonzero(m["chan_flag"])[0].tolist() == [3, 10, 11]
    assert [c for c in range(NCHANS) if m["killmask"][c] == 0] == [3, 10, 11]
    assert m["block_flag"][:7].tolist() == [0] * 5 + [1, 1]                           # the broadband blocks
    assert m["cell"][7, 1:4].tolist() == [0, 1, 0]                                    # the bad cell
    assert m["nb"][5] == 0 and m["nb"][0] == NCHANS - 3 and m["nb"][2] == NCHANS - 4  # a block without a live channel


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("zero_dm", [False, True])
@pytest.mark.parametrize("nbits", [2, 8])
def test_clean_equals_oracle(nbits, zero_dm, in_place):
    x = _case(nbits)
    want, m = _oracle(nbits, zero_dm)
    rows = _rows(x, nbits)
    rows[:, NSAMPS:] = 5  # the padding must come through untouched
    out = None if in_place else torch.full_like(rows, 9)
    got, mask = ops.rfi_clean(rows, NSAMPS, nbits, _bias(nbits), KILL, block=BLOCK, zero_dm=zero_dm, out=out)
    _check_mask(mask, m)
    assert (got.data_ptr() == rows.data_ptr()) == in_place
    assert np.array_equal(_raw(got, NSAMPS, nbits), want)
    assert bool((got[:, NSAMPS:] == (5 if in_place else 9)).all())
    if not in_place:
        assert np.array_equal(_raw(rows, NSAMPS, nbits), x)  # the input is not written
    assert want.min() >= 0 and want.max() <= (1 << nbits) - 1
    if not zero_dm:  # unflagged cells are the input
        keep = np.repeat(m["cell"] == 0, BLOCK, axis=1)[:, :NSAMPS]
        assert np.array_equal(want[keep], x[keep])


@pytest.mark.parametrize("zero_dm", [False, True])
def test_clean_tile_is_a_block(zero_dm):
    # rfi_tile() divides every legal block length, so no tile straddles a block
    # edge; the closest shape is a block of one tile, with a ragged end
    nsamps, nbits = 9 * T + 37, 8
    rng = np.random.default_rng(3)
    x = _noise(rng, nbits, 24, nsamps)
    x[:, 4 * T:5 * T] += 50
    x[5, T:2 * T] += 60
    want, m = ref.rfi_clean(x, T, nbits, None, zero_dm=zero_dm)
    assert m["block_flag"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and m["cell"][5, 1] == 1
    got, mask = ops.rfi_clean(_rows(x, nbits), nsamps, nbits, 128, block=T, zero_dm=zero_dm)
    _check_mask(mask, m)
    assert np.array_equal(_raw(got, nsamps, nbits), want)


@pytest.mark.parametrize("nbits", [2, 8])
def test_zero_dm_clamps_at_both_ends(nbits):
    V = (1 << nbits) - 1
    nchans, nsamps = 16, 3 * T + 5
    rng = np.random.default_rng(nbits)
    x = rng.integers(0, V + 1, (nchans, nsamps))
    x[:, 10::40] = V   # most of the band high, two channels at 0: they clamp at 0
    x[:2, 10::40] = 0
    x[:, 20::40] = 0   # most of the band low, two channels at V: they clamp at V
    x[:2, 20::40] = V
    want, m = ref.rfi_clean(x, T, nbits, None, thresh=1e9, zero_dm=True)
    assert not m["cell"].any()
    Z = x.sum(axis=0)
    unclamped = x - ((2 * Z + nchans) // (2 * nchans))[None, :] + np.repeat(m["G"], T)[None, :nsamps]
    assert unclamped.min() < 0 and unclamped.max() > V and want.min() == 0 and want.max() == V
    got, mask = ops.rfi_clean(_rows(x, nbits), nsamps, nbits, _bias(nbits), block=T, thresh=1e9, zero_dm=True)
    _check_mask(mask, m)
    assert np.array_equal(_raw(got, nsamps, nbits), want)
    # the apply step alone, from the oracle's mask
    got2 = ops.rfi_apply(_rows(x, nbits), nsamps, nbits, m, T, _bias(nbits), zero_dm=True)
    assert np.array_equal(_raw(got2, nsamps, nbits), want)


# -------------------------------------------------------- file round trip ---
@pytest.mark.parametrize("nbits,zero_dm", [(2, False), (8, True)])
def test_file_round_trip_both_drivers(tmp_path, nbits, zero_dm):
    x = _case(nbits)
    hdr = synthetic.make_header(nchans=NCHANS, nbits=nbits, tsamp=64e-6)
    fil = str(tmp_path / "in.fil")
    sigproc.write_filterbank(fil, hdr, x.T.astype(np.uint8))
    killfile = str(tmp_path / "kill.txt")
    open(killfile, "w").write("".join(f"{k}\n" for k in KILL))
    want, m = _oracle(nbits, zero_dm)
    size = sigproc.read_header(fil)["size"]
    head = open(fil, "rb").read()[:size]
    outs = {}
    for name, cmd in (("native", [os.path.join(REPO, "bin", "rficlean")]),
                      ("python", [sys.executable, "-m", "peasoup_amd", "clean"])):
        o = {k: str(tmp_path / f"{name}.{k}") for k in ("fil", "mask", "kill")}
        args = ["-i", fil, "-o", o["fil"], "-k", killfile, "--mask_out", o["mask"], "--kill_out", o["kill"],
                "--rfi_block", str(BLOCK)] + (["--zero_dm"] if zero_dm else [])
        r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(o["fil"], "rb").read()
        assert raw[:size] == head and len(raw) == os.path.getsize(fil)  # the header bytes verbatim
        assert np.array_equal(sigproc.read_filterbank(o["fil"]).data.T.astype(np.int64), want)
        assert C.read_killfile(o["kill"], NCHANS) == (m["killmask"], True)
        f = RfiMaskFile(o["mask"])
        assert f.header["nbits"] == nbits and f.header["zero_dm"] == int(zero_dm) and f.header["tsamp"] == 64e-6
        assert f.header["block"] == BLOCK and f.header["nsamps"] == NSAMPS
        for k in ("chan_flag", "block_flag", "cell", "fill", "G"):
            assert np.array_equal(getattr(f, k), m[k]), k
        assert not any(os.path.exists(p + ".tmp") for p in o.values())
        outs[name] = o
    for k in ("fil", "mask", "kill"):  # the two drivers write the same bytes
        assert open(outs["native"][k], "rb").read() == open(outs["python"][k], "rb").read(), k


# ------------------------------------------------------------- end to end ---
# One dispersed burst, four DM-0 broadband impulses and one noisy channel in an
# 8-bit filterbank whose band (400 -> 337 MHz) sweeps 10.6 ms per unit DM.
E2E_N = 1 << 15
E2E_TSAMP = 1e-3
E2E_BURST = synthetic.BurstSpec(time=12.0, dm=25.0, width=8e-3, amplitude=0.5)
E2E_IMPULSES = (5.0, 9.0, 20.0, 26.0)
E2E_RFI = tuple(synthetic.RfiSpec("impulse", time=t, duration=4e-3, amplitude=1.0) for t in E2E_IMPULSES) + \
    (synthetic.RfiSpec("channel", channel=10, amplitude=2.0),)
E2E_FLAGS = ["--dm_start", "0", "--dm_end", "50", "--dm_pulse_width", "4000", "-t", "1", "--rfi_block", "1024"]


def _e2e_header():
    return synthetic.make_header(nchans=64, nbits=8, tsamp=E2E_TSAMP, fch1=400.0, foff=-1.0)


@functools.lru_cache(maxsize=None)
def _e2e_values():
    v = synthetic.generate(E2E_N, _e2e_header(), [], seed=77, bursts=[E2E_BURST], rfi=E2E_RFI)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _e2e_oracle(clean):
    """The NumPy chain: (reference.rfi_clean,) reference.dedisperse, reference.sp_*; returns
    (candidates, dm_list)."""
    hdr = _e2e_header()
    vals = _e2e_values().astype(np.int64)
    kill = None
    if clean:
        y, m = ref.rfi_clean(vals.T, 1024, 8, None, zero_dm=True)
        vals, kill = y.T, m["killmask"]
    dms = list(C.generate_dm_list(0.0, 50.0, E2E_TSAMP, 4000.0, hdr["fch1"], hdr["foff"], 64, 1.10))
    delays = ref.delay_table(64, E2E_TSAMP, hdr["fch1"], hdr["foff"])
    trials = ref.dedisperse(vals, ref.dm_offsets(dms, delays), 8, kill)
    n = trials.shape[1]
    baseline = min(max(int(np.ceil(2.0 / E2E_TSAMP)), 64), n)
    widths = ref.sp_widths(n, 4096)
    events = []
    for d in range(len(dms)):
        for k, (mx, am) in enumerate(ref.sp_block_maxima(ref.sp_boxcar_snr(trials[d], baseline, widths))):
            events += [(int(a), k, float(s), d) for s, a in zip(mx, am) if s >= 6.5]
    return ref.sp_cluster_ref(events, dms, float(delays[-1]) * E2E_TSAMP, E2E_TSAMP), dms


def _at_impulse(time_s, width):
    return any(abs(time_s - t) <= (width + 4) * E2E_TSAMP for t in E2E_IMPULSES)


def _check_e2e(raw, cleaned, dms):
    """raw / cleaned: candidate lists as (snr, time_s, width, dm_idx), S/N descending."""
    assert raw and _at_impulse(raw[0][1], raw[0][2]), raw[:3]             # without --rfi an impulse ranks first
    assert cleaned, "no candidates after cleaning"
    snr, time_s, width, dm_idx = cleaned[0]
    want = int(np.argmin(np.abs(np.asarray(dms) - E2E_BURST.dm)))
    assert abs(dm_idx - want) <= 1 and abs(time_s - E2E_BURST.time) <= width * E2E_TSAMP, cleaned[:3]
    assert not [c for c in cleaned if c[3] == 0 and _at_impulse(c[1], c[2])]  # none at an impulse at the lowest DM


def test_end_to_end_zero_dm_uncovers_the_burst(tmp_path):
    tup = lambda cs: [(c["snr"], c["time_s"], c["width"], c["dm_idx"]) for c in cs]  # noqa: E731
    (raw, dms), (cleaned, _) = _e2e_oracle(False), _e2e_oracle(True)
    _check_e2e(tup(raw), tup(cleaned), dms)   # the fixture itself, on the NumPy chain
    fil = str(tmp_path / "e2e.fil")
    sigproc.write_filterbank(fil, _e2e_header(), _e2e_values())
    got = {}
    for name, extra in (("raw", []), ("clean", ["--rfi", "--zero_dm", "--rfi_mask_out", str(tmp_path / "e2e.mask")])):
        ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", fil, "-o", str(tmp_path / f"{name}.txt")] + E2E_FLAGS + extra)
        assert ok and a.rfi == bool(extra)
        res = C.run_sp_pipeline(a)
        assert np.allclose(res.dm_list, dms)
        got[name] = [(c.snr, c.time_s, c.width, c.dm_idx) for c in res.candidates]
        C.write_sp_output(a.outfilename, a, res)
        head = [ln for ln in open(a.outfilename) if ln.startswith("# rfi:")]
        assert len(head) == (2 if extra else 0) and (not extra or "zero_dm: 1" in head[1])
    _check_e2e(got["raw"], got["clean"], dms)
    want, m = ref.rfi_clean(_e2e_values().astype(np.int64).T, 1024, 8, None, zero_dm=True)
    f = RfiMaskFile(str(tmp_path / "e2e.mask"))
    assert np.array_equal(f.cell, m["cell"]) and np.array_equal(f.fill, m["fill"]) and np.array_equal(f.G, m["G"])
    # the Python driver: the same candidates as the native pipeline
    py_out = str(tmp_path / "py.txt")
    r = subprocess.run([sys.executable, "-m", "peasoup_amd", "sps", "-i", fil, "-o", py_out] + E2E_FLAGS +
                       ["--rfi", "--zero_dm"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    body = lambda p: [ln for ln in open(p) if not ln.startswith("#")]  # noqa: E731
    assert body(py_out) == body(str(tmp_path / "clean.txt"))
    assert [ln for ln in open(py_out) if ln.startswith("# rfi:")] == \
        [ln for ln in open(str(tmp_path / "clean.txt")) if ln.startswith("# rfi:")]


# -------------------------------------------------------------- flags off ---
GOLDEN_FLAGS_OFF = os.path.join(REPO, "tests", "golden", "spsearch_flags_off.output")
FLAGS_OFF_CMD = ["-i", "tests/data/tutorial.fil", "--dm_start", "0", "--dm_end", "60", "-t", "1", "--min_snr", "7"]


def _without_timers(text):
    """The output but for the two wall-clock figures of its third header line."""
    import re

    return re.sub(r"  searching: \S+ s  total: \S+ s", "", text)


def test_flags_off_output_equals_the_parent(tmp_path):
    """Without --rfi the spsearch output is the parent's, byte for byte, but
    for the two wall-clock figures in the header (they differ from run to run
    of one binary).  The golden copy was written by the parent commit's
    bin/spsearch with FLAGS_OFF_CMD from the repository root."""
    out = str(tmp_path / "off.output")
    r = subprocess.run([os.path.join(REPO, "bin", "spsearch")] + FLAGS_OFF_CMD + ["-o", out], capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    got, want = open(out).read(), open(GOLDEN_FLAGS_OFF).read()
    assert "searching:" in got and _without_timers(got) == _without_timers(want)
    assert len(got.splitlines()) > 5  # candidates, not only a header
