"""RFI excision, CPU side (csrc/include/psoup/rfi.hpp): the NumPy oracle on
hand-made tables (the MAD = 0 rule, the even-count median, promotion order, a
dead channel, killed channels outside the shares, a short last block), the
native rfi_flag against the oracle flag for flag, option parsing, the mask file
(Python writer, Python reader, native writer and reader) and the native unit
tests."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from peasoup_amd import _C as C
from peasoup_amd.utils import reference as ref
from peasoup_amd.utils.outputs import RfiMaskFile, write_rfi_mask

L = 256


def _table(nchans, nsamps, block=L, mean=2, var=1):
    """Block sums of channels whose every block has this mean and variance."""
    lens = ref.rfi_block_lengths(nsamps, block)
    S1 = np.tile(mean * lens, (nchans, 1)).astype(np.int64)
    S2 = np.tile(lens * (var + mean * mean), (nchans, 1)).astype(np.int64)
    return S1, S2, lens


def _set(S1, S2, lens, c, b, mean, var):
    S1[c, b] = mean * lens[b]
    S2[c, b] = lens[b] * (var + mean * mean)


def _native(S1, S2, nsamps, block, kill, thresh=5.0, chan_frac=0.3, block_frac=0.3):
    p = C.RfiParams(block, thresh, chan_frac, block_frac, False)
    return C.rfi_flag(S1.astype(np.uint64), S2.astype(np.uint64), nsamps, [] if kill is None else list(kill), p)


def _same(mask, m):
    for k in ("chan_flag", "block_flag", "cell", "fill", "G", "nb"):
        assert np.array_equal(np.asarray(getattr(mask, k)), m[k]), k
    assert list(mask.killmask) == m["killmask"]


def test_rdiv():
    assert [ref.rfi_rdiv(a, n) for a, n in [(0, 3), (1, 2), (1, 3), (2, 3), (7, 2), (10, 4), (9, 4)]] == \
        [0, 1, 0, 1, 4, 3, 2]
    rng = np.random.default_rng(1)
    for a, n in zip(rng.integers(0, 1 << 40, 200), rng.integers(1, 1 << 24, 200)):
        a, n = int(a), int(n)
        assert C.rfi_rdiv(a, n) == ref.rfi_rdiv(a, n) == (2 * a + n) // (2 * n)


def test_mad_zero_rule_and_short_last_block():
    nsamps = 5 * L + 100  # the last block is 100 samples long
    S1, S2, lens = _table(3, nsamps)
    assert lens.tolist() == [L] * 5 + [100]
    _set(S1, S2, lens, 1, 2, 3, 1)   # another mean, same variance
    _set(S1, S2, lens, 2, 5, 2, 2)   # another variance in the short block
    m = ref.rfi_flag(S1, S2, nsamps, L, None, 5.0, 0.5, 0.5)
    want = np.zeros((3, 6), dtype=np.uint8)
    want[1, 2] = want[2, 5] = 1      # MAD is 0 in both statistics: any difference flags, nothing else does
    assert np.array_equal(m["cell"], want)
    assert not m["chan_flag"].any() and not m["block_flag"].any() and m["killmask"] == [1, 1, 1]
    assert m["fill"].tolist() == [2, 2, 2] and m["G"].tolist() == [2] * 6 and m["nb"].tolist() == [3, 3, 2, 3, 3, 2]
    _same(_native(S1, S2, nsamps, L, None, 5.0, 0.5, 0.5), m)


def test_even_count_median():
    # means 1, 2, 3, 10: the median is 2.5 and the MAD 1, so the last block is
    # 7.5 MADs out; a lower-middle median would make it 8
    nsamps = 4 * L
    S1, S2, lens = _table(1, nsamps)
    for b, mean in enumerate([1, 2, 3, 10]):
        _set(S1, S2, lens, 0, b, mean, 1)
    out = ref.rfi_flag(S1, S2, nsamps, L, None, 5.2, 0.9, 0.9)  # 5.2 * 1.4826 = 7.71
    assert out["cell"].tolist() == [[0, 0, 0, 0]]
    _same(_native(S1, S2, nsamps, L, None, 5.2, 0.9, 0.9), out)
    out = ref.rfi_flag(S1, S2, nsamps, L, None, 5.0, 0.9, 0.9)  # 5.0 * 1.4826 = 7.41
    assert out["cell"].tolist() == [[0, 0, 0, 1]]
    assert out["fill"].tolist() == [2]
    _same(_native(S1, S2, nsamps, L, None, 5.0, 0.9, 0.9), out)


def test_promotion_uses_the_flags_before_any_promotion():
    nsamps = 10 * L
    S1, S2, lens = _table(4, nsamps)
    for b in range(4):
        _set(S1, S2, lens, 0, b, 5, 1)  # 4 of 10 cells of channel 0: promoted whole at 0.3
    _set(S1, S2, lens, 1, 9, 5, 1)      # block 9: 1 of 4 channels, below 0.3
    m = ref.rfi_flag(S1, S2, nsamps, L, None, 5.0, 0.3, 0.3)
    assert m["chan_flag"].tolist() == [1, 0, 0, 0]
    # channel 0's promotion does not count towards block 9 (that would be 2 of 4)
    assert m["block_flag"].tolist() == [0] * 10
    assert m["cell"][0].all() and m["cell"][1].tolist() == [0] * 9 + [1] and not m["cell"][2:].any()
    assert m["killmask"] == [0, 1, 1, 1] and m["fill"].tolist() == [0, 2, 2, 2]
    assert m["nb"].tolist() == [3] * 9 + [2]
    _same(_native(S1, S2, nsamps, L, None), m)
    # and a block's promotion does not count towards a channel: blocks 0..2 have 2 of 4 flagged
    S1, S2, lens = _table(4, nsamps)
    for b in range(3):
        _set(S1, S2, lens, 0, b, 5, 1)
        _set(S1, S2, lens, 1, b, 5, 1)
    m = ref.rfi_flag(S1, S2, nsamps, L, None, 5.0, 0.3, 0.3)
    assert m["block_flag"].tolist() == [1, 1, 1] + [0] * 7 and not m["chan_flag"].any()  # 3 of 10 is not above 0.3
    assert m["cell"][:, :3].all() and not m["cell"][:, 3:].any() and m["nb"].tolist() == [0, 0, 0] + [4] * 7
    assert m["G"].tolist() == [0, 0, 0] + [2] * 7
    _same(_native(S1, S2, nsamps, L, None), m)


def test_dead_and_killed_channels():
    nsamps = 5 * L + 100
    S1, S2, lens = _table(4, nsamps)
    _set(S1, S2, lens, 1, 2, 3, 1)
    S1[3], S2[3] = 2 * lens, 4 * lens   # constant 2: variance 0, dead
    kill = [1, 1, 0, 1]
    m = ref.rfi_flag(S1, S2, nsamps, L, kill, 5.0, 0.5, 0.5)
    assert m["chan_flag"].tolist() == [0, 0, 1, 1] and m["killmask"] == [1, 1, 0, 0]
    # block 2: channels 1 and 3 of the 3 live ones -> promoted; with the killed
    # channel in the share it would be 3 of 4 everywhere else (1 of 3 is right)
    assert m["block_flag"].tolist() == [0, 0, 1, 0, 0, 0]
    assert m["cell"][2].all() and m["cell"][3].all() and m["cell"][0].tolist() == [0, 0, 1, 0, 0, 0]
    assert m["fill"].tolist() == [2, 2, 0, 0] and m["nb"].tolist() == [2, 2, 0, 2, 2, 2]
    _same(_native(S1, S2, nsamps, L, kill, 5.0, 0.5, 0.5), m)
    # every channel killed: nothing live, no block promotion, everything flagged
    m = ref.rfi_flag(S1, S2, nsamps, L, [0, 0, 0, 0])
    assert m["cell"].all() and not m["block_flag"].any() and m["killmask"] == [0] * 4
    _same(_native(S1, S2, nsamps, L, [0, 0, 0, 0]), m)


@pytest.mark.parametrize("seed,nbits,block,nsamps", [(0, 8, 256, 5000), (1, 2, 256, 4096), (2, 8, 512, 7001),
                                                     (3, 4, 1024, 9000)])
def test_native_flag_equals_oracle_on_random_sums(seed, nbits, block, nsamps):
    rng = np.random.default_rng(seed)
    V = (1 << nbits) - 1
    x = np.clip(np.rint(rng.normal(V / 2, max(V / 5, 0.6), (12, nsamps))), 0, V).astype(np.int64)
    x[2] = np.clip(x[2] + rng.integers(-2, 3, nsamps) * (V // 3 + 1), 0, V)   # noisy channel
    x[:, 3 * block:5 * block] = np.minimum(x[:, 3 * block:5 * block] + V // 4 + 1, V)  # broadband blocks
    x[5, block:2 * block] = V                                                   # a bad cell
    x[7] = 0                                                                    # dead
    kill = [1] * 12
    kill[9] = 0
    S1, S2 = ref.rfi_block_sums(x, block)
    for thresh, cf, bf in [(5.0, 0.3, 0.3), (3.0, 0.1, 0.5), (8.0, 0.9, 0.05)]:
        m = ref.rfi_flag(S1, S2, nsamps, block, kill, thresh, cf, bf)
        _same(_native(S1.astype(np.int64), S2.astype(np.int64), nsamps, block, kill, thresh, cf, bf), m)
    assert m["cell"][7].all() and m["cell"][9].all() and m["killmask"][7] == 0 and m["killmask"][9] == 0


def test_oracle_apply_identities():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (8, 3 * L + 10))
    y, m = ref.rfi_clean(x, L, 2, thresh=1e9)  # nothing flagged
    assert not m["cell"].any() and np.array_equal(y, x)
    y, m = ref.rfi_clean(x, L, 2, thresh=1e9, zero_dm=True)
    assert y.min() >= 0 and y.max() <= 3
    Z = x.sum(axis=0)
    zbar = (2 * Z + 8) // 16
    assert np.array_equal(y, np.clip(x - zbar[None, :] + np.repeat(m["G"], L)[None, :x.shape[1]], 0, 3))


def test_rfi_cmdline_defaults_and_flags():
    ok, exit_now, a = C.parse_rfi_cmdline(["rficlean", "-i", "x.fil"])
    assert ok and not exit_now and a.infilename == "x.fil"
    assert (a.rfi_block, a.rfi_thresh, a.rfi_chan_frac, a.rfi_block_frac) == (4096, 5.0, 0.3, 0.3)
    assert not a.zero_dm and not a.verbose
    assert a.outfilename == a.killfilename == a.maskfilename == a.killoutfilename == ""
    ok, _, a = C.parse_rfi_cmdline(["rficlean", "-i", "x.fil", "-o", "y.fil", "-k", "k.txt", "--mask_out", "m.mask",
                                    "--kill_out", "ko.txt", "--rfi_block", "1024", "--rfi_thresh", "4.5",
                                    "--rfi_chan_frac", "0.2", "--rfi_block_frac", "0.4", "--zero_dm", "-v"])
    assert ok and (a.outfilename, a.killfilename, a.maskfilename, a.killoutfilename) == \
        ("y.fil", "k.txt", "m.mask", "ko.txt")
    assert (a.rfi_block, a.rfi_thresh, a.rfi_chan_frac, a.rfi_block_frac) == (1024, 4.5, 0.2, 0.4)
    assert a.zero_dm and a.verbose
    p = C.rfi_params_from(a)
    assert (p.block, p.thresh, p.chan_frac, p.block_frac, p.zero_dm) == (1024, 4.5, 0.2, 0.4, True)
    ok, exit_now, _ = C.parse_rfi_cmdline(["rficlean", "-h"])
    assert ok and exit_now
    assert not C.parse_rfi_cmdline(["rficlean"])[0]  # -i is required
    for bad in (["--rfi_block", "1000"], ["--rfi_block", "128"], ["--rfi_block", "131072"], ["--rfi_thresh", "-1"]):
        assert not C.parse_rfi_cmdline(["rficlean", "-i", "x.fil"] + bad)[0]
    assert C.rfi_tile() == 256 and all(b % C.rfi_tile() == 0 for b in range(256, 65537, 256))


def test_mask_file_python_and_native(tmp_path):
    nsamps = 5 * L + 100
    S1, S2, lens = _table(4, nsamps)
    _set(S1, S2, lens, 1, 2, 3, 1)
    S1[3], S2[3] = 2 * lens, 4 * lens
    m = ref.rfi_flag(S1, S2, nsamps, L, [1, 1, 0, 1], 5.0, 0.5, 0.5)
    hdr = {"nbits": 2, "zero_dm": True, "nsamps": nsamps, "block": L, "tsamp": 64e-6, "thresh": 5.0,
           "chan_frac": 0.5, "block_frac": 0.5}
    py_path, nat_path = str(tmp_path / "py.mask"), str(tmp_path / "native.mask")
    write_rfi_mask(py_path, hdr, m)
    f = RfiMaskFile(py_path)
    assert f.header == dict(hdr, nchans=4, nblk=6, zero_dm=1)
    for k in ("chan_flag", "block_flag", "cell", "fill", "G"):
        assert np.array_equal(getattr(f, k), m[k]) and getattr(f, k).dtype == m[k].dtype
    assert f.killmask == m["killmask"]
    raw = open(py_path, "rb").read()
    assert raw[:8] == b"PSMASK01" and len(raw) == 8 + 16 + 16 + 32 + 4 + 6 + 24 + 16 + 24
    assert np.frombuffer(raw, "<u4", 4, 8).tolist() == [4, 6, 2, 1]
    assert np.frombuffer(raw, "<u8", 2, 24).tolist() == [nsamps, L]
    assert np.frombuffer(raw, "<f8", 4, 40).tolist() == [64e-6, 5.0, 0.5, 0.5]
    # the native writer gives the same bytes, the native reader the same mask
    p = C.RfiParams(L, 5.0, 0.5, 0.5, True)
    nat = _native(S1, S2, nsamps, L, [1, 1, 0, 1], 5.0, 0.5, 0.5)
    C.write_rfi_mask(nat_path, nat, p, C.RfiMaskHeader(2, 64e-6))
    assert open(nat_path, "rb").read() == raw and not os.path.exists(nat_path + ".tmp")
    back, p2, h2 = C.read_rfi_mask(py_path)
    _same(back, m)
    assert (p2.block, p2.thresh, p2.chan_frac, p2.block_frac, p2.zero_dm, h2.nbits, h2.tsamp) == \
        (L, 5.0, 0.5, 0.5, True, 2, 64e-6)
    with pytest.raises(ValueError):
        open(str(tmp_path / "bad.mask"), "wb").write(raw[:-1])
        RfiMaskFile(str(tmp_path / "bad.mask"))
    kpath = str(tmp_path / "kill.txt")
    C.write_killfile(kpath, m["killmask"])
    assert open(kpath).read() == "1\n1\n0\n0\n"
    assert C.read_killfile(kpath, 4) == (m["killmask"], True)


def test_native_unit_tests(tmp_path):
    exe = os.path.join(REPO, "bin", "psoup_rfi_unit_tests")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_sp_cmdline_rfi_flags():
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", "x.fil"])
    assert ok and not a.rfi and not a.zero_dm and a.rfi_maskfilename == ""
    assert (a.rfi_block, a.rfi_thresh, a.rfi_chan_frac, a.rfi_block_frac) == (4096, 5.0, 0.3, 0.3)
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", "x.fil", "--rfi"])
    assert ok and a.rfi and not a.zero_dm
    ok, _, a = C.parse_sp_cmdline(["spsearch", "-i", "x.fil", "--zero_dm", "--rfi_block", "512", "--rfi_thresh", "4",
                                   "--rfi_chan_frac", "0.25", "--rfi_block_frac", "0.5", "--rfi_mask_out", "m.mask"])
    assert ok and a.rfi and a.zero_dm and a.rfi_maskfilename == "m.mask"  # --zero_dm implies --rfi
    p = C.sp_rfi_params(a)
    assert (p.block, p.thresh, p.chan_frac, p.block_frac, p.zero_dm) == (512, 4.0, 0.25, 0.5, True)
    assert not C.parse_sp_cmdline(["spsearch", "-i", "x.fil", "--rfi", "--rfi_block", "1000"])[0]
    res = C.SpResult()
    assert res.rfi_comment == ""


def test_synthetic_rfi_injection():
    from peasoup_amd.utils import synthetic

    hdr = synthetic.make_header(nchans=16, nbits=8, tsamp=1e-3)
    base = synthetic.generate(4096, hdr, [], seed=3)
    assert np.array_equal(synthetic.generate(4096, hdr, [], seed=3, rfi=()), base)  # existing arguments: same output
    imp = synthetic.RfiSpec("impulse", time=1.0, duration=4e-3, amplitude=1.0)
    cell = synthetic.RfiSpec("cell", channel=5, time=2.0, duration=0.1, amplitude=1.0)
    chan = synthetic.RfiSpec("channel", channel=9, amplitude=2.0)
    v = synthetic.generate(4096, hdr, [], seed=3, rfi=[imp, cell, chan], chunk=1000).astype(np.int64)
    d = v - base
    touched = np.zeros(d.shape, dtype=bool)
    touched[1000:1004, :] = True
    touched[2000:2100, 5] = True
    touched[:, 9] = True
    assert not d[~touched].any()
    sigma = 255 / 4.0
    unclipped = (base[1000:1004] > 0) & (v[1000:1004] < 255)
    unclipped[:, 9] = False
    assert np.abs(d[1000:1004][unclipped] - sigma).max() <= 1 and (d[2000:2100, 5] >= 0).all() and d[2000:2100, 5].max() >= 63
    assert v[:, 9].std() > 1.5 * base[:, 9].std()
    # write and packed take the same keyword
    assert np.array_equal(synthetic.packed(512, hdr, [], seed=3, rfi=[imp]),
                          synthetic.pack_samples(synthetic.generate(512, hdr, [], seed=3, rfi=[imp]), 8))
    with pytest.raises(ValueError):
        synthetic.generate(64, hdr, [], seed=3, rfi=[synthetic.RfiSpec("comb")])
