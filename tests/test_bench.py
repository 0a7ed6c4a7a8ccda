"""bench.py's command line: --steps sets the timed steps, ms_per_step is in
the result line, --dump-outputs writes the last timed step's candidates as
float64 arrays (the same from run to run for the same arguments), --full is
accepted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO  # (puts the repository root on sys.path)

import bench


def _tree(C):
    a = C.Candidate(1.5, 2, -3.0, 4, 55.5, 3.25)
    b = C.Candidate(2.5, 3, 1.0, 1, 22.0, 6.5)
    b.assoc = [C.Candidate(3.5, 4, 0.0, 0, 11.0, 13.0)]
    a.assoc = [b]
    a.is_physical = True
    a.ddm_snr_ratio = 0.75
    return [a, C.Candidate(9.0, 7, 2.0, 0, 10.0, 50.0)]


def test_dump_outputs_layout(C, tmp_path):
    rows = bench.dump_outputs(str(tmp_path), C.CandidateBag(_tree(C)), seed=1)
    assert rows == {"candidates": 2, "candidate_members": 4}
    top = np.load(tmp_path / "candidates.npy")
    mem = np.load(tmp_path / "candidate_members.npy")
    assert top.dtype == np.float64 and mem.dtype == np.float64
    col = {k: i for i, k in enumerate(bench.CANDIDATE_COLUMNS)}
    assert top.shape == (2, len(col)) and mem.shape == (4, len(bench.MEMBER_COLUMNS))
    assert top[0, col["snr"]] == 55.5 and top[0, col["nassoc"]] == 2 and top[1, col["nassoc"]] == 0
    assert top[0, col["is_physical"]] == 1.0 and top[0, col["ddm_snr_ratio"]] == 0.75
    # members: the candidate itself, then its tree depth first
    assert mem[:, 0].tolist() == [0, 0, 0, 1]
    assert mem[:, bench.MEMBER_COLUMNS.index("freq")].tolist() == [3.25, 6.5, 13.0, 50.0]


def test_dump_outputs_empty_and_sampled(C, tmp_path, monkeypatch):
    assert bench.dump_outputs(str(tmp_path / "e"), C.CandidateBag(), seed=1) == {"candidates": 0,
                                                                                  "candidate_members": 0}
    assert np.load(tmp_path / "e" / "candidates.npy").shape == (0, len(bench.CANDIDATE_COLUMNS))
    assert np.load(tmp_path / "e" / "candidate_members.npy").shape == (0, len(bench.MEMBER_COLUMNS))
    # over the size limit: a seeded sample of the rows, in order, within the limit
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * (4096 + 8 * len(bench.CANDIDATE_COLUMNS) * 10))
    cands = [C.Candidate(1.0, i, 0.0, 0, 10.0 + i, 1.0 + i) for i in range(100)]
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), C.CandidateBag(cands), seed=7)["candidates"] == 100
    top = np.load(tmp_path / "a" / "candidates.npy")
    assert top.shape[0] == 10 and np.all(np.diff(top[:, 1]) > 0)
    for name in ("candidates.npy", "candidate_members.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES


# a short series with injected pulsars, so that the dumped list is not empty
SMALL = ["--gpus", "1", "--log2n", "20", "--signal"]


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + SMALL + extra, capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return d, _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d / "a")])


@pytest.mark.gpu
def test_bench_result_line_and_dump(dumped):
    d, res = dumped
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "trials/s" and res["higher_is_better"] is True and res["dtype"] == "fp32"
    # value and ms_per_step describe the same three timed steps
    assert res["value"] == pytest.approx(res["config"]["global_batch"] / (1e-3 * res["ms_per_step"]), rel=1e-3)
    assert res["config"]["full"] is False
    top = np.load(d / "a" / "candidates.npy")
    mem = np.load(d / "a" / "candidate_members.npy")
    assert top.dtype == np.float64 and mem.dtype == np.float64
    n = res["config"]["candidates_after_distill"]
    assert n > 0 and res["config"]["outputs_dumped"] == {"candidates": n, "candidate_members": len(mem)}
    assert top.shape == (n, len(bench.CANDIDATE_COLUMNS))
    col = {k: i for i, k in enumerate(bench.CANDIDATE_COLUMNS)}
    assert len(mem) == n + int(top[:, col["nassoc"]].sum())
    assert np.all(np.isfinite(top)) and np.all(top[:, col["snr"]] >= 9.0) and np.all(top[:, col["freq"]] > 0)
    assert top.nbytes + mem.nbytes <= bench.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_bench_dump_repeats_and_full_is_accepted(dumped):
    """The same arguments (other than the number of steps and --full, which
    change no input) give the same dumped arrays in a new process."""
    d, _ = dumped
    res = _bench(["--steps", "1", "--warmup", "0", "--full", "--dump-outputs", str(d / "b")])
    assert res["steps"] == 1 and res["warmup"] == 0 and res["config"]["full"] is True
    for name in ("candidates.npy", "candidate_members.npy"):
        assert np.array_equal(np.load(d / "a" / name), np.load(d / "b" / name)), name
