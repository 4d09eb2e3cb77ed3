"""bench.py's launcher contract (no GPU needed): --gpus N starts N ranks
itself when no launcher did, and refuses a launcher whose WORLD_SIZE is not N
before anything touches a GPU."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stderr
    assert p.stdout == ""


def test_launcher_command_runs_n_ranks_of_this_script():
    cmd = bench.launcher_cmd(8, ["--gpus", "8", "--steps", "3"], port=29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29555" in cmd
    i = cmd.index(os.path.join(REPO, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "3"]


def test_self_launch_only_without_a_launcher(monkeypatch):
    calls = []
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd: calls.append(cmd) or 7)
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    class A:
        gpus = 4
    assert bench.launch_or_check(A, ["--gpus", "4"]) == 7            # the child's exit code
    assert len(calls) == 1 and "--nproc-per-node=4" in calls[0]
    A.gpus = 1
    assert bench.launch_or_check(A, ["--gpus", "1"]) is None         # one GPU: run here
    monkeypatch.setenv("WORLD_SIZE", "4")
    A.gpus = 4
    assert bench.launch_or_check(A, ["--gpus", "4"]) is None         # under torch.distributed.run
    assert len(calls) == 1


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_measures_only_the_timed_steps(monkeypatch):
    """Without --full the legs after the timed region are off; with it they
    keep their own switches."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    assert a.no_queries and not a.e2e and a.cpu_sample == 0
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert not a.no_queries and a.e2e and a.cpu_sample == 25_000
    a = _parse(monkeypatch, "--full", "--no-queries", "--no-e2e", "--cpu-sample", "0")
    assert a.no_queries and not a.e2e and a.cpu_sample == 0


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_holds_only_float_arrays_within_the_size_limit(tmp_path):
    import numpy as np
    bench.write_dump(str(tmp_path / "d"), {"a": np.arange(3, dtype=np.float64), "b": np.ones(2, np.float32)}, "p_")
    assert sorted(os.listdir(tmp_path / "d")) == ["p_a.npy", "p_b.npy"]
    assert np.load(tmp_path / "d" / "p_a.npy").tolist() == [0.0, 1.0, 2.0]
    with pytest.raises(AssertionError):
        bench.write_dump(str(tmp_path / "e"), {"a": np.arange(3)})
    with pytest.raises(AssertionError):
        bench.write_dump(str(tmp_path / "e"), {"a": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()
