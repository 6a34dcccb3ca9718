"""bench.py's launch decision (VERDICT r05 "do this" #1): `--gpus N` either runs as
one rank of an N-rank job, starts the N ranks itself (torch.distributed.run as a child
process), or refuses; a 1-GPU line is never printed for an N-GPU request. CPU only:
the decision is made before any GPU call."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_single_gpu_runs_in_process():
    assert bench.launch_decision(1, {}, 0, []) == ("run", 1)


def test_rank_of_driver_job_runs_with_its_world():
    env = {"WORLD_SIZE": "8", "RANK": "3", "LOCAL_RANK": "3"}
    assert bench.launch_decision(8, env, 8, ["--gpus", "8"]) == ("run", 8)


def test_world_size_disagreeing_with_gpus_is_refused():
    kind, why = bench.launch_decision(2, {"WORLD_SIZE": "4"}, 8, ["--gpus", "2"])
    assert kind == "error" and "WORLD_SIZE=4" in why
    kind, _ = bench.launch_decision(1, {"WORLD_SIZE": "2"}, 8, [])
    assert kind == "error"


def test_more_gpus_than_visible_is_refused():
    kind, why = bench.launch_decision(2, {}, 1, ["--gpus", "2"])
    assert kind == "error" and "1 GPU(s) visible" in why


def test_n_gpus_spawns_torchrun_child_with_same_arguments():
    argv = ["--gpus", "4", "--steps", "7", "--warmup", "2"]
    kind, cmd = bench.launch_decision(4, {}, 8, argv, master_port=29555)
    assert kind == "spawn"
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd and "--master-port=29555" in cmd
    script = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[script + 1:] == argv  # each rank sees WORLD_SIZE = 4 = --gpus: ("run", 4)


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_of_oversized_resources_stays_within_64_mb(tmp_path):
    """--dump-outputs at the real cap with every resource above it (a grid of more than
    1 M probes): the files together are at most 64 MB; a sample is distinct, ordered
    elements, the same on every call; fp16 NaN / inf become the finite codes."""
    import numpy as np

    assert bench.DUMP_BUDGET_BYTES == 64_000_000 and len(bench.DUMP_RESOURCES) == 4
    n = bench.DUMP_MAX_ELEMENTS + 100_001
    ramp = np.arange(n, dtype=np.float32)  # exact: n < 2^24
    bits = np.zeros(n, np.uint16)
    bits[0::3], bits[1::3], bits[2::3] = 0x3C00, 0x7E00, 0xFC00  # 1, NaN, -inf
    for name, _ in bench.DUMP_RESOURCES:
        bench.dump_array(str(tmp_path / f"{name}.npy"), ramp if name == "probe_offsets" else bits)
    assert sum(os.path.getsize(tmp_path / f"{name}.npy") for name, _ in bench.DUMP_RESOURCES) <= 64_000_000
    a = np.load(tmp_path / "probe_offsets.npy")
    assert a.dtype == np.float32 and a.size == bench.DUMP_MAX_ELEMENTS
    assert np.all(np.diff(a) > 0) and a[-1] < n  # distinct elements of the input, in order
    bench.dump_array(str(tmp_path / "again.npy"), ramp)
    assert np.array_equal(np.load(tmp_path / "again.npy"), a)
    h = np.load(tmp_path / "surfels.npy")
    assert h.dtype == np.float32 and set(np.unique(h)) == {1.0, bench.DUMP_NAN, -bench.DUMP_INF}
    want = np.array([1.0, bench.DUMP_NAN, -bench.DUMP_INF], np.float32)[a.astype(np.int64) % 3]
    assert np.array_equal(h, want)  # the same indices for the same length


def test_dump_keeps_small_resources_whole(tmp_path):
    import numpy as np

    x = np.array([0x0000, 0x3C00, 0x7C00, 0x7E00, 0xC000], np.uint16)  # 0, 1, +inf, NaN, -2
    bench.dump_array(str(tmp_path / "x.npy"), x)
    assert np.array_equal(np.load(tmp_path / "x.npy"), np.array([0.0, 1.0, bench.DUMP_INF, bench.DUMP_NAN, -2.0], np.float32))


def _dry(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--dry-run"], capture_output=True, text=True, env=e, timeout=300)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1])


def test_dry_run_reports_world_size():
    rc, d = _dry()
    assert rc == 0 and d["decision"] == "run" and d["world_size"] == 1
    rc, d = _dry("--gpus", "2", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert rc == 0 and d["decision"] == "run" and d["world_size"] == 2


def test_dry_run_without_gpus_fails_nonzero():
    # this container has no GPU: a 2-GPU request must fail, not print a 1-GPU line
    rc, d = _dry("--gpus", "2", env={"HIP_VISIBLE_DEVICES": ""})
    assert rc != 0 and d["decision"] == "error" and d["world_size"] is None
