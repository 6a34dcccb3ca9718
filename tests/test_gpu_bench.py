"""bench.py's plain run and its --dump-outputs on a small workload (64,000 triangles,
8^3 probes x 64 rays), in this process: the result line's fields, exactly --steps timed
steps, no side lines without --full, and dumps that repeat bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--triangles", "64000", "--grid", "8", "--rays", "64", "--steps", "3", "--warmup", "1"]
NAMES = [n for n, _ in bench.DUMP_RESOURCES]
FULL_ONLY = ("roofline", "kernels_ms", "update_ms", "per_ray", "reference_windows", "c2", "c5", "c3", "cpu_baseline", "ao_bake",
             "lighting_compose", "rt_reflections")


def _run(capsys, *extra):
    assert bench.main(SMALL + list(extra)) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_line_and_repeatable_dump(capsys, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 50_000)  # the atlases and surfels of this grid take the sampled path
    j = _run(capsys, "--dump-outputs", str(tmp_path / "a"))
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1
    assert j["unit"] == "Mrays/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0
    # value and ms_per_step describe the same three steps of 512 probes x 64 rays
    assert j["value"] == pytest.approx(512 * 64 / j["ms_per_step"] / 1e3, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in j]
    _run(capsys, "--dump-outputs", str(tmp_path / "b"))
    for name in NAMES:
        a = np.load(tmp_path / "a" / f"{name}.npy")
        b = np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and 0 < a.size <= 50_000
        assert np.isfinite(a).all(), name  # non-finite fp16 values are written as finite codes
        assert np.array_equal(a, b), name
        assert np.any(a != 0), name
    # the offsets (512 probes x 4 floats) are whole; the fp16 resources are sampled
    assert np.load(tmp_path / "a" / "probe_offsets.npy").size == 512 * 4
    assert np.load(tmp_path / "a" / "surfels.npy").size == 50_000


def test_steps_sets_the_frames_run(capsys, tmp_path):
    """One more timed step is one more update: the dumps of 3 and of 4 steps differ."""
    _run(capsys, "--dump-outputs", str(tmp_path / "s3"))
    assert bench.main(SMALL[:-4] + ["--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "s4")]) == 0
    capsys.readouterr()
    a = np.load(tmp_path / "s3" / "surfels.npy")
    b = np.load(tmp_path / "s4" / "surfels.npy")
    assert a.shape == b.shape and not np.array_equal(a, b)
