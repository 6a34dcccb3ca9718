"""Which instances a vertex range touches and which a refit must re-derive (csrc/vertex_dirty.h,
the host side of ark_ddgi_update_geometry) as a stand-alone program (tests/cpp/vertex_dirty_test.cpp:
a table of disjoint, abutting and overlapping spans, shared meshes, empty ranges and ranges
past the pool; the version bookkeeping over a simulated chain of refits and one install)
built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program, as
test_lbvh_plan_sanitizers.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vertex_dirty_under_sanitizers(tmp_path):
    exe = str(tmp_path / "vertex_dirty_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "arkoserenderer_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "vertex_dirty_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
