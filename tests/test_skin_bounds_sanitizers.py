"""The host side of skinning (csrc/skinning_host.cpp: registration's checks, the restatement of
k_skin_vertices, the pose bound the refit is given) as a stand-alone program
(tests/cpp/skin_bounds_test.cpp: for random and adversarial poses - translations of 1e4,
scales of 1e-3 and 1e3, weight sums of 0.9 and 1.1, negative morph weights, a vertex on one
joint only, a joint no vertex uses - the bound contains every restated position; every
refusal returns its error and leaves the registry as it was) built with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and run as a program, as
test_copy_book_sanitizers.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skin_bounds_under_sanitizers(tmp_path):
    exe = str(tmp_path / "skin_bounds_test")
    csrc = os.path.join(ROOT, "arkoserenderer_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "skin_bounds_test.cpp"), os.path.join(csrc, "skinning_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
