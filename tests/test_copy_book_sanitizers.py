"""The record of what a scene's three geometry copies hold (csrc/copy_book.h: transforms,
inflations, vertex versions, validity, the rotation's order, "the next refit reaches every
node") as a stand-alone program (tests/cpp/copy_book_test.cpp: the store's lifecycle events
driven against a model of the device state - the sequences of test_gpu_refit_sequences.py,
mixed pose and vertex updates, a failed refit, a failed vertex staging, installs with and
without a forward refit, a new scene - with the dirty counts asserted) built with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and run as a program, as
test_vertex_dirty_sanitizers.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_copy_book_under_sanitizers(tmp_path):
    exe = str(tmp_path / "copy_book_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "arkoserenderer_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "copy_book_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
