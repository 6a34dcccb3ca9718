"""The record of a context's frames in flight (csrc/frame_book.h: which stream each part of an
update runs on and what it waits for), as a stand-alone program (tests/cpp/frame_book_test.cpp):
against the rule it replaced, against a model of the two queues, and as named cases. Built with
g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program, as
test_shade_schedule.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "frame_book_test.cpp")]


def test_frame_book_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_book_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "arkoserenderer_amd", "csrc")] + SOURCES + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "table: OK" in r.stdout and "serial sweep: OK" in r.stdout and r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
