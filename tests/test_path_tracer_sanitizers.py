"""The host restatement of the path tracer (csrc/path_tracer.h, path_tracer_host.cpp) as a
stand-alone program (tests/cpp/path_tracer_test.cpp: 1 x 1 and 1 x 97 images, hole records, a
spot light on a shading point - the NaN length -, zero lights, accumulate and reset, the
refusals) built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a
program, as test_rt_shadows_sanitizers.py does. CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_path_tracer_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "path_tracer_test")
    csrc = os.path.join(ROOT, "arkoserenderer_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "path_tracer_test.cpp"), os.path.join(csrc, "path_tracer_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
