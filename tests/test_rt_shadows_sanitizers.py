"""The host restatement of the ray-traced local-light shadow masks (csrc/rt_shadows.h,
rt_shadows_host.cpp) as a stand-alone program (tests/cpp/rt_shadows_test.cpp: random depth
planes, 1 x 1 and 1 x 97 images, 16 lights, a light at a shading point - the NaN rule -, an
all-sky plane, hole records, the refusals) built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program, as test_skin_bounds_sanitizers.py does.
CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rt_shadows_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rt_shadows_test")
    csrc = os.path.join(ROOT, "arkoserenderer_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "rt_shadows_test.cpp"), os.path.join(csrc, "rt_shadows_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
