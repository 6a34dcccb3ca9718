"""The host restatement of the reflection denoiser passes (csrc/refl_denoise.h,
refl_denoise_host.cpp) as a stand-alone program (tests/cpp/refl_denoise_test.cpp: 1 x 1,
1 x 97, 8 x 8, 9 x 7 and 29 x 19 images, a first frame and two more, reprojection UVs far
outside [0, 1], all-sky planes, inf and NaN radiance, guard words around every plane, the
refusals) built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a
program, as test_rt_shadows_sanitizers.py does. It also prints the measured error of exp and
pow(x, 512) against glibc. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refl_denoise_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "refl_denoise_test")
    csrc = os.path.join(ROOT, "arkoserenderer_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "refl_denoise_test.cpp"), os.path.join(csrc, "refl_denoise_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
    assert "exp on [-20, 0]: max error" in r.stdout and "pow(x, 512) on [0.9, 1]: max error" in r.stdout
