"""The serial restatement of the SAH pass of the device BVH builds (ARK_DDGI_FLAG_GPU_REBUILD_SAH)
as a stand-alone program (tests/cpp/lbvh_sah_test.cpp: 257 and 4,099 triangles, coincident
triangles; the world and the light-space build) built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program, as test_sun_rebuild_policy.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [
    os.path.join(ROOT, "tests", "cpp", "lbvh_sah_test.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_builder.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "sun_bvh.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "lbvh_host.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh8_check.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_debug.cpp"),
]


def test_sah_pass_restatement_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lbvh_sah_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "arkoserenderer_amd", "csrc")] + SOURCES + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("OK")
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr
