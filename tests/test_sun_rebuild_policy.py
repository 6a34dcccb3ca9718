"""The rebuild policy with ARK_DDGI_FLAG_GPU_REBUILD_SUN (csrc/scene_rebuild_policy.h) and the
serial restatement of the device build of the sun's light-space BVH8, as a stand-alone
program (tests/cpp/sun_policy_test.cpp) built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program, as test_sanitizers.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [
    os.path.join(ROOT, "tests", "cpp", "sun_policy_test.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_builder.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "sun_bvh.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "lbvh_host.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh8_check.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_debug.cpp"),
]


def test_sun_policy_and_lbvh_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sun_policy_test")
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
    assert "with the bit: OK" in r.stdout and "without the bit" in r.stdout
    assert "ERROR: " not in r.stderr
