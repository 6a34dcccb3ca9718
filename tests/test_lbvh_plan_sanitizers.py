"""The collapse plan of the device BVH builds (ARK_DDGI_FLAG_GPU_REBUILD_PLAN) as a stand-alone
program (tests/cpp/lbvh_plan_test.cpp: the plan against a brute force over every cut of every
binary tree of 2 to 10 primitives, the 257-, 4,099-triangle and coincident builds of the world
and the light-space tree, the rounds above the treelets) built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program, as test_lbvh_sah_sanitizers.py does. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [
    os.path.join(ROOT, "tests", "cpp", "lbvh_plan_test.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_builder.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "sun_bvh.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "lbvh_host.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh8_check.cpp"),
    os.path.join(ROOT, "arkoserenderer_amd", "csrc", "bvh_debug.cpp"),
]


def test_collapse_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lbvh_plan_test")
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
