"""The probe rays' hit candidates (csrc/seed_cache.h), the parts that need no GPU: the
direction -> texel function, the guard over cache words, and the host simulator's candidate
mode (tools/sim), which must find the closest hits its plain mode finds."""
import os
import sys

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "sim"))

NONE = 0xFFFFFFFF


def _texel(lib, d):
    return int(lib.ark_ddgi_debug_seed_texel(float(d[0]), float(d[1]), float(d[2])))


def test_texel_range_and_coverage():
    """Every direction of a dense set - the axes, the octant seams (a zero component), the
    folds of the lower hemisphere, scaled and denormal lengths, zero and non-finite vectors -
    maps into [0, T^2); the dense set reaches every texel."""
    lib = abi.load_library()
    T2 = 16 * 16
    rng = np.random.default_rng(3)
    dense = rng.normal(size=(40_000, 3))
    dense /= np.linalg.norm(dense, axis=1, keepdims=True)
    axes = [(sx * (a == 0), sx * (a == 1), sx * (a == 2)) for a in range(3) for sx in (1.0, -1.0)]
    seams = []
    for t in np.linspace(0.0, 2.0 * np.pi, 257):
        c, s = float(np.cos(t)), float(np.sin(t))
        seams += [(c, s, 0.0), (c, 0.0, s), (0.0, c, s), (c, s, -0.0), (c, s, -1e-30), (c, s, 1e-30)]
    diag = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    odd = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (1e-40, 0.0, 0.0), (0.0, -1e-45, 0.0), (3e38, 3e38, -3e38), (float("inf"), 0.0, 0.0),
           (float("nan"), 1.0, 0.0), (0.0, 0.0, float("-inf")), (float("nan"),) * 3]
    seen = set()
    for d in list(dense) + axes + seams + diag + odd + [tuple(1e-3 * np.asarray(v)) for v in dense[:500]]:
        t = _texel(lib, d)
        assert 0 <= t < T2, (d, t)
        seen.add(t)
    assert len(seen) == T2
    # opposite directions never share a texel, +z and -z land in the centre and a corner
    assert _texel(lib, (0, 0, 1)) != _texel(lib, (0, 0, -1))
    for d in dense[:2000]:
        assert _texel(lib, d) != _texel(lib, -d)


def test_candidate_guard():
    """The lookup's guard: only records of the opaque class [first, end) pass; the sentinel,
    records of the other classes and indices past the array are "no candidate"."""
    ok = abi.load_library().ark_ddgi_debug_seed_candidate_ok
    first, end, records = 0, 1000, 1500  # opaque [0, 1000), masked and blend [1000, 1500)
    assert ok(0, first, end) == 1 and ok(999, first, end) == 1
    assert ok(1000, first, end) == 0 and ok(records - 1, first, end) == 0  # other classes
    assert ok(records, first, end) == 0 and ok(0x7FFFFFFF, first, end) == 0 and ok(0x80000000, first, end) == 0  # past the array
    assert ok(NONE, first, end) == 0 and ok(NONE, 0, NONE) == 0  # the sentinel, whatever the range
    assert ok(0, 0, 0) == 0 and ok(NONE, 0, 0) == 0  # no opaque class
    assert ok(4, 5, 9) == 0 and ok(5, 5, 9) == 1 and ok(8, 5, 9) == 1 and ok(9, 5, 9) == 0  # a range that does not start at 0
    rng = np.random.default_rng(1)
    for w in rng.integers(0, 1 << 32, 2000, dtype=np.uint64):
        assert ok(int(w), 100, 70_000) == (1 if 100 <= int(w) < 70_000 else 0)


def test_flag_value():
    from arkoserenderer_amd import ddgi as D

    assert abi.ARK_DDGI_FLAG_NO_RAY_SEEDS == 0x100 and D.DDGIConfig().ray_seeds
    grid = D.ProbeGrid((2, 2, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert D.desc_for(grid, 10.0, D.DDGIConfig()).flags & abi.ARK_DDGI_FLAG_NO_RAY_SEEDS == 0
    assert D.desc_for(grid, 10.0, D.DDGIConfig(ray_seeds=False)).flags == abi.ARK_DDGI_FLAG_NO_RAY_SEEDS


def test_simulator_candidate_mode_keeps_hits():
    """20,000-triangle soup, 12 probes x 64 rays, 4 updates: with a 16 x 16 cache, with
    explicit candidates (every ray offered the same record; every ray offered a random one) and
    without any, the simulator's dual step returns the same closest hits and distances; the
    cache's candidates are hit and save node visits."""
    import bvhsim
    import seed_stats as T

    sim = bvhsim.load()
    tris = T.world_triangles(S.soup(20_000, extent=7.0))
    rng = np.random.default_rng(9)
    origins = rng.uniform(1.0, 6.0, size=(12, 3)).astype(np.float32)
    rays, probe_of = T.probe_rays(origins, 64, 4, 10000.0)
    n = rays.shape[1]
    base, hit0, t0 = T.trace(sim, tris, rays, probe_of, 12, 0, 4)
    assert 0 < int(base[:, 2].sum()) and np.all(base[:, 4] == 0)
    cached, hit1, t1 = T.trace(sim, tris, rays, probe_of, 12, 16, 4)
    assert np.array_equal(hit0, hit1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
    assert cached[0, 4] == 0 and np.array_equal(cached[0], base[0])  # a cold cache: the plain traversal
    held, got = int(cached[1:, 4].sum()), int(cached[1:, 5].sum())
    print(f"simulator, 16 x 16 cache: {held} of {3 * n} rays held a candidate, {got} were hit; node visits {base[1:, 0].sum()} -> {cached[1:, 0].sum()}")
    # (64 rays fill at most a quarter of a probe's 256 texels per update, and only hits fill)
    assert held > 0 and got > 0 and int(cached[1:, 0].sum()) < int(base[1:, 0].sum())
    records = int(hit0.max(initial=0, where=hit0 != NONE)) + 1
    some = int(hit0[hit0 != NONE][0])
    for cand in (np.full(n, some, np.uint32), rng.integers(0, records, n).astype(np.uint32), np.full(n, NONE, np.uint32)):
        fo, hit2, t2 = T.trace(sim, tris, rays[:1], probe_of, 12, 0, 4, candidates=cand)
        assert np.array_equal(hit2[0], hit0[0]) and np.array_equal(t2[0].view(np.uint32), t0[0].view(np.uint32))
        assert int(fo[0, 4]) == int(np.count_nonzero(cand != NONE))
