"""k_shadow_gen, k_trace_shadow and k_shade in their three schedules against oracle_shade (bit for
bit) and against the float64 model of hit shading (tests/hit_shading_model.py), on the planted
hits of tests/hit_shading_inputs.py through ark_ddgi_debug_shade, with the constants
tests/test_hit_shading_model.py measured on the CPU (the model's precision, never the
kernels'). The real-update test at the end plants what ark_ddgi_update itself recorded.

Schedules (csrc/shade_schedule.h): "listed" is the shadow-ray generator's (any spot light, no
light, or the sun alone under ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE or ARK_DDGI_FLAG_NO_SUN_COVER_MAP);
"sun_only" is k_shade resolving the sun's rays from the cover map with its deferred pass. Each
runs with counting off and on (the counting instances of the kernels).
"""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import hit_shading_inputs as HI
import hit_shading_model as M
import test_hit_shading_model as T

pytestmark = pytest.mark.gpu

CASES = T.CASES
POISON = 0x5555

# schedule -> DDGIConfig fields
VARIANTS = {
    "default": {},
    "no_fused_sun_shade": dict(fused_sun_shade=False),
    "no_sun_cover_map": dict(sun_cover_map=False),
}


# the sun alone, in a direction whose cover map set_scene builds: the default variant runs the sun-only schedule
SUN_ONLY = ("lights_sun", "sun_grazing_ndotv", "sun_along_ray")


def sun_alone(case):
    return case["sun"] is not None and not case["spots"]


def variants_of(case):
    """(variant, counting) of every schedule the case admits: the flags change the schedule of
    the sun alone only."""
    names = sorted(VARIANTS) if sun_alone(case) else ["default"]
    return [(v, c) for v in names for c in (False, True)]


def context_for(case, variant="default", scene=None):
    cfg = HI.config(case)
    for k, v in VARIANTS[variant].items():
        setattr(cfg, k, v)
    ctx = D.DDGIContext(HI.GRID, case["z_far"], cfg, 0, case["shard"][0], case["shard"][1])
    ctx.set_scene(scene if scene is not None else case["scene"])
    ctx.set_sun_only_small_windows(True)
    if case.get("atlas"):
        irr, vis = HI.ATLASES[case["atlas"]]()
        ctx.write(abi.ARK_DDGI_ATLAS_IRRADIANCE, irr)
        ctx.write(abi.ARK_DDGI_ATLAS_VISIBILITY, vis)
        ctx.write(abi.ARK_DDGI_PROBE_OFFSETS, case["offsets"])
    return ctx


@functools.lru_cache(maxsize=None)
def gpu_shade(name, variant, counting):
    """(the whole surfel image, the window's light words, the schedule) of ark_ddgi_debug_shade."""
    case = CASES[name]
    ctx = context_for(case, variant)
    ctx.write(abi.ARK_DDGI_SURFELS, np.full(case["kmax"] * case["rmax"] * 4, POISON, np.uint16))
    ctx.set_counting(counting)
    assert ctx.debug_shade(HI.frame_params(case), case["hits"]) == 0
    ctx.synchronize()
    image = ctx.read(abi.ARK_DDGI_SURFELS)
    bits = T.window_of(case, ctx.read(abi.ARK_DDGI_DEBUG_SHADOW_BITS))
    sched = ctx.shade_schedule()
    assert ctx.next_probe_index() == 0  # the rolling window did not advance
    ctx.close()
    return image, bits, sched


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return bool(np.all((a == b) | (T.is_nan16(a) & T.is_nan16(b))))


def front_rays(case):
    h = case["hits"]
    return (h["instance"] != M.MISS) & (h["t"] > 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_equal_oracle_shade(name):
    """Every schedule the case admits: the window's surfels equal oracle_shade's bit for bit,
    every window surfel is written over the pattern and every other one keeps its bytes; where
    the schedule writes every front hit's light word, the words equal the oracle's."""
    case = CASES[name]
    want, want_bits = T.oracle_shade(name)
    keep = np.ones((case["kmax"], case["rmax"]), bool)
    keep[:case["W"], :case["params"]["R"]] = False
    front = front_rays(case)
    lights = (case["sun"] is not None) + len(case["spots"])
    seen = set()
    for variant, counting in variants_of(case):
        image, bits, sched = gpu_shade(name, variant, counting)
        what = f"{name} {variant} counting={counting}"
        got = T.window_of(case, image)
        assert same_bits(got, want), f"{what}: {np.count_nonzero((got != want) & ~(T.is_nan16(got) & T.is_nan16(want)))} channels differ from oracle_shade"
        assert np.all(image.reshape(case["kmax"], case["rmax"], 4)[keep] == POISON), f"{what}: a surfel outside the window changed"
        # a written surfel cannot keep the pattern in all four channels: no distance of a case is 85.3
        assert not np.any(got[:, 3] == POISON), f"{what}: {np.count_nonzero(got[:, 3] == POISON)} window surfels not written"
        sun_only = bool(sched["sun_only"])
        if name in SUN_ONLY:
            assert sun_only == (variant == "default"), (what, sched)
        elif not (sun_alone(case) and variant == "default"):  # (a sun along the horizon: set_scene may build no cover map)
            assert not sun_only, (what, sched)
        seen.add(sun_only)
        if lights and (not sun_only or counting):
            assert np.array_equal(bits[front], want_bits[front]), f"{what}: {np.count_nonzero(bits[front] != want_bits[front])} light words differ from the oracle's"
    assert seen == ({True, False} if name in SUN_ONLY else {False}) or name.startswith("sun_ldotn")


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_against_model(name):
    """The kernels against the float64 model with the CPU file's constants: they leave the same
    share of channels outside the bound as the oracle does."""
    case = CASES[name]
    m64 = T.model(name, "float64")[0]
    flips = np.zeros(case["W"] * case["params"]["R"], bool)
    flips[sorted(case["flip_rays"])] = True
    d_orc, _ = T.compare(case, T.oracle_shade(name)[0], None, m64, flips)
    for variant, counting in variants_of(case):
        image, bits, sched = gpu_shade(name, variant, counting)
        lit = None
        if (case["sun"] is not None or case["spots"]) and (not sched["sun_only"] or counting):
            lit = np.where(front_rays(case), bits & 0xFFFF, 0)
        d, bad = T.compare(case, T.window_of(case, image), lit, m64, flips)
        T.report(f"{name} kernels {variant} counting={counting}", d)
        assert not bad, bad
        assert np.mean(d > T.ULP_BOUND) == np.mean(d_orc > T.ULP_BOUND) if d.size else True


def test_spot_at_the_hit_point():
    """Hazard 15 on the device: the spot at a ray's own hit point (the oracle's test builds it) is
    lit, not occluded (a NaN tmax), and the surfel's colour is NaN; equal to the oracle's."""
    import oracle_lib as O

    case = HI.spot_at_hit_case()
    j = case["spot_at_ray"]
    slot, sample = divmod(j, case["params"]["R"])
    d = np.zeros(3, np.float32)
    O.load().oracle_rotated_fib(int(case["probes"][slot]), sample, case["params"]["R"], case["params"]["frame"], d.ctypes.data)
    point = HI.rays32(case)[0][j] + case["hits"]["t"][j] * d
    sc = HI.scene_with(None, [HI.spot(point)])
    orc = T.oracle_for(case, sc)
    assert orc.shade(HI.frame_params(case), case["hits"]) == 0
    want = T.window_of(case, orc.read(abi.ARK_DDGI_SURFELS))
    want_bits = T.window_of(case, orc.read(O.ORACLE_SHADOW_BITS))
    orc.close()
    ctx = context_for(case, scene=sc)
    assert ctx.debug_shade(HI.frame_params(case), case["hits"]) == 0
    ctx.synchronize()
    got = T.window_of(case, ctx.read(abi.ARK_DDGI_SURFELS))
    bits = T.window_of(case, ctx.read(abi.ARK_DDGI_DEBUG_SHADOW_BITS))
    ctx.close()
    assert same_bits(got, want) and np.array_equal(bits, want_bits)
    assert got[j, :3].tolist() == [0x7E00] * 3 and bits[j] == 1


def test_refused_records_launch_nothing():
    case = CASES["mixed_r16_a"]
    ctx = context_for(case)
    ctx.write(abi.ARK_DDGI_SURFELS, np.full(case["kmax"] * case["rmax"] * 4, POISON, np.uint16))
    k = int(np.flatnonzero(case["hits"]["instance"] != M.MISS)[-1])
    for field, value in (("instance", len(case["scene"].instances)), ("primitive", 1000), ("t", np.nan), ("t", 1e-5), ("t", 2 * HI.Z_FAR), ("u", np.nan),
                         ("v", -0.01), ("u", 0.999)):
        hits = case["hits"].copy()
        hits[field][k] = value
        if field == "u" and value == 0.999:
            hits["v"][k] = 0.01
        assert ctx.debug_shade(HI.frame_params(case), hits) == abi.ARK_DDGI_E_INVALID_ARGUMENT, (field, value)
    ctx.synchronize()
    assert np.all(ctx.read(abi.ARK_DDGI_SURFELS) == POISON)
    assert ctx.debug_shade(HI.frame_params(case), case["hits"]) == 0
    ctx.synchronize()
    assert same_bits(T.window_of(case, ctx.read(abi.ARK_DDGI_SURFELS)), T.oracle_shade("mixed_r16_a")[0])
    ctx.close()


def test_debug_entry_equals_a_real_update():
    """A real ark_ddgi_update of the features scene (two frames, K < N), its hit records read
    back and mapped to (instance, primitive) through the downloaded triangle records, then
    planted in a second context that shares the scene: the surfels are the update's, byte for byte."""
    import scenes

    cfg = D.DDGIConfig(rays_per_probe=37, probe_updates_per_frame=23, max_rays_per_probe=40, max_probe_updates=23)
    sc = scenes.features_scene()
    a = D.DDGIContext(HI.GRID, HI.Z_FAR, cfg)
    a.set_scene(sc)
    a.write(abi.ARK_DDGI_PROBE_OFFSETS, CASES["mixed_r16_a"]["offsets"])
    p = [D.frame_params(cfg, HI.GRID, D.AppState(f), (41 * f) % HI.N_PROBES, light_pre_exposure=1.0, environment_brightness=0.5) for f in range(2)]
    a.update(p[0])
    a.synchronize()
    before = {w: a.read(w) for w in (abi.ARK_DDGI_ATLAS_IRRADIANCE, abi.ARK_DDGI_ATLAS_VISIBILITY, abi.ARK_DDGI_PROBE_OFFSETS)}
    a.update(p[1])
    a.synchronize()
    surfels = a.read(abi.ARK_DDGI_SURFELS)
    n = 23 * 37
    rec = a.read(abi.ARK_DDGI_DEBUG_HITS).view(np.uint32).reshape(-1, 4)[:n]  # {t, u, v, tri}
    records = a.world_records()
    hits = np.zeros(n, D.SHADE_HIT_DTYPE)
    tri = rec[:, 3]
    hit = tri != 0xFFFFFFFF
    assert hit.any() and (~hit).any() and np.all(tri[hit] < len(records))
    hits["instance"] = np.where(hit, records[np.where(hit, tri, 0), 9], 0xFFFFFFFF)
    hits["primitive"] = np.where(hit, records[np.where(hit, tri, 0), 10], 0)
    hits["t"], hits["u"], hits["v"] = (np.where(hit, rec[:, k].view(np.float32), 0).astype(np.float32) for k in (0, 1, 2))
    assert not np.any(hits["instance"][hit] == 0xFFFFFFFF)  # no hit names a hole
    b = D.DDGIContext(HI.GRID, HI.Z_FAR, cfg)
    b.share_scene(a)
    for w, x in before.items():
        b.write(w, x)
    b.write(abi.ARK_DDGI_SURFELS, np.full(23 * 40 * 4, POISON, np.uint16))
    assert b.debug_shade(p[1], hits) == 0
    b.synchronize()
    got = b.read(abi.ARK_DDGI_SURFELS)
    case = dict(W=23, kmax=23, rmax=40, params=dict(R=37))
    assert np.array_equal(T.window_of(case, got), T.window_of(case, surfels))
    assert np.array_equal(b.read(abi.ARK_DDGI_DEBUG_HITS).view(np.uint32).reshape(-1, 4)[:n], rec)
    b.close()
    a.close()
