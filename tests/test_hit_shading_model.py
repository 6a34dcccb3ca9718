"""Probe hit shading (the hit record to the surfel: opaque.rchit, brdf.glsl, the IES lookup, the
texture fetch, raygen.rgen's miss, indirect term and back-face rule) against a float64 model
written from the shaders (tests/hit_shading_model.py), on planted hits built to reach every
term (tests/hit_shading_inputs.py). CPU only: the oracle's side, through oracle_shade;
tests/test_gpu_hit_shading.py holds the HIP kernels to the oracle bit for bit and to the same
model with the same constants.

The bound is the model's own precision (EXPERIMENTS.md "Hit shading against a float64 model"):
the float32 instance of the model against the float64 one, in fp16 ulps of the stored channel.
MEASURED[case] is the smallest whole number of fp16 ulps that at least 99 % of a case's
channels stay within. The stored format is so much coarser than float32 that every figure but
one is 0: the float32 model differs from the float64 one only where a value falls within
float32's error of an fp16 rounding boundary. The grazing highlights (NdotV and NdotL of 1e-3
under V_SmithGGXCorrelated's 1 / (NdotL + NdotV)) measure 1. One ulp is added because the
oracle and the kernels evaluate pow, atan and acos with ark_fmath.h's powf_, atan2f_ and acosf_
where the model has numpy's: powf_ in F_Schlick (every lit light's specular, clearcoat and
diffuse terms and the indirect term) and in the sRGB decode of base colour texels, atan2f_ and
acosf_ in the IES lookup (every spot term) and in sphericalUvFromDirection (every miss). At
most OUTLIER_CAP of a case's channels may lie outside ULP_BOUND: a condition, not a
measurement. Decisions (lit lights, angleV <= 0, every fetch's texel, the angleH clamp, NaN)
are compared exactly; a ray whose decisions differ between the float32 and the float64 model
is a flip, allowed only where the case lists it (a light placed on a discontinuity that holds
in fp32 only), excluded from the value check and held to NaN for NaN.
"""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import hit_shading_inputs as HI
import hit_shading_model as M
import oracle_lib as O
from parity import make_desc

# case: fp16 ulps holding 99 % of the channels, float32 model against float64 model
MEASURED = {name: 0 for name in HI.cases()}
MEASURED["grazing_highlights"] = 1
LIBM_TERMS_ULP = 1  # powf_ / atan2f_ / acosf_ against numpy's (the module docstring names the terms)
ULP_BOUND = max(MEASURED.values()) + LIBM_TERMS_ULP
OUTLIER_CAP = 0.01
FLIP_CAP = 0.01

CASES = HI.cases()


def ulps16(a, b):
    """|a - b| in fp16 ulps between two arrays of fp16 codes; NaN against NaN is 0, equal
    infinities are 0, NaN against a number 65535."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    key = lambda x: np.where(x & 0x8000, -(x & 0x7FFF).astype(np.int32), (x & 0x7FFF).astype(np.int32))  # noqa: E731
    d = np.abs(key(a) - key(b))
    na, nb = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return np.where(na & nb, 0, np.where(na | nb, 65535, d))


def percentile_figure(d):
    """The smallest whole number of fp16 ulps that at least 99 % of `d` stay within."""
    d = np.sort(np.asarray(d).reshape(-1))
    return int(d[int(np.ceil(0.99 * d.size)) - 1]) if d.size else 0


def is_nan16(c):
    return (np.asarray(c) & 0x7FFF) > 0x7C00


def oracle_for(case, scene=None):
    orc = O.Oracle(make_desc(HI.GRID, case["z_far"], HI.config(case), shard_rank=case["shard"][0], shard_count=case["shard"][1]))
    orc.set_scene(scene if scene is not None else case["scene"])
    irr, vis = HI.ATLASES[case["atlas"]]()
    orc.write(abi.ARK_DDGI_ATLAS_IRRADIANCE, irr)
    orc.write(abi.ARK_DDGI_ATLAS_VISIBILITY, vis)
    orc.write(abi.ARK_DDGI_PROBE_OFFSETS, case["offsets"])
    return orc


def window_of(case, image):
    """[W * R, ...] of a [kmax][rmax] surfel image or a [kmax * rmax] per-ray array indexed
    slot * R + sample."""
    W, R = case["W"], case["params"]["R"]
    image = np.asarray(image)
    if image.ndim == 1 and image.dtype != np.uint16:
        return image[:W * R]
    return image.reshape(case["kmax"], case["rmax"], 4)[:W, :R].reshape(W * R, 4)


@functools.lru_cache(maxsize=None)
def oracle_shade(name):
    """(surfel codes [W * R, 4], light words [W * R]) of oracle_shade on the case's hits."""
    case = CASES[name]
    orc = oracle_for(case)
    poison = np.full(case["kmax"] * case["rmax"] * 4, 0x5555, np.uint16)
    orc.write(abi.ARK_DDGI_SURFELS, poison)
    assert orc.shade(HI.frame_params(case), case["hits"]) == 0
    image = orc.read(abi.ARK_DDGI_SURFELS)
    bits = window_of(case, orc.read(O.ORACLE_SHADOW_BITS))
    orc.close()
    # surfel slots in [R, Rmax) and beyond the window keep their bytes
    keep = np.ones((case["kmax"], case["rmax"]), bool)
    keep[:case["W"], :case["params"]["R"]] = False
    assert np.all(image.reshape(case["kmax"], case["rmax"], 4)[keep] == 0x5555), name
    return window_of(case, image), bits


@functools.lru_cache(maxsize=None)
def model(name, dtype_name, mut=None):
    """The model on the case's hits, with the occlusion the oracle's own shadow rays found."""
    c = CASES[name]
    irr, vis = HI.ATLASES[c["atlas"]]()
    stats = {}
    out = M.shade(c["scene"], HI.model_grid(), irr, vis, c["offsets"], c["params"], c["hits"], oracle_shade(name)[1] >> 16, np.dtype(dtype_name).type, mut,
                  stats, c["shard"])
    return out, stats


def flipped(a, b):
    """[n] bool: rays with a decision that differs between two results of the model."""
    n = len(a["lit"])
    f = np.zeros(n, bool)
    for k in a["decisions"]:
        if k != "nan":
            f |= (a["decisions"][k] != b["decisions"][k]).reshape(n, -1).any(1)
    return f


def compare(case, codes, lit, want, flips):
    """Surfel codes and lit masks against the float64 model's `want`; `flips`: the rays left
    out of the value check. Returns (ulps of the compared channels, what breaks the check)."""
    bad = []
    codes = np.asarray(codes, np.uint16).reshape(want["codes"].shape)
    if not np.array_equal(is_nan16(codes)[~flips], is_nan16(want["codes"])[~flips]):
        bad.append(f"NaN masks differ on {np.count_nonzero((is_nan16(codes) != is_nan16(want['codes']))[~flips].any(1))} rays")
    if lit is not None and not np.array_equal(np.asarray(lit)[~flips], want["lit"][~flips]):
        bad.append(f"lit masks differ on {np.count_nonzero((np.asarray(lit) != want['lit'])[~flips])} rays")
    d = ulps16(codes, want["codes"])[~flips & ~case["class_only"]].reshape(-1)
    share = float(np.mean(d > ULP_BOUND)) if d.size else 0.0
    if share > OUTLIER_CAP:
        bad.append(f"{share:.3%} of the channels beyond {ULP_BOUND} fp16 ulps")
    return d, bad


def report(what, d):
    hist = np.bincount(np.minimum(d, 3), minlength=4).tolist()
    print(f"{what}: channels at 0, 1, 2, more fp16 ulps {hist}, 99 % within {percentile_figure(d)}, outside the bound {np.mean(d > ULP_BOUND) if d.size else 0:.3%}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_what_it_was_built_for(name):
    case = CASES[name]
    for dtype_name, reach in (("float64", case["reach"]), ("float32", case["reach32"])):
        st = model(name, dtype_name)[1]
        for key, least in reach.items():
            assert st.get(key, 0) >= least, (name, dtype_name, key, st.get(key, 0), least)
    assert case["W"] * case["params"]["R"] <= 2 * 1024 + 37
    assert all(t.width <= 16 and t.height <= 16 for t in case["scene"].textures)


def test_cases_cover_the_issue():
    P = [c["params"] for c in CASES.values()]
    assert {1, 16, 37, 64} <= {p["R"] for p in P} and (37, 40) in {(c["params"]["R"], c["rmax"]) for c in CASES.values()}
    assert {1, 1023, 1024, 1025, 2 * 1024 + 37} <= {c["W"] * c["params"]["R"] for c in CASES.values()}
    assert any(p["first"] + p["K"] > HI.N_PROBES for p in P) and any(p["K"] < HI.N_PROBES for p in P)
    assert (1, 2) in {c["shard"] for c in CASES.values()} and CASES["zslab_rank1"]["W"] < CASES["zslab_rank1"]["params"]["K"]
    assert {0, 1, 2, 3, 11} <= {(c["sun"] is not None) + len(c["spots"]) for c in CASES.values()}
    assert {"a", "b", "b_inf"} <= {c["atlas"] for c in CASES.values()}
    assert any(c["z_far"] > 65504 for c in CASES.values())
    sc, names = HI.scene()
    formats = {t.format for t in sc.textures}
    assert formats == {abi.ARK_TEX_RGBA8_UNORM, abi.ARK_TEX_RGBA8_SRGB, abi.ARK_TEX_R32F, abi.ARK_TEX_RGBA32F}
    wraps = {t.wrap for t in sc.textures}
    assert {abi.ARK_WRAP_REPEAT, abi.ARK_WRAP_CLAMP_TO_EDGE, abi.ARK_WRAP_MIRRORED_REPEAT} <= wraps and any(w & abi.ARK_WRAP_PER_AXIS for w in wraps)
    env = sc.textures[sc.environment_texture]
    assert (env.width, env.height) == (8, 4)
    dets = [np.linalg.det(i["object_to_world"].reshape(3, 4)[:, :3]) for i in sc.instances]
    assert any(d < 0 for d in dets) and {int(i["hit_mask"]) for i in sc.instances} >= {abi.ARK_RT_HIT_MASK_OPAQUE, abi.ARK_RT_HIT_MASK_MASKED}
    assert sc.triangle_count <= 100
    # every instance is shaded somewhere, the mirrored and the scaled one on the barycentric case
    seen = set()
    for name in CASES:
        seen |= set(model(name, "float64")[1].get("front_by_instance", {}))
    assert seen == set(range(len(sc.instances)))
    assert {4, names["box_scaled"]} <= set(model("barycentrics", "float64")[1]["front_by_instance"])
    # the back faces beside an fp16 rounding boundary: the three neighbours do not store one value
    assert len(set(oracle_shade("backs")[0][:3, 3].tolist())) >= 2
    # the chunks of one kind
    for name, kind in (("misses_seam", "miss"), ("backs", "back"), ("fronts", "front")):
        st = model(name, "float64")[1]
        assert st[kind] == st["rays"] == 1024


def test_model_precision_sets_the_bound():
    """float32 model against float64 model on every case: prints and asserts the measured
    figures, the cap on the outliers and the flips."""
    for name, case in CASES.items():
        m32, m64 = model(name, "float32")[0], model(name, "float64")[0]
        flips = flipped(m32, m64)
        assert set(np.flatnonzero(flips).tolist()) <= case["flip_rays"], (name, np.flatnonzero(flips))
        assert np.mean(flips) <= FLIP_CAP or case["flip_rays"], name
        d, bad = compare(case, m32["codes"], m32["lit"], m64, flips)
        report(f"{name} float32 model ({int(flips.sum())} flips)", d)
        assert not bad, (name, bad)
        assert percentile_figure(d) == MEASURED[name], (name, percentile_figure(d))
        assert np.array_equal(m32["decisions"]["nan"][~flips], m64["decisions"]["nan"][~flips]), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_shade_against_model(name):
    """oracle_shade on the planted hits against the float64 model; its lit masks are the
    model's except on the case's listed flips."""
    case = CASES[name]
    codes, bits = oracle_shade(name)
    m64 = model(name, "float64")[0]
    flips = np.zeros(len(bits), bool)
    flips[sorted(case["flip_rays"])] = True
    d, bad = compare(case, codes, bits & 0xFFFF, m64, flips)
    report(f"{name} oracle", d)
    assert not bad, bad
    # the oracle is an fp32 evaluation: its decisions that show (lit masks, NaN) are the float32 model's
    m32 = model(name, "float32")[0]
    assert np.array_equal(bits & 0xFFFF, m32["lit"]), name
    assert np.array_equal(is_nan16(codes), is_nan16(m32["codes"])), name


def test_spot_at_the_hit_point():
    """A spot at a ray's own fp32 hit point (origin + t dir as the oracle computes it): distance 0,
    the attenuation inf, the direction to the light NaN, the shadow ray's tmax NaN - it counts
    as lit and not occluded (hazard 15), and the surfel's colour is NaN, stored 0x7e00."""
    case = HI.spot_at_hit_case()
    j = case["spot_at_ray"]
    slot, sample = divmod(j, case["params"]["R"])
    d = np.zeros(3, np.float32)
    O.load().oracle_rotated_fib(int(case["probes"][slot]), sample, case["params"]["R"], case["params"]["frame"], d.ctypes.data)
    origin = HI.rays32(case)[0][j]  # position + offset: one fp32 addition, the same on every side
    point = origin + case["hits"]["t"][j] * d
    sc = HI.scene_with(None, [HI.spot(point)])
    orc = oracle_for(case, sc)
    assert orc.shade(HI.frame_params(case), case["hits"]) == 0
    codes = window_of(case, orc.read(abi.ARK_DDGI_SURFELS))
    bits = window_of(case, orc.read(O.ORACLE_SHADOW_BITS))
    orc.close()
    assert bits[j] == 1, hex(int(bits[j]))  # lit, not occluded
    assert codes[j, :3].tolist() == [0x7E00] * 3 and codes[j, 3] == np.float16(case["hits"]["t"][j]).view(np.uint16)
    others = np.delete(np.arange(len(bits)), j)
    assert not is_nan16(codes[others]).any()
    # the float32 model with the spot at its own fp32 hit point: the same class
    st = {}
    irr, vis = HI.ATLASES[case["atlas"]]()
    m32 = M.shade(case["scene"], HI.model_grid(), irr, vis, case["offsets"], case["params"], case["hits"], np.zeros(len(bits), np.uint32), np.float32, None, st)
    assert st["spot_distance_zero"] == 1 and is_nan16(m32["codes"][j, :3]).all() and m32["lit"][j] == 1


def real_update():
    """Two updates of the features scene with K < N; the state before the second one."""
    import scenes

    cfg = D.DDGIConfig(rays_per_probe=37, probe_updates_per_frame=23, max_rays_per_probe=40, max_probe_updates=23)
    case = dict(z_far=HI.Z_FAR, shard=(0, 1), kmax=23, rmax=40, W=23, params=dict(R=37, K=23), atlas=None, class_only=np.zeros(23 * 37, bool))
    sc = scenes.features_scene()
    orc = O.Oracle(make_desc(HI.GRID, HI.Z_FAR, cfg))
    orc.set_scene(sc)
    orc.write(abi.ARK_DDGI_PROBE_OFFSETS, HI.cases()["mixed_r16_a"]["offsets"])
    p = [D.frame_params(cfg, HI.GRID, D.AppState(f), (41 * f) % HI.N_PROBES, light_pre_exposure=1.0, environment_brightness=0.5) for f in range(2)]
    orc.update(p[0])
    before = {w: orc.read(w) for w in (abi.ARK_DDGI_ATLAS_IRRADIANCE, abi.ARK_DDGI_ATLAS_VISIBILITY, abi.ARK_DDGI_PROBE_OFFSETS)}
    orc.update(p[1])
    return case, sc, orc, p[1], before


def test_oracle_update_on_a_real_scene():
    """A real update: the model from the oracle's own per-ray hits and occlusion words stays
    within the bound of its surfels, and oracle_shade fed those hits reproduces them byte for byte."""
    case, sc, orc, p, before = real_update()
    surfels = orc.read(abi.ARK_DDGI_SURFELS)
    hits = orc.read(O.ORACLE_SHADE_HITS)[:case["W"] * 37]
    bits = orc.read(O.ORACLE_SHADOW_BITS)[:case["W"] * 37]
    kinds = (np.count_nonzero(hits["instance"] == O.MISS), np.count_nonzero((hits["instance"] != O.MISS) & (hits["t"] < 0)), np.count_nonzero(bits >> 16))
    print(f"real update: {len(hits)} rays, {kinds[0]} misses, {kinds[1]} back faces, {kinds[2]} rays with an occluded light")
    assert all(k > 0 for k in kinds)
    params = dict(frame=p.frame_index, first=p.first_probe_index, K=p.probe_updates, R=p.rays_per_probe, ambient=p.ambient_amount,
                  environment_multiplier=p.environment_multiplier, z_far=HI.Z_FAR)
    assert params["first"] + params["K"] > HI.N_PROBES or params["first"] > 0
    want = M.shade(sc, HI.model_grid(), before[abi.ARK_DDGI_ATLAS_IRRADIANCE], before[abi.ARK_DDGI_ATLAS_VISIBILITY], before[abi.ARK_DDGI_PROBE_OFFSETS],
                   params, hits, bits >> 16, np.float64)
    d, bad = compare(case, window_of(case, surfels), bits & 0xFFFF, want, np.zeros(len(hits), bool))
    report("real update, oracle", d)
    assert not bad, bad
    # the same state before the second update, shaded from the recorded hits
    twin = O.Oracle(make_desc(HI.GRID, HI.Z_FAR, D.DDGIConfig(rays_per_probe=37, probe_updates_per_frame=23, max_rays_per_probe=40, max_probe_updates=23)))
    twin.set_scene(sc)
    for w, a in before.items():
        twin.write(w, a)
    twin.write(abi.ARK_DDGI_SURFELS, np.full(23 * 40 * 4, 0x5555, np.uint16))
    assert twin.shade(p, hits) == 0
    got = twin.read(abi.ARK_DDGI_SURFELS)
    assert np.array_equal(window_of(case, got), window_of(case, surfels))
    assert np.array_equal(twin.read(O.ORACLE_SHADOW_BITS)[:len(bits)], bits)
    assert np.array_equal(twin.read(O.ORACLE_SHADE_HITS)[:len(hits)], hits)


def test_oracle_shade_refuses_bad_records():
    case = CASES["mixed_r16_a"]
    orc = oracle_for(case)
    p = HI.frame_params(case)
    n_inst = len(case["scene"].instances)
    for field, value in (("instance", n_inst), ("primitive", 1000), ("t", np.nan), ("t", np.inf), ("t", 1e-5), ("t", -1e-5), ("t", 2 * HI.Z_FAR),
                         ("u", np.nan), ("v", np.inf), ("u", -0.01), ("v", -0.01), ("u", 0.9)):
        hits = case["hits"].copy()
        k = int(np.flatnonzero(hits["instance"] != O.MISS)[3])
        hits[field][k] = value
        if field == "u" and value == 0.9:
            hits["v"][k] = 0.2
        assert orc.shade(p, hits) == abi.ARK_DDGI_E_INVALID_ARGUMENT, (field, value)
    assert orc.shade(p, case["hits"]) == 0
    orc.close()


def detects(mut):
    """(case, what breaks) of the first case on which the mutated float64 model against the
    oracle breaks the check, i.e. on which test_oracle_shade_against_model would fail; and the
    share of all cases' channels the mutation moves."""
    hit, moved, total = None, 0, 0
    for name, case in CASES.items():
        want, right = model(name, "float64", mut)[0], model(name, "float64")[0]
        moved += int(np.count_nonzero(want["codes"] != right["codes"]))
        total += want["codes"].size
        if hit is None:
            codes, bits = oracle_shade(name)
            flips = np.zeros(len(bits), bool)
            flips[sorted(case["flip_rays"])] = True
            _, bad = compare(case, codes, bits & 0xFFFF, want, flips)
            if bad:
                hit = (name, bad)
    return hit, moved / total


@pytest.mark.parametrize("mut", sorted(M.MUTATIONS))
def test_inputs_detect_mutation(mut):
    """The inputs can tell a wrong shader from a right one: each one-line mutation of the
    model breaks the check against the oracle on at least one case."""
    hit, share = detects(mut)
    assert hit is not None, f"no case detects: {M.MUTATIONS[mut]}"
    print(f"{mut}: moves {share:.2%} of the cases' channels; first detected by {hit[0]}: {hit[1][0]}")
