"""The DDGI write side (irradiance and visibility blend, border copy, probe offsets) against a
float64 model written from the shaders (tests/probe_update_model.py), on planted inputs built
to reach every term (tests/probe_update_inputs.py). CPU only: the oracle's side, through
oracle_blend; tests/test_gpu_probe_update_model.py holds the HIP kernels to the same model and
the same constants.

The bound is the model's own precision (EXPERIMENTS.md "The write side against a float64
model"): the float32 instance of the model against the float64 one. Atlases in fp16 ulps of
the stored channel over the texels of the window's tiles, interior and border: MEASURED[case]
holds the smallest whole numbers of fp16 ulps that at least 99 % of a case's irradiance and
visibility channels stay within, ULP_BOUND is the largest of them, and at most OUTLIER_CAP of
the channels of either atlas of any case may lie outside it. The stored format is so much
coarser than float32 that every figure is 0: the float32 model differs from the float64 one
only where a value falls within float32's error of an fp16 rounding boundary, in at most
0.69 % of a case's channels (visibility at sharpness 80). Offsets as float32 relative error
against maxOffset: OFFSET_BOUND is twice the measured maximum, the path-tracer tests'
convention. NaN masks are compared exactly, texels outside the window byte for byte.
"""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import abi
import oracle_lib as O
import probe_update_inputs as PI
import probe_update_model as M
from parity import make_desc

# case: (irradiance, visibility) fp16 ulps holding 99 % of the channels, float32 model against float64 model
MEASURED = {
    "k1_r1": (0, 0),
    "k3_r3_wrap": (0, 0),
    "k4_r16_counts": (0, 0),
    "k5_r37_edges": (0, 0),
    "k7_r37_wrap": (0, 0),
    "whole_r16_clear": (0, 0),
    "whole_r16": (0, 0),
    "k5_r16_quarter": (0, 0),
    "k4_r37_sharp80": (0, 0),
    "k8_r512": (0, 0),
    "slab_rank0": (0, 0),
    "slab_rank1": (0, 0),
    "k5_r16_open": (0, 0),
}
ULP_BOUND = max(max(v) for v in MEASURED.values())
OUTLIER_CAP = 0.01
# float32 model against float64 model, largest offset error of any case relative to maxOffset
# (k8_r512: sums of about 36 directions, normalised at a tenth to a fifth of their summands' length)
OFFSET_MEASURED_MAX = 3.97e-6
OFFSET_BOUND = 2 * OFFSET_MEASURED_MAX

CASES = PI.cases()


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
    return int(d[int(np.ceil(0.99 * d.size)) - 1])


def is_nan16(c):
    return (np.asarray(c) & 0x7FFF) > 0x7C00


def compare(case, got, want):
    """`got` = (irr codes, vis codes, offsets) against the float64 model's `want`. Returns the
    figures and the list of what breaks the check (empty: the check holds)."""
    fig, bad = {}, []
    for name, res, g, w, ch in (("irradiance", M.IRRADIANCE_RES, got[0], want[0], 3), ("visibility", M.VISIBILITY_RES, got[1], want[1], 2)):
        g = np.asarray(g, np.uint16).reshape(w.shape)
        mask = PI.window_mask(case, res)
        if not np.array_equal(g[~mask], w[~mask]):
            bad.append(f"{name}: {np.count_nonzero(g[~mask] != w[~mask])} channels outside the window's tiles differ")
        if not np.array_equal(is_nan16(g), is_nan16(w)):
            bad.append(f"{name}: NaN masks differ in {np.count_nonzero(is_nan16(g) != is_nan16(w))} channels")
        if name == "irradiance" and np.any(g[mask][:, 3] != w[mask][:, 3]):
            bad.append("irradiance: alpha differs")
        d = ulps16(g[mask][:, :ch], w[mask][:, :ch]).reshape(-1)
        fig[name] = d
        share = float(np.mean(d > ULP_BOUND))
        if share > OUTLIER_CAP:
            bad.append(f"{name}: {share:.3%} of the window's channels beyond {ULP_BOUND} fp16 ulps")
    go = np.asarray(got[2], np.float64).reshape(case["grid"].count, -1)[:, :3]
    wo = np.asarray(want[2], np.float64)
    if not np.array_equal(np.isnan(go), np.isnan(wo)):
        bad.append("offsets: NaN masks differ")
    with np.errstate(invalid="ignore"):
        rel = np.abs(go - wo) / PI.max_offset(case["g"])
        rel = np.where(np.isnan(go) | np.isnan(wo) | (go == wo), 0.0, rel)
    fig["offsets"] = float(rel.max())
    if not fig["offsets"] <= OFFSET_BOUND:
        bad.append(f"offsets: {fig['offsets']:.3g} of maxOffset off, bound {OFFSET_BOUND:.3g}")
    outside = np.ones(case["grid"].count, bool)
    outside[case["probes"]] = False
    if not case["params"]["update_offsets"]:
        outside[:] = True
    if not np.array_equal(go[outside].astype(np.float32).view(np.uint32), case["offsets"][outside, :3].view(np.uint32)):
        bad.append("offsets: a probe outside the window moved")
    return fig, bad


@functools.lru_cache(maxsize=None)
def model(name, dtype_name, mut=None):
    c = CASES[name]
    stats = {}
    out = M.update(c["grid"], c["params"], c["surfels"], c["irr"], c["vis"], c["offsets"], np.dtype(dtype_name).type, mut, stats, c["shard"])
    return out, stats


def oracle_for(case):
    orc = O.Oracle(make_desc(PI.probe_grid(case), case["z_far"], PI.config(case), shard_rank=case["shard"][0], shard_count=case["shard"][1]))
    orc.write(abi.ARK_DDGI_SURFELS, case["surfels"])
    orc.write(abi.ARK_DDGI_ATLAS_IRRADIANCE, case["irr"])
    orc.write(abi.ARK_DDGI_ATLAS_VISIBILITY, case["vis"])
    orc.write(abi.ARK_DDGI_PROBE_OFFSETS, case["offsets"])
    return orc


def read_all(src):
    return (src.read(abi.ARK_DDGI_ATLAS_IRRADIANCE), src.read(abi.ARK_DDGI_ATLAS_VISIBILITY), src.read(abi.ARK_DDGI_PROBE_OFFSETS))


@functools.lru_cache(maxsize=None)
def oracle_blend(name):
    case = CASES[name]
    orc = oracle_for(case)
    orc.blend(PI.frame_params(case))
    out = read_all(orc)
    orc.close()
    return out


def report(what, fig):
    hist = lambda d: np.bincount(np.minimum(d, 3), minlength=4).tolist()  # noqa: E731
    print(f"{what}: irradiance channels at 0, 1, 2, more fp16 ulps {hist(fig['irradiance'])} (outside the bound {np.mean(fig['irradiance'] > ULP_BOUND):.3%}), "
          f"visibility {hist(fig['visibility'])} ({np.mean(fig['visibility'] > ULP_BOUND):.3%}), offsets {fig['offsets']:.3g} of maxOffset")


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_what_it_was_built_for(name):
    """The model's own intermediate counts: texels under epsilon, rays per offset class, clamped
    distances, probes per offset branch. Every distance word equals what k_shade derives from
    the hit record; planted atlases are border-consistent."""
    case = CASES[name]
    _, st = model(name, "float64")
    for key, least in case["reach"].items():
        if key == "back_counts_has":
            assert set(least) <= set(st["back_counts"]), (name, st["back_counts"])
        else:
            assert st[key] >= least, (name, key, st[key], least)
    R, W = case["params"]["R"], len(case["probes"])
    assert np.array_equal(case["surfels"][:W, :R, 3], PI.surfel_distance(case["hits"]["t"], case["hits"]["tri"], case["z_far"]))
    for atlas, res in ((case["irr"], M.IRRADIANCE_RES), (case["vis"], M.VISIBILITY_RES)):
        assert np.array_equal(M.copy_borders(case["grid"], atlas.copy(), res), atlas)
    assert case["grid"].count <= 24 and W * R <= 8 * 512


def test_cases_cover_the_issue():
    """Windows, ray counts, sharpness modes, hystereses and the distance edges of the list."""
    P = [c["params"] for c in CASES.values()]
    assert {1, 3, 4, 5, 7, 24} <= {p["K"] for p in P}
    assert {1, 3, 16, 37, 512} <= {p["R"] for p in P}
    assert {(37, 40), (16, 64), (37, 72)} <= {(c["params"]["R"], c["rmax"]) for c in CASES.values()}
    assert {50.0, 1.0, 8.0, 64.0, 7.3, 0.25, 80.0} <= {p["sharpness"] for p in P}
    assert {0.0, 0.98, 1.0} <= {p["hysteresis_irradiance"] for p in P} | {p["hysteresis_visibility"] for p in P}
    assert any(p["first"] + p["K"] > c["grid"].count for p, c in zip(P, CASES.values()))
    assert any(p["frame"] >= M.PARAM_SPACING for p in P)
    assert {c["shard"] for c in CASES.values()} >= {(0, 1), (0, 2), (1, 2)}
    # slab ranks: compacted slots, fewer than the window's K
    assert len(CASES["slab_rank0"]["probes"]) + len(CASES["slab_rank1"]["probes"]) == 7 and len(CASES["slab_rank0"]["probes"]) not in (0, 7)
    # the distance edges, as the stored fp16 words
    edges = CASES["k5_r37_edges"]
    words = set(edges["surfels"][0, :37, 3].tolist())
    g = edges["g"]
    f16 = lambda v: int(np.float16(v).view(np.uint16))  # noqa: E731
    md, mo = PI.max_distance(g), PI.max_offset(g)
    want = [0x0000, 0x8000, 0x0001, 0x8001, 0x7C00, 0xFC00] + [f16(s * PI.f16_step(v, n)) for v in (md, mo) for n in (-1, 0, 1) for s in (1, -1)]
    assert set(want) <= words, sorted(set(want) - words)
    assert float(np.float16(md)) == md and float(np.float16(mo)) == mo
    op = CASES["k5_r16_open"]
    assert np.count_nonzero(op["surfels"][0, :16, :3] == 0x7C00) == 1 and np.count_nonzero(is_nan16(op["surfels"][1, :16, :3])) == 1
    assert is_nan16(op["surfels"][2, 4, 3]) and (op["surfels"][:5, :16, 3] == 0x7C00).any()
    assert np.isnan(op["offsets"]).sum() == 1 and np.isinf(op["offsets"]).sum() == 1


def test_model_precision_sets_the_bound():
    """float32 model against float64 model on every case: prints and asserts the measured
    figures and the cap; the offset decisions (branch, clamp) are the same wherever the float64
    model is not within OFFSET_BOUND of the clamp's threshold."""
    worst = 0.0
    for name, case in CASES.items():
        (m32, s32), (m64, s64) = model(name, "float32"), model(name, "float64")
        fig, bad = compare(case, m32, m64)
        report(f"{name} float32 model", fig)
        assert not bad, (name, bad)
        assert (percentile_figure(fig["irradiance"]), percentile_figure(fig["visibility"])) == MEASURED[name], name
        worst = max(worst, fig["offsets"])
        if case["params"]["update_offsets"]:
            assert s32["branch"] == s64["branch"], name
            for c32, c64, margin in zip(s32["clamp"], s64["clamp"], s64["clamp_margin"]):
                assert c32 == c64 or margin <= OFFSET_BOUND, name
    print(f"largest offset error {worst:.3g} of maxOffset")
    assert 0.5 * OFFSET_MEASURED_MAX < worst <= OFFSET_MEASURED_MAX


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_blend_against_model(name):
    """oracle_blend on the planted surfels against the float64 model."""
    fig, bad = compare(CASES[name], oracle_blend(name), model(name, "float64")[0])
    report(f"{name} oracle", fig)
    assert not bad, bad


def real_surfel_case(offsets_on):
    """A real update of the features scene on planted atlases and offsets: the oracle traces and
    shades, its surfels are read back, and the model does the step from the planted state.
    (Not hysteresis 0.5: where every ray of a texel is clamped, the new value is maxDistance up
    to float32 rounding, and its mean with an fp16 texel lies on an fp16 rounding tie that this
    rounding decides - 1.2 % of the channels then differ, float32 model against float64 model.)"""
    import scenes

    g = dict(dims=(3, 2, 3), spacing=(1.5, 1.25, 1.5), origin=(-1.5, 0.5, -1.5))
    grid = PI.model_grid(g)
    rng = np.random.default_rng(31 + offsets_on)
    irr, vis = PI.random_atlases(rng, grid, g)
    off = np.zeros((grid.count, 4), np.float32)
    off[:, :3] = (rng.random((grid.count, 3)) - 0.5) * 0.4
    params = dict(frame=4 + offsets_on, first=13, K=9, R=32, hysteresis_irradiance=0.93, hysteresis_visibility=0.93, sharpness=50.0, delta_time=1.0 / 60.0,
                  update_offsets=offsets_on)
    case = dict(name=f"real_{offsets_on}", g=g, grid=grid, z_far=100.0, kmax=9, rmax=32, shard=(0, 1), params=params, irr=irr, vis=vis, offsets=off,
                probes=M.window_probes(grid, 13, 9))
    return case, scenes.features_scene()


@pytest.mark.parametrize("offsets_on", [0, 1])
def test_oracle_update_on_real_surfels_against_model(offsets_on):
    case, scene = real_surfel_case(offsets_on)
    orc = O.Oracle(make_desc(PI.probe_grid(case), case["z_far"], PI.config(case)))
    orc.set_scene(scene)
    for which, key in ((abi.ARK_DDGI_ATLAS_IRRADIANCE, "irr"), (abi.ARK_DDGI_ATLAS_VISIBILITY, "vis"), (abi.ARK_DDGI_PROBE_OFFSETS, "offsets")):
        orc.write(which, case[key])
    orc.update(PI.frame_params(case))
    surfels = orc.read(abi.ARK_DDGI_SURFELS).reshape(case["kmax"], case["rmax"], 4)
    assert np.count_nonzero(surfels[..., :3]) > 0 and len(set(surfels[..., 3].reshape(-1).tolist())) > 50
    want = M.update(case["grid"], case["params"], surfels, case["irr"], case["vis"], case["offsets"], np.float64)
    fig, bad = compare(case, read_all(orc), want)
    report(case["name"], fig)
    assert not bad, bad


def detects(mut):
    """(case, what breaks) of the first case on which the mutated float64 model against the
    oracle breaks the check, i.e. on which test_oracle_blend_against_model would fail; the
    shares of the window's channels (both atlases) and of its offset components the mutation moves."""
    hit, moved, total, off_moved, off_total = None, 0, 0, 0, 0
    for name, case in CASES.items():
        want, right = model(name, "float64", mut)[0], model(name, "float64")[0]
        for res, k in ((M.IRRADIANCE_RES, 0), (M.VISIBILITY_RES, 1)):
            mask = PI.window_mask(case, res)
            moved += int(np.count_nonzero(want[k][mask] != right[k][mask]))
            total += int(want[k][mask].size)
        if case["params"]["update_offsets"]:
            a, b = want[2][case["probes"]], right[2][case["probes"]]
            off_moved += int(np.count_nonzero((a != b) & ~(np.isnan(a) & np.isnan(b))))
            off_total += 3 * len(case["probes"])
        if hit is None:
            _, bad = compare(case, oracle_blend(name), want)
            if bad:
                hit = (name, bad)
    return hit, moved / total, off_moved / off_total


@pytest.mark.parametrize("mut", sorted(set(M.MUTATIONS) - set(M.IDENTITIES)))
def test_inputs_detect_mutation(mut):
    """The inputs can tell a wrong shader from a right one: each one-line mutation of the
    model breaks the check against the oracle on at least one case."""
    hit, share, off_share = detects(mut)
    assert hit is not None, f"no case detects: {M.MUTATIONS[mut]}"
    print(f"{mut}: moves {share:.2%} of the windows' atlas channels and {off_share:.2%} of their offset components; first detected by {hit[0]}: {hit[1][0]}")


def test_window_only_borders_are_an_identity():
    """Copying the borders of the window's tiles only is the one listed mutation no case can
    detect, by argument: every planted atlas is border-consistent (the function under test made
    it so), the update writes no interior outside the window, so the all-tile pass rewrites
    every other border with the value it already holds. That is the equivalence the kernel
    rests on; on a border-inconsistent atlas the two would differ, and one tile
    of such an atlas shows that the mutation is not an identity in general."""
    for name, case in CASES.items():
        a, b = model(name, "float64", "borders_of_window_only")[0], model(name, "float64")[0]
        assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])), name
    case = CASES["k4_r16_counts"]
    irr = case["irr"].copy()
    outside = [p for p in range(case["grid"].count) if p not in set(case["probes"].tolist())][0]
    tx, ty = M.tile_coord(case["grid"], [outside])
    irr[ty[0] * 10, tx[0] * 10 + 3, 0] ^= 0x0100  # a border texel that is not its source's copy
    args = (case["grid"], case["params"], case["surfels"], irr, case["vis"], case["offsets"], np.float64)
    assert not np.array_equal(M.update(*args, "borders_of_window_only")[0], M.update(*args)[0])
