"""k_probe_update and k_probe_offsets against oracle_blend (bit for bit) and against the float64
model of the write side (tests/probe_update_model.py), on the planted inputs of
tests/probe_update_inputs.py through ark_ddgi_debug_probe_update, with the constants
tests/test_probe_update_model.py measured on the CPU (the model's precision, never the
kernel's). The two real-update tests at the end use ark_ddgi_update only.
"""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import probe_update_inputs as PI
import probe_update_model as M
import test_probe_update_model as T

pytestmark = pytest.mark.gpu

CASES = T.CASES
POISON = 0x5555  # 85.3: no irradiance (at most 65504 ^ 0.2 = 9.2, alpha 0) or visibility (at most 1.5 and 2.25) channel of a case
ATLASES = ((abi.ARK_DDGI_ATLAS_IRRADIANCE, "irr", M.IRRADIANCE_RES), (abi.ARK_DDGI_ATLAS_VISIBILITY, "vis", M.VISIBILITY_RES))


def planted_context(case, irr=None, vis=None):
    ctx = D.DDGIContext(PI.probe_grid(case), case["z_far"], PI.config(case), 0, case["shard"][0], case["shard"][1])
    ctx.write(abi.ARK_DDGI_SURFELS, case["surfels"])
    ctx.write(abi.ARK_DDGI_ATLAS_IRRADIANCE, case["irr"] if irr is None else irr)
    ctx.write(abi.ARK_DDGI_ATLAS_VISIBILITY, case["vis"] if vis is None else vis)
    ctx.write(abi.ARK_DDGI_PROBE_OFFSETS, case["offsets"])
    return ctx


@functools.lru_cache(maxsize=None)
def gpu_blend(name):
    case = CASES[name]
    ctx = planted_context(case)
    ctx.debug_probe_update(PI.frame_params(case), case["hits"] if case["params"]["update_offsets"] else None)
    ctx.synchronize()
    out = T.read_all(ctx)
    assert ctx.next_probe_index() == 0  # the rolling window did not advance
    ctx.close()
    return out


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.dtype == np.uint16:
        return bool(np.all((a == b) | (T.is_nan16(a) & T.is_nan16(b))))
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_equal_oracle_blend(name):
    got, want = gpu_blend(name), T.oracle_blend(name)
    for what, g, w in zip(("irradiance", "visibility", "offsets"), got, want):
        assert same_bits(g, w), f"{name}: {what} differs from oracle_blend in {np.count_nonzero(np.asarray(g) != np.asarray(w))} elements"
    assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[1]) > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_against_model(name):
    fig, bad = T.compare(CASES[name], gpu_blend(name), T.model(name, "float64")[0])
    T.report(f"{name} kernels", fig)
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["params"]["hysteresis_irradiance"] == 0.0 and c["params"]["hysteresis_visibility"] == 0.0))
def test_every_window_texel_is_written_and_no_other(name):
    """Hysteresis 0: the old texel has weight 0, so a finite pattern planted over the window's
    tiles (interior and border) must be gone afterwards; every other tile keeps its bytes."""
    case = CASES[name]
    planted = {}
    for _, key, res in ATLASES:
        a = case[key].copy()
        a[PI.window_mask(case, res)] = POISON
        planted[key] = a
    ctx = planted_context(case, planted["irr"], planted["vis"])
    ctx.debug_probe_update(PI.frame_params(case), case["hits"])
    ctx.synchronize()
    for which, key, res in ATLASES:
        got = ctx.read(which).reshape(planted[key].shape)
        mask = PI.window_mask(case, res)
        assert mask.any() and not np.any(got[mask] == POISON), f"{name} {key}: {np.count_nonzero(got[mask] == POISON)} channels of the window still hold the pattern"
        assert np.array_equal(got[~mask], planted[key][~mask]), f"{name} {key}: a tile outside the window changed"
    ctx.close()


def real_update(case, scene):
    """ark_ddgi_update on planted atlases and offsets; returns (surfels, (irr, vis, offsets))."""
    ctx = D.DDGIContext(PI.probe_grid(case), case["z_far"], PI.config(case))
    ctx.set_scene(scene)
    for which, key in ((abi.ARK_DDGI_ATLAS_IRRADIANCE, "irr"), (abi.ARK_DDGI_ATLAS_VISIBILITY, "vis"), (abi.ARK_DDGI_PROBE_OFFSETS, "offsets")):
        ctx.write(which, case[key])
    ctx.update(PI.frame_params(case))
    ctx.synchronize()
    surfels = ctx.read(abi.ARK_DDGI_SURFELS).reshape(case["kmax"], case["rmax"], 4)
    out = T.read_all(ctx)
    ctx.close()
    return surfels, out


def test_debug_entry_equals_a_real_update():
    """The new entry against the update it is cut from: a real update with offsets off, then its
    surfels and the same pre-update atlases planted in a second context (which has no scene)."""
    case, scene = T.real_surfel_case(0)
    surfels, want = real_update(case, scene)
    assert np.count_nonzero(surfels[..., :3]) > 0
    ctx = planted_context(dict(case, surfels=surfels))
    ctx.debug_probe_update(PI.frame_params(case))
    ctx.synchronize()
    got = T.read_all(ctx)
    ctx.close()
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


@pytest.mark.parametrize("offsets_on", [0, 1])
def test_real_update_against_model(offsets_on):
    """ark_ddgi_update alone (none of the debug entry's code): planted atlases and offsets, the
    surfels read back, the step modelled from the planted state."""
    case, scene = T.real_surfel_case(offsets_on)
    surfels, got = real_update(case, scene)
    assert np.count_nonzero(surfels[..., :3]) > 0 and len(set(surfels[..., 3].reshape(-1).tolist())) > 50
    want = M.update(case["grid"], case["params"], surfels, case["irr"], case["vis"], case["offsets"], np.float64)
    fig, bad = T.compare(case, got, want)
    T.report(f"{case['name']} kernels", fig)
    assert not bad, bad
