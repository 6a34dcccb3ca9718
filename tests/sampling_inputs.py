"""Inputs of the DDGI read-side model tests (test infrastructure): cases designed texel by
texel so that every term of probeSampling.glsl:64-163 carries weight in the output.

A case is a dict: name, grid (ddgi.ProbeGrid), cfg, z_far, atlas (the name of its pair of
atlases; `atlases_of` gives their fp16 codes), width, height, camera, planes, flag_sets,
toleranced (False: only the class of the result is compared, test_sampling_model.py). Every
case has at most about 2,500 pixels.

Grid G1: dims (5, 3, 4), spacing (0.625, 0.5, 0.25), origin (-1.25, -1.0, 0.125): anisotropic,
the smallest spacing is z (minDistanceBetweenProbes != spacing.x), everything dyadic, and
z in [0.125, 0.875] lies inside the depth range, so the affine camera below maps the depth
plane to world z unchanged.

The affine camera: view_from_pixel maps (x + 0.5, y + 0.5, depth, 1) to
(a (x + 0.5) + b, c (y + 0.5) + d, depth, 1), the other two matrices are the identity. With
dyadic a, b, c, d the world position of a pixel is exact in fp32 and in fp64.
"""
from __future__ import annotations

import functools

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import compose_inputs as CI
import ddgi_sampling_model as M

G1 = D.ProbeGrid((5, 3, 4), (0.625, 0.5, 0.25), (-1.25, -1.0, 0.125))
G1_CFG = D.DDGIConfig(rays_per_probe=16, probe_updates_per_frame=60, max_rays_per_probe=16, max_probe_updates=60)
# case c: the features scene's room, same anisotropy (min spacing is y)
GC = D.ProbeGrid((6, 4, 5), (0.625, 0.5, 0.75), (-1.5, 0.25, -1.5))
GC_CFG = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=120, max_rays_per_probe=64, max_probe_updates=120,
                      clear_overflow_mode=abi.ARK_DDGI_CLEAR_OVERFLOW_MAX_FINITE)
Z_FAR = 100.0

FLAG_SETS = [  # test_gpu_compose.FLAG_SETS
    abi.ARK_COMPOSE_DEFAULT_FLAGS,
    abi.ARK_COMPOSE_DEFAULT_FLAGS & ~abi.ARK_COMPOSE_USE_BENT_NORMAL,
    abi.ARK_COMPOSE_DIFFUSE_GI,
    abi.ARK_COMPOSE_DIFFUSE_GI | abi.ARK_COMPOSE_USE_BENT_NORMAL | abi.ARK_COMPOSE_MATERIAL_COLOR,
    abi.ARK_COMPOSE_DIRECT_LIGHT | abi.ARK_COMPOSE_SKIN_DIFFUSE_LIGHT | abi.ARK_COMPOSE_GLOSSY_GI,
]
GI_ONLY = [abi.ARK_COMPOSE_DIFFUSE_GI]


def model_grid(grid):
    return M.Grid(grid.grid_dimensions, grid.probe_spacing, grid.offset_to_first)


def cell_diagonal(grid):
    return float(np.linalg.norm(np.asarray(grid.probe_spacing, np.float64)))


@functools.lru_cache(maxsize=None)
def atlases_a():
    """Random positive irradiance, every probe's tile around its own level (log-uniform over
    a factor of 30 between probes, so a wrong probe or tile shows), and a visibility mean
    between 0.2 and 1.5 cell diagonals with a finite variance, y = x^2 + positive noise."""
    rng = np.random.default_rng(2024)
    g = model_grid(G1)
    X, Y, Z = g.dims
    Hi, Wi, _ = g.atlas_shape(M.IRRADIANCE_RES, 4)
    level = np.exp(rng.uniform(np.log(0.05), np.log(1.5), (Z, X * Y, 3)))
    irr = np.repeat(np.repeat(level, 10, 0), 10, 1) * rng.uniform(0.6, 1.4, (Hi, Wi, 3))
    irr = np.concatenate([irr, np.ones((Hi, Wi, 1))], -1)
    Hv, Wv, _ = g.atlas_shape(M.VISIBILITY_RES, 2)
    diag = cell_diagonal(G1)
    mean = diag * (0.2 + 1.3 * rng.random((Hv, Wv)) ** 2)  # denser at the short end: more taps beyond the mean
    second = mean * mean + rng.uniform(0.005, 0.2, (Hv, Wv))
    vis = np.stack([mean, second], -1)
    return CI.f16(irr).reshape(-1), CI.f16(vis).reshape(-1)


@functools.lru_cache(maxsize=None)
def atlases_b():
    """Atlas a with planted texels: irradiance 0; variance +inf and NaN (the state after a
    first frame with the default clear); negative mean distance."""
    rng = np.random.default_rng(2025)
    irr, vis = (x.copy() for x in atlases_a())
    irr = irr.reshape(-1, 4)
    irr[rng.random(len(irr)) < 0.04, :3] = 0
    vis = vis.reshape(-1, 2)
    r = rng.random(len(vis))
    vis[r < 0.03, 1] = 0x7C00
    vis[(r >= 0.03) & (r < 0.06), 1] = 0x7E00
    vis[(r >= 0.06) & (r < 0.09), 0] |= 0x8000
    return irr.reshape(-1), vis.reshape(-1)


@functools.lru_cache(maxsize=None)
def oracle_c():
    """The oracle after two updates of the features scene with the max-finite clear: real,
    correlated atlases with y ~ x^2. Kept open: the tests compose on it."""
    import oracle_lib as O
    import scenes
    from parity import make_desc

    orc = O.Oracle(make_desc(GC, Z_FAR, GC_CFG))
    orc.set_scene(scenes.features_scene())
    for f in range(2):
        orc.update(D.frame_params(GC_CFG, GC, D.AppState(f), 0, light_pre_exposure=1.0, environment_brightness=0.5))
    return orc


@functools.lru_cache(maxsize=None)
def atlases_c():
    orc = oracle_c()
    return orc.read(abi.ARK_DDGI_ATLAS_IRRADIANCE), orc.read(abi.ARK_DDGI_ATLAS_VISIBILITY)


ATLASES = {"a": atlases_a, "b": atlases_b, "c": atlases_c}


def affine_camera(a, b, c, d):
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[0, 3], m[1, 1], m[1, 3], m[2, 2], m[3, 3] = a, b, c, d, 1.0, 1.0
    eye = np.eye(4, dtype=np.float32)
    col = lambda x: np.ascontiguousarray(x.T).reshape(16)  # noqa: E731  (column-major)
    return {"view_from_pixel": col(m), "view_from_world": col(eye), "world_from_view": col(eye)}


def affine_positions(cam, width, height, depth):
    """World positions of the affine camera's pixels in float64, with the check that fp32
    arithmetic gives the same (the property the planes sweep rests on)."""
    m = np.asarray(cam["view_from_pixel"], np.float32).reshape(4, 4).T
    px, py = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    x64 = m[0, 0].astype(np.float64) * px + m[0, 3].astype(np.float64)
    y64 = m[1, 1].astype(np.float64) * py + m[1, 3].astype(np.float64)
    x32 = m[0, 0] * px.astype(np.float32) + m[0, 3]
    y32 = m[1, 1] * py.astype(np.float32) + m[1, 3]
    return np.stack([x64, y64, np.asarray(depth, np.float64)], -1), bool(np.array_equal(x32, x64) and np.array_equal(y32, y64))


def _planes(width, height, seed, depth, sky_frac=0.1):
    g = CI.gbuffer(width, height, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    depth = np.asarray(depth, np.float32).copy()
    depth[rng.random((height, width)) < sky_frac] = 1.0
    g["depth"] = depth
    return g


def _case(name, grid, cfg, atlas, width, height, camera, planes, flag_sets=GI_ONLY, toleranced=True):
    return {"name": name, "grid": grid, "cfg": cfg, "z_far": Z_FAR, "atlas": atlas, "width": width, "height": height,
            "camera": camera, "planes": planes, "flag_sets": list(flag_sets), "toleranced": toleranced}


def atlases_of(case):
    return ATLASES[case["atlas"]]()


def _keep_off_planes(z, planes, margin):
    """Moves values closer than `margin` to a plane that far away from it."""
    z = z.copy()
    for p in planes:
        near = np.abs(z - p) < margin
        z[near] = p + margin * np.where(z[near] >= p, 1.0, -1.0)
    return z


Z_PLANES = [0.125, 0.375, 0.625, 0.875]


def interior(atlas, flag_sets=GI_ONLY, width=48, height=40, seed=21, a=1 / 16, c=1 / 32, name=None):
    """x, y at odd multiples of a / 2 (never on a plane: the planes are multiples of 1/8),
    spread over the grid's cells (and a little beyond it); z = depth spread through the grid."""
    rng = np.random.default_rng(seed)
    cam = affine_camera(a, -a * (width // 2), c, -0.5 - c * (height // 2))
    depth = _keep_off_planes(rng.uniform(0.13, 0.87, (height, width)), Z_PLANES, 0.25e-3).astype(np.float32)
    return _case(name or f"interior_{atlas}", G1, G1_CFG, atlas, width, height, cam, _planes(width, height, seed, depth), flag_sets)


def planes_case():
    """Columns exactly on the x planes (px = 4, 14, 24, 34, 44), rows exactly on the y planes
    (py = 4, 12, 20), a third of the pixels exactly on a z plane and a third one fp32 ulp
    beside one; a pixel whose x and y are both on a plane keeps a generic z (at least 1e-3
    cells from a probe)."""
    W, H, a = 48, 24, 1 / 16
    rng = np.random.default_rng(31)
    cam = affine_camera(a, -1.5 - a / 2, a, -1.25 - a / 2)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    on_x, on_y = np.isin(px, (4, 14, 24, 34, 44)), np.isin(py, (4, 12, 20))
    zp = np.asarray(Z_PLANES, np.float32)[(px + py) % 4]
    kind = (px + 2 * py) % 3
    generic = _keep_off_planes(rng.uniform(0.05, 0.95, (H, W)), Z_PLANES, 0.25e-3).astype(np.float32)
    beside = np.nextafter(zp, np.where((px + py) % 2 == 0, np.float32(2), np.float32(-2)).astype(np.float32))
    depth = np.where(kind == 0, zp, np.where(kind == 1, beside, generic))
    depth = np.where(on_x & on_y, generic, depth).astype(np.float32)
    return _case("planes_a", G1, G1_CFG, "a", W, H, cam, _planes(W, H, 31, depth))


def ulp_case(side):
    """The column px = 4 one fp32 ulp beside the x plane -0.625 and the row py = 3 one ulp
    beside the y plane -0.5 (`side` = +1 or -1), z one ulp beside a z plane or generic. The
    image covers no other x or y plane: there the offset would not be representable."""
    W, H, a = 9, 7, 1 / 16
    rng = np.random.default_rng(41 + side)
    tx = np.nextafter(np.float32(-0.625), np.float32(side * 2))
    ty = np.nextafter(np.float32(-0.5), np.float32(side * 2))
    b, d = np.float64(tx) - a * 4.5, np.float64(ty) + a * 3.5  # y runs downwards: a small, representable offset
    assert np.float32(b) == b and np.float32(d) == d
    cam = affine_camera(a, b, -a, d)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    zp = np.asarray(Z_PLANES, np.float32)[(px + py) % 4]
    beside = np.nextafter(zp, np.where((px + py) % 2 == 0, np.float32(2), np.float32(-2)).astype(np.float32))
    generic = _keep_off_planes(rng.uniform(0.05, 0.95, (H, W)), Z_PLANES, 0.25e-3).astype(np.float32)
    depth = np.where(((px + py) % 2 == 0) & ~((px == 4) & (py == 3)), beside, generic).astype(np.float32)
    return _case("ulp_plus_a" if side > 0 else "ulp_minus_a", G1, G1_CFG, "a", W, H, cam, _planes(W, H, 41 + side, depth, sky_frac=0.0))


def outside_case():
    """Positions beyond the grid on all six sides and past its corners: x in (-3, 3),
    y in (-3, 1), z in (0, 1), at odd multiples of 1/32 (never on a plane)."""
    W, H, a = 24, 16, 0.25
    rng = np.random.default_rng(51)
    cam = affine_camera(a, -3.0 + 1 / 32, a, -3.0 + 1 / 32)
    depth = _keep_off_planes(rng.uniform(0.004, 0.996, (H, W)), Z_PLANES, 0.25e-3).astype(np.float32)
    return _case("outside_a", G1, G1_CFG, "a", W, H, cam, _planes(W, H, 51, depth))


def perspective_case(atlas):
    """compose_inputs.camera: a divide by w that is not 1, rotated view and world matrices."""
    W, H = 40, 30
    rng = np.random.default_rng(61)
    if atlas == "c":
        grid, cfg, cam = GC, GC_CFG, CI.camera(W, H, eye=(0.3, 1.2, 2.2), target=(0.0, 0.9, 0.0))
        depth = rng.uniform(0.90, 0.97, (H, W))  # 1 to 3.2 units in front of the eye
    else:
        grid, cfg, cam = G1, G1_CFG, CI.camera(W, H, eye=(0.4, 0.3, 2.6), target=(0.0, -0.5, 0.5))
        depth = rng.uniform(0.942, 0.9625, (H, W))  # 1.7 to 2.6 units: through the grid
    return _case(f"perspective_{atlas}", grid, cfg, atlas, W, H, cam, _planes(W, H, 61, depth))


def at_probes_case():
    """Pixels exactly at probe positions: normalize(probePos - P) = normalize(0). Not
    toleranced: oracle and kernel must agree bitwise, the model in the class of result."""
    cam = affine_camera(0.625, -1.25 - 0.3125, 0.5, -1.0 - 0.25)
    px, py = np.meshgrid(np.arange(5), np.arange(3))
    depth = np.asarray(Z_PLANES, np.float32)[(px + py) % 4]
    return _case("at_probes_a", G1, G1_CFG, "a", 5, 3, cam, _planes(5, 3, 71, depth, sky_frac=0.0), toleranced=False)


def remap_case(width, height):
    """Tile-remap targets (test_gpu_sampling_model.py): the interior sweep at another size."""
    a = 1 / 32 if width > 1 else 1 / 16
    return interior("a", width=width, height=height, seed=81 + width, a=a, c=1 / 8 if height > 1 else 1 / 16, name=f"remap_{width}x{height}")


@functools.lru_cache(maxsize=None)
def compose_cases():
    return (interior("a", FLAG_SETS), interior("b"), planes_case(), ulp_case(+1), ulp_case(-1), outside_case(),
            perspective_case("a"), perspective_case("b"), perspective_case("c"), at_probes_case())


REMAP_SIZES = ((130, 9), (65, 5), (1, 1))


def probe_debug_samples(grid=G1):
    """Every probe of the grid with the 12 x 12 sphere samples. Checks in float64 that
    (pos + 1e-4 - origin) / spacing stays 1e-5 away from an integer, so the fp32 truncation
    of baseGridCoord cannot select another probe."""
    g = model_grid(grid)
    sphere = D.DDGIProbeDebug.sphere_samples(12, 12)
    n = grid.probe_count()
    probes = np.repeat(np.arange(n, dtype=np.uint32), len(sphere))
    dirs = np.tile(sphere, (n, 1))
    dirs[np.all(dirs == 0, axis=1)] = (0, 1, 0)
    rel = (M.probe_coord(g, np.arange(n)) * g.spacing(np.float64) + np.float64(np.float32(1e-4))) / g.spacing(np.float64)
    assert np.all(np.abs(rel - np.rint(rel)) >= 1e-5), "change the grid: a probe sits on a truncation boundary"
    return probes, dirs


DEBUG_MODES = ((abi.ARK_PROBE_DEBUG_IRRADIANCE, 0.01), (abi.ARK_PROBE_DEBUG_DISTANCE, 0.05), (abi.ARK_PROBE_DEBUG_DISTANCE2, 0.002))
DEBUG_ATLASES = ("a", "b")
