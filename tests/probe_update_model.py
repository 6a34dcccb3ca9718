"""numpy model of the DDGI write side, written from the shaders (test infrastructure).

What is restated, vectorised over the window's probes and a tile's texels, every function in
a `dtype` of np.float32 or np.float64 (the float32 instance rounds after every operation and
sums in ray order without contraction; the float64 one is the reference the oracle and the
HIP kernels are compared with). The integer hash states and the fp16 inputs are exact in both.

  common/random.glsl:17-66                 rand_xorshift, wang_hash, seedRandom, randomFloat,
                                           randomPointOnSphere
  common.glsl:4-7, :121-142                PI, TWO_PI, GOLDEN_RATIO, sphericalFibonacciSample,
                                           axisAngleRotate
  common/octahedral.glsl:12-41             signNotZero, octahedralDecode
  ddgi/common.glsl:12-67                   calculateRotatedSphericalFibonacciSample,
                                           calculateAtlasCoords, calculateAtlasTexelCoord
  ddgi/probeUpdateIrradiance.comp:22-79    main
  ddgi/probeUpdateVisibility.comp:24-64    main
  ddgi/probeBorderCopyCorners.comp:21-52   main
  ddgi/probeBorderCopyEdges.comp:23-58     main
  ddgi/probeUpdateOffset.comp:27-97        main
  DDGINode.cpp:132-259                     the order of the passes and their push constants

Calls nothing of the library or the oracle. One step at a time: the "old" texel of the blend
is always the planted one. The border pass covers all N tiles, as the shader's dispatch does
(DDGINode.cpp:209-233).

Rules of the model where GLSL leaves a result open (what the oracle and
the kernels do):
  - min(abs(NaN), maxDistance) = maxDistance (fmin: the operand that is not NaN);
  - pow(x < 0, y) = NaN for the non-integral exponents the write side uses, pow(0, y > 0) = 0,
    pow(+inf, y > 0) = +inf;
  - normalize(0) = 0 * inversesqrt(0) = 0 * inf = NaN in every component;
  - a NaN is stored as fp16 0x7e00, a value beyond 65520 as an infinity.

`mut` names one one-line mutation of the shaders (MUTATIONS): tests/test_probe_update_model.py
uses them to show that the inputs of tests/probe_update_inputs.py tell a wrong shader from a
right one. `stats`, when given, receives the counts the cases are designed for.
"""
from __future__ import annotations

import numpy as np

IRRADIANCE_RES = 8   # shared/DDGIData.h DDGI_IRRADIANCE_RES
VISIBILITY_RES = 16  # DDGI_VISIBILITY_RES
ATLAS_PADDING = 1    # DDGI_ATLAS_PADDING
PARAM_SPACING = 512  # ddgi/common.glsl:17

MUTATIONS = {
    "irradiance_weight_signed": "irradiance weight dot(texel, ray) without max(0, .) (probeUpdateIrradiance.comp:44)",
    "sharpness_plus_one": "visibility weight raised to sharpness + 1 (probeUpdateVisibility.comp:46)",
    "distance_unclamped": "surfel distance not clamped to maxDistance (:51)",
    "distance_signed": "min(distance, maxDistance) without abs (:51)",
    "square_before_clamp": "second moment from min(distance^2, maxDistance) (:51-53)",
    "epsilon_without_rays": "epsilon = 1e-9 without the ray count (:57, probeUpdateIrradiance.comp:52)",
    "gamma_2_2": "irradiance stored with exponent 1 / 2.2 instead of 1 / 5 (probeUpdateIrradiance.comp:57)",
    "mix_swapped": "mix(old, new, hysteresis) (probeUpdateIrradiance.comp:77, probeUpdateVisibility.comp:62)",
    "hystereses_exchanged": "irradiance blended with the visibility hysteresis and the reverse (DDGINode.cpp:176, :191)",
    "max_distance_from_min_spacing": "gridMaxSpacing from the smallest spacing (DDGINode.cpp:148)",
    "tile_column_x_plus_zX": "tile column x + z X instead of x + y X (ddgi/common.glsl:58)",
    "corner_source_off_by_one": "corner copied from the source corner itself, not the texel inside it (probeBorderCopyCorners.comp:41-44)",
    "edge_not_reversed": "edge copied in the same direction instead of mirrored (probeBorderCopyEdges.comp:49)",
    "borders_of_window_only": "borders copied for the window's tiles only (DDGINode.cpp:203 TODO); an identity on border-consistent inputs",
    "backface_threshold_strict": "back-face share > 0.25 instead of >= (probeUpdateOffset.comp:71)",
    "near_front_from_max_distance": "near front faces closer than 1.5 max spacing instead of maxOffset (:56)",
    "step_sign_flipped": "step away from the back faces instead of towards them (:72)",
    "offset_clamp_dropped": "new offset not clamped to maxOffset (:88-90)",
    "exp_for_exp2": "exp instead of exp2 in the lerp (:93)",
    "frame_not_wrapped": "seed from frameIdx instead of frameIdx % 512 (ddgi/common.glsl:18)",
    "fibonacci_n_minus_one": "spherical Fibonacci with i / (n - 1) (common.glsl:126)",
    "rotation_transposed": "rotation by the transposed matrix: the angle negated (common.glsl:141)",
}
# mutations that change nothing on border-consistent inputs, by argument (see the tests)
IDENTITIES = ("borders_of_window_only",)


def lit(x, T):
    """An fp32 literal or uniform of the shader as a value of dtype T."""
    return T(np.float32(x))


def texels(codes16, T):
    """fp16 texel codes (uint16) decoded exactly."""
    return np.asarray(codes16, np.uint16).view(np.float16).astype(T)


def to_f16_codes(a):
    """The RGBA16F / RG16F store: round to nearest even, a NaN as 0x7e00."""
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.asarray(a).astype(np.float16)
    c = h.view(np.uint16).copy()
    c[np.isnan(h)] = 0x7E00
    return c


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def length(a):
    return np.sqrt(dot(a, a))


def normalize(a):
    """v * inversesqrt(dot(v, v)); the zero vector gives 0 * inf = NaN."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = a.dtype.type(1) / np.sqrt(dot(a, a))
        return a * s[..., None]


def power(x, y):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.power(x, x.dtype.type(y))


def mix(x, y, a):
    """GLSL mix(x, y, a) = x * (1 - a) + y * a."""
    T = x.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        return x * (T(1) - a) + y * a


def sign_not_zero(f):  # octahedral.glsl:12-15
    T = f.dtype.type
    return np.where(f >= 0, T(1), T(-1))


def octahedral_decode(ox, oy):  # octahedral.glsl:35-41
    T = ox.dtype.type
    z = T(1) - np.abs(ox) - np.abs(oy)
    fx = (T(1) - np.abs(oy)) * sign_not_zero(ox)
    fy = (T(1) - np.abs(ox)) * sign_not_zero(oy)
    neg = z < 0
    return normalize(np.stack([np.where(neg, fx, ox), np.where(neg, fy, oy), z], -1))


# --- random.glsl -------------------------------------------------------------

def wang_hash(seed):  # :32-40
    seed = np.asarray(seed, np.uint32)
    with np.errstate(over="ignore"):
        seed = (seed ^ np.uint32(61)) ^ (seed >> np.uint32(16))
        seed = seed * np.uint32(9)
        seed = seed ^ (seed >> np.uint32(4))
        seed = seed * np.uint32(0x27D4EB2D)
        seed = seed ^ (seed >> np.uint32(15))
    return seed


def rand_xorshift(state):  # :17-24
    state = np.asarray(state, np.uint32)
    state = state ^ (state << np.uint32(13))
    state = state ^ (state >> np.uint32(17))
    state = state ^ (state << np.uint32(5))
    return state


def two_pi(T):
    return T(2) * lit(3.14159265358979323846, T)  # common.glsl:4-5, fp32 constants


def random_float(state, T):  # :50-53; float(uint) rounds to nearest in fp32
    state = rand_xorshift(state)
    return state, state.astype(T) * lit(1.0 / 4294967296.0, T)


def spherical_fibonacci(R, T, mut=None):  # common.glsl:121-130
    i = np.arange(R).astype(T)
    theta = two_pi(T) * i / lit(1.618034, T)
    n = T(R - 1) if mut == "fibonacci_n_minus_one" and R > 1 else T(R)
    with np.errstate(invalid="ignore"):
        phi = np.arccos(T(2) * (i / n) - T(1))
    sin_phi = np.sin(phi)
    return np.stack([np.cos(theta) * sin_phi, np.sin(theta) * sin_phi, np.cos(phi)], -1)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotated_fibonacci(probes, R, frame, T, mut=None):
    """calculateRotatedSphericalFibonacciSample for every (probe, sample): [K, R, 3]."""
    probes = np.asarray(probes, np.uint32)
    frame_term = np.uint32(frame) if mut == "frame_not_wrapped" else np.uint32(frame % PARAM_SPACING)
    with np.errstate(over="ignore"):
        state = wang_hash(np.uint32(PARAM_SPACING) * probes + frame_term)  # ddgi/common.glsl:18
    state, f = random_float(state, T)  # randomPointOnSphere, random.glsl:55-66
    theta = two_pi(T) * f
    state, f = random_float(state, T)
    u = T(2) * f - T(1)
    sr = np.sqrt(T(1) - u * u)
    axis = np.stack([sr * np.cos(theta), sr * np.sin(theta), u], -1)[:, None, :]  # [K, 1, 3]
    state, f = random_float(state, T)
    angle = two_pi(T) * f  # ddgi/common.glsl:22
    if mut == "rotation_transposed":
        angle = -angle
    s, c = np.sin(angle)[:, None, None], np.cos(angle)[:, None, None]
    v = spherical_fibonacci(R, T, mut)[None, :, :]  # [1, R, 3]
    # common.glsl:141: v * cosTheta + cross(k, v) * sinTheta + k * dot(k, v) * (1.0 - cosTheta)
    return v * c + cross(axis, v) * s + axis * dot(axis, v)[..., None] * (T(1) - c)


# --- grid and atlas addressing -----------------------------------------------

class Grid:
    """gridDimensions, probeSpacing, offsetToFirst (fp32 uniforms)."""

    def __init__(self, dims, spacing, origin):
        self.dims = tuple(int(d) for d in dims)
        self.spacing32 = np.asarray(spacing, np.float32)
        self.origin32 = np.asarray(origin, np.float32)

    @property
    def count(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def atlas_shape(self, res, channels):
        X, Y, Z = self.dims
        side = res + 2 * ATLAS_PADDING
        return (Z * side, X * Y * side, channels)


def tile_coord(grid, probe_idx, mut=None):
    """calculateAtlasCoords + probeAtlasTileCoord (ddgi/common.glsl:36-58): tile (column, row)."""
    X, Y, Z = grid.dims
    probe_idx = np.asarray(probe_idx, np.int64)
    sheet_probe = probe_idx % (X * Z)
    sheet = probe_idx // (X * Z)
    x, z = sheet_probe % X, sheet_probe // X
    if mut == "tile_column_x_plus_zX":
        return (x + z * X) % (X * Y), z  # (kept inside the atlas)
    return x + sheet * X, z


def window_probes(grid, first, K, shard=(0, 1)):
    """The window's probes by slot: slot s <-> probe (first + s) % N (probeUpdate*.comp:26-28).
    A Z-slab rank keeps the probes of its slab [r Z / P, (r + 1) Z / P), in window order at
    compacted slots."""
    X, Y, Z = grid.dims
    probes = (np.arange(min(K, grid.count)) + first % grid.count) % grid.count
    rank, world = shard
    if world > 1:
        z = (probes % (X * Z)) // X
        probes = probes[(z >= rank * (Z // world)) & (z < (rank + 1) * (Z // world))]
    return probes


def texel_directions(res, T):
    """octahedralDecode(2 * tileUV - 1) of every tile texel, index ty * res + tx."""
    t = (np.arange(res).astype(T) + T(0.5)) / T(res)
    c = T(2) * t - T(1)
    ox, oy = np.meshgrid(c, c)  # ox varies along tx
    return octahedral_decode(ox.reshape(-1), oy.reshape(-1))


def border_map(res, mut=None):
    """(dst y, dst x, src y, src x) of a tile's 4 res + 4 border texels, tile-local
    (probeBorderCopyCorners.comp, probeBorderCopyEdges.comp)."""
    side = res + 2 * ATLAS_PADDING
    rows = []
    for cy in range(2):  # corners :32-44
        for cx in range(2):
            sx, sy = (cx + 1) % 2, (cy + 1) % 2
            dX, dY = cx * (side - 1), cy * (side - 1)
            sX, sY = sx * (side - 1), sy * (side - 1)
            if mut != "corner_source_off_by_one":
                sX += 1 if sx == 0 else -1
                sY += 1 if sy == 0 else -1
            rows.append((dY, dX, sY, sX))
    corner = [(0, 0), (1, 0), (1, 1), (0, 1)]  # edges :32-49
    step_dir = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    for side_idx in range(4):
        ind = step_dir[(side_idx + 1) % 4]
        cX, cY = corner[side_idx][0] * (side - 1), corner[side_idx][1] * (side - 1)
        sdx, sdy = step_dir[side_idx]
        for step in range(res):
            dX, dY = cX + (step + 1) * sdx, cY + (step + 1) * sdy
            back = (step + 1) if mut == "edge_not_reversed" else (res - step)
            sX, sY = (cX + ind[0]) + back * sdx, (cY + ind[1]) + back * sdy
            rows.append((dY, dX, sY, sX))
    return np.asarray(rows, np.int64)


def copy_borders(grid, atlas, res, tiles=None, mut=None):
    """The border pass in place over `atlas` [H, W, C] (any dtype): all tiles, or `tiles`
    = (columns, rows)."""
    X, Y, Z = grid.dims
    side = res + 2 * ATLAS_PADDING
    if tiles is None:
        tx, ty = np.meshgrid(np.arange(X * Y), np.arange(Z))
        tiles = (tx.reshape(-1), ty.reshape(-1))
    m = border_map(res, mut)
    oy, ox = (np.asarray(tiles[1]) * side)[:, None], (np.asarray(tiles[0]) * side)[:, None]
    atlas[oy + m[:, 0], ox + m[:, 1]] = atlas[oy + m[:, 2], ox + m[:, 3]]
    return atlas


# --- the passes --------------------------------------------------------------

def _interior(res, tile_x, tile_y):
    """Atlas (row, column) of the tiles' interior texels, [K, res * res] each (calculateAtlasTexelCoord)."""
    side = res + 2 * ATLAS_PADDING
    ty, tx = np.divmod(np.arange(res * res), res)
    ay = ATLAS_PADDING + tile_y[:, None] * side + ty[None, :]
    ax = ATLAS_PADDING + tile_x[:, None] * side + tx[None, :]
    return ay, ax


def update(grid, params, surfels16, irr16, vis16, offsets, dtype, mut=None, stats=None, shard=(0, 1)):
    """One probe update, steps 3 to 6 of DDGINode.cpp:170-256.

    params: dict(frame, first, K, R, hysteresis_irradiance, hysteresis_visibility, sharpness,
    delta_time, update_offsets). surfels16: uint16 [slots, Rmax, 4] (the surfel image, slot
    major). irr16 / vis16: the pre-update atlases as fp16 codes. offsets: float32 [N, 4] (xyz
    used). Returns (irr codes [Hi, Wi, 4], vis codes [Hv, Wv, 2], offsets [N, 3] of `dtype`)."""
    T = dtype
    R = int(params["R"])
    probes = window_probes(grid, int(params["first"]), int(params["K"]), shard)
    K = len(probes)
    irr = np.array(irr16, np.uint16).reshape(grid.atlas_shape(IRRADIANCE_RES, 4))
    vis = np.array(vis16, np.uint16).reshape(grid.atlas_shape(VISIBILITY_RES, 2))
    off_out = np.asarray(offsets, np.float32).reshape(grid.count, 4)[:, :3].astype(T)
    st = stats if stats is not None else {}
    surf = texels(np.asarray(surfels16, np.uint16).reshape(-1, np.asarray(surfels16).shape[-2], 4)[:K, :R], T)  # [K, R, 4]
    rays = rotated_fibonacci(probes, R, int(params["frame"]), T, mut)  # [K, R, 3]
    h_irr, h_vis = lit(params["hysteresis_irradiance"], T), lit(params["hysteresis_visibility"], T)
    if mut == "hystereses_exchanged":
        h_irr, h_vis = h_vis, h_irr
    eps = lit(1e-9, T) if mut == "epsilon_without_rays" else lit(1e-9, T) * T(R)
    tile_x, tile_y = tile_coord(grid, probes, mut)
    spacing = grid.spacing32.astype(T)

    # probeUpdateIrradiance.comp
    tex = texel_directions(IRRADIANCE_RES, T)  # [64, 3]
    acc = np.zeros((K, tex.shape[0], 3), T)
    tw = np.zeros((K, tex.shape[0]), T)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(R):
            w = dot(tex[None, :, :], rays[:, s, None, :])  # :44
            if mut != "irradiance_weight_signed":
                w = np.fmax(T(0), w)
            acc = acc + w[..., None] * surf[:, s, None, :3]  # :48
            tw = tw + w  # :49
        st["irr_texels"] = st.get("irr_texels", 0) + tw.size
        st["irr_under_epsilon"] = st.get("irr_under_epsilon", 0) + int(np.count_nonzero(tw < eps))
        new = acc / np.fmax(tw, eps)[..., None]  # :53
        gamma = lit(1.0 / 2.2, T) if mut == "gamma_2_2" else lit(1.0, T) / lit(5.0, T)
        new = power(new, gamma)  # :57
        ay, ax = _interior(IRRADIANCE_RES, tile_x, tile_y)
        old = texels(irr[ay, ax, :3], T)  # :59
        new = mix(old, new, h_irr) if mut == "mix_swapped" else mix(new, old, h_irr)  # :77
    irr[ay, ax, :3] = to_f16_codes(new)
    irr[ay, ax, 3] = 0  # :78, vec4(newIrradiance, 0.0)

    # probeUpdateVisibility.comp
    tex = texel_directions(VISIBILITY_RES, T)  # [256, 3]
    grid_max = np.min(spacing) if mut == "max_distance_from_min_spacing" else np.max(spacing)  # DDGINode.cpp:148
    max_distance = T(1.5) * grid_max  # :50
    sharp = lit(params["sharpness"], T) + (T(1) if mut == "sharpness_plus_one" else T(0))
    dist = surf[..., 3]
    with np.errstate(invalid="ignore", over="ignore"):
        if mut == "distance_unclamped":
            d = np.abs(dist)
        elif mut == "distance_signed":
            d = np.fmin(dist, max_distance)
        else:
            d = np.fmin(np.abs(dist), max_distance)  # :51
        d2 = np.fmin(np.abs(dist) * np.abs(dist), max_distance) if mut == "square_before_clamp" else d * d
        st["rays"] = st.get("rays", 0) + dist.size
        st["clamped_distances"] = st.get("clamped_distances", 0) + int(np.count_nonzero(np.abs(dist) > max_distance))
        nv = np.zeros((K, tex.shape[0], 2), T)
        tw = np.zeros((K, tex.shape[0]), T)
        for s in range(R):
            w = power(np.fmax(T(0), dot(tex[None, :, :], rays[:, s, None, :])), sharp)  # :46
            nv = nv + w[..., None] * np.stack([d[:, s], d2[:, s]], -1)[:, None, :]  # :53
            tw = tw + w  # :54
        st["vis_texels"] = st.get("vis_texels", 0) + tw.size
        st["vis_under_epsilon"] = st.get("vis_under_epsilon", 0) + int(np.count_nonzero(tw < eps))
        st["vis_between_epsilons"] = st.get("vis_between_epsilons", 0) + int(np.count_nonzero((tw < lit(1e-9, T) * T(R)) & (tw > lit(1e-9, T))))
        new = nv / np.fmax(tw, eps)[..., None]  # :58
        ay, ax = _interior(VISIBILITY_RES, tile_x, tile_y)
        old = texels(vis[ay, ax], T)  # :61
        new = mix(old, new, h_vis) if mut == "mix_swapped" else mix(new, old, h_vis)  # :62
    vis[ay, ax] = to_f16_codes(new)

    # probeBorderCopyCorners.comp, probeBorderCopyEdges.comp: every tile (DDGINode.cpp:209-233)
    tiles = (tile_x, tile_y) if mut == "borders_of_window_only" else None
    copy_borders(grid, irr, IRRADIANCE_RES, tiles, mut)
    copy_borders(grid, vis, VISIBILITY_RES, tiles, mut)

    # probeUpdateOffset.comp
    if params["update_offsets"]:
        max_offset = np.min(spacing) / T(2)  # DDGINode.cpp:248-249
        near_limit = max_distance if mut == "near_front_from_max_distance" else max_offset
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            near = (dist > 0) & (dist < near_limit)  # :56, on the stored fp16 values
            back = ~near & (dist < 0)  # :59
            acc_near = np.zeros((K, 3), T)
            acc_back = np.zeros((K, 3), T)
            for s in range(R):  # :54-63, in ray order
                acc_near = acc_near + np.where(near[:, s, None], rays[:, s], T(0))
                acc_back = acc_back + np.where(back[:, s, None], rays[:, s], T(0))
            n_near, n_back = near.sum(1), back.sum(1)
            share = n_back.astype(T) / T(R)
            many_back = share > lit(0.25, T) if mut == "backface_threshold_strict" else share >= lit(0.25, T)  # :71
            some_near = ~many_back & (n_near >= 1)  # :76
            current = off_out[probes]
            step = lit(0.125, T)
            sign = T(-1) if mut == "step_sign_flipped" else T(1)
            offset = np.where(many_back[:, None], sign * normalize(acc_back) * step,
                              np.where(some_near[:, None], -(normalize(acc_near) * step), -(current * step)))  # :72-83
            new_off = current + offset  # :85
            clamp = length(new_off) > max_offset  # :88
            if mut != "offset_clamp_dropped":
                new_off = np.where(clamp[:, None], max_offset * normalize(new_off), new_off)  # :89
            x = -lit(10.0, T) * lit(params["delta_time"], T)
            new_off = mix(new_off, current, np.exp(x) if mut == "exp_for_exp2" else np.exp2(x))  # :93
        off_out[probes] = new_off
        st["branch_back"] = st.get("branch_back", 0) + int(many_back.sum())
        st["branch_near"] = st.get("branch_near", 0) + int(some_near.sum())
        st["branch_relax"] = st.get("branch_relax", 0) + int((~many_back & ~some_near).sum())
        st["clamped_offsets"] = st.get("clamped_offsets", 0) + int(clamp.sum())
        st["near_rays"] = st.get("near_rays", 0) + int(near.sum())
        st["back_rays"] = st.get("back_rays", 0) + int(back.sum())
        st["other_rays"] = st.get("other_rays", 0) + int(dist.size - near.sum() - back.sum())
        st["back_counts"] = st.get("back_counts", []) + [int(v) for v in n_back]
        st["branch"] = st.get("branch", []) + [int(v) for v in np.where(many_back, 0, np.where(some_near, 1, 2))]
        st["clamp"] = st.get("clamp", []) + [bool(v) for v in clamp]
        # how far a decision lies from its threshold, and how well the direction sums are conditioned
        taken = np.where(many_back[:, None], acc_back, acc_near)
        cnt = np.where(many_back, n_back, n_near)
        with np.errstate(invalid="ignore", divide="ignore"):
            st["sum_condition"] = st.get("sum_condition", []) + [float(v) for v in np.where(cnt > 0, length(taken) / np.maximum(cnt, 1), np.inf)]
            st["clamp_margin"] = st.get("clamp_margin", []) + [float(v) for v in np.abs(length(current + offset) - max_offset) / max_offset]
    return irr, vis, off_out
