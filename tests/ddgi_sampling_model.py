"""numpy model of the DDGI read side, written from the shaders (test infrastructure).

What is restated, vectorised over pixels, every function in a `dtype` of np.float32 or
np.float64 (the float32 instance rounds after every operation, the float64 one is the
reference the oracle and the HIP kernels are compared with):

  common/octahedral.glsl:12-41            signNotZero, octahedralEncode, octahedralDecode
  ddgi/probeSampling.glsl:9-27            calculateAtlasSampleUV
  ddgi/probeSampling.glsl:52-62           baseGridCoord, gridCoordToPosition
  ddgi/probeSampling.glsl:64-163          sampleDynamicDiffuseGlobalIllumination
  lighting/lightingCompose.comp:45-153    main, WITH_DDGI = 1
  common/camera.glsl:101-106              unprojectPixelCoordAndDepthToViewSpace
  common/brdf.glsl:24-30, :70-89, :127    F_Schlick, specularBRDF's F, diffuseBRDF
  ddgi/probeDebug.frag:23-45              the three visualisations
  ddgi/common.glsl:69-77                  calculateProbePosition

Rules of the model:
  - a constant the shader writes as an fp32 literal is that fp32 value in both dtypes (`lit`);
  - comparisons on unrounded inputs (depth < 1 - 1e-6, bentCone >= 0) are made on the stored
    values, so they are exact in both dtypes;
  - max / min / clamp return the operand that is not NaN (fmax / fmin), pow(0, y > 0) = 0,
    normalize(0) = 0 * inf = NaN, a NaN is stored as 0x7e00;
  - the atlas fetch is linear, clamp-to-edge, LOD 0, over fp16 texels decoded exactly, as
    a + (b - a) t, x first.

`mut` names one one-line mutation of the shader (MUTATIONS): tests/test_sampling_model.py
uses them to show that the inputs of tests/sampling_inputs.py tell a wrong shader from a
right one. `stats`, when given, receives the shares the cases are designed for.
"""
from __future__ import annotations

import numpy as np

IRRADIANCE_RES = 8   # shared/DDGIData.h DDGI_IRRADIANCE_RES
VISIBILITY_RES = 16  # DDGI_VISIBILITY_RES
ATLAS_PADDING = 1    # DDGI_ATLAS_PADDING
IRRADIANCE_GAMMA = 5.0  # DDGI_IRRADIANCE_GAMMA

# ARK_COMPOSE_* (include/ark_ddgi.h), the shader's `constants`
DIRECT_LIGHT, SKIN_DIFFUSE_LIGHT, DIFFUSE_GI, BAKED_OCCLUSION = 1 << 0, 1 << 1, 1 << 2, 1 << 3
USE_BENT_NORMAL, BENT_NORMAL_OCCLUSION, SCREEN_SPACE_OCCLUSION, GLOSSY_GI, MATERIAL_COLOR = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8

DEBUG_IRRADIANCE, DEBUG_DISTANCE, DEBUG_DISTANCE2 = 1, 2, 3

MUTATIONS = {
    "wrap_shading_weight": "the #else wrap-shading weight instead of the smooth back-face weight (:104-115)",
    "offset_bits_xz_swapped": "probe coordinate from offset bits with x and z swapped, trilinear weight from the right ones (:81)",
    "tile_coord_x_plus_zX": "tile coordinate (x + z X, y) instead of (x + y X, z) (:12)",
    "neighbour_wraps": "neighbour coordinate wraps at the grid edge instead of clamping (:81)",
    "no_trilinear_floor": "trilinear floor 0.001 removed (:86)",
    "min_spacing_is_x": "minDistanceBetweenProbes = probeSpacing.x (:92)",
    "bias_weights_swapped": "selfShadowBias from 0.8 N + 0.2 V (:93)",
    "visibility_along_plus_dir": "visibility sampled along +directionToProbe (:119)",
    "backface_from_biased_dir": "back-face weight from the biased direction (:108)",
    "chebyshev_squared": "Chebyshev weight squared instead of cubed (:127)",
    "no_chebyshev_floor": "the 0.05 floor removed (:130)",
    "no_crush": "crush removed (:139-141)",
    "gamma_exponent_5": "decode exponent 5 instead of 2.5, final square kept (:149)",
    "no_half_texel": "bilinear fetch without the half-texel offset",
    "unnormalised_bent_normal": "bent normal passed on without the division by its length (lightingCompose.comp:117)",
    "fudge_always": "F and metallic applied without hasReflections (lightingCompose.comp:143)",
    "no_baked_occlusion": "baked occlusion ignored (lightingCompose.comp:80-82)",
    "debug_exponent_2_5": "the debug view's irradiance exponent 2.5 (probeSampling.glsl:40)",
}


def lit(x, T):
    """An fp32 literal of the shader as a value of dtype T."""
    return T(np.float32(x))


def pi(T):
    return lit(3.14159265358979323846, T)  # common.glsl:4 PI, an fp32 constant


def texels(codes16, T):
    """fp16 texel codes (uint16) decoded exactly."""
    return np.asarray(codes16, np.uint16).view(np.float16).astype(T)


def to_f16_codes(a):
    """The RGBA16F store: round to nearest even, a NaN as 0x7e00."""
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
    with np.errstate(divide="ignore", invalid="ignore"):
        s = a.dtype.type(1) / np.sqrt(dot(a, a))
        return a * s[..., None]


def clamp(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def power(x, y):
    """pow(x, y): pow(0, y > 0) = 0; a negative base with an integral exponent is defined
    (DESIGN §5 item 11)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.power(x, x.dtype.type(y))


def sign_not_zero(f):  # octahedral.glsl:12-20
    T = f.dtype.type
    return np.where(f >= 0, T(1), T(-1))


def octahedral_encode(v):  # octahedral.glsl:23-31
    T = v.dtype.type
    l1norm = np.abs(v[..., 0]) + np.abs(v[..., 1]) + np.abs(v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = T(1) / l1norm
        rx, ry = v[..., 0] * inv, v[..., 1] * inv
        fx = (T(1) - np.abs(ry)) * sign_not_zero(rx)
        fy = (T(1) - np.abs(rx)) * sign_not_zero(ry)
    neg = v[..., 2] < 0
    return np.where(neg, fx, rx), np.where(neg, fy, ry)


def octahedral_decode(ox, oy):  # octahedral.glsl:35-41
    T = ox.dtype.type
    z = T(1) - np.abs(ox) - np.abs(oy)
    fx = (T(1) - np.abs(oy)) * sign_not_zero(ox)
    fy = (T(1) - np.abs(ox)) * sign_not_zero(oy)
    neg = z < 0
    return normalize(np.stack([np.where(neg, fx, ox), np.where(neg, fy, oy), z], -1))


def fetch_linear(tex, u, v, half_texel=True):
    """texture(): linear, clamp to edge, LOD 0. tex: [H, W, C] texels already decoded."""
    T = tex.dtype.type
    H, W = tex.shape[:2]
    off = T(0.5) if half_texel else T(0)
    x, y = u * T(W) - off, v * T(H) - off
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f)[..., None], (y - y0f)[..., None]
    x0, y0 = np.nan_to_num(x0f).astype(np.int64), np.nan_to_num(y0f).astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        top = tex[ya, xa] + (tex[ya, xb] - tex[ya, xa]) * fx
        bot = tex[yb, xa] + (tex[yb, xb] - tex[yb, xa]) * fx
        return top + (bot - top) * fy


class Grid:
    """DDGIProbeGridData: gridDimensions, probeSpacing, offsetToFirst (fp32 uniforms)."""

    def __init__(self, dims, spacing, origin):
        self.dims = tuple(int(d) for d in dims)
        self.spacing32 = np.asarray(spacing, np.float32)
        self.origin32 = np.asarray(origin, np.float32)

    def spacing(self, T):
        return self.spacing32.astype(T)

    def origin(self, T):
        return self.origin32.astype(T)

    def atlas_shape(self, res, channels):
        X, Y, Z = self.dims
        side = res + 2 * ATLAS_PADDING
        return (Z * side, X * Y * side, channels)


def atlas_sample_uv(grid, coord, direction, res, mut=None):  # probeSampling.glsl:9-27
    T = direction.dtype.type
    X, Y, Z = grid.dims
    if mut == "tile_coord_x_plus_zX":
        tile_x, tile_y = coord[..., 0] + coord[..., 2] * X, coord[..., 1]
    else:
        tile_x, tile_y = coord[..., 0] + coord[..., 1] * X, coord[..., 2]  # :12
    side = res + 2 * ATLAS_PADDING
    first_x, first_y = ATLAS_PADDING + tile_x * side, ATLAS_PADDING + tile_y * side  # :15
    ex, ey = octahedral_encode(direction)
    tx = (ex * T(0.5) + T(0.5)) * T(res)  # :18
    ty = (ey * T(0.5) + T(0.5)) * T(res)
    ax, ay = first_x.astype(T) + tx, first_y.astype(T) + ty  # :21
    H, W, _ = grid.atlas_shape(res, 1)
    return ax * (T(1) / T(W)), ay * (T(1) / T(H))  # :24, invAtlasTextureSize = 1 / textureSize


def base_grid_coord(grid, position):  # probeSampling.glsl:52-57
    T = position.dtype.type
    rel = (position - grid.origin(T)) / grid.spacing(T)
    c = np.trunc(np.nan_to_num(rel)).astype(np.int64)  # ivec3(): toward zero
    return np.clip(c, 0, np.asarray(grid.dims) - 1), rel


def grid_coord_to_position(grid, coord, T):  # probeSampling.glsl:59-62
    return grid.origin(T) + coord.astype(T) * grid.spacing(T)


def sample_ddgi(grid, irr, vis, P, N, V, mut=None, stats=None):
    """sampleDynamicDiffuseGlobalIllumination (probeSampling.glsl:64-163). irr [Hi, Wi, 4] and
    vis [Hv, Wv, 2] are decoded atlases; P, N, V are [n, 3]."""
    T = P.dtype.type
    dims = np.asarray(grid.dims)
    spacing = grid.spacing(T)
    base, rel = base_grid_coord(grid, P)  # :67
    base_pos = grid_coord_to_position(grid, base, T)  # :68
    sum_irr = np.zeros(P.shape, T)
    sum_w = np.zeros(P.shape[0], T)
    alpha = clamp((P - base_pos) / spacing, T(0), T(1))  # :74
    half = mut != "no_half_texel"
    n_weighted = n_crushed = 0
    for i in range(8):
        offset = np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])  # :80
        # swapped in :81 alone: swapped in :80, for :81 and :86 alike, the bits only reorder the sum
        coord_offset = offset[::-1] if mut == "offset_bits_xz_swapped" else offset
        if mut == "neighbour_wraps":
            coord = (base + coord_offset) % dims
        else:
            coord = np.clip(base + coord_offset, 0, dims - 1)  # :81
        off = offset.astype(T)
        tri = (T(1) - alpha) * (T(1) - off) + alpha * off  # mix(1 - alpha, alpha, offset)
        if mut != "no_trilinear_floor":
            tri = np.fmax(lit(0.001, T), tri)  # :86
        trilinear = tri[..., 0] * tri[..., 1] * tri[..., 2]  # :87
        weight = np.ones(P.shape[0], T)  # :89
        shadow_bias = lit(0.3, T)  # :91
        min_dist = spacing[0] if mut == "min_spacing_is_x" else np.fmin(spacing[0], np.fmin(spacing[1], spacing[2]))  # :92
        wn, wv = (lit(0.8, T), lit(0.2, T)) if mut == "bias_weights_swapped" else (lit(0.2, T), lit(0.8, T))
        bias = (N * wn + V * wv) * (lit(0.75, T) * min_dist) * shadow_bias  # :93
        biased = P + bias  # :94
        probe_pos = grid_coord_to_position(grid, coord, T)  # :99
        to_probe = probe_pos - biased  # :100
        dir_to_probe = normalize(to_probe)  # :101
        unbiased_dir = normalize(probe_pos - P)  # :103
        backface_dir = dir_to_probe if mut == "backface_from_biased_dir" else unbiased_dir
        if mut == "wrap_shading_weight":
            w = (dot(backface_dir, N) + T(1)) * T(0.5)
            weight = weight * (w * w + lit(0.2, T))  # :114
        else:
            floor_ = lit(0.02, T)  # :106
            weight = weight * (floor_ + (T(1) - floor_) * power(clamp(dot(backface_dir, N), T(0), T(1)), 0.25))  # :108
        vis_dir = dir_to_probe if mut == "visibility_along_plus_dir" else -dir_to_probe
        u, v = atlas_sample_uv(grid, coord, vis_dir, VISIBILITY_RES, mut)
        vd = fetch_linear(vis, u, v, half)  # :119
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            mean = vd[..., 0]  # :120
            variance = np.abs(vd[..., 1] - mean * mean)  # :121
            dist = length(to_probe)  # :122
            taken = dist > mean  # :125
            d = dist - mean
            cheb = variance / (variance + d * d)  # :126
            cheb = cheb * cheb if mut == "chebyshev_squared" else cheb * cheb * cheb  # :127
            cheb = np.where(taken, cheb, T(1))
            if mut != "no_chebyshev_floor":
                cheb = np.fmax(lit(0.05, T), cheb)  # :130
            weight = weight * cheb  # :131
            weight = np.fmax(lit(0.000001, T), weight)  # :135
            crush = lit(0.2, T)  # :138
            crushed = weight < crush  # :139
            if mut != "no_crush":
                weight = np.where(crushed, weight * ((weight * weight) * (T(1) / (crush * crush))), weight)  # :140
            weight = weight * trilinear  # :143
        n_weighted += int(np.count_nonzero(taken & np.isfinite(variance)))
        n_crushed += int(np.count_nonzero(crushed))
        u, v = atlas_sample_uv(grid, coord, normalize(N), IRRADIANCE_RES, mut)
        probe_irr = fetch_linear(irr, u, v, half)[..., :3]  # :146
        exponent = IRRADIANCE_GAMMA if mut == "gamma_exponent_5" else IRRADIANCE_GAMMA * 0.5
        probe_irr = power(probe_irr, exponent)  # :149
        with np.errstate(invalid="ignore", over="ignore"):
            sum_irr = sum_irr + weight[..., None] * probe_irr  # :151
            sum_w = sum_w + weight  # :152
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out = sum_irr / sum_w[..., None]  # :155
        out = out * out  # :158
        out = out * (T(0.5) * pi(T))  # :160
    if stats is not None:
        stats["taps"] = stats.get("taps", 0) + 8 * P.shape[0]
        stats["weighted_taps"] = stats.get("weighted_taps", 0) + n_weighted
        stats["crushed_taps"] = stats.get("crushed_taps", 0) + n_crushed
        outside = np.any((rel < 0) | (rel >= (dims - 1)), axis=-1)
        stats["positions"] = stats.get("positions", 0) + P.shape[0]
        stats["clamped_positions"] = stats.get("clamped_positions", 0) + int(np.count_nonzero(outside))
    return out


def _mat(m, T):
    """Column-major float[16] -> [4, 4] with M[r, c]."""
    return np.asarray(m, np.float32).reshape(4, 4).T.astype(T)


def _mul_dir(M, v):  # mat3(M) * v
    return np.stack([M[r, 0] * v[..., 0] + M[r, 1] * v[..., 1] + M[r, 2] * v[..., 2] for r in range(3)], -1)


def _mul_point(M, x, y, z, w):  # M * vec4
    return [M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] * w for r in range(4)]


SKY_THRESHOLD = np.float32(1.0) - np.float32(1e-6)  # `1.0 - 1e-6`, folded in fp32


def lighting_compose(grid, irr16, vis16, width, height, flags, camera, planes, dtype, mut=None, stats=None):
    """lightingCompose.comp main() for every pixel; returns the colour before the RGBA16F
    store as [H, W, 4] of `dtype` (to_f16_codes gives the stored texels). An absent plane
    reads 0 (the node's black stand-ins)."""
    T = dtype
    n = width * height
    irr = texels(np.asarray(irr16).reshape(grid.atlas_shape(IRRADIANCE_RES, 4)), T)
    vis = texels(np.asarray(vis16).reshape(grid.atlas_shape(VISIBILITY_RES, 2)), T)

    def half4(name):
        p = planes.get(name)
        return np.zeros((n, 4), T) if p is None else texels(p, T).reshape(n, 4)

    def unorm4(name):
        p = planes.get(name)
        return np.zeros((n, 4), T) if p is None else np.asarray(p).reshape(n, 4).astype(T) / T(255)

    base_color = unorm4("base_color")[:, :3] if flags & MATERIAL_COLOR else np.ones((n, 3), T)  # :51-54
    direct = half4("direct_light") if flags & DIRECT_LIGHT else np.zeros((n, 4), T)  # :56-60
    rgb, alpha_out = direct[:, :3].copy(), direct[:, 3].copy()
    if flags & SKIN_DIFFUSE_LIGHT:  # :62-65, diffuseBRDF() = vec3(1) / vec3(PI)
        rgb = rgb + half4("diffuse_irradiance")[:, :3] * base_color * (T(1) / pi(T))
    ao = np.ones(n, T)  # :67-70
    if flags & SCREEN_SPACE_OCCLUSION and planes.get("screen_space_occlusion") is not None:
        ao = np.asarray(planes["screen_space_occlusion"], np.float32).reshape(n).astype(T)
    depth32 = np.zeros(n, np.float32) if planes.get("depth") is None else np.asarray(planes["depth"], np.float32).reshape(n)
    lit_px = np.nonzero(depth32 < SKY_THRESHOLD)[0]  # :73, on the stored values
    if lit_px.size:
        s = lit_px
        material = unorm4("material")[s]  # :75-78
        metallic, occlusion = material[:, 1], material[:, 2]
        a = ao[s]
        if flags & BAKED_OCCLUSION and mut != "no_baked_occlusion":
            a = np.fmin(a, occlusion)  # :80-82
        refl = half4("reflections")[s, :3]  # :84-85
        rdir = half4("reflection_direction")[s, :3]
        has_refl = dot(rdir, rdir) > lit(1e-4, T)  # :89
        px = (s % width).astype(T) + T(0.5)  # camera.glsl:103, pixelCoord + vec2(0.5)
        py = (s // width).astype(T) + T(0.5)
        vp = _mul_point(_mat(camera["view_from_pixel"], T), px, py, depth32[s].astype(T), T(1))
        pos = np.stack([vp[0] / vp[3], vp[1] / vp[3], vp[2] / vp[3]], -1)  # camera.glsl:104
        V = -normalize(pos)  # :94
        nv = half4("normal_velocity")[s]
        N = octahedral_decode(nv[:, 0], nv[:, 1])  # :95, encoding.glsl:17-20
        L = _mul_dir(_mat(camera["view_from_world"], T), rdir)  # :96
        Hv = normalize(L + V)  # brdf.glsl:72
        LdotH = clamp(dot(L, Hv), T(0), T(1))  # brdf.glsl:77
        f0 = lit(0.04, T) * (T(1) - metallic)[:, None] + base_color[s] * metallic[:, None]  # brdf.glsl:82, mix
        F = f0 + (T(1) - f0) * power(T(1) - LdotH, 5.0)[:, None]  # brdf.glsl:28-30
        c = rgb[s]
        if flags & GLOSSY_GI:  # :101-105
            c = np.where(has_refl[:, None], c + base_color[s] * refl * T(0.25), c)
        if flags & DIFFUSE_GI:  # :108-148
            bent = half4("bent_normal")[s]
            use_bent = (bent[:, 3] >= 0) if flags & USE_BENT_NORMAL else np.zeros(s.size, bool)  # :114
            W_ = _mat(camera["world_from_view"], T)
            with np.errstate(invalid="ignore", divide="ignore"):
                blen = length(bent[:, :3])  # :116
                bdir = bent[:, :3] if mut == "unnormalised_bent_normal" else bent[:, :3] / blen[:, None]  # :117
            ndir = normalize(_mul_dir(W_, N))  # :122
            sample_dir = np.where(use_bent[:, None], bdir, ndir)
            if flags & BENT_NORMAL_OCCLUSION:
                a = np.where(use_bent, np.fmin(a, blen), a)  # :118-120
            wp = _mul_point(W_, pos[:, 0], pos[:, 1], pos[:, 2], T(1))  # :126
            wpos = np.stack(wp[:3], -1)
            wview = normalize(_mul_dir(W_, V))  # :127
            gi = sample_ddgi(grid, irr, vis, wpos, sample_dir, wview, mut, stats)  # :129-135
            fudge = np.ones(s.size, T) if mut == "fudge_always" else has_refl.astype(T)  # :143
            with np.errstate(invalid="ignore", over="ignore"):
                diffuse = base_color[s] * (T(1) - metallic * fudge)[:, None] * (T(1) - F * fudge[:, None])  # :145
                c = c + diffuse * gi * a[:, None]  # :147
        rgb[s] = c
    return np.concatenate([rgb, alpha_out[:, None]], -1).reshape(height, width, 4)  # :152


def probe_coord(grid, probe_idx):
    """ddgi/common.glsl calculateAtlasCoords + :74: x fastest, then z, then y (sheets)."""
    X, Y, Z = grid.dims
    probe_idx = np.asarray(probe_idx, np.int64)
    sheet = probe_idx % (X * Z)
    return np.stack([sheet % X, probe_idx // (X * Z), sheet // X], -1)


def probe_debug(grid, irr16, vis16, mode, distance_scale, probes, dirs, dtype, mut=None):
    """probeDebug.frag:23-45 on (probe, normal) samples; returns [n, 4] of `dtype`."""
    T = dtype
    irr = texels(np.asarray(irr16).reshape(grid.atlas_shape(IRRADIANCE_RES, 4)), T)
    vis = texels(np.asarray(vis16).reshape(grid.atlas_shape(VISIBILITY_RES, 2)), T)
    d = normalize(np.asarray(dirs, np.float32).astype(T))  # :25
    pos = grid.origin(T) + probe_coord(grid, probes).astype(T) * grid.spacing(T)  # ddgi/common.glsl:76
    coord, _ = base_grid_coord(grid, pos + lit(1e-4, T))  # :26
    u, v = atlas_sample_uv(grid, coord, d, IRRADIANCE_RES)
    exponent = IRRADIANCE_GAMMA * 0.5 if mut == "debug_exponent_2_5" else IRRADIANCE_GAMMA
    irradiance = power(fetch_linear(irr, u, v)[..., :3], exponent)  # :28, probeSampling.glsl:38-41
    u, v = atlas_sample_uv(grid, coord, d, VISIBILITY_RES)
    visibility = fetch_linear(vis, u, v)  # :29
    scale = lit(distance_scale, T)
    out = np.ones((len(d), 4), T)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == DEBUG_IRRADIANCE:  # :32-34
            out[:, :3] = irradiance
        elif mode == DEBUG_DISTANCE:  # :35-38
            out[:, :3] = (scale * visibility[:, 0])[:, None]
            out[visibility[:, 0] < 0, :3] = (1, 0, 1)
        elif mode == DEBUG_DISTANCE2:  # :39-41
            out[:, :3] = (scale * visibility[:, 1])[:, None]
        else:
            out[:, :3] = (1, 0, 1)  # :44
    return out
