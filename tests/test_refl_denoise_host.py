"""The host restatement of the reflection denoiser passes (csrc/refl_denoise.h,
refl_denoise_host.cpp; ark_ddgi_debug_refl_denoise_host) without a GPU: known answers of the
shared functions, and the four passes against a numpy model written from the shader text
(historyCopy.comp, reproject.comp, prefilter.comp, resolveTemporal.comp and the ffx headers),
vectorised over the image, which rounds to fp16 exactly where the shaders pack or store.

The bound. The restatement evaluates fp32 in the shaders' operation order; the model
evaluates the same formulas with numpy's operations in `dtype`. How far two correct
evaluations may lie apart is measured as the float64 model against the float32 model over
the three-frame sequence (test_model_precision_sets_the_bound prints and asserts it): at
least 99 % of the texels of every plane and frame agree within 1 fp16 ulp (the fp16
roundings absorb fp32 rounding noise except at a rounding boundary). One more ulp is
allowed for exp and pow, which the restatement evaluates as exp2f_(x log2 e) and powf_
(measured against glibc by tests/cpp/refl_denoise_test.cpp: 15.6 and 71 fp32 ulps, i.e.
under 0.04 fp16 ulps, enough to move a value across a rounding boundary): ULP_BOUND = 2 fp16
ulps for every plane, R32F planes compared after rounding to fp16. Texels outside the bound
are threshold flips (the 0.9 disocclusion test, the similarity tests, the ClipAABB branch,
the uv range test) and what they feed: at most 1 % of a plane (OUTLIER_CAP). The seed is
chosen so that the model's own f32-against-f64 run stays within that."""
import numpy as np
import pytest

from arkoserenderer_amd import abi, ddgi
import refl_denoise_inputs as I

ULP_BOUND = 2
OUTLIER_CAP = 0.01
SIZES = [(29, 19), (64, 40)]
HALTON = [(0, 1), (-2, 1), (2, -3), (-3, 0), (1, 2), (-1, -2), (3, 0), (-3, 3), (0, -3), (-1, -1), (2, 1), (-2, -2), (1, 0), (0, 2), (3, -1)]


def _kat(which, values, n_out):
    a = np.ascontiguousarray(values, np.float32)
    out = np.zeros(n_out, np.float32)
    rc = abi.load_library().ark_ddgi_debug_refl_denoise_kat(which, a.ctypes.data, a.size, out.ctypes.data, out.size)
    assert rc == 0, rc
    return out


# ---- known answers ------------------------------------------------------------------------


def test_round_up8_is_the_shaders():
    assert [_kat(abi.ARK_REFL_KAT_ROUND_UP8, [v], 1)[0] for v in (29, 32, 0, 1, 8, 1920, 1080)] == [37, 32, 0, 9, 8, 1920, 1080]


def test_kernel_weight():
    for i in range(-4, 5):
        got = _kat(abi.ARK_REFL_KAT_KERNEL_WEIGHT, [i], 1)[0]
        assert abs(got - np.exp(-3.0 * i * i / 25.0)) <= 4e-7 * np.exp(-3.0 * i * i / 25.0), i
    assert _kat(abi.ARK_REFL_KAT_KERNEL_WEIGHT, [0], 1)[0] == 1.0


def test_clip_aabb_inside_and_outside():
    lo, hi = [0.0, 1.0, 2.0], [2.0, 3.0, 4.0]
    inside = [1.5, 1.25, 3.75]
    assert np.array_equal(_kat(abi.ARK_REFL_KAT_CLIP_AABB, lo + hi + inside, 3), np.float32(inside))  # returned as is
    # outside: towards the centre (1, 2, 3) until the largest |component / (extent + 0.001)| is 1
    out = _kat(abi.ARK_REFL_KAT_CLIP_AABB, lo + hi + [5.0, 2.0, 3.5], 3)
    want = np.float32([1.0, 2.0, 3.0]) + np.float32([4.0, 0.0, 0.5]) / (np.float32(4.0) / np.float32(1.001))
    assert np.allclose(out, want, rtol=1e-6) and abs(out[0] - 2.001) < 1e-6
    # on the box's face plus the 0.001 slack: still inside
    edge = [2.0005, 2.0, 3.0]
    assert np.array_equal(_kat(abi.ARK_REFL_KAT_CLIP_AABB, lo + hi + edge, 3), np.float32(edge))


def test_tile_reduction_order_and_fp16_levels():
    """Lane (gx, gy) holds lanes[gy, gx]; a level adds 00 + 01 + 10 + 11 with 01 = (ix, oy)
    and 10 = (ox, iy), in fp32, and stores fp16. Order: 2^15, 2^-9 (01), -2^15 (10), 2^-9 (11),
    all fp16 values; 2^-9 is half an fp32 ulp of 2^15, so (2^15 + 2^-9) ties to 2^15 and the
    shader's order gives 2^-9, while 00 + 10 + 01 + 11 gives 2^-8. Levels: three quads of
    2048 + 1 (a tie, stored as 2048) and one of 2048 + 1 + 1 + 1 (2051, stored as 2052) add up
    to 8196 at the next level, a tie stored as 8192; one rounding of the exact 8198 gives 8200."""
    lanes = np.zeros((8, 8, 4), np.float32)
    big, tiny = np.float32(2.0 ** 15), np.float32(2.0 ** -9)
    lanes[0, 0, 0], lanes[0, 1, 0], lanes[1, 0, 0], lanes[1, 1, 0] = big, tiny, -big, tiny
    shader = ((big + tiny) + -big) + tiny
    other = ((big + -big) + tiny) + tiny
    assert shader == tiny and other == 2 * tiny
    for gy in (0, 2):
        for gx in (0, 2):
            lanes[gy, gx, 1], lanes[gy, gx + 1, 1] = 2048, 1
    lanes[3, 2, 1] = lanes[3, 3, 1] = 1
    out = _kat(abi.ARK_REFL_KAT_TILE_REDUCTION, lanes.reshape(-1), 4)
    assert out[0] == shader
    assert out[1] == 8192.0 and np.float32(np.float16(3 * 2049.0 + 2051.0)) == 8200.0
    # the last level: lane (4, 4)'s quadrant reaches (0, 0) only at i = 8
    lanes[:] = 0
    lanes[4, 4, 3], lanes[0, 0, 3] = 3.0, 0.5
    assert _kat(abi.ARK_REFL_KAT_TILE_REDUCTION, lanes.reshape(-1), 4)[3] == 3.5


def test_half_conversion_matches_numpy():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.normal(0, 1, 4000), rng.normal(0, 1e-6, 2000), rng.normal(0, 3e4, 2000), [0.0, -0.0, 65504, 65519.99, 65520, 1e9, -1e9, np.inf, -np.inf, 2.0 ** -24,
                        2.0 ** -25, 2.0 ** -25 * 1.0001, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11]]).astype(np.float32)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).astype(np.float32)
    assert np.array_equal(_kat(abi.ARK_REFL_KAT_HALF, x, x.size).view(np.uint32), want.view(np.uint32))
    assert np.isnan(_kat(abi.ARK_REFL_KAT_HALF, [np.nan], 1)[0])


def test_exp_and_pow_close_to_libm():
    x = np.linspace(-20, 0, 5001).astype(np.float32)
    got = _kat(abi.ARK_REFL_KAT_EXP, x, x.size).astype(np.float64)
    assert np.max(np.abs(got / np.exp(x.astype(np.float64)) - 1)) < 32 * 2.0 ** -24
    b = np.linspace(0.9, 1.0, 5001).astype(np.float32)
    got = _kat(abi.ARK_REFL_KAT_POW512, b, b.size).astype(np.float64)
    assert np.max(np.abs(got / b.astype(np.float64) ** 512 - 1)) < 256 * 2.0 ** -24
    assert _kat(abi.ARK_REFL_KAT_POW512, [0.0, 1.0], 2).tolist() == [0.0, 1.0]


# ---- the numpy model of the four shaders ------------------------------------------------------


class Model:
    """One frame of RTReflectionsNode's denoiser (RTReflectionsNode.cpp:86-139) in numpy,
    arithmetic in `dtype`. fp16 planes are float16 arrays, R32F planes float32 arrays."""

    def __init__(self, dtype, w, h, cam, inputs, no_tracing=0.6, stability=0.7):
        self.T, self.w, self.h = dtype, w, h
        T = dtype
        self.m = {k: np.asarray(cam[k], np.float32).astype(T).reshape(4, 4).T for k in ddgi.REFL_DENOISE_CAMERA_KEYS}  # row-major matrices
        self.zn, self.zf = T(np.float32(cam["z_near"])), T(np.float32(cam["z_far"]))
        self.no_tracing, self.stability = T(np.float32(no_tracing)), T(np.float32(stability))
        self.radiance = inputs["radiance"].view(np.float16).astype(T)
        self.nv = inputs["normal_velocity"].view(np.float16).astype(T)
        self.depth = inputs["depth"].astype(T)
        self.roughness = inputs["material"][..., 0].astype(T) / T(255.0)
        ys, xs = np.mgrid[0:h, 0:w]
        self.xs, self.ys = xs, ys
        self.glossy = self.roughness < self.no_tracing

    # -- helpers
    def h16(self, x):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.asarray(x, self.T).astype(np.float16).astype(self.T)

    def fetch(self, plane, x, y):
        """texelFetch, 0 outside the image"""
        h, w = plane.shape[:2]
        ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
        v = plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        return np.where(ok[..., None] if v.ndim > ok.ndim else ok, v, 0)

    def bilinear(self, plane, u, v):
        """textureLod at LOD 0: bilinear, repeat"""
        T = self.T
        h, w = plane.shape[:2]
        with np.errstate(invalid="ignore", over="ignore"):
            x, y = u * T(w) - T(0.5), v * T(h) - T(0.5)
            x = np.where(np.abs(x) < 2.0 ** 30, x, 0)
            y = np.where(np.abs(y) < 2.0 ** 30, y, 0)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[..., None], (y - y0)[..., None]
        xa, xb, ya, yb = x0.astype(np.int64) % w, (x0.astype(np.int64) + 1) % w, y0.astype(np.int64) % h, (y0.astype(np.int64) + 1) % h
        with np.errstate(invalid="ignore", over="ignore"):
            top = plane[ya, xa] + (plane[ya, xb] - plane[ya, xa]) * fx
            bot = plane[yb, xa] + (plane[yb, xb] - plane[yb, xa]) * fx
            return top + (bot - top) * fy

    def exp(self, x):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return np.exp(x)

    def lin(self, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.zn * self.zf / ((d * (self.zf - self.zn)) - self.zf)

    @staticmethod
    def dot(a, b):
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]

    def length(self, a):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.sqrt(self.dot(a, a))

    def normalize(self, a):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return a * (self.T(1.0) / np.sqrt(self.dot(a, a)))[..., None]

    def decode(self, e):
        T = self.T
        x, y = e[..., 0], e[..., 1]
        z = T(1.0) - np.abs(x) - np.abs(y)
        sx, sy = np.where(x >= 0, T(1), T(-1)), np.where(y >= 0, T(1), T(-1))
        nx, ny = np.where(z < 0, (T(1.0) - np.abs(y)) * sx, x), np.where(z < 0, (T(1.0) - np.abs(x)) * sy, y)
        return self.normalize(np.stack([nx, ny, z], -1))

    def mat3(self, M, v):
        return np.stack([M[r, 0] * v[..., 0] + M[r, 1] * v[..., 1] + M[r, 2] * v[..., 2] for r in range(3)], -1)

    def mat4(self, M, v):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([M[r, 0] * v[..., 0] + M[r, 1] * v[..., 1] + M[r, 2] * v[..., 2] + M[r, 3] * v[..., 3] for r in range(4)], -1)

    def luminance(self, c):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.fmax(self.dot(c, np.array([0.299, 0.587, 0.114], np.float32).astype(self.T)), self.T(np.float32(0.001)))

    def temporal_variance(self, a, b):
        la, lb = self.luminance(a), self.luminance(b)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(la - lb) / np.fmax(np.fmax(la, lb), self.T(0.5))
            return d * d

    def mix(self, x, y, a):
        with np.errstate(invalid="ignore", over="ignore"):
            return x * (self.T(1.0) - a) + y * a

    def clip_aabb(self, lo, hi, s):
        T = self.T
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            c = T(0.5) * (hi + lo)
            e = T(0.5) * (hi - lo) + T(np.float32(0.001))
            v = s - c
            unit = np.abs(v / e)
            m = np.fmax(np.fmax(unit[..., 0], unit[..., 1]), unit[..., 2])
            return np.where((m > 1.0)[..., None], c + v / m[..., None], s)

    def world_normal(self):
        return self.mat3(self.m["world_from_view"], self.decode(self.nv[..., :2]))

    def moments(self):
        """EstimateLocalNeighborhoodInGroup over the fp16 tile of the noisy radiance"""
        T = self.T
        mean, var, acc = np.zeros((self.h, self.w, 3), T), np.zeros((self.h, self.w, 3), T), T(0)
        kw = lambda i: self.exp(T(np.float32(-3.0)) * T(i * i) / T(25.0))  # noqa: E731
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(-4, 5):
                for i in range(-4, 5):
                    r = self.h16(self.fetch(self.radiance, self.xs + i, self.ys + j)[..., :3])
                    wgt = kw(i) * kw(j)
                    acc = acc + wgt
                    mean = mean + r * wgt
                    var = var + r * r * wgt
            mean, var = mean / acc, var / acc
            return mean, np.abs(var - mean * mean)

    def sample_average(self, avg):
        T = self.T
        r8 = lambda v: v if v % 8 == 0 else v + 8  # noqa: E731  (RoundUp8 as the shader has it)
        u, v = (self.xs.astype(T) + T(0.5)) / T(r8(self.w)), (self.ys.astype(T) + T(0.5)) / T(r8(self.h))
        return self.bilinear(avg.astype(T), u, v)[..., :3]

    # -- passes
    def history_copy(self, st, first):
        T = self.T
        out = dict(st)
        z = np.zeros((self.h, self.w, 1), T)
        with np.errstate(over="ignore", invalid="ignore"):
            out["radiance_history"] = np.concatenate([self.radiance[..., :3], z], -1).astype(np.float16)
            out["normal_history"] = np.concatenate([self.world_normal(), z], -1).astype(np.float16)
            var = np.zeros((self.h, self.w), T) if first else st["variance"].astype(T)
            ns = np.zeros((self.h, self.w), T) if first else st["num_samples"].astype(T)
            out["depth_history"] = np.stack([self.depth, self.roughness, var, ns], -1).astype(np.float16)
        return out

    def disocclusion(self, n, hn, ld, hld):
        T = self.T
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return self.exp(-np.abs(T(1.0) - np.fmax(T(0.0), self.dot(n, hn))) * T(np.float32(1.4))) * self.exp(-np.abs(hld - ld) / ld * T(1.0))

    def reproject(self, st):
        T, w, h = self.T, self.w, self.h
        out = dict(st)
        rh, nh, dh = st["radiance_history"].astype(T), st["normal_history"].astype(T), st["depth_history"].astype(T)
        mean, variance = self.moments()
        u, v = (self.xs.astype(T) + T(0.5)) / T(w), (self.ys.astype(T) + T(0.5)) / T(h)
        normal = self.world_normal()
        radiance, ray_length = self.radiance[..., :3], self.radiance[..., 3]
        su, sv = u - self.nv[..., 2], v - self.nv[..., 3]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ndc = np.stack([u * T(2.0) - T(1.0), v * T(2.0) - T(1.0), self.depth, np.ones_like(u)], -1)
            vp = self.mat4(self.m["view_from_projection"], ndc)
            ray = vp[..., :3] / vp[..., 3:]
            sd = self.length(ray)
            ray = ray / sd[..., None] * (sd + ray_length)[..., None]
            world = self.mat4(self.m["world_from_view"], np.concatenate([ray, np.ones_like(ray[..., :1])], -1))
            pv = self.mat4(self.m["previous_frame_view_from_world"], np.concatenate([world[..., :3], np.ones_like(ray[..., :1])], -1))
            pp = self.mat4(self.m["previous_frame_projection_from_view"], pv)
            hu, hv = pp[..., 0] / pp[..., 3] * T(0.5) + T(0.5), pp[..., 1] / pp[..., 3] * T(0.5) + T(0.5)
            s_n, h_n = self.bilinear(nh, su, sv)[..., :3], self.bilinear(nh, hu, hv)[..., :3]
            s_r, h_r = self.bilinear(rh, su, sv)[..., :3], self.bilinear(rh, hu, hv)[..., :3]
            s_d, h_d = self.bilinear(dh, su, sv), self.bilinear(dh, hu, hv)
            nn = self.normalize(normal)
            h_sim, s_sim = self.dot(self.normalize(h_n), nn), self.dot(self.normalize(s_n), nn)
            take_hit = (h_sim > T(np.float32(0.9999))) & (h_sim + T(np.float32(1.0e-3)) > s_sim) & \
                       (np.abs(h_d[..., 1] - self.roughness) < np.abs(s_d[..., 1] - self.roughness) + T(np.float32(1.0e-3)))
            d = s_r - mean
            take_surface = ~take_hit & (self.dot(d, d) < T(1.5) * self.length(variance))
            rejected = ~take_hit & ~take_surface
            hn = np.where(take_hit[..., None], h_n, s_n)
            hld = self.lin(np.where(take_hit, h_d[..., 0], s_d[..., 0]))
            ru, rv = np.where(take_hit, hu, su), np.where(take_hit, hv, sv)
            repro = np.where(take_hit[..., None], h_r, s_r)
            ld = self.lin(self.depth)
            factor = self.disocclusion(normal, hn, ld, hld)
            thr = T(np.float32(0.9))
            done = factor > thr
            search = ~done & (factor < thr)
            f2, ru2, rv2 = factor.copy(), ru.copy(), rv.copy()
            du, dv = T(1.0) / T(w), T(1.0) / T(h)
            for y in (-1, 0, 1):
                for x in (-1, 0, 1):
                    qu, qv = ru2 + T(x) * du, rv2 + T(y) * dv
                    wgt = self.disocclusion(normal, self.bilinear(nh, qu, qv)[..., :3], ld, self.lin(self.bilinear(dh, qu, qv)[..., 0]))
                    better = search & (wgt > f2)
                    f2, ru2, rv2 = np.where(better, wgt, f2), np.where(better, qu, ru2), np.where(better, qv, rv2)
            repro = np.where(search[..., None], self.bilinear(rh, ru2, rv2)[..., :3], repro)
            factor, ru, rv = np.where(search, f2, factor), np.where(search, ru2, ru), np.where(search, rv2, rv)
            slow = ~done & (factor < thr)
            fu, fv = T(w) * ru + T(0.5), T(h) * rv + T(0.5)
            uvx, uvy = fu - np.floor(fu), fv - np.floor(fv)
            cx, cy = T(w) * ru - T(0.5), T(h) * rv - T(0.5)
            tx = np.where(np.abs(cx) < 2.0 ** 30, np.trunc(cx), -2.0 ** 30).astype(np.int64)
            ty = np.where(np.abs(cy) < 2.0 ** 30, np.trunc(cy), -2.0 ** 30).astype(np.int64)
            rad4, nrm4, dep4, w4 = [], [], [], []
            for k in range(4):
                x, y = tx + (k & 1), ty + (k >> 1)
                rad4.append(self.fetch(rh, x, y)[..., :3])
                nrm4.append(self.fetch(nh, x, y)[..., :3])
                dep4.append(self.lin(self.fetch(dh, x, y)[..., 0]))
                w4.append(np.where(self.disocclusion(normal, nrm4[k], ld, dep4[k]) > thr / T(2.0), T(1.0), T(0.0)))
            w4 = [w4[0] * (T(1.0) - uvx) * (T(1.0) - uvy), w4[1] * uvx * (T(1.0) - uvy), w4[2] * (T(1.0) - uvx) * uvy, w4[3] * uvx * uvy]
            ws = np.fmax(w4[0] + w4[1] + w4[2] + w4[3], T(np.float32(1.0e-3)))
            w4 = [a / ws for a in w4]
            s_rad = rad4[0] * w4[0][..., None] + rad4[1] * w4[1][..., None] + rad4[2] * w4[2][..., None] + rad4[3] * w4[3][..., None]
            s_dep = dep4[0] * w4[0] + dep4[1] * w4[1] + dep4[2] * w4[2] + dep4[3] * w4[3]
            s_nrm = nrm4[0] * w4[0][..., None] + nrm4[1] * w4[1][..., None] + nrm4[2] * w4[2][..., None] + nrm4[3] * w4[3][..., None]
            repro = np.where(slow[..., None], s_rad, repro)
            factor = np.where(slow, self.disocclusion(normal, s_nrm, ld, s_dep), factor)
            factor = np.where(~done & (factor < thr), T(0.0), factor)
            # FFX_DNSR_Reflections_Reproject
            in_range = ~rejected & (ru > 0) & (rv > 0) & (ru < 1) & (rv < 1)
            drvn = self.bilinear(dh, ru, rv)
            ns = drvn[..., 3] * factor
            s_max = np.fmax(T(8.0), T(32.0) * (T(1.0) - self.exp(-self.roughness * T(100.0))))
            ns = np.fmin(s_max, ns + T(1.0))
            new_var = self.temporal_variance(radiance, repro)
            keep = in_range & ~(factor < thr)
            var_mix = self.mix(new_var, drvn[..., 2], T(1.0) / ns)
            g = self.glossy
            z = np.zeros((h, w, 1), T)
            out["reprojected"] = np.where(g[..., None], np.where(keep[..., None], np.concatenate([repro, z], -1), 0), st["reprojected"].astype(T)).astype(np.float16)
            out["variance"] = np.where(g, np.where(keep, var_mix, T(1.0)), st["variance"].astype(T)).astype(np.float32)
            out["num_samples"] = np.where(g, np.where(keep, ns, T(1.0)), st["num_samples"].astype(T)).astype(np.float32)
            rad = np.where((g & keep)[..., None], self.mix(radiance, repro, T(np.float32(0.3))), radiance)
            wgt = np.fmax(self.exp(-self.luminance(rad) * T(np.float32(0.3))), T(np.float32(1.0e-2)))
            rad = rad * wgt[..., None]
            bad = ~np.isfinite(rad).all(-1) | (wgt > 1.0e3)
            rad, wgt = np.where(bad[..., None], 0, rad), np.where(bad, 0, wgt)
            # 8 x 8 -> 1, fp16 at every level, 00 + 01 + 10 + 11
            ty_, tx_ = (h + 7) // 8, (w + 7) // 8
            lanes = np.zeros((ty_ * 8, tx_ * 8, 4), T)
            lanes[:h, :w] = np.concatenate([rad, wgt[..., None]], -1)
            a = self.h16(lanes)
            while a.shape[0] > ty_:
                a = self.h16(a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2])
            out["average_radiance"] = np.concatenate([a[..., :3] / np.fmax(a[..., 3:], T(np.float32(1.0e-3))), np.zeros((ty_, tx_, 1), T)], -1).astype(np.float16)
        return out

    def prefilter(self, st):
        T, w, h = self.T, self.w, self.h
        out = dict(st)
        var_plane = st["variance"].astype(T)
        avg = self.sample_average(st["average_radiance"])

        def tile(x, y):  # LoadNeighborhood through the fp16 tile; depth stays as computed
            ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
            rad = self.h16(self.fetch(self.radiance, x, y)[..., :3])
            var = self.h16(self.fetch(var_plane, x, y))
            nrm = self.h16(self.decode(self.fetch(self.nv, x, y)[..., :2]))
            dep = np.abs(self.lin(np.where(ok, self.fetch(self.depth, x, y), T(0))))
            return rad, var, nrm, dep

        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            c_rad, c_var, c_nrm, c_dep = tile(self.xs, self.ys)
            rw = lambda n_rad: np.fmax(self.exp(-(T(np.float32(0.6)) + c_var * T(np.float32(0.1))) * self.length(avg - n_rad)), T(np.float32(1.0e-2)))  # noqa: E731
            acc_w = rw(c_rad)
            acc_rad = c_rad * acc_w[..., None]
            acc_var = c_var * acc_w * acc_w
            vw = np.fmax(T(np.float32(0.1)), T(1.0) - self.exp(-(c_var * T(np.float32(4.4)))))
            for dx, dy in HALTON:
                n_rad, n_var, n_nrm, n_dep = tile(self.xs + dx, self.ys + dy)
                wgt = np.power(np.fmax(self.dot(c_nrm, n_nrm), T(0.0)), T(512.0))
                wgt = wgt * self.exp(-np.abs(c_dep - n_dep) * c_dep * T(4.0))
                wgt = wgt * rw(n_rad)
                wgt = wgt * vw
                acc_w = acc_w + wgt
                acc_rad = acc_rad + wgt[..., None] * n_rad
                acc_var = acc_var + wgt * wgt * n_var
            needs = (c_var > 0) & self.glossy & ~(self.roughness < T(np.float32(0.001)))
            res_rad = np.where(needs[..., None], acc_rad / acc_w[..., None], c_rad)
            res_var = np.where(needs, acc_var / (acc_w * acc_w), c_var)
            out["resolved"] = np.concatenate([res_rad, res_var[..., None]], -1).astype(np.float16)
        return out

    def resolve_temporal(self, st):
        T = self.T
        out = dict(st)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            new = self.h16(self.radiance[..., :3])
            new_var = st["variance"].astype(T)
            ns = st["num_samples"].astype(T)
            avg = self.sample_average(st["average_radiance"])
            old = st["reprojected"].astype(T)[..., :3]
            mean, variance = self.moments()
            std = (np.sqrt(variance) + self.length(mean - avg)[..., None]) * self.stability * T(np.float32(1.4))
            mean = self.mix(mean, avg, T(np.float32(0.2)))
            clipped_old = self.clip_aabb(mean - std, mean + std, old)
            weight = T(1.0) - T(1.0) / np.fmax(ns, T(1.0))
            sig = self.mix(new, avg, (T(1.0) / np.fmax(ns + T(1.0), T(1.0)))[..., None])
            sig = self.clip_aabb(avg - std * T(1.0), avg + std * T(1.0), sig)
            sig = self.mix(sig, clipped_old, weight[..., None])
            var = self.mix(self.temporal_variance(sig, clipped_old), new_var, weight)
            bad = ~np.isfinite(sig).all(-1) | ~np.isfinite(var)
            sig, var = np.where(bad[..., None], 0, sig), np.where(bad, 0, var)
            g = self.glossy
            out["temporal_accumulation"] = np.concatenate([np.where(g[..., None], sig, new), np.where(g, var, new_var)[..., None]], -1).astype(np.float16)
        return out

    def frame(self, st, first):
        if first:
            st = self.history_copy(st, True)
        return self.history_copy(self.resolve_temporal(self.prefilter(self.reproject(st))), False)


def _model_state(w, h):
    return {k: (v.view(np.float16) if v.dtype == np.uint16 else v) for k, v in I.fresh_planes(w, h).items()}


_MODEL_CACHE = {}


def model_sequence(dtype, w, h):
    """The model over the three-frame sequence from zeroed planes, once per (dtype, size)."""
    key = (np.dtype(dtype).name, w, h)
    if key not in _MODEL_CACHE:
        st, out = _model_state(w, h), []
        for f, (cam, planes) in enumerate(I.sequence(w, h)):
            st = Model(dtype, w, h, cam, planes).frame(st, f == 0)
            out.append(st)
        _MODEL_CACHE[key] = out
    return _MODEL_CACHE[key]


def ulps16(a, b):
    """|a - b| in fp16 ulps per texel channel (values rounded to fp16 first); NaN against NaN
    is 0, NaN against a number 65535."""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = np.asarray(a).astype(np.float16), np.asarray(b).astype(np.float16)
    key = lambda x: np.where(x.view(np.int16) < 0, -(x.view(np.int16) & 0x7FFF).astype(np.int32), x.view(np.int16).astype(np.int32))  # noqa: E731
    d = np.abs(key(a) - key(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 65535, d))


def _outlier_fraction(a, b):
    d = ulps16(a, b)
    d = d.reshape(d.shape[0], d.shape[1], -1).max(-1)
    return float(np.mean(d > ULP_BOUND)), d


@pytest.mark.parametrize("w,h", SIZES)
def test_model_precision_sets_the_bound(w, h):
    """float64 against float32 model: the measured part of the bound (ULP_BOUND - 1) holds on
    all but OUTLIER_CAP of every plane, so the seed keeps the threshold flips under the cap too."""
    m32, m64 = model_sequence(np.float32, w, h), model_sequence(np.float64, w, h)
    for f in range(3):
        for k in I.WRITTEN:
            frac, d = _outlier_fraction(m32[f][k], m64[f][k])
            measured = float(np.mean(d > ULP_BOUND - 1))
            print(f"{w}x{h} frame {f} {k}: f32 vs f64 model: {100 * measured:.2f} % above {ULP_BOUND - 1} ulp, {100 * frac:.2f} % above {ULP_BOUND}")
            assert frac <= measured <= OUTLIER_CAP, (f, k, measured)


@pytest.mark.parametrize("w,h", SIZES)
def test_host_restatement_matches_model(w, h):
    host, model = I.host_sequence(w, h), model_sequence(np.float32, w, h)
    for f in range(3):
        for k in I.WRITTEN:
            hv = host[f][k].view(np.float16) if host[f][k].dtype == np.uint16 else host[f][k]
            frac, d = _outlier_fraction(hv, model[f][k])
            print(f"{w}x{h} frame {f} {k}: host vs f32 model: {100 * frac:.2f} % outside {ULP_BOUND} ulp, {100 * np.mean(d == 0):.1f} % equal")
            assert frac <= OUTLIER_CAP, (f, k, frac)


def test_partial_stores_keep_a_poison_pattern():
    """reproject stores reprojected / variance / num_samples of glossy pixels only; the six
    other planes are written whole."""
    w, h = 29, 19
    cam, planes = I.sequence(w, h)[0]
    st = I.fresh_planes(w, h, poison=True)
    ddgi.refl_denoise_host(w, h, cam, dict(planes, **st), abi.ARK_REFL_DENOISE_FIRST_FRAME)
    g = I.glossy(planes)
    assert g.any() and (~g).any()
    for k in I.WRITTEN:
        a = st[k].reshape(st[k].shape[0], st[k].shape[1], -1)
        poisoned = np.all(a == (I.POISON16 if a.dtype == np.uint16 else I.POISON32), axis=-1)
        if k in I.PARTIAL:
            assert poisoned[~g].all() and not poisoned[g].any(), k
        else:
            assert not poisoned.any(), k


def test_disabled_copies_radiance_and_nothing_else():
    w, h = 29, 19
    cam, planes = I.sequence(w, h)[1]
    st = I.fresh_planes(w, h, poison=True)
    ddgi.refl_denoise_host(w, h, cam, dict(planes, **st), abi.ARK_REFL_DENOISE_DISABLED)
    assert np.array_equal(st["resolved"], planes["radiance"])
    fresh = I.fresh_planes(w, h, poison=True)
    assert all(np.array_equal(st[k], fresh[k]) for k in I.WRITTEN if k != "resolved")


def test_inputs_cover_the_cases():
    w, h = 64, 40
    seq = I.sequence(w, h)
    r = seq[0][1]["material"][..., 0]
    assert (r == 0).any() and (r == 160).any() and (r == 230).any() and ((r > 0) & (r < 153)).any()
    assert 0.05 < np.mean(seq[0][1]["depth"] == 1.0) < 0.2
    rad = seq[1][1]["radiance"].view(np.float16)
    assert np.isinf(rad[..., :3]).any() and np.isnan(rad[..., :3]).any() and (rad[..., 3] < 0).any() and (rad[..., 3] > 5).any() and ((rad[..., 3] > 0) & (rad[..., 3] < 0.5)).any()
    mv = seq[1][1]["normal_velocity"].view(np.float16)[..., 2:]
    assert np.abs(mv.astype(np.float32)).max() * w > 0.5  # the camera moves by a good part of a texel at least
    # both outcomes of reprojection occur in the host's frames 1 and 2
    host = I.host_sequence(w, h)
    g = I.glossy(seq[1][1])
    for f in (1, 2):
        ns = host[f]["num_samples"][g]
        assert (ns > 1).any() and (ns == 1).any()
