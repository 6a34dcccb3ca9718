"""A three-frame input sequence for the reflection denoiser tests, on reflection_inputs'
camera and G-buffer: frame 0 is the first frame, frames 1 and 2 see the same G-buffer through
a translated and rotated camera, with motion vectors derived from the two cameras (frame 0's previous camera is one
before the sequence). The upper
half of the image is a smooth surface (a depth ramp, one normal, slowly varying radiance) so
that reprojection accepts history there; the lower half keeps reflection_inputs' random
planes, where it mostly rejects it. Ray lengths mix short, long and negative (back-face)
values; roughness bytes include 0 (a mirror: prefilter copies), values under the node's 0.6
threshold, and 160 and 230 (not glossy); a tenth of the pixels is sky; a few radiance texels
are +inf and NaN. Also the host restatement's planes after every frame, computed once."""
import functools

import numpy as np

import reflection_inputs as RI
from arkoserenderer_amd import abi, ddgi

NEAR, FAR = 0.1, 100.0
EYES = ((0.0, 1.2, 3.0), (0.03, 1.21, 2.97), (0.07, 1.19, 2.95))
TARGETS = ((0.0, 0.6, 0.0), (0.02, 0.6, 0.0), (0.05, 0.62, 0.0))
EYE_BEFORE, TARGET_BEFORE = (-0.02, 1.19, 3.02), (-0.01, 0.61, 0.0)  # the frame before the first: a first frame after a resize has one
WRITTEN = tuple(k for k, _, _, _ in abi.REFL_DENOISE_PLANES if k not in abi.REFL_DENOISE_INPUTS)
PARTIAL = ("reprojected", "variance", "num_samples")  # reproject stores glossy pixels only
POISON16, POISON32 = 0x5A5A, np.float32(-7.25)


def _inv_col(m16):
    """column-major float32[16] of the inverse of a column-major float32[16] matrix"""
    return np.linalg.inv(np.asarray(m16, np.float64).reshape(4, 4).T).T.reshape(16).astype(np.float32)


def cameras(width, height):
    """One denoiser camera dict per frame: the current CameraState matrices, the previous
    frame's view and projection (frame 0: the camera before the sequence, so that its history
    - a copy of its own planes - is sampled between texels like any other), z_near and z_far."""
    def view_proj(eye, target):
        c = RI.camera(width, height, eye=eye, target=target, near=NEAR, far=FAR)
        return c, {"view_from_world": _inv_col(c["world_from_view"]), "projection_from_view": _inv_col(c["view_from_projection"])}

    out, p = [], view_proj(EYE_BEFORE, TARGET_BEFORE)[1]
    for eye, target in zip(EYES, TARGETS):
        c, cur = view_proj(eye, target)
        out.append(dict(c, previous_frame_view_from_world=p["view_from_world"], previous_frame_projection_from_view=p["projection_from_view"], z_near=NEAR, z_far=FAR))
        p = cur
    return out


def _motion_vectors(cam, depth):
    """uv - previous uv of every pixel's surface point (pointing from previous to current)."""
    h, w = depth.shape
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = (xs + 0.5) / w, (ys + 0.5) / h
    m = lambda k: np.asarray(cam[k], np.float64).reshape(4, 4).T  # noqa: E731
    ndc = np.stack([u * 2 - 1, v * 2 - 1, depth.astype(np.float64), np.ones((h, w))], -1)
    view = ndc @ m("view_from_projection").T
    view /= view[..., 3:]
    world = view @ m("world_from_view").T
    pp = (world @ m("previous_frame_view_from_world").T) @ m("previous_frame_projection_from_view").T
    pu, pv = pp[..., 0] / pp[..., 3] * 0.5 + 0.5, pp[..., 1] / pp[..., 3] * 0.5 + 0.5
    return np.stack([u - pu, v - pv], -1)


def sequence(width, height, seed=11):
    """[(camera, planes)] for three frames; planes: radiance and normal_velocity uint16
    [h, w, 4] (fp16 words), depth float32 [h, w], material uint8 [h, w, 4]."""
    rng = np.random.default_rng(seed)
    cams = cameras(width, height)
    gb, _ = RI.gbuffer(width, height, cams[0], seed=seed)
    depth, mat = gb["depth"].copy(), gb["material"].copy()
    nv = gb["normal_velocity"].view(np.float16).copy()
    top = max(1, height // 2)
    ys, xs = np.mgrid[0:height, 0:width]
    smooth = (0.97 + 0.01 * xs / max(1, width) + 0.005 * ys / max(1, height)).astype(np.float32)
    depth[:top] = smooth[:top]
    depth[:top][rng.random((top, width)) < 0.1] = 1.0  # sky in the smooth half too
    nv[:top, :, 0], nv[:top, :, 1] = 0.05, 0.1         # one view-space normal, towards the viewer
    mat[:top, :, 0] = 60
    mat[:top][rng.random((top, width)) < 0.1, 0] = 230
    mat[:top][rng.random((top, width)) < 0.05, 0] = 160
    mat.reshape(-1, 4)[rng.integers(0, width * height, max(1, width * height // 20)), 0] = 0  # mirrors
    base = 1.0 + 0.5 * np.sin(xs / 5.0)[..., None] + 0.25 * np.cos(ys / 7.0)[..., None] + np.array([0.0, 0.2, 0.4])
    frames = []
    for f, cam in enumerate(cams):
        noise = rng.uniform(-0.15, 0.15, (height, width, 3))
        rad = np.empty((height, width, 4), np.float32)
        rad[..., :3] = rng.uniform(0.0, 4.0, (height, width, 3))
        rad[:top, :, :3] = (base + noise)[:top]
        kind = rng.random((height, width))
        rad[..., 3] = np.where(kind < 0.4, rng.uniform(0.02, 0.5, (height, width)), np.where(kind < 0.8, rng.uniform(5.0, 60.0, (height, width)), -rng.uniform(0.05, 8.0, (height, width))))
        flat = rad.reshape(-1, 4)
        n = width * height
        for k, value in enumerate((np.inf, np.nan, np.inf)):
            flat[(7 * f + 13 * k + n // 3) % n, k % 3] = value
        nvf = nv.copy()
        nvf[..., 2:4] = _motion_vectors(cam, depth)
        frames.append((cam, {"radiance": rad.astype(np.float16).view(np.uint16), "depth": depth.copy(), "material": mat.copy(), "normal_velocity": nvf.view(np.uint16)}))
    return frames


def fresh_planes(width, height, poison=False):
    """The nine written planes as numpy arrays: zeroed (the caller's duty), or every one
    filled with a poison pattern."""
    out = {}
    for k in WRITTEN:
        shape, dtype = ddgi.refl_denoise_plane_shape(k, width, height)
        out[k] = np.full(shape, (POISON16 if dtype == np.uint16 else POISON32) if poison else 0, dtype)
    return out


def glossy(planes, threshold=0.6):
    return planes["material"][..., 0].astype(np.float32) / np.float32(255.0) < np.float32(threshold)


def frame_flags(f):
    return abi.ARK_REFL_DENOISE_FIRST_FRAME if f == 0 else 0


@functools.lru_cache(maxsize=None)
def host_sequence(width, height, seed=11):
    """The host restatement over the sequence from zeroed planes: per frame a dict of copies
    of the nine written planes. Computed once per size; do not modify."""
    state, out = fresh_planes(width, height), []
    for f, (cam, planes) in enumerate(sequence(width, height, seed)):
        ddgi.refl_denoise_host(width, height, cam, dict(planes, **state), frame_flags(f))
        out.append({k: v.copy() for k, v in state.items()})
    return out
