"""Inputs for the skinning tests (inputs only; every case is deterministic) and a float64
evaluation of skinning.comp:35-98 written from the shader, independently of csrc/skinning.h."""
from __future__ import annotations

import numpy as np

from arkoserenderer_amd import ddgi as D

LDS_JOINTS = 256  # skin::kLdsJoints (csrc/skinning.h)


def rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_rotation(rng, angle: float) -> np.ndarray:
    """A rotation by at most `angle` radians about a random axis (Rodrigues)."""
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    a = rng.uniform(-angle, angle)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def joint_matrices(rng, joints: int, translate: float = 1.0, spread: float = 0.6) -> np.ndarray:
    """joints x 4 x 4 float32 row-major: a rotation times a uniform scale in [0.5, 2], and a
    translation. As in a posed skeleton, whose neighbouring joints differ by a limited
    rotation, every joint is one common random rotation times a rotation of at most
    `spread` radians: a blend of four of them stays well-conditioned."""
    M = np.zeros((joints, 4, 4), np.float32)
    base = rotation(rng)
    for j in range(joints):
        M[j, :3, :3] = base @ small_rotation(rng, spread) * rng.uniform(0.5, 2.0)
        M[j, :3, 3] = rng.uniform(-translate, translate, 3)
        M[j, 3] = (0, 0, 0, 1)
    return M


def column_major(M: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(M, np.float32).transpose(0, 2, 1))


def random_skin(seed: int, n: int, joints: int, K: int, first_vertex: int = 0, skeleton: bool = True, influences: int = 4):
    """A random skin of n vertices: unit normals and tangents (K = 0 cases scale them
    themselves), `influences` non-zero weights per vertex summing to 1, K morph targets of
    small deltas. Returns (D.Skin, dict of its arrays)."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    V = np.zeros((n, 9), np.float32)
    V[:, 0:2] = rng.uniform(0, 1, (n, 2))
    nrm = rng.normal(size=(n, 3))
    V[:, 2:5] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3)))
    V[:, 5:8] = tan / np.linalg.norm(tan, axis=1, keepdims=True)
    V[:, 8] = rng.choice([-1.0, 1.0], n)
    ji = jw = None
    if skeleton:
        ji = rng.integers(0, joints, (n, 4)).astype(np.uint32)
        w = rng.uniform(0.05, 1.0, (n, 4))
        w[:, influences:] = 0.0
        jw = (w / w.sum(1, keepdims=True)).astype(np.float32)
    morph = None
    if K:
        morph = rng.uniform(-0.2, 0.2, (K, n, 9)).astype(np.float32)
    skin = D.Skin(first_vertex, P, V, ji, jw, joints if skeleton else 0, morph)
    return skin, dict(positions=P, vertices=V, joint_indices=ji, joint_weights=jw, morph_targets=morph)


def reference_f64(arr: dict, M: np.ndarray | None, mw, prev=None):
    """skinning.comp:35-98 in float64 from the fp32 inputs. M: joints x 4 x 4 row-major (None:
    no skeleton). Returns positions, normals, tangents (xyz), velocities, and the per
    coordinate sum of the magnitudes of the position's terms (sum_j sum_c |w_j M_j,rc p_c|,
    the translation's term included, with p the morphed position's term magnitudes)."""
    P = arr["positions"].astype(np.float64)
    V = arr["vertices"].astype(np.float64)
    N, T = V[:, 2:5].copy(), V[:, 5:8].copy()
    mag = np.abs(P)
    K = 0 if arr["morph_targets"] is None else len(arr["morph_targets"])
    if K:
        for k in range(K):
            d = arr["morph_targets"][k].astype(np.float64)
            w = float(np.float32(mw[k]))
            P = P + d[:, 0:3] * w
            N = N + d[:, 3:6] * w
            T = T + d[:, 6:9] * w
            mag = mag + np.abs(d[:, 0:3] * w)
        N = N / np.linalg.norm(N, axis=1, keepdims=True)
        T = T / np.linalg.norm(T, axis=1, keepdims=True)
        T = T - N * np.sum(N * T, axis=1, keepdims=True)
        T = T / np.linalg.norm(T, axis=1, keepdims=True)
    terms = mag
    if M is not None:
        Md = np.asarray(M, np.float32).astype(np.float64)
        ji, jw = arr["joint_indices"], arr["joint_weights"].astype(np.float64)
        A = np.einsum("vq,vqrc->vrc", jw, Md[ji])  # n x 4 x 4
        absA = np.einsum("vq,vqrc->vrc", jw, np.abs(Md[ji]))
        terms = np.einsum("vrc,vc->vr", absA[:, :3, :3], mag) + absA[:, :3, 3]
        P = np.einsum("vrc,vc->vr", A[:, :3, :3], P) + A[:, :3, 3]
        with np.errstate(all="ignore"):
            try:
                NT = np.linalg.inv(A[:, :3, :3]).transpose(0, 2, 1)
            except np.linalg.LinAlgError:
                NT = np.full((len(P), 3, 3), np.nan)
        N = np.einsum("vrc,vc->vr", NT, N)
        T = np.einsum("vrc,vc->vr", NT, T)
    vel = np.zeros_like(P) if prev is None else P - np.asarray(prev, np.float32).astype(np.float64)
    return P, N, T, vel, terms
