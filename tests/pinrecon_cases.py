"""Scenes and rigs the pinhole reconstruction tests share (tests/test_pinhole_reconstruct_cpu.py, the GPU tests of
tests/test_pinhole_reconstruct.py): the cameras of tests/stereo_calib_cases.py scaled to small frames, and pairs of
textured planes rendered into both cameras by inverse mapping, the way tests/npsgbm.py renders its plane for the
omnidirectional rig -- each pixel's ray (the model's undistort_points) is cut with the scene and a random texture is
read there bilinearly.

Lengths are millimetres; the scene is given in camera 1's frame.
"""
import functools

import numpy as np

import npcalib
import nprectify as N
import stereo_calib_cases as SC

W0, H0 = SC.SIZE   # 1280 x 960: the size G1_TRUE / G2_TRUE are stated for


def camera(g, size):
    """(K, D) of a camera of stereo_calib_cases at size = (w, h): the focal lengths and cx scale with w / 1280, the
    principal point keeps its offset from the centre row"""
    w, h = size
    s = w / W0
    K = np.array([[g[0] * s, 0.0, g[2] * s], [0.0, g[1] * s, h / 2 + (g[3] - H0 / 2) * s], [0.0, 0.0, 1.0]])
    return K, np.array(g[4:9], np.float64)


def rig(name):
    """(R, T) of `head` or of a rig of stereo_calib_cases.RIGS"""
    om, T = (SC.OM_TRUE, SC.T_TRUE) if name == "head" else SC.rig_of(name)[:2]
    return npcalib.rodrigues(np.asarray(om, np.float64)), np.asarray(T, np.float64)


def cameras(size):
    return camera(SC.G1_TRUE, size) + camera(SC.G2_TRUE, size)   # K1, D1, K2, D2


# a scene is a list of (depth Z, x_max) planes Z = const in camera 1's frame, nearest first: a ray takes the first plane
# it meets at X < x_max (None: no limit)
PLANE = ((800.0, None),)
STEP = ((700.0, 40.0), (1000.0, None))
TEXEL = 14.0   # mm: about two pixels of a 160 x 120 frame at 800 mm


def _texture(rng, cn):
    return rng.integers(30, 256, (256, 256, cn)).astype(np.float64)


def _sample(tex, X, Y):
    u, v = X / TEXEL, Y / TEXEL
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = (u - u0)[:, None], (v - v0)[:, None]
    n = tex.shape[0]
    a, b, c, d = tex[v0 % n, u0 % n], tex[v0 % n, (u0 + 1) % n], tex[(v0 + 1) % n, u0 % n], tex[(v0 + 1) % n, (u0 + 1) % n]
    return (1 - fu) * (1 - fv) * a + fu * (1 - fv) * b + (1 - fu) * fv * c + fu * fv * d


@functools.lru_cache(maxsize=None)
def render(scene, rig_name="head", size=(160, 120), cn=1, seed=3):
    """(image1, image2) uint8 [h, w] or [h, w, 3], read-only"""
    rng = np.random.default_rng(seed)
    w, h = size
    K1, D1, K2, D2 = cameras(size)
    R, T = rig(rig_name)
    texs = [_texture(rng, cn) for _ in scene]
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px = np.stack([jj.ravel(), ii.ravel()], -1)
    out = []
    for K, D, second in ((K1, D1, False), (K2, D2, True)):
        xy = N.undistort_points(px, K, D)
        ray = np.concatenate([xy, np.ones((len(xy), 1))], 1)
        org, dirs = (-R.T @ T, ray @ R) if second else (np.zeros(3), ray)   # X2 = R X1 + T
        val = np.zeros((len(px), cn))
        todo = np.ones(len(px), bool)
        for (Z, x_max), tex in zip(scene, texs):
            t = (Z - org[2]) / dirs[:, 2]
            P = org + t[:, None] * dirs
            hit = todo & (t > 0) & (True if x_max is None else P[:, 0] < x_max)
            val[hit] = _sample(tex, P[hit, 0], P[hit, 1])
            todo &= ~hit
        img = np.rint(val).astype(np.uint8).reshape(h, w, cn)
        img = np.ascontiguousarray(img[:, :, 0] if cn == 1 else img)
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def true_depth(scene, frame, rect_R1):
    """float64 [h, w]: camera 1's depth Z of what the pixel of the rectified (output-frame) image 1 sees, from the
    output frame's P1 and the library's or the model's R1"""
    w, h = frame["size"]
    P = np.asarray(frame["P1"], np.float64)[:, :3]
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([jj, ii, np.ones_like(jj)], -1) @ np.linalg.inv(P @ np.asarray(rect_R1)).T   # rays in camera 1's frame
    out = np.full((h, w), np.nan)
    todo = np.ones((h, w), bool)
    for Z, x_max in scene:
        t = Z / d[..., 2]
        hit = todo & (t > 0) & (True if x_max is None else t * d[..., 0] < x_max)
        out[hit] = Z
        todo &= ~hit
    return out
