"""Seeded synthetic views for the pinhole calibrateCamera tests (tests/test_calibrate_camera*.py).

One camera, 1280 x 960, fx 900, fy 905, cx 655, cy 470, k1 -0.25, k2 0.08, p1 1e-3, p2 -5e-4, k3 0, sees a planar
grid of 40 mm pitch (millimetres throughout; a grid of more than 121 corners shrinks its pitch to stay 400 mm
wide) tilted 10 to 45 degrees about an axis that turns from view to view, 0.5 to 1.2 m away, so that both focal
lengths are observable.  Pixels are float64 projections through npcalib.project, optionally with Gaussian noise.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import npcalib

SIZE = (1280, 960)
G_TRUE = np.array([900.0, 905.0, 655.0, 470.0, -0.25, 0.08, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0])
G_RATIONAL = np.array([900.0, 905.0, 655.0, 470.0, -0.25, 0.08, 1e-3, -5e-4, 0.01, 0.02, -0.01, 0.005])

RAGGED = (6, 64, 65, 117, 1024, 88, 20, 65, 64)


@dataclasses.dataclass
class Case:
    off: np.ndarray     # [V + 1]
    obj: np.ndarray     # [C, 3]
    img: np.ndarray     # [C, 2]
    g: np.ndarray       # [12] the parameters the pixels were made with
    poses: np.ndarray   # [V, 6] (rvec, tvec)

    @property
    def n_views(self):
        return len(self.off) - 1

    def view(self, v):
        return slice(int(self.off[v]), int(self.off[v + 1]))

    def permuted(self, order):
        """The same views in another order."""
        sl = [self.view(v) for v in order]
        off = np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.int32)
        return Case(off, np.concatenate([self.obj[s] for s in sl]), np.concatenate([self.img[s] for s in sl]), self.g,
                    self.poses[list(order)])


def grid(n, relief=0.0):
    """n corners of a near-square grid centred on the origin; relief (mm) lifts them off the plane."""
    w = int(np.ceil(np.sqrt(n)))
    pitch = min(40.0, 400.0 / max(w - 1, 1))
    i = np.arange(n)
    a, b = i % w, i // w
    X = np.stack([pitch * (a - 0.5 * (w - 1)), pitch * (b - 0.5 * ((n - 1) // w)),
                  relief * np.sin(0.7 * b + 1.3 * a)], axis=1)
    return X.astype(np.float64)


def make(corners, seed, noise=0.0, relief=0.0, g=G_TRUE, view_r=None):
    """One view per entry of `corners`.  view_r: {view: rotation vector} for views whose rotation is prescribed."""
    rng = np.random.default_rng(seed)
    obj, img, poses, off = [], [], [], [0]
    for v, n in enumerate(corners):
        tilt = np.deg2rad(rng.uniform(10.0, 45.0))
        phi = 2.399963 * v + rng.uniform(0.0, 0.5)   # the golden angle: axes spread over the circle
        r = np.array([tilt * np.cos(phi), tilt * np.sin(phi), rng.uniform(-0.3, 0.3)])
        if view_r and v in view_r:
            r = np.asarray(view_r[v], np.float64)
        t = np.array([rng.uniform(-60.0, 60.0), rng.uniform(-40.0, 40.0), rng.uniform(500.0, 1200.0)])
        X = grid(n, relief)
        obj.append(X)
        img.append(npcalib.project(X, r, t, g))
        poses.append(np.concatenate([r, t]))
        off.append(off[-1] + n)
    img = np.concatenate(img)
    if noise:
        img = img + noise * rng.standard_normal(img.shape)
    return Case(np.asarray(off, np.int32), np.concatenate(obj), img, np.asarray(g, np.float64).copy(), np.asarray(poses))


# cv::CALIB_* (include/mcc.h: MCC_CALIB_*)
USE_GUESS, FIX_ASPECT, FIX_PP, ZERO_TANGENT, FIX_FOCAL, FIX_K1, FIX_K2, FIX_K3, RATIONAL = 1, 2, 4, 8, 16, 32, 64, 128, 16384
FIX_K4, FIX_K5, FIX_K6 = 2048, 4096, 8192
ALL_FIXED = USE_GUESS | FIX_PP | ZERO_TANGENT | FIX_FOCAL | FIX_K1 | FIX_K2 | FIX_K3


# What tests/npcalib.py resolves on the noisy cases below, measured once: its largest last
# Gauss-Newton step (dK relative in fx fy cx cy, dD, dr, dt in mm) and its largest gamma at its own minimum.
REF_RESOLUTION = dict(dK=1.1e-8, dD=3.9e-6, dr=7.2e-9, dt=6.8e-6, gamma=5.2e-8)


def noisy_cases():
    """(name, case, flags, nd, guess) of every noisy input of tests/test_calibrate_camera.py; guess is the 12-vector
    handed over as K and D with USE_GUESS, else None.  tests/test_calibrate_camera_cpu.py checks that the reference
    handles each of them."""
    out = [(f"17x{n}", make([n] * 17, seed=100 + n, noise=0.2), 0, 5, None) for n in (64, 65, 88)]
    c = make([88] * 17, seed=188, noise=0.2)
    off1 = c.g * 1.01
    pp = off1.copy()
    pp[2:4] = (640.0, 480.0)          # a principal point that is not the truth stays where it is put
    fl = off1.copy()
    fl[0:2] = c.g[0:2] * 1.002        # and so do focal lengths
    out += [("k3_tangent", c, FIX_K3 | ZERO_TANGENT, 5, None),
            ("principal", c, FIX_PP | USE_GUESS, 5, pp),
            ("aspect", c, FIX_ASPECT, 5, None),
            ("focal", c, FIX_FOCAL | USE_GUESS, 5, fl),
            ("relief", make([88] * 17, seed=189, noise=0.2, relief=30.0), USE_GUESS, 5, off1),
            # unequal corner counts under noise: idle lanes (6, 20), 1024 corners, a view's sum in its own slot
            ("ragged9", make(RAGGED, seed=177, noise=0.2), 0, 5, None),
            ("nd4", c, 0, 4, None),
            ("fix_k1_k2", c, USE_GUESS | FIX_K1 | FIX_K2, 5, off1)]
    return out


NEAR_ZERO_VIEW = 2


def step_cases():
    """(name, case, flags, nd, guess) of tests/test_calibrate_camera_steps.py and tests/test_pincalib_step_cpu.py:
    the smallest inputs whose Levenberg-Marquardt trajectory from the guess reaches each path of the trial
    kernels.  Every one starts from a guess (USE_GUESS is in the flags), so that state 0 is known."""
    far = make(RAGGED, seed=77, noise=0.2)
    g_far = far.g.copy()
    g_far[0:2] *= 1.5                 # far enough for a rejected trial: the stored sums are read again
    asp = make([65] * 17, seed=165, noise=0.2)
    nd4 = make([20] * 5, seed=129, noise=0.2)          # groups of 3 + 2 views
    g_nd4 = nd4.g.copy()
    g_nd4[0:2] *= 1.5                 # from 1 % off this case is at its minimum after five steps, and the sixth
    #                                   decision is no longer clear (MARGIN); from here all six steps are far from it
    rat = make([88] * 10, seed=310, g=G_RATIONAL)      # exact: k4 .. k6 are not determined under noise
    four = make([4] * 65, seed=465, noise=0.2)         # groups of 9 views, the last of 2
    # one view almost parallel to the image plane: k_pc_lin's only run of so3_jac's series (|r_v| < 1e-2).  The draw
    # (of 40 tried) on which that view stays under 1e-2 on all six steps; 20 noisy corners hold its tilt to 2e-2 only
    nzv = make([20] * 5, seed=612, noise=0.2, view_r={NEAR_ZERO_VIEW: np.random.default_rng(613).normal(0.0, 2e-3, 3)})
    return [("ragged9/far", far, USE_GUESS, 5, g_far),
            ("17x65/aspect", asp, USE_GUESS | FIX_ASPECT, 5, asp.g * 1.05),
            ("5x20/nd4_pp", nd4, USE_GUESS | FIX_PP, 4, g_nd4),
            ("10x88/rational_k5", rat, USE_GUESS | RATIONAL | FIX_K5, 8, rat.g * 1.01),
            ("65x4", four, USE_GUESS, 5, four.g * 1.01),
            ("5x20/near_zero_view", nzv, USE_GUESS, 5, nzv.g * 1.01)]


# What the step tests walk and where they compare a step with npcalib.lm_step:
K_STEPS = 6        # accepted steps from the start
GAMMA_MIN = 1e-4   # below it J^T e is mostly cancellation; its rounding, about 1e-16 / gamma relative, would set rho
RMS_MIN = 1e-4     # px.  A residual is a difference of pixels near 1.3e3, so an entry carries about 2^-53 * 1.3e3 =
#                    1.4e-13 px of rounding, 1.4e-9 of an rms of 1e-4 px: under that (exact data only, close to the
#                    minimum) the residual's own rounding would set rho, whatever the solver does
MARGIN = 1e-9      # every accept / reject decision on these walks has |en / err - 1| >= MARGIN: the device and the
#                    reference differ near 1e-14 there, so both take the same one


def step_checked(gamma, rms):
    return gamma >= GAMMA_MIN and rms >= RMS_MIN


def state0(flags, nd, guess):
    """The globals mcc_calibrate_camera starts from under USE_GUESS, and the aspect ratio it holds: the guess
    with p1 = p2 = 0 under ZERO_TANGENT, k3 = 0 at nd = 4, the slots past nd at 0 and fx = a fy under FIX_ASPECT."""
    g = np.zeros(12)
    g[:4 + nd] = np.asarray(guess, np.float64)[:4 + nd]
    aspect = float(g[0] / g[1]) if flags & FIX_ASPECT else 0.0
    if flags & ZERO_TANGENT:
        g[6:8] = 0.0
    if nd == 4:
        g[8] = 0.0
    if aspect > 0:
        g[0] = aspect * g[1]
    return g, aspect


def lm_lambdas(rejections):
    """lambda at the start of every accepted step, given the rejections before each: the documented policy from
    1e-3, x 10 on a rejection, x 0.1 floored at 1e-12 on an accepted step."""
    lam, out = 1e-3, []
    for r in rejections:
        out.append(lam)
        for _ in range(r):
            lam = lam * 10.0
        lam = max(lam * 0.1, 1e-12)
    return out


def reference_start(c, flags, mask, guess):
    """The globals tests/npcalib.py starts from: the truth at the free slots, and at the fixed ones what the
    library holds there (the guess, or zero distortion without one)."""
    g = c.g.copy()
    for k in range(12):
        if not mask[k] and not (k == 0 and flags & FIX_ASPECT):
            g[k] = guess[k] if guess is not None else (0.0 if k >= 4 else g[k])
    return g


def guess_KD(guess, nd):
    K = np.array([[guess[0], 0, guess[2]], [0, guess[1], guess[3]], [0, 0, 1.0]])
    return K, np.asarray(guess[4:4 + nd], np.float64).copy()
