"""A reference for calibrateCamera's answer that shares nothing with the device code (float64 NumPy).

mcc_calibrate_camera starts from a closed form, runs Levenberg-Marquardt with an analytic Jacobian and solves
every trial by the block-arrow elimination.  This module does none of that: it starts from the parameters
the data were made with, takes its Jacobian by central differences of its own projection, and solves the
dense least-squares problem with lstsq.

  project(X, r, t, g)                     cv::projectPoints' model, g = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
  gauss_newton(case, g0, poses0, mask)    the least-squares minimum next to the start: g, poses, rms, steps
  gamma(case, g, poses, mask)             sqrt(g^T H^-1 g) / |e| over the free parameters: 0 at a minimum
  rms(case, g, poses)

`case` is anything with off [V + 1], obj [C, 3], img [C, 2] (tests/calib_cases.py).  mask is the 0/1 vector of free
global slots; aspect > 0 ties fx = aspect fy (then mask[0] is 0 and the fy column carries both).
"""
from __future__ import annotations

import numpy as np


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def project(X, r, t, g):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = np.asarray(g, np.float64)
    Xc = X @ rodrigues(r).T + np.asarray(t, np.float64)
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    cd = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def _tied(g, aspect):
    g = np.array(g, np.float64)
    if aspect > 0:
        g[0] = aspect * g[1]
    return g


def residuals(case, g, poses):
    """observed - projected, [2C]."""
    e = np.empty((len(case.obj), 2))
    for v in range(len(case.off) - 1):
        s = slice(int(case.off[v]), int(case.off[v + 1]))
        e[s] = case.img[s] - project(case.obj[s], poses[v, :3], poses[v, 3:], g)
    return e.ravel()


def rms(case, g, poses):
    e = residuals(case, g, poses)
    return float(np.sqrt(e @ e / len(case.obj)))


def _jacobian(case, g, poses, free, aspect):
    """d projected / d (free globals, every pose) by central differences, [2C, len(free) + 6V]."""
    V, C = len(case.off) - 1, len(case.obj)
    J = np.zeros((2 * C, len(free) + 6 * V))
    for c, k in enumerate(free):
        # the pixels are linear in fx fy cx cy k1 k2 p1 p2 k3, so a central difference is exact at any step
        # and a long one keeps its rounding small; k4 k5 k6 enter through the denominator
        h = (1e-3 if k < 9 else 1e-5) * max(1.0, abs(g[k]))
        gp, gm = np.array(g), np.array(g)
        gp[k] += h
        gm[k] -= h
        J[:, c] = (residuals(case, _tied(gm, aspect), poses) - residuals(case, _tied(gp, aspect), poses)) / (2 * h)
    for v in range(V):
        s = slice(int(case.off[v]), int(case.off[v + 1]))
        rows = slice(2 * s.start, 2 * s.stop)
        for k in range(6):
            h = 1e-6 * max(1.0, abs(poses[v, k]))
            pp, pm = poses[v].copy(), poses[v].copy()
            pp[k] += h
            pm[k] -= h
            J[rows, len(free) + 6 * v + k] = (project(case.obj[s], pp[:3], pp[3:], g) -
                                              project(case.obj[s], pm[:3], pm[3:], g)).ravel() / (2 * h)
    return J


def gauss_newton(case, g0, poses0, mask, aspect=0.0, max_steps=50, tol=1e-8, return_last=False):
    """Undamped Gauss-Newton from (g0, poses0) until a step is below tol of the parameters' norm.
    Returns g, poses, rms and the number of steps taken (max_steps + 1 when it did not get there); with
    return_last also the last step as (dg [12], dposes [V, 6]): what the result itself is uncertain by.
    tol: the pose columns are differences of pixels near 1e3 (rounding 1e-13) over h = 1e-6, so an entry carries
    1e-7 of noise on a magnitude of 1e3, and the steps stop shrinking at about 1e-9 of |x|; the rms is stable to
    1e-14 relative from there on.  1e-8 sits one decade above that floor."""
    free = [k for k in range(12) if mask[k]]
    g, poses = _tied(g0, aspect), np.array(poses0, np.float64)
    for step in range(1, max_steps + 1):
        e = residuals(case, g, poses)
        J = _jacobian(case, g, poses, free, aspect)
        d = np.linalg.lstsq(J, e, rcond=None)[0]
        xn = np.sqrt(g[free] @ g[free] + (poses * poses).sum())
        g_before = g.copy()
        g[free] += d[:len(free)]
        g = _tied(g, aspect)
        poses += d[len(free):].reshape(-1, 6)
        if np.linalg.norm(d) < tol * xn or step == max_steps:
            steps = step if np.linalg.norm(d) < tol * xn else max_steps + 1
            out = (g, poses, rms(case, g, poses), steps)
            return out + ((g - g_before, d[len(free):].reshape(-1, 6)),) if return_last else out


def gamma(case, g, poses, mask, aspect=0.0):
    """The cosine of the angle between the residual and the Jacobian's column space (free parameters only)."""
    free = [k for k in range(12) if mask[k]]
    g = _tied(g, aspect)
    e = residuals(case, g, np.asarray(poses, np.float64))
    J = _jacobian(case, g, np.asarray(poses, np.float64), free, aspect)
    p = J @ np.linalg.lstsq(J, e, rcond=None)[0]   # the projection of e on the column space: |p|^2 = g^T H^-1 g
    return float(np.linalg.norm(p) / max(np.linalg.norm(e), 1e-300))
