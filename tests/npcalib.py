"""A reference for calibrateCamera's answer that shares nothing with the device code (float64 NumPy).

mcc_calibrate_camera starts from a closed form, runs Levenberg-Marquardt with an analytic Jacobian and solves
every trial by the block-arrow elimination.  This module does none of that: it starts from the parameters
the data were made with, takes its Jacobian by central differences of its own projection, and solves the
dense least-squares problem with lstsq.  lm_step, the reference of one Levenberg-Marquardt trial, takes its
Jacobian by complex-step differentiation of a second projection (exact to rounding: there is no difference
to cancel) and solves the damped problem as a dense lstsq on the augmented matrix, never normal equations.

  project(X, r, t, g)                     cv::projectPoints' model, g = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
  gauss_newton(case, g0, poses0, mask)    the least-squares minimum next to the start: g, poses, rms, steps
  gamma(case, g, poses, mask)             sqrt(g^T H^-1 g) / |e| over the free parameters: 0 at a minimum
  rms(case, g, poses)
  lm_step(case, g, poses, mask, lam)      one damped step from (g, poses): the minimiser of
                                          |e - J d|^2 + lam d^T diag(J^T J) d, with J exact to rounding
  lm_rejections(case, g, poses, mask, lam)  the trials rejected before one is accepted, and that step
  rho(J, free, test, ref)                 |J (d_test - d_ref)| / |J d_ref|: two steps' difference in pixels

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


def gamma(case, g, poses, mask, aspect=0.0, lin=None):
    """The cosine of the angle between the residual and the Jacobian's column space (free parameters only).
    lin = (J, e) as lm_step returns them at the same point saves forming them again."""
    free = [k for k in range(12) if mask[k]]
    g = _tied(g, aspect)
    if lin is None:
        lin = (_jacobian(case, g, np.asarray(poses, np.float64), free, aspect),
               residuals(case, g, np.asarray(poses, np.float64)))
    J, e = lin
    p = J @ np.linalg.lstsq(J, e, rcond=None)[0]   # the projection of e on the column space: |p|^2 = g^T H^-1 g
    return float(np.linalg.norm(p) / max(np.linalg.norm(e), 1e-300))


# ---------------------------------------------------------------- one damped step, exact Jacobian
def _rodrigues_c(w):
    """rodrigues for a complex w (analytic continuation: th = sqrt(w . w), no conjugate); near th = 0 the
    limit forms sin th / th = 1 - th^2 / 6 and (1 - cos th) / th^2 = 1 / 2 - th^2 / 24."""
    w = np.asarray(w, np.complex128)
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if abs(t2) < 1e-12:
        a, b = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        th = np.sqrt(t2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t2
    return np.eye(3) + a * Wx + b * (Wx @ Wx)


def _project_c(X, r, t, g):
    """project() once more, on complex parameters (no float64 casts)."""
    Xc = X @ _rodrigues_c(r).T + np.asarray(t, np.complex128)
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    cd = (1 + r2 * (g[4] + r2 * (g[5] + r2 * g[8]))) / (1 + r2 * (g[9] + r2 * (g[10] + r2 * g[11])))
    xd = x * cd + 2 * g[6] * x * y + g[7] * (r2 + 2 * x * x)
    yd = y * cd + g[6] * (r2 + 2 * y * y) + 2 * g[7] * x * y
    return np.stack([g[0] * xd + g[2], g[1] * yd + g[3]], axis=1)


def exact_jacobian(case, g, poses, free, aspect=0.0, h=1e-30):
    """d projected / d (free globals, every pose) by complex steps, [2C, len(free) + 6V]: Im f(x + ih) / h has no
    subtraction, so every entry is exact to the rounding of one evaluation.  aspect > 0: the fy column moves fx
    along (g[0] = aspect g[1])."""
    V, C = len(case.off) - 1, len(case.obj)
    J = np.zeros((2 * C, len(free) + 6 * V))
    g = np.asarray(g, np.float64)
    for v in range(V):
        s = slice(int(case.off[v]), int(case.off[v + 1]))
        rows = slice(2 * s.start, 2 * s.stop)
        X = np.asarray(case.obj[s], np.float64)
        for c, k in enumerate(free):
            gc = g.astype(np.complex128)
            gc[k] += 1j * h
            if aspect > 0:
                gc[0] = aspect * gc[1]
            J[rows, c] = _project_c(X, poses[v, :3], poses[v, 3:], gc).imag.ravel() / h
        for k in range(6):
            pc = np.asarray(poses[v], np.complex128).copy()
            pc[k] += 1j * h
            J[rows, len(free) + 6 * v + k] = _project_c(X, pc[:3], pc[3:], g).imag.ravel() / h
    return J


def lm_step(case, g, poses, mask, lam, aspect=0.0, lin=None):
    """The Levenberg-Marquardt trial step from (g, poses) at damping lam: the d over the free globals and every
    pose that minimises |e - J d|^2 + lam d^T diag(J^T J) d.  Returns (dg [12], dposes [V, 6], J, e); dg is 0 at
    fixed slots, and under aspect dg[0] = aspect dg[1] (_tied's convention: fx follows fy).

    The solve is lstsq on the augmented matrix [J; sqrt(lam colsumsq(J)) I] with its columns scaled to unit
    length in J (y = |J_k| d_k turns it into [J^; sqrt(lam) I] y ~ [e; 0], the same minimiser, and keeps lstsq's
    rank cut-off away from the slots whose columns are 1e6 apart in length).  lin = (J, e) of an earlier call at
    the same point saves forming them again for another lam."""
    free = [k for k in range(12) if mask[k]]
    g = _tied(g, aspect)
    poses = np.array(poses, np.float64)
    if lin is None:
        lin = exact_jacobian(case, g, poses, free, aspect), residuals(case, g, poses)
    J, e = lin
    n = np.sqrt((J * J).sum(axis=0))
    n[n == 0.0] = 1.0
    A = np.vstack([J / n, np.sqrt(lam) * np.eye(J.shape[1])])
    y = np.linalg.lstsq(A, np.concatenate([e, np.zeros(J.shape[1])]), rcond=None)[0]
    d = y / n
    dg = np.zeros(12)
    dg[free] = d[:len(free)]
    if aspect > 0:
        dg[0] = aspect * dg[1]
    return dg, d[len(free):].reshape(-1, 6), J, e


def lm_rejections(case, g, poses, mask, lam, aspect=0.0, max_tries=10):
    """The trials Levenberg-Marquardt rejects at (g, poses) before it accepts one: the first j with
    rms(state + lm_step at lam 10^j) <= rms(state).  Returns (j, the accepted step as lm_step returns it, the
    ratio en / err of every trial's squared errors, the accepted one last)."""
    g = _tied(g, aspect)
    err = rms(case, g, poses) ** 2
    lin, ratios = None, []
    for j in range(max_tries):
        dg, dp, J, e = lm_step(case, g, poses, mask, lam, aspect, lin)
        lin = (J, e)
        ratios.append(rms(case, _tied(g + dg, aspect), poses + dp) ** 2 / err)
        if ratios[-1] <= 1.0:
            return j, (dg, dp, J, e), ratios
        lam = lam * 10.0
    raise RuntimeError(f"no accepted step within {max_tries} trials: {ratios}")


def rho(J, free, test, ref):
    """|J (d_test - d_ref)| / |J d_ref| for two steps given as (dg [12], dposes [V, 6]): their difference where it
    is observable, in pixels, so that it does not inherit J^T J's conditioning."""
    vec = lambda s: np.concatenate([np.asarray(s[0], np.float64)[free], np.asarray(s[1], np.float64).ravel()])
    dr = vec(ref)
    return float(np.linalg.norm(J @ (vec(test) - dr)) / np.linalg.norm(J @ dr))
