"""A reference for the pinhole stereoCalibrate's answer that shares nothing with the device code (float64 NumPy).

mcc_stereo_calibrate linearises each camera on its own, carries the second camera's sums to the view's and the
rig's coordinates by two 6 x 6 maps after the reduction, and solves every trial by the block-arrow elimination
of a 30-wide global block.  This module does none of that: it states the objective -- both cameras' pixels
through npcalib's projection, camera 2 seeing the point R_v X + t_v through the rig pose (om, T) -- takes its
Jacobian by complex steps of that statement and solves dense least-squares problems with lstsq: no
elimination, no chain rule after a reduction, no normal equations.

The 30 global slots are g = om [3] | T [3] | camera 1's fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 | camera 2's.
ties = (aspect1, aspect2, same): aspect > 0 holds that camera's fx = aspect fy; same holds camera 2's fx, fy at
camera 1's (then slots 18, 19 are not free and camera 1's columns carry both cameras').

  tied(g, ties)                               the slots with the ties applied, in the library's order
  residuals(case, g, poses)                   observed - projected, camera 1's [2C] then camera 2's [2C]
  view_sq(case, g, poses)                     [V, 2] squared error per view and camera
  rms(case, g, poses)                         sqrt(sum |e|^2 / (2 C)), as cv::stereoCalibrate returns it
  exact_jacobian(case, g, poses, free, ties)  d projected / d (free slots, every pose), [4C, len(free) + 6V]
  gauss_newton(case, g0, poses0, mask, ties)  the least-squares minimum next to the start
  gamma, lm_step, lm_rejections, rho          as in npcalib

`case` is a stereo_calib_cases.StereoCase (off, obj, img1, img2).  mask is the 0/1 vector of the 30 slots.
"""
from __future__ import annotations

import numpy as np

import npcalib

NO_TIES = (0.0, 0.0, 0)
RIG, CAM1, CAM2 = 0, 6, 18


def tied(g, ties):
    a1, a2, same = ties
    g = np.array(g)
    if same:
        g[CAM2:CAM2 + 2] = g[CAM1:CAM1 + 2]
    if a1 > 0:
        g[CAM1] = a1 * g[CAM1 + 1]
    if a2 > 0:
        g[CAM2] = a2 * g[CAM2 + 1]
    return g


def project2(X, g, pose):
    """Both cameras' pixels of the points X at the view pose (r, t) in camera 1: [n, 2] each."""
    X1 = np.asarray(X, np.float64) @ npcalib.rodrigues(pose[:3]).T + pose[3:]
    return (npcalib.project(X, pose[:3], pose[3:], g[CAM1:CAM2]),
            npcalib.project(X1, g[0:3], g[3:6], g[CAM2:]))


def _project2_c(X, g, pose):
    X1 = X @ npcalib._rodrigues_c(pose[:3]).T + np.asarray(pose[3:], np.complex128)
    return (npcalib._project_c(X, pose[:3], pose[3:], g[CAM1:CAM2]),
            npcalib._project_c(X1, g[0:3], g[3:6], g[CAM2:]))


def residuals(case, g, poses):
    C = len(case.obj)
    e = np.empty((2, C, 2))
    for v in range(case.n_views):
        s = case.view(v)
        p1, p2 = project2(case.obj[s], g, poses[v])
        e[0, s] = case.img1[s] - p1
        e[1, s] = case.img2[s] - p2
    return e.ravel()


def view_sq(case, g, poses):
    e = residuals(case, g, poses).reshape(2, -1, 2)
    return np.array([[(e[c, case.view(v)] ** 2).sum() for c in range(2)] for v in range(case.n_views)])


def rms(case, g, poses):
    e = residuals(case, g, poses)
    return float(np.sqrt(e @ e / (2 * len(case.obj))))


def exact_jacobian(case, g, poses, free, ties=NO_TIES, h=1e-30):
    """Complex steps: Im f(x + ih) / h has no subtraction, so every entry is exact to the rounding of one
    evaluation.  The ties are applied to the perturbed slots, so a tied slot moves with the one it follows."""
    V, C = case.n_views, len(case.obj)
    J = np.zeros((2, C, 2, len(free) + 6 * V))
    g = np.asarray(g, np.float64)
    for v in range(V):
        s = case.view(v)
        X = np.asarray(case.obj[s], np.float64)
        for c, k in enumerate(free):
            gc = g.astype(np.complex128)
            gc[k] += 1j * h
            p1, p2 = _project2_c(X, tied(gc, ties), poses[v])
            J[0, s, :, c] = p1.imag / h
            J[1, s, :, c] = p2.imag / h
        for k in range(6):
            pc = np.asarray(poses[v], np.complex128).copy()
            pc[k] += 1j * h
            p1, p2 = _project2_c(X, g, pc)
            J[0, s, :, len(free) + 6 * v + k] = p1.imag / h
            J[1, s, :, len(free) + 6 * v + k] = p2.imag / h
    return J.reshape(4 * C, -1)


def _free(mask):
    return [k for k in range(30) if mask[k]]


def gauss_newton(case, g0, poses0, mask, ties=NO_TIES, max_steps=50, tol=1e-10, return_last=False):
    """Undamped Gauss-Newton from (g0, poses0) until a step is below tol of the parameters' norm.  Returns g,
    poses, rms and the number of steps taken (max_steps + 1 when it did not get there); with return_last also
    the last step as (dg [30], dposes [V, 6]): what the result itself is uncertain by.  The Jacobian is exact to
    rounding, so the steps shrink to about 1e-12 of |x|; 1e-10 sits above that floor."""
    free = _free(mask)
    g, poses = tied(np.asarray(g0, np.float64), ties), np.array(poses0, np.float64)
    for step in range(1, max_steps + 1):
        e = residuals(case, g, poses)
        J = exact_jacobian(case, g, poses, free, ties)
        n = np.sqrt((J * J).sum(axis=0))
        n[n == 0.0] = 1.0
        d = np.linalg.lstsq(J / n, e, rcond=None)[0] / n
        xn = np.sqrt(g[free] @ g[free] + (poses * poses).sum())
        g_before = g.copy()
        g[free] += d[:len(free)]
        g = tied(g, ties)
        poses = poses + d[len(free):].reshape(-1, 6)
        if np.linalg.norm(d) < tol * xn or step == max_steps:
            steps = step if np.linalg.norm(d) < tol * xn else max_steps + 1
            out = (g, poses, rms(case, g, poses), steps)
            return out + ((g - g_before, d[len(free):].reshape(-1, 6)),) if return_last else out


def gamma(case, g, poses, mask, ties=NO_TIES, lin=None):
    """The cosine of the angle between the residual and the Jacobian's column space (free parameters only)."""
    g = tied(g, ties)
    if lin is None:
        lin = (exact_jacobian(case, g, np.asarray(poses, np.float64), _free(mask), ties),
               residuals(case, g, np.asarray(poses, np.float64)))
    J, e = lin
    n = np.sqrt((J * J).sum(axis=0))
    n[n == 0.0] = 1.0
    p = (J / n) @ np.linalg.lstsq(J / n, e, rcond=None)[0]
    return float(np.linalg.norm(p) / max(np.linalg.norm(e), 1e-300))


def lm_step(case, g, poses, mask, lam, ties=NO_TIES, lin=None):
    """The Levenberg-Marquardt trial step from (g, poses) at damping lam: the d over the free slots and every
    pose that minimises |e - J d|^2 + lam d^T diag(J^T J) d, by lstsq on the augmented, column-scaled matrix
    (npcalib.lm_step's form).  Returns (dg [30], dposes [V, 6], J, e); dg is 0 at fixed slots and follows the
    ties at tied ones."""
    free = _free(mask)
    g = tied(g, ties)
    poses = np.array(poses, np.float64)
    if lin is None:
        lin = exact_jacobian(case, g, poses, free, ties), residuals(case, g, poses)
    J, e = lin
    n = np.sqrt((J * J).sum(axis=0))
    n[n == 0.0] = 1.0
    A = np.vstack([J / n, np.sqrt(lam) * np.eye(J.shape[1])])
    y = np.linalg.lstsq(A, np.concatenate([e, np.zeros(J.shape[1])]), rcond=None)[0]
    d = y / n
    dg = np.zeros(30)
    dg[free] = d[:len(free)]
    dg = tied(g + dg, ties) - g
    return dg, d[len(free):].reshape(-1, 6), J, e


def lm_rejections(case, g, poses, mask, lam, ties=NO_TIES, max_tries=10):
    """The trials Levenberg-Marquardt rejects at (g, poses) before it accepts one.  Returns (j, the accepted step
    as lm_step returns it, the ratio en / err of every trial's squared errors, the accepted one last)."""
    g = tied(g, ties)
    err = rms(case, g, poses) ** 2
    lin, ratios = None, []
    for j in range(max_tries):
        dg, dp, J, e = lm_step(case, g, poses, mask, lam, ties, lin)
        lin = (J, e)
        ratios.append(rms(case, tied(g + dg, ties), poses + dp) ** 2 / err)
        if ratios[-1] <= 1.0:
            return j, (dg, dp, J, e), ratios
        lam = lam * 10.0
    raise RuntimeError(f"no accepted step within {max_tries} trials: {ratios}")


def rho(J, free, test, ref):
    """|J (d_test - d_ref)| / |J d_ref| for two steps given as (dg [30], dposes [V, 6])."""
    return npcalib.rho(J, free, test, ref)


def essential(om, T):
    R = npcalib.rodrigues(om)
    Tx = np.array([[0.0, -T[2], T[1]], [T[2], 0.0, -T[0]], [-T[1], T[0], 0.0]])
    return Tx @ R


def fundamental(g, E=None):
    """F = K2^-T E K1^-1 scaled to F[2, 2] = 1."""
    E = essential(g[0:3], g[3:6]) if E is None else E
    K = lambda c: np.array([[c[0], 0.0, c[2]], [0.0, c[1], c[3]], [0.0, 0.0, 1.0]])
    F = np.linalg.inv(K(g[CAM2:CAM2 + 4])).T @ E @ np.linalg.inv(K(g[CAM1:CAM1 + 4]))
    return F / F[2, 2] if F[2, 2] != 0 else F
