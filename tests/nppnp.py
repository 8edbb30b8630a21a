"""A reference for solvePnP's answer that is neither of the project's solvers (float64 NumPy).

mcc::pnp::solvePnP (host/pnp.cpp) and k_pnp (csrc/mcc_pnp_device.hpp) share their closed-form start and
their Levenberg-Marquardt policy, so "the GPU reached the host's rms" cannot see a fault the two have in
common, nor a Jacobian that is slightly wrong and still descends.  This module has neither: it starts
from the pose the data were made with, takes its Jacobian by central differences of
npmodel.project_pinhole, and knows nothing of planes, homographies or DLTs.

  refine(obj, img, K, D, r0, t0)       the least-squares minimum next to (r0, t0): r, t, rms
  stationarity(obj, img, K, D, r, t)   how far a pose is from any minimum, dimensionless
  compose_truth(pose, Ro, to)          the pose that maps a rigidly moved target to the same pixels
  log_so3(R)                           matrix -> vector at every angle in [0, pi]
"""
from __future__ import annotations

import numpy as np

import npmodel as N


def _pixels(obj, K, D, x):
    return N.project_pinhole(obj, x[:3], x[3:], K, D).ravel()


def _linearise(obj, img, K, D, x):
    """Residual e = observed - projected [2n] and J = d projected / d (r, t) [2n, 6]."""
    e = np.asarray(img, np.float64).ravel() - _pixels(obj, K, D, x)
    J = N.fd_jacobian(lambda p: _pixels(obj, K, D, p), x, range(6), h=1e-6)
    return e, J


def refine(obj, img, K, D, r0, t0, max_steps=100):
    """Damped Gauss-Newton on the reprojection error from (r0, t0): the full step, halved until the sum
    of squares decreases (at most ten times), until no such step decreases it.  Returns r, t, rms."""
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    x = np.concatenate([np.asarray(r0, np.float64), np.asarray(t0, np.float64)])
    e, J = _linearise(obj, img, K, D, x)
    f = e @ e
    for _ in range(max_steps):
        d = np.linalg.solve(J.T @ J, J.T @ e)
        alpha, moved = 1.0, False
        for _ in range(11):
            xn = x + alpha * d
            en = np.asarray(img, np.float64).ravel() - _pixels(obj, K, D, xn)
            if en @ en < f:
                x, f, moved = xn, en @ en, True
                break
            alpha *= 0.5
        if not moved:
            break
        e, J = _linearise(obj, img, K, D, x)
    return x[:3].copy(), x[3:].copy(), float(np.sqrt(f / len(obj)))


def stationarity(obj, img, K, D, r, t):
    """gamma = sqrt(g^T H^-1 g) / |e| with g = J^T e, H = J^T J from the reference Jacobian: the cosine
    of the angle between the residual and the Jacobian's column space, zero at a minimum."""
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    e, J = _linearise(obj, img, K, D, np.concatenate([np.asarray(r, np.float64), np.asarray(t, np.float64)]))
    g = J.T @ e
    return float(np.sqrt(max(g @ np.linalg.solve(J.T @ J, g), 0.0)) / np.linalg.norm(e))


def log_so3(R):
    """Matrix -> vector for theta in [0, pi].  Away from pi the skew part gives the axis; near pi, where
    it vanishes, the axis is the largest column of the symmetric part (R + R^T) / 2 - c I = (1 - c) k k^T
    and the skew part only gives its sign."""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if c > -0.5:
        return v * (0.5 if s < 1e-8 else th / (2.0 * s))   # sin(th) / th = 1 to 1e-16 below 1e-8
    S = 0.5 * (R + R.T) - c * np.eye(3)
    k = S[:, int(np.argmax(np.diag(S)))]
    k = k / np.linalg.norm(k)
    if k @ v < 0:
        k = -k
    return th * k


def compose_truth(pose, Ro, to):
    """A target moved by X' = Ro X + to is seen at the same pixels from the pose (r', t') with
    R' = R Ro^T and t' = t - R' to, for pose = (r, t)."""
    r, t = pose
    Ro = np.asarray(Ro, np.float64).reshape(3, 3)
    Rn = N.rodrigues(r) @ Ro.T
    return log_so3(Rn), np.asarray(t, np.float64) - Rn @ np.asarray(to, np.float64)
