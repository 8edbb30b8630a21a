"""tests/nppnp.py, the NumPy reference that tests/test_pnp_generic.py holds k_pnp to, checked on its own
(no GPU): a reference that is wrong would make those tests assert the wrong thing.

* log_so3 inverts npmodel.rodrigues at every angle, pi and its neighbourhood included;
* compose_truth: the moved target under the composed pose lands on the pixels of the original;
* refine: on exact data started off the truth it returns the truth; on noisy data it ends at a point
  where the gradient J^T e of a Jacobian taken with another step vanishes;
* stationarity is near zero there and first order in a displacement from it: a pose moved by d along
  a parameter has gamma = |J d| / |e| to first order, which is what makes it a measure of "stalled short
  of the minimum"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npmodel as N  # noqa: E402
import nppnp as P  # noqa: E402

K = np.array([[1200.0, 0, 960], [0, 1180, 540], [0, 0, 1]])
D = np.array([-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003, 1e-3, -5e-4, -8e-4, 3e-4])
PI = np.pi


def _grid(n=30, relief=20.0):
    i = np.arange(n)
    a, b = i % 6, i // 6
    return np.stack([40.0 * a - 100, 40.0 * b - 80, relief * np.sin(0.7 * b + 1.3 * a)], 1)


@pytest.mark.parametrize("r", [(0, 0, 0), (1e-9, 0, 0), (0, 5e-3, 0), (0.3, -0.4, 0.2), (1.2, 0.1, -0.2), (0.1, 0.1, 3.0),
                               (2.2, -2.2, 0.01), (PI, 0, 0), (0, PI - 1e-7, 0), ((PI - 1e-4) * 0.6, (PI - 1e-4) * 0.8, 0),
                               (0, 0, PI - 1e-10), (-1.8, 1.8, 1.8)])
def test_log_so3_inverts_rodrigues(r):
    r = np.array(r, float)
    got = P.log_so3(N.rodrigues(r))
    assert np.abs(N.rodrigues(got) - N.rodrigues(r)).max() < 1e-15
    if np.linalg.norm(r) < PI - 1e-9:   # (at pi itself r and -r are one rotation)
        assert np.abs(got - r).max() < 1e-14


def test_compose_truth_keeps_the_pixels():
    obj = _grid()
    Ro, to = N.rodrigues([0.7, -0.5, 0.3]), np.array([5000.0, -3000.0, 2000.0])
    for r, t in [((0.0, 0.0, 0.0), (40.0, -30.0, 1300.0)), ((PI, 0.0, 0.0), (-35.0, 30.0, 1250.0)),
                 ((1.2, 0.1, -0.2), (20.0, -25.0, 1450.0))]:
        rn, tn = P.compose_truth((np.array(r), np.array(t)), Ro, to)
        a = N.project_pinhole(obj, r, t, K, D)
        b = N.project_pinhole(obj @ Ro.T + to, rn, tn, K, D)
        assert np.abs(a - b).max() < 1e-9   # 6 m coordinates: 1e-12 mm of rounding, times f / Z


def test_refine_returns_the_truth_on_exact_data():
    obj = _grid()
    r, t = np.array([0.3, -0.4, 0.2]), np.array([-50.0, 30.0, 1300.0])
    img = N.project_pinhole(obj, r, t, K, D)
    r1, t1, rms = P.refine(obj, img, K, D, r + [0.02, -0.01, 0.015], t + [5.0, -4.0, 20.0])
    assert rms < 1e-9 and np.abs(r1 - r).max() < 1e-10 and np.abs(t1 - t).max() < 1e-7


def test_refine_ends_where_the_gradient_vanishes_and_stationarity_measures_the_distance():
    rng = np.random.default_rng(7)
    obj = _grid()
    r, t = np.array([0.3, -0.4, 0.2]), np.array([-50.0, 30.0, 1300.0])
    img = N.project_pinhole(obj, r, t, K, D) + 0.2 * rng.normal(size=(len(obj), 2))
    r1, t1, rms = P.refine(obj, img, K, D, r, t)
    assert 0.1 < rms < 0.5
    x = np.concatenate([r1, t1])
    f = lambda p: N.project_pinhole(obj, p[:3], p[3:], K, D).ravel()   # noqa: E731
    J = N.fd_jacobian(f, x, range(6), h=1e-5)                           # another step than refine's
    e = img.ravel() - f(x)
    g = J.T @ e
    assert np.sqrt(g @ np.linalg.solve(J.T @ J, g)) / np.linalg.norm(e) < 1e-6
    assert P.stationarity(obj, img, K, D, r1, t1) < 1e-6
    # moved by d, gamma is |J d| / |e| to first order (second order: the relative size of the step, 1e-3)
    for k, d in ((1, 1e-5), (5, 1e-2)):
        dx = np.zeros(6)
        dx[k] = d
        want = np.linalg.norm(J @ dx) / np.linalg.norm(e)
        got = P.stationarity(obj, img, K, D, r1 + dx[:3], t1 + dx[3:])
        assert abs(got - want) < 1e-2 * want + 1e-6, (k, got, want)
