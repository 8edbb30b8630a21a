"""Oracle vs the committed golden fixtures (tests/golden/*.npz, made by tests/golden/make_golden.py).

Also pins SURVEY.md 8(c) (vi): the faithful dense-CG deltaX and the exact Schur deltaX agree.
CPU only: the GPU path is checked against the same fixtures in tests/test_gpu_parity.py.
"""
import glob
import os
import sys

import numpy as np
import pytest

from multi_camera_calibration_amd import rig
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))
REGEN = make_golden.CASES


def _name(path):
    return os.path.splitext(os.path.basename(path))[0]


@pytest.fixture(scope="module", params=FIXTURES, ids=_name)
def fx(request):
    g = dict(np.load(request.param))   # plain arrays, allow_pickle stays False
    return _name(request.param), g, rig.problem_from_arrays(g)


def test_fixture_set_complete():
    assert sorted(_name(f) for f in FIXTURES) == sorted(REGEN)


def test_generator_reproduces_inputs(fx):
    name, g, p = fx
    q = REGEN[name]()
    if isinstance(q, tuple):
        q, extra = q
        for k, v in extra.items():
            assert np.array_equal(g[k], v), (name, k)
    for f in rig._ARRAY_FIELDS:
        a, b = getattr(p, f), getattr(q, f)
        assert (a is None) == (b is None), f
        if a is not None:
            assert np.array_equal(a, b), (name, f)


def test_oracle_matches_fixture(fx):
    name, g, p = fx
    o = O.Oracle(p)
    resid = np.concatenate([o.edge_linearize(p.x0, e)[2] for e in range(p.n_edges)]).astype(np.float32)
    assert np.array_equal(resid, g["resid"]), name
    blocks = [o.edge_linearize(p.x0, int(e)) for e in g["es"]]
    jc = np.concatenate([b[0] for b in blocks])
    jp = np.concatenate([b[1] for b in blocks])
    assert np.abs(jc - g["jc_s"]).max() <= 1e-12 * max(1.0, np.abs(g["jc_s"]).max())
    assert np.abs(jp - g["jp_s"]).max() <= 1e-12 * np.abs(g["jp_s"]).max()
    d, j = o.linearize_solve(p.x0, "schur")
    assert np.abs(j - g["jte"]).max() <= 1e-12 * np.abs(g["jte"]).max()
    assert np.abs(d - g["delta"]).max() <= 1e-9 * np.abs(g["delta"]).max()
    e, m = o.project_error(p.x0)
    assert np.array_equal(e, g["pe_edge"]) and m == float(g["pe_mean"])
    x, mean, iters, change = o.optimize(p.x0, int(g["crit"][0]), int(g["crit"][1]), float(g["crit_eps"]))
    assert iters == int(g["iters_opt"]), name
    assert np.abs(x - g["x_opt"]).max() <= 1e-5 * np.abs(g["x_opt"]).max()
    assert abs(mean - float(g["mean_opt"])) <= 1e-6


def test_faithful_cg_final_iterate(fx):
    """The whole optimizeExtrinsics loop with the reference's own solver in every step (dense
    J^T J + Jacobi-CG solved twice, src/multicalib.cpp:462-514, 565-592) reproduces the fixture's
    final iterate, and the exact Schur solve the GPU path restates reaches the SAME float32
    parameters bit for bit, in the same number of iterations (the CG's cond*eps departure from the
    exact solution never survives the float32 rounding of G and x)."""
    name, g, p = fx
    o = O.Oracle(p)
    x, mean, iters, change = o.optimize(p.x0, int(g["crit"][0]), int(g["crit"][1]), float(g["crit_eps"]),
                                        solver="cg")
    assert iters == int(g["iters_opt_cg"]) and np.array_equal(x, g["x_opt_cg"]), name
    assert mean == float(g["mean_opt_cg"])
    assert int(g["iters_opt"]) == int(g["iters_opt_cg"]), name
    assert np.array_equal(g["x_opt"], g["x_opt_cg"]), name
    assert float(g["mean_opt"]) == float(g["mean_opt_cg"]), name


def test_dense_j_solver_matches_cg():
    """The materialised dense J + gemm products (the ref-faithful CPU baseline's cost model,
    src/mymulticalib.cpp:683, 802-803) give the same normal equations and step as the per-edge
    accumulation of the same products."""
    p = rig.make_config("config1")
    o = O.Oracle(p)
    d1, j1 = o.linearize_solve(p.x0, "cg")
    d2, j2 = o.linearize_solve(p.x0, "dense_j")
    assert np.abs(j1 - j2).max() <= 1e-12 * np.abs(j1).max()
    assert np.abs(d1 - d2).max() <= 1e-9 * np.abs(d1).max()


def test_cg_agrees_with_schur(fx):
    """8(c)(vi): the reference's dense J^T J + Jacobi-CG x2 (src/multicalib.cpp:565-592) and the
    exact block Schur/Cholesky solve give the same deltaX (CG to DBL_EPSILON tolerance)."""
    name, g, p = fx
    assert np.abs(g["delta_cg"] - g["delta"]).max() <= 1e-6 * np.abs(g["delta"]).max(), name


def test_residual_scale_sane(fx):
    """Synthetic corners carry 0.2 px noise and x0 is perturbed: residuals are O(1..10) px and the
    converged reference metric (half the mean L2 error for pinhole) is ~0.12 px except for the
    MyMulti back-side case, whose omitted chain term (src/mymulticalib.cpp:516) stalls it."""
    name, g, p = fx
    assert np.isfinite(g["resid"]).all() and np.abs(g["resid"]).max() < 200
    if name == "tutorial_stereo_v20":
        assert float(g["mean_opt"]) < 0.5   # real corners: the calibrations' rms is ~0.47 px
    elif name != "pinhole_back_v8":
        assert float(g["mean_opt"]) < 0.3
