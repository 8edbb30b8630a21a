"""k_group's phase 0 (mcc_group.hpp: the scalar batch from the host-built group header, one vector batch
into registers, the first round's corners committed to LDS after the photo work) on the smallest rigs
at which it can go wrong, at both lane widths (MCC_FUSED=0 MCC_GROUP=1, 32 lanes and MCC_GROUP_LANES=16):

  case      rig                                              what it exercises
  c4_v3     config4, 3 views (11 edges)                      one partial group: np < 4, gne < 16, clamped header lanes
  c4_v5     config4, 5 views (19 edges)                      a full group plus a one-photo group
  c4_vis    config4, 24 views, visibility 0.5 (56 edges)     photos with 1-4 edges, uneven groups, short lists
  c4_b13x9  config4, 8 views, 13 x 9 board (117 corners)     second chunk restaged after the deferred first commit
  c4_b5x4   config4, 8 views, 5 x 4 board (20 corners)       fewer corners than lanes per edge
  pin_c20   config2, 20 cameras, 6 views (m = 114)           several rounds per group: edges past the header, rb > 0
  c5_v6     config5, 6 views                                 BACK / double-side variant, the transform's thread

Each case is checked
  1. against the CPU oracle at tests/test_gpu_parity.py's bars (residuals bitwise up to float32 rounding
     ties, JTE 1e-9 and delta 1e-6 relative, optimize_extrinsics under COUNT+EPS with 200 iterations: the
     oracle's iteration count and <= 1 ulp per float32 parameter);
  2. bit for bit against the commit before the batching: tests/golden/group_phase0/parent.npz, recorded
     once on the GPU from a build of that commit by tools/make_group_phase0_golden.py (the fixture lives in
     a subdirectory because tests/golden/*.npz are the problem fixtures other suites enumerate).
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ulp import f32_ulp_diff  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    "make_group_phase0_golden", os.path.join(os.path.dirname(HERE), "tools", "make_group_phase0_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "group_phase0", "parent.npz")
_PROBLEMS = {}
_ORACLE = {}


def _problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = MG.CASES[name]()
    return _PROBLEMS[name]


def _oracle_results(name):
    """The oracle's outputs of one rig, computed once for both lane widths."""
    if name not in _ORACLE:
        p = _problem(name)
        o = O.Oracle(p)
        resid = np.concatenate([o.edge_linearize(p.x0, e)[2] for e in range(p.n_edges)]).astype(np.float32)
        d_ref, j_ref = o.linearize_solve(p.x0, "schur")
        x_ref, _, it_ref, _ = o.optimize(p.x0, crit_type=3, max_count=200, eps=MG.eps_of(p))
        _ORACLE[name] = (resid, d_ref, j_ref, x_ref, it_ref)
    return _ORACLE[name]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", params=[(n, l) for n in sorted(MG.CASES) for l in MG.LANES],
                ids=lambda c: f"{c[0]}-{c[1]}")
def case(request):
    name, lanes = request.param
    p = _problem(name)
    ba = MG.make(p, MG.group_env(lanes))
    yield name, lanes, p, ba
    ba.close()


def test_takes_k_group(case):
    name, lanes, p, g = case
    assert g.step_kernels() == "k_group", (name, lanes)


def test_against_oracle(case):
    name, lanes, p, g = case
    resid, d_ref, j_ref, x_ref, it_ref = _oracle_results(name)
    # test_residuals_bitwise's rule
    r = g.residuals(p.x0)
    diff = r != resid
    assert diff.mean() <= 1e-5 + 1.0 / r.size, f"{name}: {diff.sum()} residuals differ"
    if diff.any():
        assert np.abs(r[diff].view(np.int32) - resid[diff].view(np.int32)).max() <= 1
    d, j = g.compute_jacobian_extrinsic(p.x0)
    print(name, lanes, "jte rel", np.abs(j - j_ref).max() / np.abs(j_ref).max(),
          "delta rel", np.abs(d - d_ref).max() / np.abs(d_ref).max())
    assert np.abs(j - j_ref).max() <= 1e-9 * np.abs(j_ref).max(), name
    assert np.abs(d - d_ref).max() <= 1e-6 * np.abs(d_ref).max(), name
    x, _, it, _ = g.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=MG.eps_of(p))
    ulp = f32_ulp_diff(x, x_ref)
    print(name, lanes, "iters", it, it_ref, "max ulp", int(ulp.max()))
    assert it == it_ref, (name, it, it_ref)
    assert ulp.max() <= 1, (name, int(ulp.max()), int((ulp > 0).sum()))


def test_bitwise_against_parent(case, golden):
    name, lanes, p, g = case
    got = MG.record(g, p)
    for k, v in got.items():
        want = golden[f"{name}/{lanes}/{k}"]
        assert v.shape == want.shape and np.array_equal(v, want), (name, lanes, k)
