"""k_group's edge round (mcc_group.hpp: group_prologue's entry loops, the record scatter after the
butterfly, group_chain) on the smallest rigs at which it can go wrong and which tests/test_group_phase0.py
does not cover, at both lane widths (MCC_FUSED=0 MCC_GROUP=1, 32 lanes and MCC_GROUP_LANES=16):

  case          rig                                               what it exercises
  pin_rational  config2, 4 views, 8 distortion terms              the pinhole sweep record's 18-word intrinsics copy
  pin_prism     config2, 4 views, 12 terms                        the same, thin-prism instantiation
  pin_tilt      config2, 4 views, 14 terms (tilted sensor)        the 27-word copy (matTilt), the 256-VGPR variants
  back          MyMulti ring rig, 4 cameras x 4 views             BACK edges: second compose_motion, three-factor maps
  c5_v3         config5, 3 views (24 edges)                       DoubleSide, 8-edge photos: fewer photos than slots
  c4_pi         config4, 4 views, one photo turned                an edge in cvRodrigues2's theta ~ pi branch (cold loop);
                                                                  the edge is one whose float32 pose the branch's
                                                                  ill-conditioned angle cannot move (pi_branch)
  c4_single     config4, 5 views, photo 0 with one edge           empty edge slots in the prologue and the chain

Each case is checked
  1. against the CPU oracle at tests/test_gpu_parity.py's bars (residuals bitwise up to float32 rounding
     ties, JTE 1e-9 and delta 1e-6 relative, optimize_extrinsics under COUNT+EPS with 200 iterations: the
     oracle's iteration count and <= 1 ulp per float32 parameter);
  2. bit for bit against the commit before this test (the one before the edge round's issue priority):
     tests/golden/group_edge_round/parent.npz, recorded once on the GPU from a build of that commit by
     tools/make_group_edge_round_golden.py (whose --oracle mode checks the rigs on the CPU).
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
    "make_group_edge_round_golden", os.path.join(os.path.dirname(HERE), "tools", "make_group_edge_round_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "group_edge_round", "parent.npz")
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
    # every figure first, then test_gpu_parity.py's bars in its order (test_residuals_bitwise's rule first)
    r = g.residuals(p.x0)
    diff = r != resid
    rulp = int(np.abs(r[diff].view(np.int32).astype(np.int64) - resid[diff].view(np.int32)).max()) if diff.any() else 0
    d, j = g.compute_jacobian_extrinsic(p.x0)
    jrel, drel = np.abs(j - j_ref).max() / np.abs(j_ref).max(), np.abs(d - d_ref).max() / np.abs(d_ref).max()
    x, _, it, _ = g.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=MG.eps_of(p))
    ulp = f32_ulp_diff(x, x_ref)
    print(name, lanes, "residuals differing", int(diff.sum()), "of", r.size, "by at most", rulp, "ulp; jte rel", jrel,
          "delta rel", drel, "iters", it, it_ref, "max ulp", int(ulp.max()))
    assert diff.mean() <= 1e-5 + 1.0 / r.size, f"{name}: {diff.sum()} residuals differ"
    assert rulp <= 1
    assert jrel <= 1e-9, name
    assert drel <= 1e-6, name
    assert it == it_ref, (name, it, it_ref)
    assert ulp.max() <= 1, (name, int(ulp.max()), int((ulp > 0).sum()))


def test_bitwise_against_parent(case, golden):
    name, lanes, p, g = case
    got = MG.record(g, p)
    for k, v in got.items():
        want = golden[f"{name}/{lanes}/{k}"]
        assert v.shape == want.shape and np.array_equal(v, want), (name, lanes, k)
