"""k_group's photo phase (mcc_group.hpp, from the barrier that ends the rounds to the slot stores: the Hpp
sums, one lane's Cholesky per photo, the U / Y' tasks, the pair tasks with their H-way sum, and the stores
of Y', z', gp, the error flag and the norm chunks' input, which follow the slot stores) on the smallest rigs
at which its task decomposition can go wrong.  tools/make_group_photo_phase_golden.py lists the cases with
what each is there for: groups of 1, 2, 3, 4 and more photos with unequal edge counts, H = 1, 2, 4, 8, 16
and 32 (every level of the lane sum), the BACK instantiation, a group with a
second round, and the two shapes at which a task loop takes a second pass (630 pair tasks against 512
threads; 288 U / Y' tasks against the 256 threads of the 16-lane kernel).  test_cases_have_their_shapes
checks those claims against the host planner's index structures (no GPU).

Every case runs folded (where the planner folds: m <= 30) and with MCC_GFOLD=0, always MCC_FUSED=0
MCC_GROUP=1, and is compared bit for bit with the commit before the change:
tests/golden/group_photo_phase/parent.npz, recorded once on the GPU from a build of that commit by
tools/make_group_photo_phase_golden.py (MCC_LIB pointing at that build), holds the parameters after 3
free-running steps (the third consumes the Y', z' and gp that the moved stores wrote) and the result of
optimize_extrinsics from x0.  A photo block reported not positive definite (MCC_FAULT_PHOTO) must still
fail the step with MCC_ENOTPD in both forms: the moved error flag and the norm chunks' flag word.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_plan as TP  # noqa: E402  (the host planner's runner)
from multi_camera_calibration_amd import api  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    "make_group_photo_phase_golden", os.path.join(os.path.dirname(HERE), "tools", "make_group_photo_phase_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

GOLDEN = os.path.join(HERE, "golden", "group_photo_phase", "parent.npz")
_PROBLEMS = {}


def _problem(name):
    make = MG.CASES[name][0]
    if make not in _PROBLEMS:
        _PROBLEMS[make] = make()
    return _PROBLEMS[make]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_cases_have_their_shapes(name, tmp_path_factory):
    """The host planner's groups of the case are what the case is listed for."""
    exe = str(tmp_path_factory.mktemp("photo_plan") / "test_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(TP.ROOT, "tests", "cpp", "test_plan.cpp"),
                    os.path.join(TP.CSRC, "mcc_plan.cpp"), "-o", exe], check=True)
    _, lanes, _, want = MG.CASES[name]
    o = TP.Plan(TP._run(exe, TP._blob(tmp_path_factory, _problem(name)), mode="full", **MG.case_env(name, "fold")))
    got = MG.shapes(o, lanes)
    assert o.use_group == 1 and o.group_lanes == lanes and bool(o.gfold) == (o.m <= 30), name
    assert got == dict(dict(uy2=False, pair2=False), **want), (name, got)


@pytest.fixture(scope="module", params=[(n, f) for n in sorted(MG.CASES) for f in MG.FORMS], ids=lambda c: f"{c[0]}-{c[1]}")
def case(request):
    name, form = request.param
    p = _problem(name)
    ba = MG.make(p, MG.case_env(name, form))
    yield name, form, p, ba
    ba.close()


@pytest.mark.gpu
def test_bitwise_against_parent(case, golden):
    name, form, p, g = case
    assert g.step_kernels() == "k_group", (name, form)
    assert g.folded() == (form == "fold" and MG.CASES[name][3]["m"] <= 30), (name, form)
    got = MG.record(g, p)
    for k, v in got.items():
        want = golden[f"{name}/{form}/{k}"]
        assert v.shape == want.shape and np.array_equal(v, want), (name, form, k)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(MG.FORMS))
def test_not_positive_definite_photo_fails_the_step(form):
    name = MG.FAULT_CASE
    p = _problem(name)
    g = MG.make(p, dict(MG.case_env(name, form), MCC_FAULT_PHOTO=str(MG.FAULT_PHOTO)))
    try:
        assert g.step_kernels() == "k_group" and g.folded() == (form == "fold")
        g.set_params(p.x0)
        with pytest.raises(api.MccError) as e:
            g.step(MG.STEPS)
            g.check()
        assert "(-3)" in str(e.value) and "photo normal-equation block is not positive definite" in str(e.value), str(e.value)
    finally:
        g.close()
