"""k_group's entry (mcc_group.hpp: the role dispatch on the leading, preloaded kernel parameters; the group
path's one scalar batch of state words, header ranges and phase 0's pointers; the stop test ahead of
every store) on the smallest rigs at which its role and range logic can go wrong, at both lane widths
(MCC_FUSED=0 MCC_GROUP=1, 32 lanes and MCC_GROUP_LANES=16):

  case           rig                                          what it exercises
  c4_v3          config4, 3 views                             one partial group + spare + trailing workgroups
  c4_v3_nofold   the same, MCC_GFOLD=0                        no trailing roles
  c4_v3_nospare  the same, MCC_SMALL_WARM=0                   no spare: every role index shifts by one
  c4_v64_dyn     config4, 64 views, MCC_FOLD_DYN=1            16 groups take the 8 tasks by ticket
  c4_v3_first    the same, MCC_FOLD_CONSUMERS_FIRST=1         the FIRST instantiation
  c4_v5          config4, 5 views                             a full group plus a one-photo group; the stop path
  c4_vis         config4, 24 views, visibility 0.5            uneven groups
  pin_c20        config2, 20 cameras, 6 views (m = 114)       k_group -> k_schur -> k_solve, several rounds
  c5_v6          config5, 6 views                             the BACK instantiation

For every case the host planner (tests/cpp/test_plan.cpp, run with the case's settings and the device's CU
count) must report what the case is about (MCC.CASES' third entry: fold, spare, ticket, FIRST, ...): a
switch that the planner drops on the rig fails test_plan_is_the_case's.

Every case is compared bit for bit with the commit before the change: tests/golden/group_entry/parent.npz,
recorded once on the GPU from a build of that commit by tools/make_group_entry_golden.py.  The stop path
(c4_v5): optimize_extrinsics(crit_type=1, max_count=k) for k = 0, 1, 3 -- the launches after the stop, up
to the end of the 8-step graph, must change nothing: parameters, iteration count and meanReProjError are
the golden's.
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
_spec = importlib.util.spec_from_file_location(
    "make_group_entry_golden", os.path.join(os.path.dirname(HERE), "tools", "make_group_entry_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "group_entry", "parent.npz")
_PROBLEMS = {}


def _problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = MG.CASES[name][0]()
    return _PROBLEMS[name]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The plan's scalars of (case, lanes) from the host-only planner at this device's CU count."""
    d = tmp_path_factory.mktemp("entry_plan")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cu_exe = str(d / "cu_count")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    os.path.join(TP.ROOT, "tests", "cpp", "cu_count.cpp"), "-o", cu_exe, "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    n_cu = int(subprocess.run([cu_exe], capture_output=True, text=True, timeout=60, check=True).stdout)
    exe = str(d / "test_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(TP.ROOT, "tests", "cpp", "test_plan.cpp"),
                    os.path.join(TP.CSRC, "mcc_plan.cpp"), "-o", exe], check=True)
    blobs = {}

    def run(name, lanes):
        if name not in blobs:
            blobs[name] = TP._blob(tmp_path_factory, _problem(name))
        return TP.Plan(TP._run(exe, blobs[name], n_cu=n_cu, n_cu_dev=n_cu, **MG.case_env(name, lanes))).scalars()
    return run


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", params=[(n, l) for n in sorted(MG.CASES) for l in MG.LANES],
                ids=lambda c: f"{c[0]}-{c[1]}")
def case(request):
    name, lanes = request.param
    p = _problem(name)
    ba = MG.make(p, MG.case_env(name, lanes))
    yield name, lanes, p, ba
    ba.close()


def test_plan_is_the_case(case, planner):
    name, lanes, p, g = case
    got = planner(name, lanes)
    want = dict(MG.CASES[name][2], group_lanes=lanes)
    assert {k: got[k] for k in want} == want, (name, lanes)
    assert g.photo_groups() == got["n_pgroups"] and g.folded() == bool(got["gfold"]), (name, lanes)


def test_bitwise_against_parent(case, golden):
    name, lanes, p, g = case
    assert g.step_kernels() == "k_group", (name, lanes)
    got = MG.record(g, p)
    for k, v in got.items():
        want = golden[f"{name}/{lanes}/{k}"]
        assert v.shape == want.shape and np.array_equal(v, want), (name, lanes, k)


@pytest.mark.parametrize("k", MG.STOP_COUNTS)
@pytest.mark.parametrize("lanes", MG.LANES)
def test_stop_path(lanes, k, golden):
    name = MG.STOP_CASE
    p = _problem(name)
    g = MG.make(p, MG.case_env(name, lanes))
    try:
        assert g.step_kernels() == "k_group", (name, lanes)
        x, mean, it, _ = g.optimize_extrinsics(p.x0, crit_type=1, max_count=k)
        g.check()
    finally:
        g.close()
    pre = f"{name}/{lanes}/stop{k}_"
    print(name, lanes, "max_count", k, "iters", it, "mean", mean)
    assert it == int(golden[pre + "iters"]), (it, int(golden[pre + "iters"]))
    assert np.array_equal(np.asarray(x), golden[pre + "x"])
    assert np.float64(mean).tobytes() == golden[pre + "mean"].tobytes()
