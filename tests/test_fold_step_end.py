"""The step's end with the solve's prologue ahead of the final workgroup's poll.

k_group's folded final workgroup fetches what the stop test and the camera update need besides the
step's sums -- the state words, the early error word, the step factor (table or pow), the camera
parameters -- before it polls for the sums.  The arithmetic is the same expressions on the same inputs,
evaluated earlier, so every result is bitwise the parent commit's, recorded once from a build of that
commit (tools/make_fold_step_end_golden.py -> tests/golden/fold_step_end/parent.npz; always
MCC_FUSED=0, every rig folds):

  * three rigs for the final workgroup's thread mappings: 2 cameras (m = 6, one block, 12 views), 4
    cameras (m = 18, 6 blocks, 40 views in 10 groups: fold_final_direct), 6 cameras (m = 30, 15 blocks,
    24 views: fold_final_u) -- parameters after 1, 2, 3 and 9 free-running steps, the COUNT + EPS
    optimisation, delta / JTE of a linearize_solve (a launch with do_update = 0);
  * the stop test on the 4-camera rig: COUNT with max_count 0, 1, 5 and an EPS between the parent's 3rd
    change and its earlier ones.  mcc_optimize launches its steps in batches, so every case runs launches
    after the one that stopped the loop: the iteration count and the parameters show they did nothing
    (max_count = 0 returns x0 itself).  A further step(4) through the API starts a free run (mcc_step
    rewrites the state, `done` included), so it is compared with the parent's recorded result as well;
  * the step-factor table's end: 4 100 iterations on the 12-view rig cross k = 4095 -> 4096 and take the
    pow branch;
  * a failed launch (the spare held back beyond the poll bound) and the next optimisation on the same
    handle, on the 6-camera rig (tests/test_warm_solve.py covers config4's shape).
src/multicalib.cpp:462-514 is the loop these steps restate.
"""
import os

import numpy as np
import pytest

from multi_camera_calibration_amd import api, rig

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_step_end", "parent.npz")
RIGS = {
    "c2": lambda: rig.make_config("config4", n_cams=2, n_views=12),
    "c4": lambda: rig.make_config("config4", n_views=40),
    "c6": lambda: rig.make_config("config4", n_cams=6, n_views=24),
}
ENV = {"MCC_FUSED": "0"}
FREE_STEPS = (1, 2, 3, 9)
COUNTS = (0, 1, 5)
TABLE_END_STEPS = 4100


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def make(p, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.BundleAdjuster(p)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def same(a, b):
    """bitwise, NaNs included (none is expected: a NaN would be compared as its bits)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_optimize(ba, p, g, key, crit_type, max_count, eps):
    """one optimisation against the fixture's case `key`: parameters, count, mean, change; then step(4)"""
    x, mean, it, ch = ba.optimize_extrinsics(p.x0, crit_type=crit_type, max_count=max_count, eps=eps)
    print(key, "iters", it, "change", ch, "mean", mean)
    assert it == int(g[f"{key}/iters"]), (it, int(g[f"{key}/iters"]))
    assert np.array_equal(x, g[f"{key}/x"]) and same(x, g[f"{key}/x"])
    assert same(np.float64(ch), g[f"{key}/change"]), (ch, float(g[f"{key}/change"]))
    assert same(np.float64(mean), g[f"{key}/mean"]), (mean, float(g[f"{key}/mean"]))
    return x, it


@pytest.mark.parametrize("name", sorted(RIGS))
def test_steps_optimize_and_linearize_are_bitwise_the_parent(name, gold):
    p = RIGS[name]()
    ba = make(p, ENV)
    try:
        assert ba.step_kernels() == "k_group" and int(ba.folded()) == int(gold[f"{name}/folded"])
        assert ba.m == 6 * (p.n_cams - 1)
        for n in FREE_STEPS:
            ba.set_params(p.x0)
            ba.step(n)
            ba.check()
            xs = ba.get_params()
            assert np.array_equal(xs, gold[f"{name}/x_step{n}"]) and same(xs, gold[f"{name}/x_step{n}"]), n
        check_optimize(ba, p, gold, f"{name}/opt", 3, 200, 1e-7)
        d, j = ba.compute_jacobian_extrinsic(p.x0)
        assert np.array_equal(d, gold[f"{name}/delta"]) and same(d, gold[f"{name}/delta"])
        assert np.array_equal(j, gold[f"{name}/jte"]) and same(j, gold[f"{name}/jte"])
    finally:
        ba.close()


@pytest.mark.parametrize("case", [f"count{c}" for c in COUNTS] + ["eps3"])
def test_stop_test_on_the_four_camera_rig(case, gold):
    p = RIGS["c4"]()
    if case == "eps3":
        ch = gold["c4/eps3/changes"]
        eps = float(gold["c4/eps3/eps"])
        assert ch[2] <= eps < min(ch[0], ch[1])   # the parent's changes: stops at the 3rd iteration, not sooner
        crit, mc, want = 2, 0, 3
    else:
        crit, mc, eps = 1, int(case[5:]), 0.0
        want = mc
    ba = make(p, ENV)
    try:
        x, it = check_optimize(ba, p, gold, f"c4/{case}", crit, mc, eps)
        # the launches of the same batch that followed the stop changed nothing: the count stands, and
        # a loop stopped at its first step returns the parameters it was given
        assert it == want
        if want == 0:
            assert same(x, np.asarray(p.x0, np.float32))
        ba.step(4)
        ba.check()
        xs = ba.get_params()
        assert np.array_equal(xs, gold[f"c4/{case}/x_step4"]) and same(xs, gold[f"c4/{case}/x_step4"])
    finally:
        ba.close()


def test_step_factor_past_the_table_end(gold):
    """k = 4095 is the table's last entry, k >= 4096 is pow(0.95, k + 1) on the device"""
    p = RIGS["c2"]()
    ba = make(p, ENV)
    try:
        ba.set_params(p.x0)
        ba.step(TABLE_END_STEPS)
        ba.check()   # no error
        xs = ba.get_params()
        assert np.array_equal(xs, gold["c2/table_end/x_step"]) and same(xs, gold["c2/table_end/x_step"])
        x, _, it, ch = ba.optimize_extrinsics(p.x0, crit_type=1, max_count=TABLE_END_STEPS, eps=0.0)
        print("table end: iters", it, "change", ch)
        assert it == TABLE_END_STEPS == int(gold["c2/table_end/iters"])
        assert np.array_equal(x, gold["c2/table_end/x"]) and same(x, gold["c2/table_end/x"])
        assert same(np.float64(ch), gold["c2/table_end/change"]), (ch, float(gold["c2/table_end/change"]))
    finally:
        ba.close()


def test_failed_launch_then_same_handle_on_the_six_camera_rig(gold):
    """The spare held back 30 ms against a 3 ms poll bound: the final workgroup (fold_final_u here) gives
    up before it has read its words, whatever it fetched ahead of the poll is dropped with the launch,
    and the step fails with MCC_ETIMEOUT (-6).  The next optimisation on the SAME handle, delays off,
    is bitwise a fresh problem's, which is the parent's."""
    p = RIGS["c6"]()
    ba = make(p, dict(ENV, MCC_SPARE_DELAY_US="30000", MCC_WARM_TIMEOUT_MS="3"))
    try:
        assert ba.folded()
        with pytest.raises(api.MccError, match=r"\(-6\)"):
            ba.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=1e-7)
        ba.debug_delays(spare_delay_us=0, warm_delay_us=0, warm_timeout_ms=10000)
        x, mean, it, ch = ba.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=1e-7)
    finally:
        ba.close()
    fresh = make(p, ENV)
    try:
        xf, meanf, itf, chf = fresh.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=1e-7)
    finally:
        fresh.close()
    assert it == itf == int(gold["c6/opt/iters"]) and mean == meanf and ch == chf
    assert np.array_equal(x, xf) and same(x, xf) and same(x, gold["c6/opt/x"])
