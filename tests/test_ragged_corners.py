"""The step kernels on edges with unequal corner counts (tests/ragged_rigs.py): rig.make_rig gives every
edge the whole board, so until here every GPU test ran one count per side and nothing above 96 corners but
a uniform 117 on k_group alone.  The rigs, what each exercises and the loop it reaches:

  rig          base, board                            counts per edge                  reaches
  c4_ladder    config4 (omni, m = 18), 10 views,      the ladder 1..3, 15..17, 31..33, k_group's and k_edge's 96-corner chunk loop
               13 x 9 (117)                           47..49, 63..65, 95..98,          with part of the wave masked off (an edge
                                                      111..113, 117, shuffled          above 96 next to one below), every lane
                                                                                       tail of an edge's 16 / 32 lanes
  c4_wide      the same, groups of 24 edges           the same                         k_group's re-stage of a later round (rb > 0)
               (MCC_CUS = 2)                                                           with mixed counts
  c5_ragged    config5 (DoubleSide), 4 views,         uniform in [4, 117], a back      eight-edge photos, BACK edges, k_linearize's
               13 x 9 / 12 x 9                        side at most 108                 [5][max_cpp] staging off its maximum
  back_ragged  MyMulti BACK ring rig, 6 views         the same                         m = 42: k_schur -> k_solve behind the sweep
  c3_ragged    config3 (16 cameras, m = 90), 40 views uniform in [4, 117]              many groups; 64-edge k_photo groups
  c2_1024      config2 (pinhole, m = 18), 6 views,    uniform in [4, 1024]; edges      up to 11 chunks per edge, unequal trip counts
               32 x 32 of 10 mm (1024)                0, 1, 2 hold 1024, 1, 1023       in a wave; k_project_error's ferr[1024]

The CPU tests establish what the GPU tests assume: that edges above and below 96 corners share waves (from
the host planner's group-local edge order, tests/test_plan.py's binary), that the plan's index structures
hold on ragged input, that the oracle's two solvers agree on every rig, and that the oracle does not see a
cut of a long edge in two.  The GPU tests check every rig x form of ragged_rigs.RIGS
  1. against the oracle at tests/test_gpu_parity.py's bars, in its order;
  2. GPU against GPU across the forms of one rig (residuals at x0);
  3. GPU against GPU between a rig and split_edges(rig) (c4_ladder, c2_1024);
  4. k_project_error's per-corner errors of the 1024-, 1023- and 1-corner edges.

Measured on an MI355X (every form of every rig; the bars are test_gpu_parity's, not these figures):
  against the oracle   residuals bitwise equal everywhere (0 differing); JTE relative <= 1.1e-13 (c5_ragged; the
                       rest <= 1.1e-14); delta relative <= 5.2e-12 (back_ragged, three kernels; the rest <= 8e-13);
                       project error equal to the last bit; optimize_extrinsics 8 / 8 / 22 / 192 / 6 / 6 iterations
                       (c4_ladder, c4_wide, c5_ragged, back_ragged, c3_ragged, c2_1024) as the oracle, 0 ulp; 4
                       steps 0 ulp
  across forms         every pair of forms of every rig bitwise equal, also across prologues
  split, GPU           residuals bitwise; JTE 1.9e-16 (c4_ladder), 7.7e-17 .. 1.5e-16 (c2_1024); delta 3.0e-14 ..
                       5.9e-14 (c4_ladder), 6.9e-14 .. 1.0e-13 (c2_1024)
  split, oracle        JTE 1.9e-16, delta 5.2e-14 (c4_ladder); JTE 3.8e-16, delta 3.1e-13 (c2_1024); the same
                       optimise trajectory (bitwise equal parameters)
  k_project_error      the 1024-, 1- and 1023-corner edges: every corner's error equal to the oracle's
A library whose chunk loops drop a tail shorter than 16 corners (which a uniform 117 does not notice) fails
checks 1, 2 and 3 on every chunked form of c4_ladder and c4_wide and passes on the fused step.
"""
import os
import sys

import numpy as np
import pytest

from multi_camera_calibration_amd import api, rig
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ragged_rigs as RR  # noqa: E402
import test_gpu_parity as GP  # noqa: E402  (_eps, _param_bar: the bars)
from test_plan import _check_structure, exe, plan  # noqa: E402,F401  (exe, plan: fixtures)
from ulp import f32_ulp_diff  # noqa: E402

CHUNK = RR.CHUNK
CASES = [(r, f) for r in RR.RIGS for f in RR.RIGS[r][1]]
DISTINCT = ["c4_ladder", "c5_ragged", "back_ragged", "c3_ragged", "c2_1024"]   # (c4_wide is c4_ladder's problem)
SPLIT_RIGS = ["c4_ladder", "c2_1024"]
SPLIT_FORMS = {"g32": RR._G32, "g16": RR._G16, "three": RR._K3}


def _plan_kw(env):
    """The planner binary takes the CU count of the path rules as an argument, the library as MCC_CUS."""
    kw = dict(env)
    if "MCC_CUS" in kw:
        kw["n_cu"] = int(kw.pop("MCC_CUS"))
    return kw


def _kernels(o):
    return "k_linearize" if o.fused else "k_group" if o.use_group else "k_prep+k_edge+k_photo"


def _windows(o):
    """The corner counts of the edges that share a wave, as (round base rb, counts) per wave: k_group holds
    64 / lanes consecutive group-local edges per wave in rounds of 16; k_edge's one-wave workgroups hold 4
    consecutive device edges."""
    n = o.a("edge_n_dev")
    out = []
    if o.use_group:
        epw = 64 // o.group_lanes
        pe = o.a("pgrp_edge")
        for g in range(len(pe) - 1):
            loc = n[pe[g]:pe[g + 1]]
            for rb in range(0, len(loc), 16):
                rnd = loc[rb:rb + 16]
                out += [(rb, rnd[w:w + epw]) for w in range(0, len(rnd), epw)]
    else:
        out = [(0, n[e:e + 4]) for e in range(0, len(n), 4)]
    return out


def _mixed(w):
    return bool((w > CHUNK).any() and (w <= CHUNK).any())


def _trips_differ(w):
    return len(set((-(-w // CHUNK)).tolist())) > 1


# ------------------------------------------------------------------------------------------ CPU: the rigs

@pytest.mark.parametrize("name,form", CASES, ids=[f"{r}-{f}" for r, f in CASES])
def test_rig_mixes_counts_within_waves(plan, name, form):
    """Edges above and below 96 corners share at least 4 waves of the form's chunked kernel (k_group: 2
    consecutive group-local edges at 32 lanes, 4 at 16; k_edge: 4 consecutive device edges), so the chunk
    loop and its re-stage run with part of a wave masked off; c4_wide has such a wave in a later round of
    a group.  On c2_1024 (up to 11 chunks per edge) at least 4 waves also hold edges with different chunk
    counts: the same divergence later in the loop.  The
    fused step has no chunk loop: its photos' corner totals must differ, so that k_linearize's [5][max_cpp]
    staging is addressed off its maximum.  The plan takes the kernels the form names."""
    p = RR.problem(name)
    env, kernels = RR.RIGS[name][1][form]
    o = plan(p, mode="full", **_plan_kw(env))
    assert _kernels(o) == kernels, (name, form)
    if name == "c4_ladder":
        assert set(p.edge_n.tolist()) == set(RR.LADDER)
    if o.fused:
        cpp = np.diff(o.a("photo_corner"))
        assert len(set(cpp.tolist())) == len(cpp) > 1 and cpp.min() < o.max_cpp
        return
    ws = _windows(o)
    mixed = sum(_mixed(w) for _, w in ws)
    print(name, form, "waves", len(ws), "mixed", mixed, "unequal trips", sum(_trips_differ(w) for _, w in ws))
    assert mixed >= 4, (name, form, mixed)
    if name == "c2_1024":
        assert sum(_trips_differ(w) for _, w in ws) >= 4
    if name == "c4_wide":
        assert o.group_cap > 16 and o.n_pgroups <= RR.WIDE_CUS < -(-p.n_edges // 16)
        assert any(rb > 0 and _mixed(w) for rb, w in ws)


@pytest.mark.parametrize("name,form", [(r, f) for r, f in CASES if r in ("c4_ladder", "c4_wide", "c2_1024")],
                         ids=lambda v: v)
def test_plan_structure_on_ragged_input(plan, name, form):
    """tests/test_plan.py's structure check (info, dev2ref_corner, photo_corner, max_cpp, the groups and
    k_group's headers) on ragged counts, and on the same rig with its long edges cut in two."""
    p = RR.problem(name)
    kw = _plan_kw(RR.RIGS[name][1][form][0])
    _check_structure(p, plan(p, mode="full", **kw))
    q = RR.split_edges(p)
    assert q.n_edges == p.n_edges + int((p.edge_n > CHUNK).sum()) and q.edge_n.max() == max(CHUNK, p.edge_n.max() - CHUNK)
    if form != "default":   # (the fused step takes at most four edges per photo)
        _check_structure(q, plan(q, mode="full", **kw))


def test_thin_and_split_keep_the_corners():
    """thin keeps a sorted subset of each edge's own corners; split_edges and explode_edge keep the arrays."""
    base = rig.make_config("config4", n_views=10, board=(13, 9))
    p = RR.problem("c4_ladder")
    assert np.array_equal(p.x0, base.x0) and p.n_corners == p.edge_n.sum()
    assert np.array_equal(p.edge_off, np.concatenate([[0], np.cumsum(p.edge_n)[:-1]]))
    for e in range(p.n_edges):
        full = base.obj[base.edge_off[e]:base.edge_off[e] + base.edge_n[e]]
        mine = p.obj[p.edge_off[e]:p.edge_off[e] + p.edge_n[e]]
        idx = [int(np.nonzero((full == c).all(1))[0][0]) for c in mine]   # (a board's corners are distinct)
        assert idx == sorted(set(idx)) and len(idx) == p.edge_n[e]
        assert np.array_equal(p.img[p.edge_off[e]:p.edge_off[e] + p.edge_n[e]], base.img[base.edge_off[e] + np.array(idx)])
    q = RR.split_edges(p)
    assert q.obj is p.obj and q.img is p.img and q.edge_n.sum() == p.n_corners
    ref = lambda t: np.concatenate([t.edge_off[e] + np.arange(t.edge_n[e]) for e in range(t.n_edges)])
    assert np.array_equal(ref(q), ref(p))   # the same reference corner order
    x = RR.explode_edge(p, int(np.argmax(p.edge_n)))
    assert x.n_edges == p.edge_n.max() and np.all(x.edge_n == 1)


_ORACLE = {}


def _oracle(name):
    """The oracle's outputs of a rig, computed once for all its forms and left unchanged."""
    key = RR.RIGS[name][0]
    if key not in _ORACLE:
        p = RR.problem(name)
        o = O.Oracle(p)
        r = dict(resid=np.concatenate([o.edge_linearize(p.x0, e)[2] for e in range(p.n_edges)]).astype(np.float32))
        r["delta"], r["jte"] = o.linearize_solve(p.x0, "schur")
        r["err"], r["mean"] = o.project_error(p.x0)
        r["x_opt"], r["mean_opt"], r["it_opt"], _ = o.optimize(p.x0, crit_type=3, max_count=200, eps=GP._eps(p))
        r["x_4"], _, r["it_4"], _ = o.optimize(p.x0, crit_type=1, max_count=4)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


@pytest.mark.parametrize("name", DISTINCT)
def test_oracle_solvers_agree(name):
    """The exact Schur solve and the reference's Jacobi-CG give the same iteration count and bitwise equal
    parameters: the rig is well conditioned enough for a 1-ulp bar on the GPU's final parameters."""
    p = RR.problem(name)
    r = _oracle(name)
    x_cg, _, it_cg, _ = O.Oracle(p).optimize(p.x0, crit_type=3, max_count=200, eps=GP._eps(p), solver="cg")
    print(name, "iterations", r["it_opt"], it_cg, "parameters differing", int((x_cg != r["x_opt"]).sum()))
    assert it_cg == r["it_opt"] and np.array_equal(x_cg, r["x_opt"])


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", SPLIT_RIGS)
def test_oracle_split_invariance(name):
    """Cutting every edge above 96 corners in two (same camera, photo, side and corners) changes only the
    order of the oracle's sums: measured 1.9e-16 relative in JTE and 5.2e-14 in delta on c4_ladder, 3.8e-16
    and 3.1e-13 on c2_1024, and bitwise the same optimise trajectory."""
    p = RR.problem(name)
    r = _oracle(name)
    so = O.Oracle(RR.split_edges(p))
    d, j = so.linearize_solve(p.x0, "schur")
    x, _, it, _ = so.optimize(p.x0, crit_type=3, max_count=200, eps=GP._eps(p))
    ulp = f32_ulp_diff(x, r["x_opt"])
    print(name, "split against unsplit: jte rel", _rel(j, r["jte"]), "delta rel", _rel(d, r["delta"]), "iterations", it,
          r["it_opt"], "max ulp", int(ulp.max()))
    assert _rel(j, r["jte"]) <= 1e-9
    assert _rel(d, r["delta"]) <= 1e-6
    assert it == r["it_opt"] and ulp.max() <= 1


# ------------------------------------------------------------------------------------------ GPU

def _adjuster(p, env):
    """tests/test_gpu_parity.py's make_adjuster: the switches are read by mcc_create alone."""
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


def _tie_rule(r, ref):
    """test_gpu_parity's residual rule: (share differing, largest difference in float32 ulps)."""
    diff = r != ref
    ulp = int(np.abs(r[diff].view(np.int32).astype(np.int64) - ref[diff].view(np.int32)).max()) if diff.any() else 0
    return float(diff.mean()), ulp, int(diff.sum())


@pytest.fixture(scope="module", params=CASES, ids=[f"{r}-{f}" for r, f in CASES])
def case(request):
    name, form = request.param
    p = RR.problem(name)
    env, kernels = RR.RIGS[name][1][form]
    g = _adjuster(p, env)
    yield name, form, p, g, kernels
    g.close()


@pytest.mark.gpu
def test_form_takes_its_kernels(case):
    """As test_gpu_parity.test_forced_step_kernels: no case silently runs another kernel."""
    name, form, p, g, kernels = case
    assert g.step_kernels() == kernels, (name, form, g.step_kernels())
    if name == "c4_wide":
        assert g.photo_groups() <= RR.WIDE_CUS < -(-p.n_edges // 16), (g.photo_groups(), p.n_edges)


@pytest.mark.gpu
def test_against_oracle(case):
    """test_gpu_parity's bars, unchanged and in its order: residuals bitwise up to float32 rounding ties
    (share differing <= 1e-5 + 1/size, by 1 ulp), JTE 1e-9 and delta 1e-6 relative, compute_project_error's
    mean within 1e-6 and per edge within 1e-5, optimize_extrinsics under COUNT+EPS 200 with the oracle's
    iteration count and <= 1 ulp per float32 parameter, step(4) then get_params against the oracle's
    COUNT = 4."""
    name, form, p, g, _ = case
    ref = _oracle(name)
    r = g.residuals(p.x0)
    share, rulp, ndiff = _tie_rule(r, ref["resid"])
    d, j = g.compute_jacobian_extrinsic(p.x0)
    jrel, drel = _rel(j, ref["jte"]), _rel(d, ref["delta"])
    e, m = g.compute_project_error(p.x0)
    x, mo, it, _ = g.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=GP._eps(p))
    ulp = f32_ulp_diff(x, ref["x_opt"])
    g.set_params(p.x0)
    g.step(4)
    g.check()
    x4 = g.get_params()
    ulp4 = f32_ulp_diff(x4, ref["x_4"])
    print(name, form, "residuals differing", ndiff, "of", r.size, "by at most", rulp, "ulp; jte rel", jrel, "delta rel", drel,
          "; project error mean", abs(m - ref["mean"]), "per edge", float(np.abs(e - ref["err"]).max()), "; iters", it,
          ref["it_opt"], "mean", abs(mo - ref["mean_opt"]), "max ulp", int(ulp.max()), "; 4 steps max ulp", int(ulp4.max()))
    assert share <= 1e-5 + 1.0 / r.size, f"{name} {form}: {ndiff} residuals differ"
    assert rulp <= 1
    assert jrel <= 1e-9, (name, form)
    assert drel <= 1e-6, (name, form)
    assert abs(m - ref["mean"]) <= 1e-6
    assert np.abs(e - ref["err"]).max() <= 1e-5
    assert it == ref["it_opt"], (name, form, it, ref["it_opt"])
    assert abs(mo - ref["mean_opt"]) <= 1e-6
    GP._param_bar(name, x, ref["x_opt"])
    assert ref["it_4"] == 4
    GP._param_bar(name, x4, ref["x_4"])


# forms whose edge pose comes from group_prologue (mcc_group.hpp): k_group at either lane width and group
# width, and k_prep4
_GROUP_PROLOGUE = {"g32", "g16", "wide", "prep4"}


def _family(name, form, g):
    if form in _GROUP_PROLOGUE or (form == "default" and g.step_kernels() == "k_group"):
        return "group_prologue"
    return {"k_linearize": "edge_prologue_wave", "k_prep+k_edge+k_photo": "prep_edge"}[g.step_kernels()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", DISTINCT)
def test_residuals_across_forms(name):
    """A corner's float32 residual depends on its edge's pose and on nothing about chunking, lane mapping or
    the edges it shares a wave with.  Bitwise equal: every pair of forms whose pose comes from group_prologue
    (k_group at 32 and 16 lanes, its widened groups, k_prep4).  The fused step's edge_prologue_wave and
    k_prep's one-lane prep_edge order their FP64 chains differently: between families test_gpu_parity's tie
    rule holds (share differing <= 1e-5 + 1/size, by 1 ulp).  Measured: every pair of every rig bitwise equal."""
    p = RR.problem(name)
    forms = [(n, f) for n, f in CASES if RR.RIGS[n][0] is RR.RIGS[name][0]]
    got = []
    for n, f in forms:
        g = _adjuster(p, RR.RIGS[n][1][f][0])
        try:
            got.append((f, _family(n, f, g), g.residuals(p.x0)))
        finally:
            g.close()
    rows = []
    for i in range(len(got)):
        for k in range(i + 1, len(got)):
            share, ulp, nd = _tie_rule(got[i][2], got[k][2])
            rows.append((got[i][0], got[k][0], got[i][1] == got[k][1], share, ulp, nd))
            print(name, got[i][0], got[k][0], "same prologue" if rows[-1][2] else "other prologue", "differing", nd, "by", ulp, "ulp")
    for a, b, same, share, ulp, nd in rows:
        if same:
            assert nd == 0, (name, a, b, nd)
        else:
            assert share <= 1e-5 + 1.0 / got[0][2].size and ulp <= 1, (name, a, b, nd, ulp)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(SPLIT_FORMS))
@pytest.mark.parametrize("name", SPLIT_RIGS)
def test_split_invariance(name, form):
    """The rig against split_edges(rig) on the same kernel: the corners, their reference order and every
    edge's pose are the same, so residuals(x0) are bitwise equal; JTE and delta agree at the project's
    1e-9 / 1e-6 bars (the oracle's own split-against-unsplit difference: test_oracle_split_invariance).  No
    oracle in this check: a chunk tail that is dropped, or a first chunk that is read again, changes one
    side only.  Measured, GPU (oracle): c4_ladder JTE 1.9e-16 (1.9e-16) on all three forms, delta 5.9e-14 at
    16 lanes, 3.0e-14 at 32, 3.2e-14 on the three kernels (5.2e-14); c2_1024 JTE 1.5e-16, 7.7e-17, 7.7e-17
    (3.8e-16), delta 6.9e-14, 7.0e-14, 1.0e-13 (3.1e-13)."""
    p = RR.problem(name)
    q = RR.split_edges(p)
    env = SPLIT_FORMS[form]
    out = []
    for t in (p, q):
        g = _adjuster(t, env)
        try:
            assert g.step_kernels() == ("k_group" if form != "three" else "k_prep+k_edge+k_photo")
            out.append((g.residuals(p.x0),) + g.compute_jacobian_extrinsic(p.x0))
        finally:
            g.close()
    (r0, d0, j0), (r1, d1, j1) = out
    so = O.Oracle(q)
    d_o, j_o = so.linearize_solve(p.x0, "schur")
    ref = _oracle(name)
    print(name, form, "split against unsplit: residuals differing", int((r0 != r1).sum()), "jte rel", _rel(j1, j0), "(oracle",
          _rel(j_o, ref["jte"]), ") delta rel", _rel(d1, d0), "(oracle", _rel(d_o, ref["delta"]), ")")
    assert np.array_equal(r0, r1)
    assert _rel(j1, j0) <= 1e-9
    assert _rel(d1, d0) <= 1e-6


@pytest.mark.gpu
def test_project_error_at_the_corner_limit():
    """k_project_error (one wave per edge, __shared__ ferr[1024], a sequential float32 sum over n) on
    c2_1024's 1024-, 1-, and 1023-corner edges: every corner's error against the oracle's (its per-edge error
    of the same edge given one edge per corner) within compute_project_error's per-edge bar 1e-5; the edge's
    mean is the sequential float32 sum of the kernel's own corner errors over n, and the 1-corner edge's mean
    is its only corner's error."""
    p = RR.problem("c2_1024")
    assert p.edge_n[:3].tolist() == [1024, 1, 1023]
    g = api.BundleAdjuster(p)
    try:
        err, cerr, tot, npts, mean = g.project_error_detail(p.x0)
    finally:
        g.close()
    ref = _oracle("c2_1024")
    assert npts == 2 * p.n_corners   # (pinhole: error.total() of a two-channel Mat)
    for e in range(3):
        o, n = int(p.edge_off[e]), int(p.edge_n[e])
        c_ref, _ = O.Oracle(RR.explode_edge(p, e)).project_error(p.x0)
        mine = cerr[o:o + n]
        s = np.float32(0)
        for v in mine:
            s = np.float32(s + v)
        print("edge", e, "corners", n, "corner error max diff", float(np.abs(mine - c_ref).max()), "edge mean", err[e], "oracle",
              ref["err"][e], "own sum / n", s / np.float32(n))
        assert np.abs(mine - c_ref).max() <= 1e-5
        assert abs(err[e] - ref["err"][e]) <= 1e-5
        assert err[e] == np.float32(s / np.float32(n))
    assert err[1] == cerr[p.edge_off[1]]
    assert abs(mean - ref["mean"]) <= 1e-6
