"""Folded runs of parallel joints in hot_evaluate (ik_amd/csrc/device/chain_hot.hpp: a run is walked in the frame it is entered with,
r0, r1 shared, p~ per member, phi a sum of angles), stage-wise on the host against the oracle: the chains of tests/hot_fold_common.py
put a folded run at the tip with the leader at joint 0, in the middle before a general placement, twice in one chain, and beside
unfolded joints; Cassie's leg and UR5 as they are.  The shim tests/hot_eval/hot_fold_shim.cpp is compiled here the way
tests/test_hot_evaluate.py compiles its own.

Configurations: that file's five groups (uniform in the limits, every joint on each limit one at a time and all together, at the target,
a rotation of pi - 1e-9 / 1e-6 / 1e-2 from the target, zero) plus, per run, every member on its upper limit, on its lower limit and
alternating -- run sums of 6.6 rad (runs of two) and 9.9 rad (the run of three), beyond 2 pi, and sums that cancel with every member
on a limit.

Bars: tests/test_hot_evaluate.py's -- 1e-11 on every entry of e and J, 1e-6 a rotation by almost pi away (the band pi - 1e-2 in which
log3 takes its theta -> pi formula).  That file's uniform draws happen to stay 0.03 rad clear of pi; 256 draws on each of seven chains
do not (run3_middle: one target at pi - 0.0108), and just outside the band the regular formula is conditioned like 1 / sin^2 theta in
the oracle as in the lane program.  The bar there is 1e-11 max(1, 1e-3 / sin^2 theta) with the ORACLE's theta -- derived from the
rounding of fMt in tests/hot_fold_common.py (conditioned): 1e-11 up to pi - 0.032, 1e-10 at pi - 1e-2, never 1e-6.
One DLS step of the lane program from the same configurations, the chain's entries of q: within tests/test_gpu_full_size.py's
STEP_BAR = 1e-9 rad of the oracle's, the bar the device is held to, widened by the same factor (the step is linear in e), and 1e-6 inside
the band pi - 1e-2: the oracle's own double arithmetic is 1e-8 from its _Float128 build there and the project holds that regime to
1e-6 (tests/test_gpu_rotation_by_pi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hot_fold_common as HF
import oracle as O
from test_hot_evaluate import BAR, BAR_NEAR_PI, PI_AXES, PI_GAPS, _cases

STEP_BAR, STEP_BAR_NEAR_PI = 1e-9, 1e-6


def _theta(eo):
    """The rotation angle between frame and target, by the oracle's own error vector."""
    return np.linalg.norm(eo[:, 3:], axis=1)


@pytest.fixture(scope="module")
def shim(native_built):
    src = os.path.join(ROOT, "tests", "hot_eval", "hot_fold_shim.cpp")
    out = os.path.join(ROOT, "tests", "hot_eval", "libhot_fold_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp",
                                                    "device/chain_solver.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.hot_fold_last_error.restype = C.c_char_p
    return L


@pytest.fixture(scope="module", params=HF.CHAINS, ids=[c.name for c in HF.CHAINS])
def evaluated(request, shim):
    """Every configuration of one chain through the shim in ONE call, and the oracle's e, J and first iterate for them, computed once."""
    import ik_amd
    from ik_amd import capi
    c = request.param
    urdf = HF.chain_xml(c).encode()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(c.frame)
    flat = model.flat()
    qidx, j = [], int(flat["frame_parent"][fid])
    while j > 0:
        qidx.insert(0, int(flat["idx_q"][j]))
        j = int(flat["parent"][j])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    cases = _cases(model, om, fid)
    rows = HF.run_rows(c, lo, hi, qidx, cases[0][1])
    if len(rows):
        cases.append(("run_sums", rows, cases[0][2][:len(rows)]))
    q = np.ascontiguousarray(np.concatenate([k[1] for k in cases]))
    tg = np.ascontiguousarray(np.concatenate([k[2] for k in cases]))
    n, nv = q.shape[0], model.nv
    e, J, q1 = np.empty((n, 6)), np.empty((n, 6, nv)), np.empty_like(q)
    leader, folded, nj = (C.c_int * 8)(), (C.c_int * 8)(), C.c_int(0)
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    p = lambda a: C.c_void_p(a.ctypes.data)
    colbuf = np.empty(n * 7 * 6)
    rc = shim.hot_fold_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), p(q), p(tg), C.c_int(1), C.c_double(1e-4), p(e), p(J), p(colbuf),
                           p(q1), leader, folded, C.byref(nj))
    assert rc == 0, shim.hot_fold_last_error()
    col = colbuf[:n * nj.value * 6].reshape(n, nj.value, 6)
    ot = O.make_tasks([(fid, 0, 2, 0, None)])
    eo, Jo = np.empty_like(e), np.empty_like(J)
    for b in range(n):
        eo[b], Jo[b] = O.evaluate(om, ot, tg[b], q[b])
    q1o, _, _ = O.dls_batch(om, ot, tg, q, O.params(1, 1e-2, 1.0, -1.0))
    span, at = {}, 0
    for label, qc, _ in cases:
        span[label] = slice(at, at + qc.shape[0])
        at += qc.shape[0]
    return dict(chain=c, e=e, J=J, col=col, eo=eo, Jo=Jo, q=q, q1=q1, q1o=q1o, span=span, qidx=qidx, lo=lo, hi=hi,
                leader=list(leader)[:nj.value], folded=list(folded)[:nj.value])


def test_the_runs_are_where_the_chains_put_them(evaluated):
    c = evaluated["chain"]
    assert evaluated["leader"] == c.leader
    size = [c.leader.count(L) for L in c.leader]
    assert evaluated["folded"] == [1 if s >= 2 else 0 for s in size]     # kHotFoldMinRun = 2: every run of two or more, and no lone joint
    if c.name == "no_run":
        assert not any(evaluated["folded"])


def test_the_draws_reach_the_limits_and_sums_beyond_two_pi(evaluated):
    c, q, qidx, lo, hi = (evaluated[k] for k in ("chain", "q", "qidx", "lo", "hi"))
    if c.name not in HF.MADE_UP or not HF.runs(c):
        return      # (the fixture robots' own limits decide what their runs reach)
    s = evaluated["span"]["run_sums"]
    for members in HF.runs(c):
        idx = [qidx[j] for j in members]
        assert (q[s][:, idx] == hi[idx]).all(axis=1).any() and (q[s][:, idx] == lo[idx]).all(axis=1).any()
        phi = q[s][:, idx].sum(axis=1)
        assert phi.max() > 2 * np.pi and phi.min() < -2 * np.pi
    assert HF.run_sums(c, q[evaluated["span"]["uniform"]], qidx) > np.pi


@pytest.mark.parametrize("group", ["uniform", "on_limits", "at_target", "zero", "run_sums"])
def test_error_and_jacobian_match_the_oracle(evaluated, group):
    if group not in evaluated["span"]:
        assert not HF.runs(evaluated["chain"])
        return
    s = evaluated["span"][group]
    de, dJ = np.abs(evaluated["e"][s] - evaluated["eo"][s]).max(axis=1), np.abs(evaluated["J"][s] - evaluated["Jo"][s]).max(axis=(1, 2))
    bars = HF.conditioned(_theta(evaluated["eo"][s]), BAR, BAR_NEAR_PI)
    wide = bars > BAR
    print("%s %s: max |de| %.2e, max |dJ| %.2e over %d configurations; %d more with a conditioned bar (up to %.1e): %.2e, %.2e"
          % (evaluated["chain"].name, group, de[~wide].max(initial=0.0), dJ[~wide].max(initial=0.0), (~wide).sum(), wide.sum(), bars.max(), de[wide].max(initial=0.0), dJ[wide].max(initial=0.0)))
    assert np.isfinite(evaluated["e"][s]).all() and np.isfinite(evaluated["J"][s]).all()
    assert (de < bars).all() and (dJ < bars).all(), (int(np.argmax(de / bars)), de.max(), dJ.max())
    if group == "at_target":
        assert np.abs(evaluated["e"][s]).max() < BAR


def test_error_and_jacobian_a_rotation_by_almost_pi_from_the_target(evaluated):
    s = evaluated["span"]["near_pi"]
    e, eo = evaluated["e"][s], evaluated["eo"][s]
    de, dJ = np.abs(e - eo).max(axis=1), np.abs(evaluated["J"][s] - evaluated["Jo"][s]).max(axis=(1, 2))
    gaps = np.tile(np.repeat(PI_GAPS, len(PI_AXES)), 8)
    for g in PI_GAPS:
        print("%s pi - %.0e: max |de| %.2e, max |dJ| %.2e" % (evaluated["chain"].name, g, de[gaps == g].max(), dJ[gaps == g].max()))
    assert np.isfinite(e).all() and np.isfinite(evaluated["J"][s]).all()
    assert np.abs(np.linalg.norm(eo[:, 3:], axis=1) - (np.pi - gaps)).max() < 1e-6
    assert de.max() < BAR_NEAR_PI and dJ.max() < BAR_NEAR_PI


def test_parallel_joints_share_their_angular_rows_bitwise(evaluated):
    """hot_gram and hot_step read col[leader][3..5] for every member of a run: the members' own must be the same bits, folded or not."""
    leader, col = evaluated["leader"], evaluated["col"]
    for j, L in enumerate(leader):
        if L != j:
            assert np.array_equal(col[:, j, 3:].view(np.uint64), col[:, L, 3:].view(np.uint64)), (j, L)


def test_one_step_of_the_lane_program_matches_the_oracle(evaluated):
    worst, qidx = {}, evaluated["qidx"]
    d = np.abs(evaluated["q1"] - evaluated["q1o"])[:, qidx].max(axis=1)
    bars = HF.conditioned(_theta(evaluated["eo"]), STEP_BAR, STEP_BAR_NEAR_PI)
    for group, s in evaluated["span"].items():
        worst[group] = (d[s] / bars[s]).max()
    print("%s one step, max |dq| vs oracle %.2e; worst share of its bar by group: %s (%d configurations with a bar above %g, up to %.1e)"
          % (evaluated["chain"].name, d[bars == STEP_BAR].max(), "  ".join("%s %.2e" % kv for kv in worst.items()), (bars > STEP_BAR).sum(), STEP_BAR, bars.max()))
    assert np.isfinite(evaluated["q1"]).all()
    assert (d <= bars).all(), (int(np.argmax(d / bars)), d.max())
