"""The rank rule of ik::pik on the device's lane programs compiled for the host (tests/lane_emu): the per-lane interpreter
(device/pik_solver.hpp pik_level: one-sided Jacobi, s2 > thr2), the cooperative interpreter (device/pik_coop.hpp: Cholesky-QR basis
with a fall-back to pivoted Gram-Schmidt; projector factored or dense) and the tree build (device/tree_solver.hpp PikRow: unpivoted
Gram-Schmidt), on the cases and under the acceptance rule of tests/pik_rank_common.py -- every case is built so that dropping or
keeping a direction moves the answer by 1e-2 rad or more, against a bar of 1e-8."""
import ctypes as C

import numpy as np
import pytest

import pik_rank_common as R
from test_lane_emulation import emu, pik_prm, run_pik  # noqa: F401  (emu is a fixture)
from test_lane_emulation_pik_coop import run_pik_coop


def _prm(prm_set):
    iters, step, tol, lam, da = prm_set
    return pik_prm(iters, step, tol, lam, None if da is None else list(da))


def _run(form, emu, inp, prm_set):   # noqa: F811
    run = run_pik if form == "per_lane" else run_pik_coop
    return run(emu, inp.urdf(), inp.capi_tasks(), inp.q0, inp.tg, _prm(prm_set), root=1 if inp.free_flyer else 0)


@pytest.mark.parametrize("form", ["per_lane", "coop_factored", "coop_dense"])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_interpreter_forms_under_the_rank_rule(emu, monkeypatch, case, form):   # noqa: F811
    if form != "per_lane":
        monkeypatch.setenv("IKGPU_PIK_PROJECTOR", form[len("coop_"):])
    inp = R.inputs(case)
    for prm_set in inp.param_sets():
        inp.check(form, prm_set, *_run(form, emu, inp, prm_set))


@pytest.mark.parametrize("form", ["per_lane", "coop_factored", "coop_dense"])
def test_zero_row_and_row_below_the_threshold_leave_the_same_answer(emu, monkeypatch, form):   # noqa: F811
    if form != "per_lane":
        monkeypatch.setenv("IKGPU_PIK_PROJECTOR", form[len("coop_"):])
    a, b = R.inputs("pos_w0_then_ori"), R.inputs("pos_w1e-19_then_ori")
    for sa, sb in zip(a.param_sets(), b.param_sets()):
        R.same_answer(form, sa, a.case, _run(form, emu, a, sa)[0], b.case, _run(form, emu, b, sb)[0])


def test_lambda_zero_on_the_per_lane_program(emu):   # noqa: F811
    """lambda = 0 on a level: no damping, the pseudo-inverse itself -- what only the one-sided-Jacobi program takes."""
    inp = R.inputs("full_rank_control")
    for prm_set in inp.lambda0_sets():
        inp.check("per_lane_lambda0", prm_set, *_run("per_lane", emu, inp, prm_set))


def _tree_run(emu, monkeypatch, case):   # noqa: F811
    from ik_amd import capi
    inp = R.inputs(case)
    assert inp.ik_amd.plan(inp.problem).startswith("dls_tree<NJ=7,chains=1"), inp.ik_amd.plan(inp.problem)
    urdf, tasks, q0, tg = inp.urdf(), inp.capi_tasks(), inp.q0, inp.tg
    M = sum(6 if t.type == 2 else (1 if t.type >= 3 else 3) for t in tasks)
    p = lambda a: C.c_void_p(a.ctypes.data)
    got = []
    for prm_set in inp.param_sets(tree=True):
        iters, step, tol, lam, _ = prm_set
        qo, ok, it = np.empty_like(q0), np.zeros(R.B, np.uint8), np.zeros(R.B, np.int32)
        e, J, oMf = np.empty((R.B, M)), np.empty((R.B, M, inp.nv)), np.empty((R.B, len(tasks), 12))
        monkeypatch.setenv("LANE_EMU_TREE_PIK_LAMBDA1", repr(lam[1]))
        rc = emu.lane_emu_run(urdf, C.c_size_t(len(urdf)), 1, tasks, len(tasks), 0, C.c_int64(R.B), p(q0), p(tg),
                              C.byref(capi.DlsParams(iters, lam[0], step, tol)), p(qo), p(ok), p(it), p(e), p(J), p(oMf), 1)
        monkeypatch.delenv("LANE_EMU_TREE_PIK_LAMBDA1")
        assert rc == 0, emu.lane_emu_last_error()
        inp.check("tree", prm_set, qo, ok, it)
        got.append(qo)
    return got


@pytest.mark.parametrize("case", R.TREE_CASES)
def test_tree_build_under_the_rank_rule(emu, monkeypatch, case):   # noqa: F811
    """Level 0 = a task on the foot with one row's weight at 1e-12 / 1e-19 / 0 and the pelvis pose, level 1 = the alignment row: the
    PikRow basis must keep resp. drop the row."""
    _tree_run(emu, monkeypatch, case)


def test_tree_build_zero_row_and_row_below_the_threshold_leave_the_same_answer(emu, monkeypatch):   # noqa: F811
    qa, qb = (_tree_run(emu, monkeypatch, c) for c in ("tree_pos_w0", "tree_pos_w1e-19"))
    for k, prm_set in enumerate(R.inputs("tree_pos_w0").param_sets(tree=True)):
        R.same_answer("tree", prm_set, "tree_pos_w0", qa[k], "tree_pos_w1e-19", qb[k])
