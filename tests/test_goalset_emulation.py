"""The bodies of the goal-set kernels (dls_chain_goalset_body in ik_amd/csrc/device/chain_kernel_body.hpp, hot_goalset_body in
device/chain_hot.hpp; device/goalset.hpp), compiled for the host by this test (tests/lane_emu/goalset_emu.cpp) and run lane after lane.

ikgpu_dls_goalset_batch is DEFINED through G x K single solves (include/ikgpu.h), so "right" is goalset_common.check_goalset: q / success
/ iterations equal, by np.array_equal, what the single-solve lane program (tests/lane_emu/lane_emu.cpp) returns for candidate
goal K + start; that candidate has the minimal key (exact in the success class and in the index among successes; among failures to 1e-10
in the error norm, errors from the oracle); |sqrt(err_sq) - ||e_oracle||| <= 5e-11; reachable[g] is exactly "some start of goal g met
the stop rule".  The two bounds are the multi-start tests' own (tests/multistart_common.py)."""
import ctypes as C

import numpy as np
import pytest

from conftest import urdf_path

import oracle as O
import goalset_common as GC
import test_multistart_emulation as ME

B = ME.B   # 130: two waves and a partial one at G K = 1, 130 waves at G K = 64
SHAPES = [(2, 1), (4, 1), (4, 2), (2, 8), (64, 1), (1, 8)]
CASES = [("ur5", "tool0", "general"), ("ur5", "tool0", "hot"), ("arm7", "tool", "general"), ("arm7", "tool", "device_general"),
         ("cassie_fixed", "LeftFootFront", "general"), ("cassie_fixed", "LeftFootFront", "hot")]
SEED = 0
# Every shape on every model; every program of a model at (4, 1) and (4, 2), one program per model at the other shapes (the oracle's
# errors of G K x 130 candidates are the cost of a case): the hot body where the model has one in the emulator, the device's general
# build on arm7 (hot-rtc on the device).
_LEAN = {"ur5": "hot", "arm7": "device_general", "cassie_fixed": "hot"}
MATRIX = [(n, f, prog, G, K) for (G, K) in SHAPES for (n, f, prog) in CASES if (G, K) in ((4, 1), (4, 2)) or prog == _LEAN[n]]

_p = ME._p


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/multistart.hpp",
             "device/goalset.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    single = ME._compile("lane_emu.cpp", "liblane_emu.so", chain + ("device/tree_solver.hpp", "device/tree_kernel_body.hpp", "device/generic_solver.hpp",
                                                                    "device/pik_solver.hpp", "device/coop_solver.hpp", "device/pik_coop.hpp",
                                                                    "generic_tables.hpp"))
    multi = ME._compile("multistart_emu.cpp", "libmultistart_emu.so", chain)
    goal = ME._compile("goalset_emu.cpp", "libgoalset_emu.so", chain)
    single.lane_emu_last_error.restype = C.c_char_p
    multi.multistart_emu_last_error.restype = C.c_char_p
    goal.goalset_emu_last_error.restype = C.c_char_p
    return single, multi, goal


def setup(name, frame, G, seed=SEED):
    """urdf, model, oracle model, task (ABI, oracle), q0 [B, nq], goals [G, B, 1, 12]."""
    import ik_amd
    from ik_amd import capi
    urdf = open(urdf_path(name), "rb").read()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    q0, qt = GC.goal_configurations(model, B, G, seed)
    goals = np.stack([O.fk_batch(om, qt[g], [fid]) for g in range(G)])
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    ot = O.make_tasks([(fid, 0, 2, 0, None)])
    return urdf, model, om, task, ot, q0, goals


def goalset(emu, urdf, task, q0, starts, seed, goals, prm, K, layout, optional=True):
    """One call of the goal-set lane programs.  q0 [B, nq], starts None or [K-1, B, nq], goals [G, B, 1, 12]; AoS views back.  Every output
    is exactly as long as the definition says: the emulator also runs a group of tail lanes, which must store nothing."""
    G = goals.shape[0]
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
    gi = np.ascontiguousarray(goals.reshape(G, B, 12) if layout == 1 else goals.reshape(G, B, 12).transpose(0, 2, 1))
    qo = np.full(qi.shape, np.nan)
    ok, it, gl, st, err, reach = ((np.full(B, 7, np.uint8), np.full(B, -7, np.int32), np.full(B, -7, np.int32), np.full(B, -7, np.int32),
                                   np.full(B, np.nan), np.full((G, B), 7, np.uint8)) if optional else (None,) * 6)
    rc = emu.goalset_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(B), G, K, _p(qi), _p(si), C.c_uint64(seed), _p(gi), C.byref(prm),
                             _p(qo), _p(ok), _p(it), _p(gl), _p(st), _p(err), _p(reach), layout)
    assert rc == 0, emu.goalset_emu_last_error()
    return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, gl, st, err, reach


def candidates(single, urdf, task, starts_all, goals, prm):
    """The single-solve lane program for candidate j = g K + k: start k against goal g."""
    res = []
    for g in range(goals.shape[0]):
        res += ME.single_solves(single, urdf, task, starts_all, goals[g], prm)
    return res


def norms(om, ot, goals_of, q, where=None):
    """||e|| of the oracle at q[b] against goals_of[b] [1, 12]; 0 where `where` [B] is False (entries the caller does not read)."""
    return np.array([np.linalg.norm(O.evaluate(om, ot, goals_of[b], q[b])[0]) if where is None or where[b] else 0.0 for b in range(B)])


def candidate_errors(om, ot, goals, singles, K):
    """||e||^2 of every candidate for the problems check_goalset reads them for: those no candidate solved."""
    unsolved = ~np.stack([s[1] for s in singles]).astype(bool).any(axis=0)
    return [norms(om, ot, goals[j // K], singles[j][0], unsolved) ** 2 for j in range(len(singles))]


@pytest.mark.parametrize("name,frame,program,G,K", MATRIX)
def test_goalset_program_returns_the_best_candidate(emus, monkeypatch, name, frame, program, G, K):
    from ik_amd import capi
    single, multi, emu = emus
    urdf, model, om, task, ot, q0, goals = setup(name, frame, G)
    for k, v in ME.PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    seed = 3
    gen = ME.emu_starts(multi, urdf, task, q0, K, seed) if K > 1 else np.empty((0,) + q0.shape)   # [K-1, B, nq]
    starts_all = np.concatenate([q0[None], gen])
    rows = np.arange(B)
    for max_it, tol in ((100, 1e-4), (5, -1.0)):
        prm = capi.DlsParams(max_it, 1e-2, 1.0, tol)
        singles = candidates(single, urdf, task, starts_all, goals, prm)
        errs = candidate_errors(om, ot, goals, singles, K)
        got = goalset(emu, urdf, task, q0, None, seed, goals, prm, K, 1)
        worst = GC.check_goalset(got, singles, errs, norms(om, ot, goals[got[3], rows], got[0]), K, (name, program, G, K, max_it))
        print("%s %s G=%d K=%d %s: %d of %d reached a goal, goal histogram %s; max |sqrt(err_sq) - ||e_oracle||| = %.3g"
              % (name, program, G, K, (max_it, tol), int(got[1].sum()), B, np.bincount(got[3], minlength=G).tolist(), worst))
        if tol < 0:
            assert not got[1].any() and not got[6].any()      # never-stop: nothing is reached, the arg-min of the error wins
        elif (G, K) == (4, 1) and name in ("ur5", "arm7"):
            # the workload exercises the rule: every class of it is populated at B = 130
            assert (got[1].astype(bool) & (got[3] == 0)).any(), "no problem won by goal 0"
            assert (got[1].astype(bool) & (got[3] > 0)).any(), "no problem won by a later goal"
            assert (got[1] == 0).any(), "no problem without a reached goal"
            assert (got[6] == 0).any() and (got[6] == 1).any()
        if G * K == 64 and tol < 0:
            continue   # (the other ways to make the call: under the stop rule only at 64 candidates, where each costs 8320 solves)
        # the caller's starts instead of generated ones, the other layout, and without the optional arrays: the same bits
        for starts, layout in ((gen if K > 1 else None, 1), (None, 0)):
            again = goalset(emu, urdf, task, q0, starts, seed, goals, prm, K, layout)
            for x, y in zip(again, got):
                assert np.array_equal(x, y), (name, program, G, K, max_it, layout, starts is None)
        q_only = goalset(emu, urdf, task, q0, None, seed, goals, prm, K, 0, optional=False)
        assert all(x is None for x in q_only[1:]) and np.array_equal(q_only[0], got[0])
        if G == 1:
            # one goal: the multi-start program's outputs, bit for bit
            ms = ME.multistart(multi, urdf, task, q0, None, seed, goals[0], prm, K, 1)
            for x, y, what in zip(ms, (got[0], got[1], got[2], got[4], got[5]), ("q", "success", "iterations", "winner", "err_sq")):
                assert np.array_equal(x, y), (name, program, K, max_it, what)
            assert not got[3].any() and np.array_equal(got[6][0], got[1])
        else:
            # G identical goals: goal 0 always, and the bits of the one-goal call
            same = np.broadcast_to(goals[:1], goals.shape).copy()
            rep = goalset(emu, urdf, task, q0, None, seed, same, prm, K, 1)
            one = goalset(emu, urdf, task, q0, None, seed, goals[:1], prm, K, 1)
            assert not rep[3].any(), (name, program, G, K, max_it)
            for i in (0, 1, 2, 4, 5):
                assert np.array_equal(rep[i], one[i]), (name, program, G, K, max_it, i)
            assert np.array_equal(rep[6], np.broadcast_to(one[6], (G, B)))


def test_own_columns_outside_the_support_follow_the_winning_start(emus):
    """Caller's starts whose entries OUTSIDE the support differ from q0's: the winner's own column is what a single solve clips."""
    from ik_amd import capi
    single, multi, emu = emus
    G, K = 2, 4
    urdf, model, om, task, ot, q0, goals = setup("cassie_fixed", "LeftFootFront", G)
    hi = np.asarray(model.upperPositionLimit)
    mine = ME.emu_starts(multi, urdf, task, q0, K, 3)
    mine[:, :, -1] = hi[-1] + 1.0 + np.arange(K - 1)[:, None]    # (the last entry lies outside the left leg's chain)
    prm = capi.DlsParams(100, 1e-2, 1.0, 1e-4)
    singles = candidates(single, urdf, task, np.concatenate([q0[None], mine]), goals, prm)
    errs = candidate_errors(om, ot, goals, singles, K)
    got = goalset(emu, urdf, task, q0, mine, 3, goals, prm, K, 1)
    GC.check_goalset(got, singles, errs, norms(om, ot, goals[got[3], np.arange(B)], got[0]), K, "own columns")
    assert (got[0][got[4] > 0, -1] == hi[-1]).all() and (got[4] > 0).any()
