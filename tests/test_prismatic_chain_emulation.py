"""Chains with prismatic joints through the lane emulator (tests/lane_emu/prismatic_emu.cpp: the device's per-lane chain programs
compiled for the host) against the C oracle, on the matrix of tests/prismatic_common.py.  Three programs: `runtime` (the
runtime-parameter build that reads the joint-kind mask: what the stage kernels run), `general` (the device's general build of such a
chain) and `hot` (the structure-specialised program, for the default-build cases).

Per case: FK against O.fk_batch at 1e-13, e and the dense J against O.evaluate at 1e-10, J zero outside the support and in the angular
rows of a prismatic column; step-synchronised along the oracle's trajectory, iterates 1, 2, 3, every lane within STEP_BAR = 1e-9 (rad or
m) of the oracle on every program, on-limit joints stay on the limit and entries outside the chain equal clip(q0) bit for bit; the
default rule with 100 iterations: flags and iteration counts equal to the double AND the _Float128 oracle, q within TOL = 1e-6; hot
against general within STEP_BAR.  The seven jobs on both builds of arm8 {j3, j6} / l7 and the rail UR5 against their definitions, by
np.array_equal.  tests/test_gpu_prismatic_chain.py asserts the same problems on the device."""
import functools
import os

import numpy as np
import pytest

import chain_shapes_common as CS
import goalset_common as GC
import line_common
import multistart_common as MC
import path_common
import prismatic_common as PC
import solutions_common as SC

import oracle as O

RULE = (100, 1e-4)


@pytest.fixture(scope="module")
def emu(native_built):
    return PC.compile_emulator()


def _programs(c):
    return ["runtime", "general"] + (["hot"] if c.build == "default" else [])


@functools.lru_cache(maxsize=None)
def _default_rule(c):
    """The oracle under the default rule, once per case; the double and the _Float128 oracle agree on every flag and iteration count."""
    x = PC.inputs(c)
    q_ref, ok_ref, it_ref = O.dls_batch(x.om, x.tasks, x.tg, x.q0, O.params(RULE[0], 1e-2, 1.0, RULE[1]))
    _, ok_ext, it_ext = O.dls_batch(x.om, x.tasks, x.tg, x.q0, O.params(RULE[0], 1e-2, 1.0, RULE[1]), min(4, os.cpu_count() or 1), ext="q")
    assert np.array_equal(ok_ref, ok_ext) and np.array_equal(it_ref, it_ext), "the seed no longer separates the two oracles"
    return q_ref, ok_ref, it_ref


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_stages_of_a_chain_with_prismatic_joints(emu, c):
    E = PC.Emu(emu, c)
    x = E.x
    q0, tg = np.array(x.q0), np.array(x.tg)
    d_fk = np.abs(E.run("runtime", 2, q0, tg) - O.fk_batch(x.om, q0, [x.fid])).max()
    e, J = E.run("runtime", 1, q0, tg)
    d_e = d_J = 0.0
    r0 = 3 if c.ktype == 2 else 0
    for b in range(PC.B):
        eo, Jo = O.evaluate(x.om, x.tasks, tg[b], q0[b])
        d_e, d_J = max(d_e, np.abs(e[b] - eo).max()), max(d_J, np.abs(J[b] - Jo).max())
    print("%s: max |oMf - oracle| %.2e, |e - oracle| %.2e, |J - oracle| %.2e" % (PC.case_id(c), d_fk, d_e, d_J))
    assert d_fk <= 1e-13 and d_e <= 1e-10 and d_J <= 1e-10, (d_fk, d_e, d_J)
    nv_support, nv_pris = x.support, x.support & x.prismatic        # (nq == nv on these fixed-base models: one column per entry)
    assert x.model.nq == x.model.nv
    assert (J[:, :, ~nv_support] == 0.0).all()
    if c.ktype != 0:
        assert (J[:, r0:, nv_pris] == 0.0).all()                     # a prismatic joint turns nothing
    if c == PC.ZERO_JACOBIAN:
        assert (J == 0.0).all()
    elif c.ktype != 1:
        assert (np.abs(J[:, :3, nv_pris]).max(axis=1) > 0.0).all()   # ... and moves the frame's origin


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_solve_of_a_chain_with_prismatic_joints(emu, c):
    from ik_amd import capi
    E = PC.Emu(emu, c)
    x = E.x
    q0, tg, sup = np.array(x.q0), np.array(x.tg), x.support
    one, p1 = O.params(1, 1e-2, 1.0, -1.0), capi.DlsParams(1, 1e-2, 1.0, -1.0)
    worst = dict.fromkeys(_programs(c), 0.0)
    q = q0
    for k in range(3):      # step-synchronised: from the oracle's k-th iterate, every program's next iterate
        q_next, _, _ = O.dls_batch(x.om, x.tasks, tg, q, one)
        got = {}
        for prog in _programs(c):
            got[prog], _, it = E.run(prog, 0, q, tg, p1)
            d = np.abs(got[prog] - q_next).max(axis=1)
            worst[prog] = max(worst[prog], d.max())
            assert np.isfinite(got[prog]).all() and d.max() <= PC.STEP_BAR, (prog, k, d.max(), int(d.argmax()))
            assert np.array_equal(got[prog][:, ~sup], np.clip(q, x.lo, x.hi)[:, ~sup]), (prog, k)
            if k == 0:
                assert all(got[prog][b, j] == q0[b, j] and q0[b, j] in (x.lo[j], x.hi[j]) for b, j in x.on_limit), prog
        if "hot" in got:
            assert np.abs(got["hot"] - got["general"]).max() <= PC.STEP_BAR, k
        q = q_next
    # the default rule
    q_ref, ok_ref, it_ref = _default_rule(c)
    prm = capi.DlsParams(RULE[0], 1e-2, 1.0, RULE[1])
    stopped0 = it_ref == 0
    for prog in _programs(c):
        qo, ok, it = E.run(prog, 0, q0, tg, prm)
        assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), prog
        assert np.abs(qo - q_ref).max() <= PC.TOL, (prog, np.abs(qo - q_ref).max())
        assert np.array_equal(qo[stopped0], q0[stopped0]), prog            # an iteration-0 stop returns q0 untouched
        if prog != "runtime":       # the other layout: the same bits
            for a, b_ in zip(E.run(prog, 0, q0, tg, prm, layout=0), (qo, ok, it)):
                assert np.array_equal(a, b_), prog
        if c == PC.ZERO_JACOBIAN:
            # no joint turns the frame: the turned targets run all 100 iterations with dq = 0 and fail with clip(q0); the others stop at once
            turned = np.arange(PC.B) % 2 == 1
            assert (it[turned] == RULE[0]).all() and not ok[turned].any() and np.array_equal(qo[turned], np.clip(q0, x.lo, x.hi)[turned])
            assert (it[~turned] == 0).all() and ok[~turned].all()
            assert (q0[turned] != np.clip(q0, x.lo, x.hi)[turned]).any()
    print("%s: max |q - q_oracle| per synchronised step %s; default rule: converged %d of %d, iteration counts %d .. %d"
          % (PC.case_id(c), {k: "%.2e" % v for k, v in worst.items()}, int(ok_ref.sum()), PC.B, it_ref.min(), it_ref.max()))


JOBS = [(c, prog) for c in PC.JOB_CASES for prog in ("general", "hot")]


def _job_id(v):
    return PC.case_id(v) if isinstance(v, PC.Case) else v


@pytest.mark.parametrize("c,prog", JOBS, ids=_job_id)
def test_track_multistart_solutions_and_goalset_on_a_prismatic_chain(emu, c, prog):
    from ik_amd import capi
    E = PC.Emu(emu, c)
    x = E.x
    q0, sup = np.array(x.q0), x.support
    prm = capi.DlsParams(RULE[0], 1e-2, 1.0, RULE[1])
    # track: T chained single solves
    way = np.array(PC.waypoints(c))[:, :, 0]                       # [T, B, 12]
    for p in (prm, capi.DlsParams(3, 1e-2, 1.0, -1.0)):
        qt, ok, it = E.track(prog, q0, way, p)
        qk = q0
        for k in range(PC.TRACK_T):
            qk, ok1, it1 = E.run(prog, 0, qk, way[k][:, None, :], p)
            assert np.array_equal(qt[k], qk) and np.array_equal(ok[k], ok1) and np.array_equal(it[k], it1), (k, p.stop_sq_tol)
        for a, b_ in zip(E.track(prog, q0, way, p, layout=0), (qt, ok, it)):
            assert np.array_equal(a, b_)
    # multi-start, solutions, goal set: K supplied starts on MS_B problems
    K, n = PC.MS_K, PC.MS_B
    ms, first = PC.multistart_inputs(c)
    ms = np.array(ms)
    assert len(set(first[first >= 0].tolist())) >= 2, first         # the draw puts winners into more than one lane of a group
    tg = np.array(x.tg[:n])
    norm = lambda q, t: np.array([np.linalg.norm(O.evaluate(x.om, x.tasks, t[b], q[b])[0]) for b in range(n)])
    singles = [E.run(prog, 0, ms[k], tg, prm) for k in range(K)]
    got = E.multistart(prog, ms[0], ms[1:], 0, tg, prm, K)
    MC.check_selection(got, singles, [norm(s[0], tg) ** 2 for s in singles], norm(got[0], tg), (PC.case_id(c), prog, "multistart"))
    assert len(set(got[3][got[1] != 0].tolist())) >= 2              # ... and so does the program
    for a, b_ in zip(E.multistart(prog, ms[0], ms[1:], 0, tg, prm, K, layout=0), got):
        assert np.array_equal(a, b_)
    sols = E.solutions(prog, ms[0], ms[1:], 0, tg, prm, K, K, PC.SEP)
    count, _ = SC.check_set(sols, singles, sup, PC.SEP, K, (PC.case_id(c), prog, "solutions"))
    assert count.max() >= 2 and (count == 0).any() or count.max() >= 2
    goals = np.array(PC.goalset_goals(c))                           # [G, n, 1, 12]
    cands = [E.run(prog, 0, ms[k], goals[g], prm) for g in range(PC.GS_G) for k in range(K)]
    gs = E.goalset(prog, ms[0], ms[1:], 0, goals, prm, K)
    unsolved = ~np.stack([s[1] for s in cands]).astype(bool).any(axis=0)
    errs = [np.where(unsolved, norm(cands[j][0], goals[j // K]), 0.0) ** 2 for j in range(len(cands))]
    GC.check_goalset(gs, cands, errs, norm(gs[0], goals[gs[3], np.arange(n)]), K, (PC.case_id(c), prog, "goalset"))
    assert (gs[3] == 0).any() and (gs[3] == 1).any()                # both goals win somewhere
    print("%s %s: multi-start winners %s, solutions by count %s, goal-set goals %s" % (PC.case_id(c), prog, np.bincount(got[3], minlength=K).tolist(),
                                                                                       np.bincount(count, minlength=K + 1).tolist(), np.bincount(gs[3], minlength=PC.GS_G).tolist()))


@pytest.mark.parametrize("c,prog", JOBS, ids=_job_id)
def test_line_and_path_on_a_prismatic_chain(emu, c, prog):
    from ik_amd import capi
    E = PC.Emu(emu, c)
    x = E.x
    q0, sup, B = np.array(x.q0), x.support, PC.B
    prm = capi.DlsParams(RULE[0], 1e-2, 1.0, RULE[1])
    # line: T waypoints towards one goal; the definition is the tracking program on line_targets' waypoints
    T = PC.LINE_T
    goals = np.array(PC.far_goals(c, 1))[0, :, 0]                   # [B, 12]
    W = E.line_waypoints(q0, goals, T)
    assert np.array_equal(W[T - 1], goals) and np.array_equal(E.line_waypoints(q0, goals, T, layout=0), W)
    qt, okt, itt = E.track(prog, q0, W, prm)
    want, _ = line_common.reached_from_flags(okt)
    mask = line_common.written(want, T)
    for layout in (1, 0):
        q, ok, it, reached, visited = E.line(prog, q0, goals, T, prm, layout)
        assert np.array_equal(reached, want), layout
        assert np.array_equal(q[mask], qt[mask]) and np.array_equal(ok[mask], okt[mask]) and np.array_equal(it[mask], itt[mask]), layout
        assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), layout
        assert np.array_equal(visited, np.minimum(want + 1, T)), layout
    hist = np.bincount(want, minlength=T + 1)
    assert hist[T] > 0 and hist[:T].sum() > 0, hist                 # a line that reaches its goal and one that fails on the way
    # path: P vias, T waypoints per segment, the joint-step rule -- one bound over radians and metres
    P, T = PC.PATH_PT
    N = P * T
    vias = np.array(PC.far_goals(c, P))[:, :, 0]                    # [P, B, 12]
    W = E.path_waypoints(q0, vias, T)
    assert np.array_equal(E.path_waypoints(q0, vias, T, layout=0), W)
    for s in range(P):
        assert np.array_equal(W[s * T + T - 1], vias[s]), s
    qt, okt, itt = E.track(prog, q0, W, prm)
    want, jumped = path_common.met_rule(okt, qt, q0, sup, PC.PATH_STEP)
    mask = line_common.written(want, N)
    jump, stop, complete = path_common.endings(okt, want, N)
    assert jump.sum() >= 1 and stop.sum() >= 1, (int(jump.sum()), int(stop.sum()))      # ended by the jump rule; failed its solve
    for layout in (1, 0):
        q, ok, it, reached, visited = E.path(prog, q0, vias, T, prm, PC.PATH_STEP, layout)
        assert np.array_equal(reached, want), layout
        assert np.array_equal(q[mask], qt[mask]) and np.array_equal(ok[mask], okt[mask]) and np.array_equal(it[mask], itt[mask]), layout
        assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), layout
        assert np.array_equal(visited, np.minimum(want + 1, N)), layout
    # a prismatic entry alone can end a path: its step is compared in metres with the same bound
    steps = np.abs(qt - np.concatenate([q0[None], qt[:-1]]))
    print("%s %s: line reached %s; path ended by a jump / by the stop rule / complete = %d / %d / %d, largest prismatic step on a met waypoint %.3f m"
          % (PC.case_id(c), prog, hist.tolist(), int(jump.sum()), int(stop.sum()), int(complete.sum()),
             float(np.where(line_common.written(want - 1, N)[:, :, None], steps, 0.0)[:, :, sup & x.prismatic].max())))
