"""The lane programs of the path kernels (dls_chain_path_body in ik_amd/csrc/device/chain_kernel_body.hpp, hot_path_body in
device/chain_hot.hpp) and the waypoint functions behind ikgpu_path_targets (device/line.hpp), compiled for the host by this test
(tests/lane_emu/path_emu.cpp) and run lane after lane.

ikgpu_dls_path_batch is DEFINED as ikgpu_dls_track_batch on the P x T waypoints of ikgpu_path_targets, a problem leaving at its first
waypoint that was not met: the solve met the stop rule and no support entry moved by more than max_joint_step.  So (a) the waypoints
are the emulated line's for P = 1, the vias bit for bit at the end of every segment, and oracle/twin.py's on the later segments in every
regime of the arithmetic; (b) the written slabs are np.array_equal to the emulated tracking program (tests/lane_emu/track_emu.cpp) on
those waypoints and `reached` is the numpy rule (tests/path_common.py met_rule) on what tracking returned, P = 1 without a joint-step
bound is the emulated line job, the bound is strict, and a dead group goes through no further waypoint; (c) the chained oracle agrees
on flags, iteration counts and q along the met part of every path (Cassie leg, both builds).  No reference uses the path job itself.

The draw of tests/path_common.py (inputs_exact, B = 130, three segments, SEED = 1: seed 0 leaves no complete Cassie path), P = 3, T = 6,
100 iterations, tolerance 1e-4, measured on the CPU with the emulated tracking program when this test was written -- lanes ended by a
jump with success = 1 / ended by the stop rule / complete, at the robot's max_joint_step (ur5, arm7 0.5 rad; Cassie leg 0.25 rad):
    ur5          65 /   9 / 56
    arm7         64 /  17 / 49
    cassie_fixed  7 / 122 /  1
and `reached` takes 0, T - 1, T and P T on each.  The asserts below hold these conditions on the reference before anything is compared."""
import ctypes as C

import numpy as np
import pytest

import line_common
import oracle as O
import path_common
import twin
from test_line_emulation import emu_line, emu_track, emu_waypoints, setup
from test_track_emulation import _compile, _p, PROGRAMS

B, SEED = 130, 1
SHAPES = [(1, 6), (3, 1), (2, 2), (3, 6)]
MAX_IT, TOL = 100, 1e-4


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/line.hpp",
             "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    track = _compile("track_emu.cpp", "libtrack_emu.so", chain)
    line = _compile("line_emu.cpp", "libline_emu.so", chain)
    path = _compile("path_emu.cpp", "libpath_emu.so", chain)
    for lib, name in ((track, "track_emu_last_error"), (line, "line_emu_last_error"), (path, "path_emu_last_error")):
        getattr(lib, name).restype = C.c_char_p
    return track, line, path


def emu_support(path, urdf, task, nq):
    sup = np.zeros(nq, np.uint8)
    rc = path.path_emu_support(urdf, C.c_size_t(len(urdf)), C.byref(task), _p(sup))
    assert rc == 0, path.path_emu_last_error()
    return sup.astype(bool)


def emu_path_waypoints(path, urdf, task, q0, vias, nT, layout=1):
    """line.hpp's path waypoints: [P nT, n, 12] from q0 [n, nq], vias [P, n, 12]."""
    P, n = vias.shape[:2]
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    vi = np.ascontiguousarray(vias if layout == 1 else vias.transpose(0, 2, 1))
    W = np.full((P * nT, n, 12) if layout == 1 else (P * nT, 12, n), np.nan)
    rc = path.path_emu_targets(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), P, nT, _p(qi), _p(vi), _p(W), layout)
    assert rc == 0, path.path_emu_last_error()
    return W if layout == 1 else np.ascontiguousarray(W.transpose(0, 2, 1))


def emu_path(path, urdf, task, q0, vias, nT, prm, step, layout=1, optional=True):
    """The path lane program: one call.  Returns q [P nT, n, nq] (NaN where not written), success, iters [P nT, n] (7 / -7 where not
    written), reached [n], visited [n]."""
    P, n = vias.shape[:2]
    nq, N = q0.shape[1], P * nT
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    vi = np.ascontiguousarray(vias if layout == 1 else vias.transpose(0, 2, 1))
    qt = np.full((N, n, nq) if layout == 1 else (N, nq, n), np.nan)
    ok, it, reached = (np.full((N, n), 7, np.uint8), np.full((N, n), -7, np.int32), np.full(n, -7, np.int32)) if optional else (None, None, None)
    visited = np.full(n, -7, np.int32)
    rc = path.path_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), P, nT, _p(qi), _p(vi), C.byref(prm), C.c_double(step), _p(qt), _p(ok),
                           _p(it), _p(reached), _p(visited), layout)
    assert rc == 0, path.path_emu_last_error()
    return (qt if layout == 1 else np.ascontiguousarray(qt.transpose(0, 2, 1))), ok, it, reached, visited


_drawn = {}


def drawn(name, frame, P):
    """(q0 [n, nq], vias [P, n, 12]): the first P segments of the three-segment draw of SEED, shared by every test."""
    if name not in _drawn:
        _, model, _, _ = setup(name, frame)
        q0, vias = path_common.inputs_exact(model, frame, B, 3, SEED)
        _drawn[name] = (q0, vias[:, :, 0])
    q0, vias = _drawn[name]
    return q0.copy(), np.ascontiguousarray(vias[:P])


@pytest.mark.parametrize("name,frame", line_common.ROBOTS)
def test_path_waypoints(emus, name, frame):
    """(a) P = 1 is the emulated line's waypoints bit for bit; slab s T + T - 1 is via s bit for bit; the segments s >= 1 agree with
    oracle/twin.py within line_common.WAYPOINT_BAR, a zero-length segment and the regimes of line_common.regime_goals included; both
    layouts give the same bits."""
    _, line, path = emus
    urdf, model, tm, task = setup(name, frame)
    worst = 0.0
    for P, T in SHAPES:
        q0, vias = drawn(name, frame, P)
        W = emu_path_waypoints(path, urdf, task, q0, vias, T)
        assert np.array_equal(emu_path_waypoints(path, urdf, task, q0, vias, T, layout=0), W), (P, T)
        assert np.array_equal(W[:T], emu_waypoints(line, urdf, task, q0, vias[0], T)), (P, T)
        for s in range(P):
            assert np.array_equal(W[s * T + T - 1], vias[s]), (P, T, s)
        ref = path_common.twin_waypoints(tm, frame, q0, vias, T)
        worst = max(worst, float(np.abs(W - ref).max()))
    # the regimes of the waypoint arithmetic on a LATER segment: via 0 is the pose at another configuration, via 1 a regime goal built on it
    # (theta = 0, 1e-9, at the Taylor thresholds, 2.5 rad, zero translation), via 2 = via 1: a zero-length segment
    T = 6
    q0, vias = drawn(name, frame, 1)
    q0, via0 = q0[:24], vias[0, :24]
    fid = twin.frame_id(tm, frame)
    q_at = np.array([q + 0.1 for q in q0])
    via0 = np.array([line_common.to12(twin.fk(tm, q)[1][fid]) for q in q_at])
    rg, names = line_common.regime_goals(tm, frame, q_at, T)
    vr = np.stack([via0, rg, rg])
    Wr = emu_path_waypoints(path, urdf, task, q0, vr, T)
    ref = path_common.twin_waypoints(tm, frame, q0, vr, T)
    per = {}
    for b, nm in enumerate(names):
        per[nm] = max(per.get(nm, 0.0), float(np.abs(Wr[:, b] - ref[:, b]).max()))
    for nm, err in sorted(per.items()):
        print("%s later segment, %s: max |W_emu - W_twin| = %.3g" % (name, nm, err))
    print("%s random paths: max |W_emu - W_twin| = %.3g" % (name, worst))
    assert max(worst, max(per.values())) <= line_common.WAYPOINT_BAR, (worst, per)
    assert np.array_equal(Wr[T - 1], via0) and np.array_equal(Wr[2 * T - 1], rg) and np.array_equal(Wr[3 * T - 1], rg)
    # the zero-length segment stays at the via: rotation to rounding, origin exactly (p0 + s * 0)
    assert np.abs(Wr[2 * T:, :, :9] - rg[None, :, :9]).max() < 1e-15 and np.array_equal(Wr[2 * T:, :, 9:], np.broadcast_to(rg[None, :, 9:], (T, 24, 3)))


BIT_CASES = [(n, f, 2, prog) for n, f in (("cassie_fixed", "LeftFootFront"), ("ur5", "tool0")) for prog in sorted(PROGRAMS)] + \
            [("arm7", "tool", 2, "general"), ("arm7", "tool", 2, "device_general"),
             ("cassie_fixed", "LeftFootFront", 0, "general"), ("cassie_fixed", "LeftFootFront", 0, "device_general")]   # a Position task


def _reference(track, path, urdf, task, q0, vias, T, prm, support, step):
    """The definition: the emulated tracking program on the emulated waypoints, the numpy rule on what it returned."""
    W = emu_path_waypoints(path, urdf, task, q0, vias, T)
    qt, okt, itt = emu_track(track, urdf, task, q0, W, prm)
    want, jumped = path_common.met_rule(okt, qt, q0, support, step)
    return qt, okt, itt, want, jumped


@pytest.mark.parametrize("name,frame,ktype,program", BIT_CASES)
def test_path_program_is_bit_identical_to_tracking_the_waypoints(emus, monkeypatch, name, frame, ktype, program):
    """(b) written slabs, reached, P = 1 without a bound, the strict bound, a dead group."""
    from ik_amd import capi
    track, line, path = emus
    urdf, model, tm, task = setup(name, frame, ktype)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    prm = capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL)
    support = emu_support(path, urdf, task, model.nq)
    robot_step = path_common.JOINT_STEP[name]
    for P, T in SHAPES:
        N = P * T
        q0, vias = drawn(name, frame, P)
        q0[:, -1] += 9.0 if name.startswith("cassie") else 0.0     # an entry outside the chain beyond its limit: clipped once a step was taken
        for step in (0.0, robot_step):
            qt, okt, itt, want, jumped = _reference(track, path, urdf, task, q0, vias, T, prm, support, step)
            mask = line_common.written(want, N)
            if (P, T) == (3, 6) and step > 0 and ktype == 2:
                counts = path_common.check_conditions(okt, want, P, T)          # conditions on the reference, before anything is compared
                print("%s %s: %d paths, ended by a jump / by the stop rule / complete = %d / %d / %d, reached %s"
                      % (name, program, q0.shape[0], counts[0], counts[1], counts[2], np.bincount(want, minlength=N + 1).tolist()))
            for layout in (1, 0):
                q, ok, it, reached, visited = emu_path(path, urdf, task, q0, vias, T, prm, step, layout)
                assert np.array_equal(reached, want), (name, program, P, T, step, layout)
                assert np.array_equal(q[mask], qt[mask]) and np.array_equal(ok[mask], okt[mask]) and np.array_equal(it[mask], itt[mask]), \
                    (name, program, P, T, step, layout)
                # slabs beyond the first waypoint that was not met are not written, and a dead lane goes through no further waypoint
                assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all()
                assert np.array_equal(visited, np.minimum(want + 1, N))
            q_only, none_ok, none_it, none_reached, _ = emu_path(path, urdf, task, q0, vias, T, prm, step, 0, optional=False)
            assert none_ok is None and none_it is None and none_reached is None and np.array_equal(q_only[mask], qt[mask])
        if P == 1:
            # without a bound, one segment is the line job: all four outputs and the waypoints its loop went through
            for layout in (1, 0):
                got = emu_path(path, urdf, task, q0, vias, T, prm, 0.0, layout)
                ref = emu_line(line, urdf, task, q0, vias[0], T, prm, layout)
                for x, y in zip(got, ref):
                    assert np.array_equal(x, y, equal_nan=x.dtype == np.float64), (name, program, layout)
    # the bound is strict: a threshold equal to one lane's largest step keeps the lane (>, not >=), the next float below drops it
    P, T = 3, 6
    N = P * T
    q0, vias = drawn(name, frame, P)
    qt, okt, itt, free, _ = _reference(track, path, urdf, task, q0, vias, T, prm, support, 0.0)
    steps = np.abs(qt - np.concatenate([q0[None], qt[:-1]]))[:, :, support].max(axis=2)             # [N, n]: the largest support step
    steps = np.where(line_common.written(free - 1, N) & (free[None, :] > 0), steps, 0.0)              # ... of the waypoints the stop rule met
    b = int(np.argmax((free >= 2) * steps.max(axis=0)))
    v = float(steps[:, b].max())
    assert free[b] >= 2 and v > 0.0
    for thr, keeps in ((v, True), (float(np.nextafter(v, 0.0)), False)):
        want, _ = path_common.met_rule(okt, qt, q0, support, thr)
        assert (want[b] == free[b]) == keeps and (keeps or want[b] == int(np.argmax(steps[:, b] == v))), (b, v, thr, want[b], free[b])
        _, _, _, reached, _ = emu_path(path, urdf, task, q0, vias, T, prm, thr)
        assert np.array_equal(reached, want), (name, program, thr)
    # a group of 64 lanes that all die before the end goes through fewer than P T waypoints
    want, _ = path_common.met_rule(okt, qt, q0, support, robot_step)
    dead = np.flatnonzero(want < N - 1)
    assert dead.size >= 5
    pick = np.resize(dead, 64)
    _, _, _, reached, visited = emu_path(path, urdf, task, q0[pick], np.ascontiguousarray(vias[:, pick]), T, prm, robot_step)
    assert np.array_equal(reached, want[pick]) and visited.max() < N and visited.max() == want[pick].max() + 1


@pytest.mark.parametrize("program", ["general", "hot"])
def test_path_program_matches_the_chained_oracle(emus, monkeypatch, program):
    """(c) Cassie leg: the oracle chained along the emulated waypoints agrees on flags and iteration counts on every written waypoint
    and within 1e-9 on q on every waypoint met (the project's bar, tests/test_track_emulation.py
    test_tracking_program_matches_the_chained_oracle); the joint-step rule on the oracle's own q gives the same `reached`.  The q of a
    waypoint that was not met is an unconverged iterate, or lies across a jump, and is not compared."""
    from ik_amd import capi
    _, _, path = emus
    name, frame = "cassie_fixed", "LeftFootFront"
    urdf, model, tm, task = setup(name, frame)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    support = emu_support(path, urdf, task, model.nq)
    step = path_common.JOINT_STEP[name]
    om = O.OracleModel(model.flat())
    ot = O.make_tasks([(model.getFrameId(frame), 0, 2, 0, None)])
    for P, T in SHAPES:
        N = P * T
        q0, vias = drawn(name, frame, P)
        n = q0.shape[0]
        W = emu_path_waypoints(path, urdf, task, q0, vias, T)
        q, ok, it, reached, _ = emu_path(path, urdf, task, q0, vias, T, capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL), step)
        qo, alive, worst, count = q0, np.ones(n, bool), 0.0, np.zeros(n, np.int32)
        for m in range(N):
            prev = qo
            qo, ok_ref, it_ref = O.dls_batch(om, ot, np.ascontiguousarray(W[m][:, None, :]), qo, O.params(MAX_IT, 1e-2, 1.0, TOL))
            assert np.array_equal(ok[m][alive], ok_ref[alive]) and np.array_equal(it[m][alive], it_ref[alive]), (program, P, T, m)
            met = alive & (ok_ref == 1) & ~(np.abs(qo - prev)[:, support] > step).any(axis=1)
            if met.any():
                worst = max(worst, float(np.abs(q[m][met] - qo[met]).max()))
            alive = met
            count += met
        assert np.array_equal(reached, count), (program, P, T)
        print("%s P %d T %d: %d paths, reached %s, max |q_path - q_oracle| on met waypoints = %.3g"
              % (program, P, T, n, np.bincount(reached, minlength=N + 1).tolist(), worst))
        assert worst < 1e-9
