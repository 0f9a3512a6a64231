"""Every chain length, task type, weighting and reference frame of tests/chain_shapes_common.py through the lane emulator
(tests/lane_emu/lane_emu.cpp: the device's per-lane chain program compiled for the host) against the C oracle: chains of 1 .. 8 joints
of arm8, cassie_fixed / rightknee (q indices 8 .. 11) and ur5 / wrist_1_link with reference `base`.  Both builds of the lane program:
LANE_EMU_TRIG set (the device's SMASK = 0 build, sin / cos by dsincos_fast) and unset (the runtime-parameter build).

Asserted per problem: the plan's kernel name; e, the dense J and the frame placement against O.evaluate / O.fk_batch at the bars of
tests/test_lane_emulation.py test_lane_program_stagewise (1e-11, 1e-14); for 1, 2, 3 fixed iterations and the default stop rule with 100,
success flags and iteration counts equal to the double oracle's AND the _Float128 oracle's (the seed of the shared inputs was chosen so)
and |q - q_oracle| <= 1e-9; the line job on the same problems (test_line_program_on_every_chain_shape).
tests/test_gpu_chain_shapes.py asserts the same problems on the device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chain_shapes_common as CS
from test_lane_emulation import emu, run  # noqa: F401  (emu is a fixture)
from test_track_emulation import emus  # noqa: F401  (a fixture: the single-solve and the tracking emulator)
from test_line_emulation import emus as line_emus  # noqa: F401  (a fixture: those two and the line emulator)

import oracle as O

# the emulator runs the general lane program whatever the build: one entry per distinct problem
EMU_CASES = list({(c.robot, c.frame, c.ktype, c.weighted, c.reference): c for c in reversed(CS.CASES)}.values())[::-1]


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def _task(c, x):
    from ik_amd import capi
    w = CS.weights(c)
    w = list(w) + [1.0] * (6 - len(w)) if w is not None else [1.0] * 6
    return capi.Task(x.fid, x.rid, c.ktype, 0, (C.c_double * 6)(*w))


@pytest.mark.parametrize("c", CS.CASES, ids=CS.case_id)
def test_plan_names_the_instantiation(ik, monkeypatch, c):
    x = CS.inputs(c)
    problem = CS.make_problem(c, x.model)
    if c.build == "default":
        assert ik.plan(problem) == CS.kernel_name(c, CS.hiprtc_installed())
    monkeypatch.setenv("IKGPU_CHAIN_HOT", "0")
    assert ik.plan(problem) == "dls_chain<NJ=%d,%s,general>" % (c.nj, CS.TYPE_NAMES[c.ktype])


def test_matrix_covers_every_general_instantiation_and_every_hot_length():
    assert {(c.nj, c.ktype) for c in CS.CASES if c.build == "general"} == {(nj, kt) for nj in range(1, 9) for kt in (0, 1, 2)}
    assert {c.nj for c in CS.HOT_CASES} == set(range(1, 8))
    assert len(CS.GENERAL_ARM_CASES) == 48 and len(EMU_CASES) == 53


@functools.lru_cache(maxsize=None)
def _oracle_loops(c):
    """The oracle's answers of a case under CS.RULES, computed once and shared by both builds of the lane program; the double and the
    _Float128 oracle agree on every flag and iteration count (the seed of the shared inputs was chosen so)."""
    x = CS.inputs(c)
    out = []
    for iters, tol in CS.RULES:
        q_ref, ok_ref, it_ref = O.dls_batch(x.om, x.tasks, x.tg, x.q0, O.params(iters, 1e-2, 1.0, tol))
        _, ok_ext, it_ext = O.dls_batch(x.om, x.tasks, x.tg, x.q0, O.params(iters, 1e-2, 1.0, tol), min(4, os.cpu_count() or 1), ext="q")
        assert np.array_equal(ok_ref, ok_ext) and np.array_equal(it_ref, it_ext), (iters, "the seed no longer separates the two oracles")
        out.append((q_ref, ok_ref, it_ref))
    return out


@pytest.mark.parametrize("trig", [False, True], ids=["runtime-mask", "smask0"])
@pytest.mark.parametrize("c", EMU_CASES, ids=CS.case_id)
def test_lane_program_on_every_chain_shape(emu, ik, monkeypatch, c, trig):
    from ik_amd import capi
    x = CS.inputs(c)
    urdf = x.xml.encode()
    task, M, nv = _task(c, x), CS.rows(c), x.model.nv
    q0, tg = np.array(x.q0), np.array(x.tg)
    if trig:
        monkeypatch.setenv("LANE_EMU_TRIG", "0")
    else:
        monkeypatch.delenv("LANE_EMU_TRIG", raising=False)
    # stages: the frame placement (world), e and the dense J
    *_, oMf = run(emu, urdf, task, 2, q0, tg, None, nv, M)
    assert np.abs(oMf - O.fk_batch(x.om, q0, [x.fid])).max() < 1e-14
    _, _, _, e, J, _ = run(emu, urdf, task, 1, q0, tg, None, nv, M)
    worst_e = worst_J = 0.0
    for b in range(CS.B):
        eo, Jo = O.evaluate(x.om, x.tasks, tg[b], q0[b])
        worst_e, worst_J = max(worst_e, np.abs(e[b] - eo).max()), max(worst_J, np.abs(J[b] - Jo).max())
        assert (J[b][:, ~x.support] == 0.0).all()
    assert worst_e < 1e-11 and worst_J < 1e-11, (worst_e, worst_J)
    # the loop: 1, 2, 3 fixed iterations and the default rule with 100
    worst = 0.0
    for (iters, tol), (q_ref, ok_ref, it_ref) in zip(CS.RULES, _oracle_loops(c)):
        qo, ok, it, *_ = run(emu, urdf, task, 0, q0, tg, capi.DlsParams(iters, 1e-2, 1.0, tol), nv, M)
        assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), iters
        worst = max(worst, np.abs(qo - q_ref).max())
        assert np.abs(qo - q_ref).max() <= 1e-9, (iters, np.abs(qo - q_ref).max())
        if iters == 1:     # the rewritten problems: the first iterate leaves the joint on its limit; entries outside the chain are clipped
            assert all(qo[b, j] == q0[b, j] and q0[b, j] in (x.lo[j], x.hi[j]) for b, j in x.on_limit)
            assert np.array_equal(qo[:, ~x.support], np.clip(q0, x.lo, x.hi)[:, ~x.support])
        if tol > 0:
            stopped0 = it_ref == 0
            assert np.array_equal(qo[stopped0], q0[stopped0])     # a lane that stops at iteration 0 returns q0 untouched
            if c.ktype == 0 and c.frame == "l1":
                assert stopped0.all() and (q0 > x.hi).any() and (q0 < x.lo).any()
            elif c.nj >= 3:
                assert len(set(it_ref[ok_ref != 0].tolist())) >= 2
    print("%s: max |e - e_oracle| %.2e, |J - J_oracle| %.2e, |q - q_oracle| %.2e" % (CS.case_id(c), worst_e, worst_J, worst))


# Cases in which no line fails: Position on l1 (the frame origin lies on the joint axis: the Jacobian is identically zero, the origin
# never moves and every lane stops at iteration 0) and Orientation on the tool of arm8 (eight joints for three rows)
NO_FAILING_LINE = {("arm8", "l1", 0), ("arm8", "tool", 1)}

_line_oracle = {}


def _chained_line_oracle(c, W, near):
    """The double oracle chained along the waypoints W [T, B, 12] on the near lines, a line leaving at its first failed waypoint:
    per waypoint (alive [n], q, success, iterations).  Computed once per case (both builds of the lane program are given the same
    waypoints: line.hpp has one build) with the _Float128 oracle beside it: the two agree on every flag and iteration count of every
    line still alive -- zero exclusions."""
    if c in _line_oracle:
        W0, out = _line_oracle[c]
        assert np.array_equal(W0, W)
        return out
    x = CS.inputs(c)
    prm = O.params(CS.LINE_RULE[0], 1e-2, 1.0, CS.LINE_RULE[1])
    qo = qe = x.q0[near]
    alive, out = np.ones(near.size, bool), []
    for k in range(W.shape[0]):
        tk = np.ascontiguousarray(W[k][near][:, None, :])
        qo, ok_ref, it_ref = O.dls_batch(x.om, x.tasks, tk, qo, prm)
        qe, ok_ext, it_ext = O.dls_batch(x.om, x.tasks, tk, qe, prm, min(4, os.cpu_count() or 1), ext="q")
        assert np.array_equal(ok_ref[alive], ok_ext[alive]) and np.array_equal(it_ref[alive], it_ext[alive]), (CS.case_id(c), k, "the two oracles differ on a near line")
        out.append((alive, qo, ok_ref, it_ref))
        alive = alive & (ok_ref == 1)
    _line_oracle[c] = (W.copy(), out)
    return out


@pytest.mark.parametrize("trig", [False, True], ids=["runtime-mask", "smask0"])
@pytest.mark.parametrize("c", EMU_CASES, ids=CS.case_id)
def test_line_program_on_every_chain_shape(line_emus, ik, monkeypatch, c, trig):
    """The line job (dls_chain_line_body, line.hpp) on every chain shape, T = CS.LINE_T waypoints towards CS.line_goals under the
    default stop rule.  The waypoints against oracle/twin.py with the case's reference frame (line_common.WAYPOINT_BAR), the last one
    the goal bit for bit; the written slabs, both layouts, np.array_equal to the emulated tracking program on those waypoints,
    `reached` its leading successes, the unwritten slabs untouched, visited = min(reached + 1, T); T = 1 the single solve to the goal;
    on the near lines the chained oracle's flags and iteration counts on every written waypoint and q within 1e-9 on every waypoint met
    (tests/test_line_emulation.py rule (c)).

    What the inputs have to contain (measured when they were drawn; another draw has to meet the same):
      - every case has a line that reaches the goal;
      - every Full case has a line that fails at waypoint 0 and one that fails in between;
      - every case has a failing line, but for the two of NO_FAILING_LINE;
      - every Full case with entries outside the chain has at least two pushed problems whose first step comes after waypoint 0: slab 0
        holds the entry beyond its limit and a later slab the clipped one (the `stepped` rule of dls_chain_line_body);
      - on the near lines the double and the _Float128 oracle agree on every flag and iteration count (_chained_line_oracle)."""
    from ik_amd import capi
    from test_line_emulation import emu_line, emu_track, emu_waypoints
    import line_common
    single, track, line = line_emus
    x = CS.inputs(c)
    urdf, task, T, B = x.xml.encode(), _task(c, x), CS.LINE_T, CS.B
    if trig:
        monkeypatch.setenv("LANE_EMU_TRIG", "0")
    else:
        monkeypatch.delenv("LANE_EMU_TRIG", raising=False)
    monkeypatch.delenv("LANE_EMU_HOT", raising=False)
    goals, far = CS.line_goals(c)
    q0, goals = np.array(x.q0), np.array(goals[:, 0])
    near = np.setdiff1d(np.arange(B), far)
    prm = capi.DlsParams(CS.LINE_RULE[0], 1e-2, 1.0, CS.LINE_RULE[1])
    # the waypoints, in the case's reference frame
    W = emu_waypoints(line, urdf, task, q0, goals, T)
    err = float(np.abs(W - CS.line_twin_waypoints(c)).max())
    assert err <= line_common.WAYPOINT_BAR, err
    assert np.array_equal(W[T - 1], goals)
    assert np.array_equal(emu_waypoints(line, urdf, task, q0, goals, T, layout=0), W)
    # the definition: the tracking program on those waypoints
    qt, okt, itt = emu_track(track, urdf, task, q0, W, prm)
    want, _ = line_common.reached_from_flags(okt)
    mask = line_common.written(want, T)
    for layout in (1, 0):
        q, ok, it, reached, visited = emu_line(line, urdf, task, q0, goals, T, prm, layout)
        assert np.array_equal(reached, want), layout
        assert np.array_equal(q[mask], qt[mask]) and np.array_equal(ok[mask], okt[mask]) and np.array_equal(it[mask], itt[mask]), layout
        assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), layout
        assert np.array_equal(visited, np.minimum(want + 1, T)), layout
    # T = 1: the single solve to the goal
    q1, ok1, it1, r1, _ = emu_line(line, urdf, task, q0, goals, 1, prm)
    qs, oks, its, *_ = run(single, urdf, task, 0, q0, np.ascontiguousarray(goals[:, None, :]), prm, x.model.nv, CS.rows(c))
    assert np.array_equal(q1[0], qs) and np.array_equal(ok1[0], oks) and np.array_equal(it1[0], its) and np.array_equal(r1, oks.astype(np.int32))
    # the chained oracle on the near lines
    worst, count = 0.0, np.zeros(near.size, np.int32)
    for k, (alive, qo, ok_ref, it_ref) in enumerate(_chained_line_oracle(c, W, near)):
        assert np.array_equal(ok[k][near][alive], ok_ref[alive]) and np.array_equal(it[k][near][alive], it_ref[alive]), k
        met = alive & (ok_ref == 1)
        if met.any():
            worst = max(worst, float(np.abs(q[k][near][met] - qo[met]).max()))
        count += met
    assert np.array_equal(want[near], count)
    assert worst <= 1e-9, worst
    # what the inputs contain
    hist = np.bincount(want, minlength=T + 1)
    first = np.where((itt > 0) & mask, np.arange(T)[:, None], T).min(axis=0)      # the waypoint of a problem's first step (T: none)
    late = 0
    if x.pushed is not None:
        who, two = x.pushed
        late = int(((first[who] > 0) & (first[who] < T)).sum())
        for b in who[(first[who] > 0) & (first[who] < T)]:
            assert np.array_equal(qt[0, b, two], q0[b, two]) and np.array_equal(qt[first[b], b, two], np.clip(q0[b, two], x.lo[two], x.hi[two]))
    print("%s: max |W - W_twin| %.2e, near lines max |q - q_oracle| %.2e, reached %s (far %s), pushed problems stepping late %d"
          % (CS.case_id(c), err, worst, hist.tolist(), np.bincount(want[far], minlength=T + 1).tolist(), late))
    assert hist[T] > 0, hist
    if c.ktype == 2:
        assert hist[0] > 0 and hist[1:T].sum() > 0, hist
        if x.pushed is not None:
            assert late >= 2, late
    if (c.robot, c.frame, c.ktype) in NO_FAILING_LINE:
        assert hist[T] == B, hist
        if c.ktype == 0:
            assert (itt == 0).all()
    else:
        assert hist[:T].sum() > 0, hist


@pytest.mark.parametrize("nj", [1, 2, 3, 4, 5, 6])
def test_hot_program_of_every_short_chain_compiles_for_gfx950(ik, tmp_path, monkeypatch, nj):
    """The run-time specialised hot program of arm8's l1 .. l6 (NJ = 7 is tests/test_host_logic.py's arm7) compiled for gfx950 without a
    device through ikgpu_problem_precompile: the compile runs in a child process, as the library does it at run time, into an empty
    cache directory.  A compile that fails would make the library run the general build in the program's place."""
    c = next(k for k in CS.HOT_CASES if k.nj == nj and k.reference == "universe")
    if not CS.hiprtc_installed():
        pytest.skip("hipRTC is not installed")
    problem = CS.make_problem(c, CS.inputs(c).model)
    monkeypatch.setenv("IKGPU_CACHE_DIR", str(tmp_path))
    assert ik.precompile(problem) == CS.kernel_name(c)
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].startswith("chain_hot_") and files[0].endswith(".hsaco"), files


# The tracking lane program composes its targets with the reference placement from its own place (compose_target in
# device/chain_kernel_body.hpp; the single solve uses load_target): the world-fixed references other than the universe, one length each
TRACK_CASES = [c for c in EMU_CASES if c.reference != "universe" and (c.nj in (1, 3, 4, 8) or c.robot == "ur5") and (c.weighted or c.ktype != 0)]


@pytest.mark.parametrize("c", TRACK_CASES, ids=CS.case_id)
def test_tracking_program_with_a_world_fixed_reference(emus, ik, c):
    """Three waypoints expressed in `bench` / `base` through the tracking lane program (tests/lane_emu/track_emu.cpp): the bits of three
    chained single solves, and the chained oracle's flags, iteration counts and q (1e-9, the bar of tests/test_track_emulation.py)."""
    from ik_amd import capi
    single, track = emus
    x = CS.inputs(c)
    urdf, task, way, nq, B = x.xml.encode(), _task(c, x), np.array(CS.waypoints(c)), x.model.nq, CS.B
    p = lambda a: C.c_void_p(a.ctypes.data)
    for iters, tol in ((100, 1e-4), (3, -1.0)):
        prm = capi.DlsParams(iters, 1e-2, 1.0, tol)
        qt, ok, it = np.full((3, B, nq), np.nan), np.full((3, B), 7, np.uint8), np.full((3, B), -7, np.int32)
        q0 = np.array(x.q0)
        rc = track.track_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(B), 3, p(q0), p(way), C.byref(prm), p(qt), p(ok), p(it), 1)
        assert rc == 0, track.track_emu_last_error()
        q, qo = q0, q0
        for k in range(3):
            q, ok1, it1, *_ = run(single, urdf, task, 0, q, np.ascontiguousarray(way[k]), prm, x.model.nv, CS.rows(c))
            assert np.array_equal(qt[k], q) and np.array_equal(ok[k], ok1) and np.array_equal(it[k], it1), (iters, k)
            qo, ok_ref, it_ref = O.dls_batch(x.om, x.tasks, way[k], qo, O.params(iters, 1e-2, 1.0, tol))
            assert np.array_equal(ok[k], ok_ref) and np.array_equal(it[k], it_ref), (iters, k)
            assert np.abs(qt[k] - qo).max() < 1e-9, (iters, k, np.abs(qt[k] - qo).max())
