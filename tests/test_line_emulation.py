"""The lane programs of the line kernels (dls_chain_line_body in ik_amd/csrc/device/chain_kernel_body.hpp, hot_line_body in
device/chain_hot.hpp) and the waypoint function behind ikgpu_line_targets (device/line.hpp), compiled for the host by this test
(tests/lane_emu/line_emu.cpp) and run lane after lane.

ikgpu_dls_line_batch is DEFINED as ikgpu_dls_track_batch on the waypoints of ikgpu_line_targets, a problem leaving at its first
failed waypoint.  So (a) the waypoints are held to oracle/twin.py (log3, exp3 and FK in numpy) in every regime of the arithmetic,
(b) the written slabs are np.array_equal to the emulated tracking program (tests/lane_emu/track_emu.cpp) on the emulated waypoints
and `reached` is the count of track's leading successes, a dead lane does not go through further waypoints, and T = 1 is the single
solve, and (c) the chained oracle agrees on flags, iteration counts and q along every line (Cassie leg, both builds).

Measured when this test was written (inputs of tests/line_common.py, seeds 0-3): reached spreads over 0 .. T, lines fail at once, in
between, and reach the goal; the asserts below hold that."""
import ctypes as C

import numpy as np
import pytest

from conftest import urdf_path

import line_common
import oracle as O
import twin
from test_track_emulation import _compile, _p, PROGRAMS

B, T = 130, 16
MAX_IT, TOL = 100, 1e-4


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/line.hpp",
             "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    single = _compile("lane_emu.cpp", "liblane_emu.so", chain + ("device/tree_solver.hpp", "device/tree_kernel_body.hpp", "device/generic_solver.hpp",
                                                                 "device/pik_solver.hpp", "device/coop_solver.hpp", "device/pik_coop.hpp", "generic_tables.hpp"))
    track = _compile("track_emu.cpp", "libtrack_emu.so", chain)
    line = _compile("line_emu.cpp", "libline_emu.so", chain)
    for lib, name in ((single, "lane_emu_last_error"), (track, "track_emu_last_error"), (line, "line_emu_last_error")):
        getattr(lib, name).restype = C.c_char_p
    return single, track, line


_models = {}


def setup(name, frame, ktype=2):
    import ik_amd
    from ik_amd import capi
    if name not in _models:
        urdf = open(urdf_path(name), "rb").read()
        model = ik_amd.Model.from_urdf_xml(urdf)
        _models[name] = (urdf, model, twin.load_urdf(urdf_path(name)))
    urdf, model, tm = _models[name]
    fid = model.getFrameId(frame)
    task = capi.Task(fid, 0, ktype, 0, (C.c_double * 6)(*[1.0] * 6))
    return urdf, model, tm, task


def emu_waypoints(line, urdf, task, q0, goals, nT, layout=1):
    """line.hpp's waypoints: [nT, n, 12] from q0 [n, nq], goals [n, 12]."""
    n = q0.shape[0]
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    gi = np.ascontiguousarray(goals if layout == 1 else goals.T)
    W = np.full((nT, n, 12) if layout == 1 else (nT, 12, n), np.nan)
    rc = line.line_emu_targets(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), nT, _p(qi), _p(gi), _p(W), layout)
    assert rc == 0, line.line_emu_last_error()
    return W if layout == 1 else np.ascontiguousarray(W.transpose(0, 2, 1))


def emu_line(line, urdf, task, q0, goals, nT, prm, layout=1, optional=True):
    """The line lane program: one call.  Returns q [nT, n, nq] (NaN where not written), success, iters [nT, n] (7 / -7 where not
    written), reached [n], visited [n]."""
    n, nq = q0.shape
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    gi = np.ascontiguousarray(goals if layout == 1 else goals.T)
    qt = np.full((nT, n, nq) if layout == 1 else (nT, nq, n), np.nan)
    ok, it, reached = (np.full((nT, n), 7, np.uint8), np.full((nT, n), -7, np.int32), np.full(n, -7, np.int32)) if optional else (None, None, None)
    visited = np.full(n, -7, np.int32)
    rc = line.line_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), nT, _p(qi), _p(gi), C.byref(prm), _p(qt), _p(ok), _p(it), _p(reached),
                           _p(visited), layout)
    assert rc == 0, line.line_emu_last_error()
    return (qt if layout == 1 else np.ascontiguousarray(qt.transpose(0, 2, 1))), ok, it, reached, visited


def emu_track(track, urdf, task, q0, W, prm):
    """The tracking lane program on waypoints W [nT, n, 12], AoS."""
    nT, n = W.shape[:2]
    nq = q0.shape[1]
    qt = np.full((nT, n, nq), np.nan)
    ok, it = np.full((nT, n), 7, np.uint8), np.full((nT, n), -7, np.int32)
    rc = track.track_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), nT, _p(np.ascontiguousarray(q0)), _p(np.ascontiguousarray(W)),
                             C.byref(prm), _p(qt), _p(ok), _p(it), 1)
    assert rc == 0, track.track_emu_last_error()
    return qt, ok, it


def waypoint_error(line, name, frame, seed=0):
    """Maximum entry error of the emulated waypoints against the twin: random lines up to 2.5 rad and the regimes of the arithmetic."""
    urdf, model, tm, task = setup(name, frame)
    q0, goals = line_common.inputs(model, frame, B, seed)
    worst = {}
    W = emu_waypoints(line, urdf, task, q0, goals[:, 0], T)
    worst["random lines"] = float(np.abs(W - line_common.twin_waypoints(tm, frame, q0, goals[:, 0], T)).max())
    rg, names = line_common.regime_goals(tm, frame, q0[:24], T)
    Wr = emu_waypoints(line, urdf, task, q0[:24], rg, T)
    ref = line_common.twin_waypoints(tm, frame, q0[:24], rg, T)
    for b, nm in enumerate(names):
        worst[nm] = max(worst.get(nm, 0.0), float(np.abs(Wr[:, b] - ref[:, b]).max()))
    return worst, (q0[:24], rg, names, Wr)


@pytest.mark.parametrize("name,frame", line_common.ROBOTS)
def test_waypoints_match_the_twin_in_every_regime(emus, name, frame):
    """(a) line.hpp against oracle/twin.py.  Bar: line_common.WAYPOINT_BAR, ten times the emulator's measured maximum (DESIGN.md section 5:
    2.62e-13 over the three robots, seeds 0-3, every regime below -- at log3's own threshold, 4.1e-15 elsewhere), and no more than 1e-10."""
    _, _, line = emus
    worst, (q0, rg, names, Wr) = waypoint_error(line, name, frame)
    for what, err in sorted(worst.items()):
        print("%s %s: max |W_emu - W_twin| = %.3g" % (name, what, err))
    assert max(worst.values()) <= line_common.WAYPOINT_BAR, worst
    # the regimes are what they say: the last waypoint is the goal bit for bit; with the start's own rotation every waypoint keeps it
    # to rounding and with zero translation the origin does not move
    assert np.array_equal(Wr[T - 1], rg)
    urdf, model, tm, task = setup(name, frame)
    start = np.array([line_common.to12(twin.fk(tm, q)[1][twin.frame_id(tm, frame)]) for q in q0])
    for b, nm in enumerate(names):
        if nm == "theta=0":
            assert np.abs(Wr[:, b, :9] - start[b, :9]).max() < 1e-15
        if nm == "zero translation":
            assert np.abs(Wr[:, b, 9:] - start[b, 9:]).max() < 1e-15
    # both layouts give the same bits
    assert np.array_equal(emu_waypoints(line, urdf, task, q0, rg, T, layout=0), Wr)


BIT_CASES = [(n, f, 2, prog) for n, f in (("cassie_fixed", "LeftFootFront"), ("ur5", "tool0")) for prog in sorted(PROGRAMS)] + \
            [("arm7", "tool", 2, "general"), ("arm7", "tool", 2, "device_general"),
             ("cassie_fixed", "LeftFootFront", 0, "general"), ("cassie_fixed", "LeftFootFront", 0, "device_general")]   # a Position task


@pytest.mark.parametrize("name,frame,ktype,program", BIT_CASES)
def test_line_program_is_bit_identical_to_tracking_the_waypoints(emus, monkeypatch, name, frame, ktype, program):
    """(b) written slabs, reached, the early exit of a dead lane, T = 1."""
    from ik_amd import capi
    single, track, line = emus
    urdf, model, tm, task = setup(name, frame, ktype)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    q0, goals = line_common.inputs(model, frame, B, 0)
    q0[:, -1] += 9.0 if name.startswith("cassie") else 0.0     # an entry outside the chain beyond its limit: clipped once a step was taken
    n = q0.shape[0]
    prm = capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL)
    W = emu_waypoints(line, urdf, task, q0, goals[:, 0], T)
    qt, okt, itt = emu_track(track, urdf, task, q0, W, prm)
    want, _ = line_common.reached_from_flags(okt)
    mask = line_common.written(want, T)
    # the regimes: lines that fail at once, in between, and reach the goal
    assert (want == T).any() and ((want > 0) & (want < T)).any(), np.bincount(want, minlength=T + 1)
    if ktype == 2 and name != "arm7":     # (no arm7 line and no position-only line of this draw fails at once)
        assert (want == 0).any(), np.bincount(want, minlength=T + 1)
    for layout in (1, 0):
        q, ok, it, reached, visited = emu_line(line, urdf, task, q0, goals[:, 0], T, prm, layout)
        assert np.array_equal(reached, want), (name, program, layout)
        assert np.array_equal(q[mask], qt[mask]) and np.array_equal(ok[mask], okt[mask]) and np.array_equal(it[mask], itt[mask]), (name, program, layout)
        # slabs beyond the failed waypoint are not written, and a dead lane goes through no further waypoint
        assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all()
        assert np.array_equal(visited, np.minimum(want + 1, T))
    q_only, none_ok, none_it, none_reached, _ = emu_line(line, urdf, task, q0, goals[:, 0], T, prm, 0, optional=False)
    assert none_ok is None and none_it is None and none_reached is None and np.array_equal(q_only[mask], qt[mask])
    # T = 1: the single solve to the goal
    q1, ok1, it1, r1, _ = emu_line(line, urdf, task, q0, goals[:, 0], 1, prm)
    qs, oks, its = np.empty_like(q0), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    rc = single.lane_emu_run(urdf, C.c_size_t(len(urdf)), 0, C.byref(task), 1, 0, C.c_int64(n), _p(np.ascontiguousarray(q0)), _p(np.ascontiguousarray(goals)),
                             C.byref(prm), _p(qs), _p(oks), _p(its), None, None, None, 1)
    assert rc == 0, single.lane_emu_last_error()
    assert np.array_equal(q1[0], qs) and np.array_equal(ok1[0], oks) and np.array_equal(it1[0], its) and np.array_equal(r1, oks.astype(np.int32))


@pytest.mark.parametrize("program", ["general", "hot"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_line_program_matches_the_chained_oracle(emus, monkeypatch, program, seed):
    """(c) Cassie leg: the oracle chained along the emulated waypoints agrees on flags and iteration counts on every written waypoint
    and within 1e-9 on q on every waypoint met (the bar of tests/test_track_emulation.py).  The failed waypoint's q is an unconverged
    iterate and is not compared."""
    from ik_amd import capi
    _, _, line = emus
    name, frame = "cassie_fixed", "LeftFootFront"
    urdf, model, tm, task = setup(name, frame)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    q0, goals = line_common.inputs(model, frame, B, seed)
    n = q0.shape[0]
    assert 110 <= n <= B
    W = emu_waypoints(line, urdf, task, q0, goals[:, 0], T)
    q, ok, it, reached, _ = emu_line(line, urdf, task, q0, goals[:, 0], T, capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL))
    om = O.OracleModel(model.flat())
    ot = O.make_tasks([(model.getFrameId(frame), 0, 2, 0, None)])
    qo, alive, worst, count = q0, np.ones(n, bool), 0.0, np.zeros(n, np.int32)
    for k in range(T):
        qo, ok_ref, it_ref = O.dls_batch(om, ot, np.ascontiguousarray(W[k][:, None, :]), qo, O.params(MAX_IT, 1e-2, 1.0, TOL))
        assert np.array_equal(ok[k][alive], ok_ref[alive]) and np.array_equal(it[k][alive], it_ref[alive]), (program, seed, k)
        met = alive & (ok_ref == 1)
        if met.any():
            worst = max(worst, float(np.abs(q[k][met] - qo[met]).max()))
        alive = met
        count += met
    assert np.array_equal(reached, count)
    print("%s seed %d: %d lines, reached %s, max |q_line - q_oracle| on met waypoints = %.3g"
          % (program, seed, n, np.bincount(reached, minlength=T + 1).tolist(), worst))
    assert worst <= 1e-9
