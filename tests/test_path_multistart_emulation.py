"""The pieces of the path multi-start kernels (dls_chain_path_multistart_lane, path_scout, path_multistart_key, path_multistart_store in
ik_amd/csrc/device/chain_kernel_body.hpp; hot_path_multistart_lane in device/chain_hot.hpp), compiled for the host by this test
(tests/lane_emu/path_multistart_emu.cpp) and run lane after lane in groups of K.

ikgpu_dls_path_multistart_batch is DEFINED through existing calls (include/ikgpu.h): start k solves via 0 as the single solve does, and
if it met the stop rule, reached_k is what the path call from its result through the later vias writes; the winner has the smallest
(entered ? 0 : 1, entered ? N - reached_k : err_k, k).  So the reference is the emulated multi-start pieces run on ONE start at a time
(tests/lane_emu/multistart_emu.cpp with K = 2 and both starts equal: q, flag, count and err_sq of the single solve from that start),
the emulated path program (tests/lane_emu/path_emu.cpp) from each result, and the key in numpy (tests/path_multistart_common.py);
all seven scout outputs are held to it by np.array_equal.

Classes on the emulated reference, recipe seed 1, B = 130, K = 4, (P, T) = (3, 6), the robot's max_joint_step, measured when this test
was written -- no start enters / winner complete / winner partial / winner != lowest converged / >= 2 entered starts tie on the best
reached (the double oracle of the issue: ur5 30 / 56 / 44 / 17 / 40, arm7 15 / 63 / 52 / 30 / 58, Cassie leg 0 / 33 / 97 / 2 / 130):
    ur5           general 25 / 58 / 47 / 18 / 42    device_general 30 / 55 / 45 / 15 / 36    hot 28 / 55 / 47 / 17 / 38
    arm7          general 16 / 63 / 51 / 31 / 59    device_general 17 / 62 / 51 / 30 / 59
    cassie_fixed  0 / 33 / 97 / 2 / 130 on all three programs
(the programs differ on ur5 where a start's entry solve ends within rounding of the tolerance or the path's first jump lies within
rounding of the bound; each program is held to its OWN emulated reference), and reached_all takes every value -1 .. 12 on each robot.
The asserts below hold the issue's floors (5 per class; complete, partial and tie on the one-branch Cassie leg) on the reference before
anything is compared."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import path_common
import path_multistart_common as PM
from test_line_emulation import setup
from test_path_emulation import BIT_CASES, MAX_IT, TOL, emu_path, emu_path_waypoints, emu_support
from test_track_emulation import _compile, _p, PROGRAMS

B, SEED = 130, 1
SHAPES = [(1, 6), (2, 1), (3, 6)]


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/line.hpp",
             "device/multistart.hpp", "device/pick.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    multi = _compile("multistart_emu.cpp", "libmultistart_emu.so", chain)
    path = _compile("path_emu.cpp", "libpath_emu.so", chain)
    scout = _compile("path_multistart_emu.cpp", "libpath_multistart_emu.so", chain)
    for lib, name in ((multi, "multistart_emu_last_error"), (path, "path_emu_last_error"), (scout, "path_multistart_emu_last_error")):
        getattr(lib, name).restype = C.c_char_p
    return multi, path, scout


_drawn = {}


def drawn(name, frame, P, n=B):
    if name not in _drawn:
        _, model, _, _ = setup(name, frame)
        _drawn[name] = PM.inputs(model, frame, B, SEED)
    q0, vias = _drawn[name]
    return q0[:n].copy(), np.ascontiguousarray(vias[:P, :n])


def emu_starts(multi, urdf, task, q0, K, seed):
    """The generated starts 1 .. K-1, [K-1, n, nq]."""
    out = np.full((K - 1,) + q0.shape, np.nan)
    rc = multi.multistart_emu_starts(urdf, C.c_size_t(len(urdf)), 0, C.byref(task), 1, C.c_int64(q0.shape[0]), K, _p(np.ascontiguousarray(q0)),
                                     C.c_uint64(seed), _p(out), 1)
    assert rc == 0, multi.multistart_emu_last_error()
    return out


def emu_multistart(multi, urdf, task, q0, starts, seed, tg, prm, K):
    """The emulated multi-start call (AoS): q [n, nq], success, iters, winner, err_sq."""
    n = q0.shape[0]
    qo = np.full(q0.shape, np.nan)
    ok, it, win, err = np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, np.nan)
    rc = multi.multistart_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), K, _p(np.ascontiguousarray(q0)),
                                  _p(None if starts is None else np.ascontiguousarray(starts)), C.c_uint64(seed), _p(np.ascontiguousarray(tg)),
                                  C.byref(prm), _p(qo), _p(ok), _p(it), _p(win), _p(err), 1)
    assert rc == 0, multi.multistart_emu_last_error()
    return qo, ok, it, win, err


def emu_scout(scout, urdf, task, q0, starts, seed, vias, T, prm, step, K, layout=1, optional=True):
    """One call of the scout's lane programs.  q0 [n, nq], starts None or [K-1, n, nq], vias [P, n, 12]; AoS views back:
    (q_entry, entry_success, entry_iters, winner, err_sq, reached, reached_all [K, n]), visited [waves].  Sentinels where not written."""
    P, n = vias.shape[:2]
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
    vi = np.ascontiguousarray(vias if layout == 1 else vias.transpose(0, 2, 1))
    qo = np.full(qi.shape, np.nan)
    if optional:
        ok, it, win, err = np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, np.nan)
        reached, reached_all = np.full(n, -7, np.int32), np.full((K, n), -7, np.int32)
    else:
        ok = it = win = err = reached = reached_all = None
    visited = np.full((n * K + 63) // 64, -7, np.int32)
    rc = scout.path_multistart_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), K, P, T, _p(qi), _p(si), C.c_uint64(seed), _p(vi),
                                       C.byref(prm), C.c_double(step), _p(qo), _p(ok), _p(it), _p(win), _p(err), _p(reached), _p(reached_all),
                                       _p(visited), layout)
    assert rc == 0, scout.path_multistart_emu_last_error()
    return ((qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, win, err, reached, reached_all), visited


def reference(multi, path, urdf, task, q0, starts_all, vias, T, prm, step):
    """The definition: per start the emulated single solve against via 0 with its error, the emulated path program from its result, the
    key in numpy.  Returns the seven scout outputs."""
    K, n = starts_all.shape[:2]
    P = vias.shape[0]
    N = (P - 1) * T
    singles, reached_k = [], np.zeros((K, n), np.int32)
    for k in range(K):
        s = starts_all[k]
        q, ok, it, win, err = emu_multistart(multi, urdf, task, s, s[None], 0, vias[0], prm, 2)   # both starts equal: the single solve from s
        assert (win == 0).all()
        singles.append((q, ok, it, err))
        if N > 0:
            reached_k[k] = emu_path(path, urdf, task, q, vias[1:], T, prm, step)[3]
    ok_all, err_all = np.stack([s[1] for s in singles]), np.stack([s[3] for s in singles])
    winner, reached, reached_all = PM.select(ok_all, err_all, reached_k, N)
    rows = np.arange(n)
    pick = lambda i: np.stack([s[i] for s in singles])[winner, rows]
    return pick(0), pick(1), pick(2), winner, pick(3), reached, reached_all


def assert_same(got, want, label):
    for x, y, what in zip(got, want, ("q_entry", "entry_success", "entry_iters", "winner", "err_sq", "reached", "reached_all")):
        assert np.array_equal(x, y), (label, what)


@pytest.mark.parametrize("name,frame,ktype,program", BIT_CASES)
def test_scout_is_bit_identical_to_the_definition(emus, monkeypatch, name, frame, ktype, program):
    from ik_amd import capi
    multi, path, scout = emus
    urdf, model, tm, task = setup(name, frame, ktype)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    prm = capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL)
    robot_step = path_common.JOINT_STEP[name]
    cassie = name.startswith("cassie")
    for K, n in ((2, B), (4, B), (64, 6)):
        for P, T in SHAPES:
            N = (P - 1) * T
            q0, vias = drawn(name, frame, P, n)
            q0[:, -1] += 9.0 if cassie else 0.0     # an entry outside the chain beyond its limit: clipped once a step was taken
            gen = emu_starts(multi, urdf, task, q0, K, PM.START_SEED)
            starts_all = np.concatenate([q0[None], gen])
            for step in (0.0, robot_step):
                label = (name, program, K, P, T, step)
                want = reference(multi, path, urdf, task, q0, starts_all, vias, T, prm, step)
                if (K, P, T) == (4, 3, 6) and step > 0 and ktype == 2:
                    counts = PM.check_conditions(name, PM.classes(want[6], want[3], N))     # on the reference, before anything is compared
                    print("%s %s: %s = %s; reached_all values %s" % (name, program, " / ".join(PM.CLASSES), " / ".join(map(str, counts)),
                                                                   sorted(set(want[6].ravel().tolist()))))
                    if name == "ur5":
                        assert set(range(-1, N + 1)) <= set(want[6].ravel().tolist())
                got, visited = emu_scout(scout, urdf, task, q0, None, PM.START_SEED, vias, T, prm, step, K)
                assert_same(got, want, label)
                # the wave leaves once none of its lanes is alive: its trip count is the best lane's, N at the most
                lanes = np.minimum(np.maximum(want[6], -1) + 1, N).T.reshape(-1)             # [n K]: lane b K + k goes through reached_k + 1
                waves = [int(lanes[w * 64:(w + 1) * 64].max()) for w in range(visited.size)]
                assert visited.tolist() == waves, label
                # the other layout and the caller's starts instead of generated ones: the same bits
                for starts, layout in ((None, 0), (gen, 1), (gen, 0)):
                    assert_same(emu_scout(scout, urdf, task, q0, starts, PM.START_SEED, vias, T, prm, step, K, layout)[0], got, label + (layout,))
                if (K, P, T) == (4, 3, 6) and step > 0:
                    # a wave of 64 lanes -- 16 problems x 4 starts -- that all die before the end goes through fewer than N waypoints
                    dead = np.flatnonzero(want[6].max(axis=0) < N - 1)
                    assert dead.size >= 5
                    pick = np.resize(dead, 16)
                    sub, vis = emu_scout(scout, urdf, task, q0[pick], np.ascontiguousarray(gen[:, pick]), PM.START_SEED,
                                         np.ascontiguousarray(vias[:, pick]), T, prm, step, K)
                    assert np.array_equal(sub[6], want[6][:, pick]) and np.array_equal(sub[3], want[3][pick])
                    assert vis.size == 1 and vis[0] < N and vis[0] == want[6][:, pick].max() + 1
                if cassie:
                    # the winner's own column outside the chain, clipped exactly as the single solve clips it (iters > 0), kept otherwise
                    hi = float(model.upperPositionLimit[-1])
                    assert np.array_equal(got[0][:, -1], np.where(got[2] > 0, hi, q0[:, -1]))
            if P == 1:
                # P = 1 is the emulated multi-start call on via 0, and nothing is reached
                ms = emu_multistart(multi, urdf, task, q0, None, PM.START_SEED, vias[0], prm, K)
                got, visited = emu_scout(scout, urdf, task, q0, None, PM.START_SEED, vias, T, prm, robot_step, K)
                for x, y in zip(got[:5], ms):
                    assert np.array_equal(x, y), (name, program, K)
                assert not got[5].any() and set(got[6].ravel().tolist()) <= {0, -1} and not visited.any()
    # optional outputs that are null are not written, and the ones that are given do not depend on them
    q0, vias = drawn(name, frame, 3, 40)
    full, _ = emu_scout(scout, urdf, task, q0, None, PM.START_SEED, vias, 6, prm, robot_step, 4)
    bare, _ = emu_scout(scout, urdf, task, q0, None, PM.START_SEED, vias, 6, prm, robot_step, 4, optional=False)
    assert all(x is None for x in bare[1:]) and np.array_equal(bare[0], full[0])


@pytest.mark.parametrize("program", ["general", "hot"])
def test_scout_matches_the_chained_oracle(emus, monkeypatch, program):
    """Cassie leg: the double oracle from each start against via 0, then chained along the emulated waypoints from its own result with the
    joint-step rule on its own q, and the key in numpy, agrees on winner, reached_all and the flags, and on q_entry within 1e-9 (the
    project's bar, tests/test_track_emulation.py)."""
    from ik_amd import capi
    multi, path, scout = emus
    name, frame = "cassie_fixed", "LeftFootFront"
    urdf, model, tm, task = setup(name, frame)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    support = emu_support(path, urdf, task, model.nq)
    step = path_common.JOINT_STEP[name]
    om = O.OracleModel(model.flat())
    ot = O.make_tasks([(model.getFrameId(frame), 0, 2, 0, None)])
    prm, oprm = capi.DlsParams(MAX_IT, 1e-2, 1.0, TOL), O.params(MAX_IT, 1e-2, 1.0, TOL)
    K, P, T = 4, 3, 6
    N = (P - 1) * T
    q0, vias = drawn(name, frame, P)
    n = q0.shape[0]
    starts_all = np.concatenate([q0[None], emu_starts(multi, urdf, task, q0, K, PM.START_SEED)])
    ok_all, err_all, reached_k, q_all, it_all = [], [], np.zeros((K, n), np.int32), [], []
    for k in range(K):
        q, ok, it = O.dls_batch(om, ot, np.ascontiguousarray(vias[0][:, None, :]), starts_all[k], oprm)
        err_all.append(np.array([np.sum(O.evaluate(om, ot, vias[0][b][None], q[b])[0] ** 2) for b in range(n)]))
        W = emu_path_waypoints(path, urdf, task, q, vias[1:], T)
        qo, alive = q, ok == 1
        for m in range(N):
            prev = qo
            qo, ok_m, _ = O.dls_batch(om, ot, np.ascontiguousarray(W[m][:, None, :]), qo, oprm)
            alive = alive & (ok_m == 1) & ~(np.abs(qo - prev)[:, support] > step).any(axis=1)
            reached_k[k] += alive
        ok_all.append(ok); q_all.append(q); it_all.append(it)
    winner, reached, reached_all = PM.select(np.stack(ok_all), np.stack(err_all), reached_k, N)
    got, _ = emu_scout(scout, urdf, task, q0, None, PM.START_SEED, vias, T, prm, step, K)
    rows = np.arange(n)
    assert np.array_equal(got[3], winner) and np.array_equal(got[6], reached_all) and np.array_equal(got[5], reached)
    assert np.array_equal(got[1], np.stack(ok_all)[winner, rows]) and np.array_equal(got[2], np.stack(it_all)[winner, rows])
    worst = float(np.abs(got[0] - np.stack(q_all)[winner, rows])[got[1] == 1].max())
    print("%s: classes %s, max |q_entry - q_oracle| over entered winners = %.3g" % (program, PM.classes(reached_all, winner, N), worst))
    assert worst < 1e-9
