"""Every chain length, task type, weighting and reference frame of tests/chain_shapes_common.py through the lane emulator
(tests/lane_emu/lane_emu.cpp: the device's per-lane chain program compiled for the host) against the C oracle: chains of 1 .. 8 joints
of arm8, cassie_fixed / rightknee (q indices 8 .. 11) and ur5 / wrist_1_link with reference `base`.  Both builds of the lane program:
LANE_EMU_TRIG set (the device's SMASK = 0 build, sin / cos by dsincos_fast) and unset (the runtime-parameter build).

Asserted per problem: the plan's kernel name; e, the dense J and the frame placement against O.evaluate / O.fk_batch at the bars of
tests/test_lane_emulation.py test_lane_program_stagewise (1e-11, 1e-14); for 1, 2, 3 fixed iterations and the default stop rule with 100,
success flags and iteration counts equal to the double oracle's AND the _Float128 oracle's (the seed of the shared inputs was chosen so)
and |q - q_oracle| <= 1e-9.  tests/test_gpu_chain_shapes.py asserts the same problems on the device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chain_shapes_common as CS
from test_lane_emulation import emu, run  # noqa: F401  (emu is a fixture)
from test_track_emulation import emus  # noqa: F401  (a fixture: the single-solve and the tracking emulator)

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
