"""The tree lane program in the build the LAUNCHER picks, on the CPU: tests/lane_emu/tree_emu.cpp instantiates ikdev::dls_tree_body
for the SPEC values ik_amd/csrc/problem.cpp select_tree_build + tree_build.hpp with_tree_spec yield -- the two functions
kernels.hip run_dls_tree dispatches on -- and runs every case of tests/tree_shapes_common.py lane after lane against the C oracle:
flags and iteration counts equal, q within 1e-8 rad (the bar of tests/test_lane_emulation_demo_tree.py).  The double oracle, the
_Float128 oracle and the emulator agree on every flag and count of every case and rule: that is what tree_shapes_common.SEED was
chosen for, and no lane needs an "oracle unstable" exclusion here.

Also on the host alone: the kernel name and the build string (include/ikgpu.h ikgpu_dls_tree_build_plan) of every case, and that the
matrix reaches every build string the selection can return for the four instantiated shapes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import oracle as O
import tree_shapes_common as TS

Q_BAR = 1e-8
ALL_CASES = TS.CASES + TS.EDGE_CASES


@pytest.fixture(scope="module")
def emu(native_built):
    src = os.path.join(ROOT, "tests", "lane_emu", "tree_emu.cpp")
    out = os.path.join(ROOT, "tests", "lane_emu", "libtree_emu.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "tree_build.hpp", "device/lane_math.hpp",
                                                    "device/chain_solver.hpp", "device/chain_kernel_body.hpp", "device/tree_solver.hpp",
                                                    "device/tree_kernel_body.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.tree_emu_last_error.restype = C.c_char_p
    return L


def emu_solve(L, x, rule, q0=None, tg=None, layout=1):
    """(q [B, nq], success, iterations, build string) of the case's solve under `rule` by the emulator (array-of-structures in and out)."""
    from ik_amd import api, capi
    c = x.case
    q0 = np.ascontiguousarray(x.q0 if q0 is None else q0)
    tg = np.ascontiguousarray(x.tg if tg is None else tg)
    n = q0.shape[0]
    if layout == 0:
        q0, tg = np.ascontiguousarray(q0.T), np.ascontiguousarray(tg.transpose(1, 2, 0))
    tasks = api._task_table(x.problem)
    cons, ncons = api._constraint_table(x.problem)
    prm = capi.DlsParams(rule[0], rule[1], rule[2], rule[3])
    qo = np.empty_like(q0)
    ok, it = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    build = C.create_string_buffer(96)
    xml = x.xml.encode()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.tree_emu_run(xml, C.c_size_t(len(xml)), 1 if TS.ROBOTS[c.robot].ff else 0, tasks, len(tasks), cons, ncons, C.c_int64(n), p(q0), p(tg),
                        C.byref(prm), C.c_double(rule[4] if c.pik else 0.0), p(qo), p(ok), p(it), layout, build, C.c_size_t(len(build)))
    assert rc == 0, L.tree_emu_last_error()
    return (qo.T if layout == 0 else qo), ok, it, build.value.decode()


def test_the_matrix_reaches_every_build_the_selection_can_return():
    reached = {c.build for c in TS.CASES} | {c.build_never for c in TS.CASES}
    assert reached == TS.every_build_string(), (sorted(TS.every_build_string() - reached), sorted(reached - TS.every_build_string()))
    # ... on every instantiated shape: hot / hot-never / mask, general x {folded, unfolded} x {none, posture, pik}, and on the two-chain
    # kernels the constraint cells
    for nj in (6, 7):
        for nch in (1, 2):
            cells = {(c.build.split(",refill")[0]) for c in TS.CASES if (c.nj, c.nch) == (nj, nch)} | \
                    {(c.build_never.split(",refill")[0]) for c in TS.CASES if (c.nj, c.nch) == (nj, nch)}
            want = {"hot,folded,none", "hot-never,folded,none", "mask,folded,none"}
            want |= {"general,%s,%s" % (f, e) for f in ("folded", "unfolded") for e in ("none", "posture", "pik") + (("constraint", "posture+constraint") if nch == 2 else ())}
            assert cells == want, (nj, nch, sorted(want - cells), sorted(cells - want))
    # every refill twin on both numbers of chains
    assert {(TS.CASE_BY_ID[i].nch, t) for i, t in TS.REFILL_CASES} == {(n, t) for n in (1, 2) for t in ("hot", "mask", "fold", "general")}
    for i, twin in TS.REFILL_CASES:
        assert TS.CASE_BY_ID[i].nj == 7 and TS.CASE_BY_ID[i].build.endswith(",refill=" + twin)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_kernel_name_and_build_string_by_the_host_analysis(native_built, monkeypatch, case):
    monkeypatch.setenv("IKGPU_TREE_STATIC_ROWS", "0")     # the tree kernel, not the static lane program (the suite's default)
    monkeypatch.delenv("IKGPU_DLS_KERNEL", raising=False)
    monkeypatch.delenv("IKGPU_PIK_KERNEL", raising=False)
    monkeypatch.delenv("IKGPU_TREE_NEVER_OFF", raising=False)
    for rule in TS.rules(case):
        kernel, build = TS.plan_names(case, rule)
        assert kernel == case.kernel and build == (case.build_never if rule[3] < 0 else case.build), (case.id, rule, kernel, build)
    if case.build != case.build_never:   # IKGPU_TREE_NEVER_OFF keeps the never-stop instantiation off
        monkeypatch.setenv("IKGPU_TREE_NEVER_OFF", "1")
        assert TS.plan_names(case, TS.rules(case)[0])[1] == case.build


def test_build_plan_refusals_and_problems_off_the_tree_kernel(native_built, monkeypatch):
    """ikgpu_dls_tree_build_plan: null arguments and an unknown pik_levels are refused; a problem that does not run on the tree kernel --
    a chain problem, a tree problem routed to the static lane program, ik::pik levels the tree kernel does not take -- gives ""."""
    import ik_amd
    from ik_amd import api, capi
    from conftest import urdf_path
    L = capi.lib()
    case = TS.CASE_BY_ID["nj6-ch1-folded-floating_ur5-hot"]
    model = ik_amd.Model.from_urdf_xml(TS.robot_xml(case.robot), free_flyer=True)
    problem = TS.make_problem(case, model)
    tasks = api._task_table(problem)
    prm = capi.DlsParams(100, 1e-2, 1.0, 1e-4)
    buf = C.create_string_buffer(96)
    assert L.ikgpu_dls_tree_build_plan(None, tasks, len(tasks), None, 0, C.byref(prm), 0, buf, len(buf)) == capi.ERR_INVALID
    assert L.ikgpu_dls_tree_build_plan(model._h, None, len(tasks), None, 0, C.byref(prm), 0, buf, len(buf)) == capi.ERR_INVALID
    assert L.ikgpu_dls_tree_build_plan(model._h, tasks, len(tasks), None, 0, None, 0, buf, len(buf)) == capi.ERR_INVALID
    assert L.ikgpu_dls_tree_build_plan(model._h, tasks, len(tasks), None, 0, C.byref(prm), 3, buf, len(buf)) == capi.ERR_INVALID
    monkeypatch.setenv("IKGPU_TREE_STATIC_ROWS", "0")
    assert ik_amd.tree_build(problem) == case.build
    assert ik_amd.tree_build(problem, pik_levels=1) == case.build      # one level and no secondary step IS the DLS iteration
    assert ik_amd.tree_build(problem, pik_levels=2) == ""             # the problem has one level
    monkeypatch.setenv("IKGPU_TREE_STATIC_ROWS", "12")                 # 12 rows: the static lane program takes the solve where hipRTC is installed
    assert ik_amd.tree_build(problem) in ("", case.build) and (ik_amd.tree_build(problem) == "") == ik_amd.plan(problem).startswith("dls_generic<")
    monkeypatch.setenv("IKGPU_TREE_STATIC_ROWS", "0")
    monkeypatch.setenv("IKGPU_DLS_KERNEL", "generic")
    assert ik_amd.tree_build(problem) == ""
    monkeypatch.delenv("IKGPU_DLS_KERNEL")
    chain = ik_amd.InverseKinematicsProblem(ik_amd.Model.from_urdf_file(urdf_path("ur5")))
    chain.add_frame_task("t", ik_amd.FrameTask.create(chain.model(), "tool0", ik_amd.KinematicType.Full))
    assert ik_amd.tree_build(chain) == ""


def test_one_posture_row_beyond_the_cap_plans_onto_the_generic_kernel(native_built, monkeypatch):
    monkeypatch.setenv("IKGPU_TREE_STATIC_ROWS", "0")
    kernel, build = TS.plan_names(TS.BEYOND_THE_CAP, TS.RULES[-1])
    assert kernel.startswith("dls_generic<") and build == "", (kernel, build)
    assert TS.EDGE_CASES[3].tail == TS.POSTURE_CAP and TS.BEYOND_THE_CAP.tail == TS.POSTURE_CAP + 1


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_launcher_build_on_the_emulator_matches_oracle(emu, case):
    x = TS.inputs(case)
    assert len(x.on_limit) == 10
    for rule in TS.rules(case):
        q, ok, it, build = emu_solve(emu, x, rule)
        assert build == (case.build_never if rule[3] < 0 else case.build), (case.id, rule, build)
        q_ref, ok_ref, it_ref = TS.oracle_solve(O, x, x.tg, x.q0, rule)
        if rule[3] >= 0.0:   # (under the never-stop visitor the flags and counts are max_iterations and "no" whatever the arithmetic)
            _, ok_q, it_q = TS.oracle_solve(O, x, x.tg, x.q0, rule, ext="q")
            assert np.array_equal(ok_ref, ok_q) and np.array_equal(it_ref, it_q), (case.id, rule, "the double and the _Float128 oracle part: choose another SEED")
        else:
            assert (it_ref == rule[0]).all() and not ok_ref.any()
        assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), (case.id, rule, np.flatnonzero(it != it_ref))
        d = np.abs(q - q_ref).max()
        print("%s %s: max |q_emu - q_oracle| = %.2e rad, iterations %d .. %d, success %.3f" % (case.id, rule, d, it.min(), it.max(), ok.mean()))
        assert d <= Q_BAR, (case.id, rule, d)
        if rule[0] == 1:   # the on-limit problems keep their joint on the limit
            for b, j in x.on_limit:
                assert q[b, j] == x.q0[b, j] and x.q0[b, j] in (x.lo[j], x.hi[j]), (case.id, b, j)
    # component-major input gives the same bits
    qs, oks, its, _ = emu_solve(emu, x, rule, layout=0)
    assert np.array_equal(qs, q) and np.array_equal(oks, ok) and np.array_equal(its, it)
