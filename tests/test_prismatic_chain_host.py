"""Chains with prismatic joints, what the host decides (no device, no emulator): which kernel a problem is planned on, what the
run-time compiled hot build is keyed by, and the multi-start draw.  The matrix is tests/prismatic_common.py's.

Before the chain kernels took prismatic joints every problem here was planned on dls_generic<...>: the name assertions fail there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chain_shapes_common as CS
import multistart_common as MC
import prismatic_common as PC
from conftest import urdf_path


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_a_chain_with_prismatic_joints_is_planned_on_the_chain_kernel(ik, monkeypatch, c):
    x = PC.inputs(c)
    assert (x.support & x.prismatic).any()
    problem = PC.make_problem(c, x.model)
    general = PC.kernel_name(c, "general")
    hot_shape = c.ktype == 2 and not c.weighted and c.nj <= 7       # a Full, unit-weight chain of at most seven joints
    monkeypatch.delenv("IKGPU_CHAIN_HOT", raising=False)
    monkeypatch.delenv("IKGPU_RTC", raising=False)
    want = PC.kernel_name(c, "hot-rtc") if hot_shape and CS.hiprtc_installed() else general
    assert ik.plan(problem) == want
    assert not ik.plan(problem).endswith(",hot>")                  # never a pre-built program: those are chains of revolute joints
    monkeypatch.setenv("IKGPU_RTC", "0")
    assert ik.plan(problem) == general
    monkeypatch.delenv("IKGPU_RTC")
    monkeypatch.setenv("IKGPU_CHAIN_HOT", "0")
    assert ik.plan(problem) == general
    monkeypatch.setenv("IKGPU_DLS_KERNEL", "generic")              # the route these problems took before
    assert ik.plan(problem).startswith("dls_generic<")


def test_the_prismatic_elbow_has_the_prebuilt_programs_code_and_does_not_get_it(ik, monkeypatch):
    """UR5 with a sliding elbow has UR5's placement code.  The revolute UR5 plans the pre-built hot program; the other must not."""
    monkeypatch.delenv("IKGPU_CHAIN_HOT", raising=False)
    c = next(k for k in PC.CASES if k.robot == "ur5_elbow")
    revolute = ik.Model.from_urdf_xml(open(urdf_path("ur5")).read())
    p = ik.InverseKinematicsProblem(revolute)
    p.add_frame_task("t", ik.FrameTask.create(revolute, "tool0", ik.KinematicType.Full, "base"))
    assert ik.plan(p) == "dls_chain<NJ=6,full,hot>"
    assert ik.plan(PC.make_problem(c, PC.inputs(c).model)) in ("dls_chain<NJ=6,full,hot-rtc>", "dls_chain<NJ=6,full,general>")


@pytest.mark.parametrize("c", PC.HOT_CASES, ids=PC.case_id)
def test_the_hot_program_of_a_prismatic_chain_compiles_for_gfx950(ik, tmp_path, monkeypatch, c):
    """ikgpu_problem_precompile without a device, into an empty cache directory (tests/test_chain_shapes_emulation.py does the same
    for chains of revolute joints).  A compile that fails would make the library run the general build in the program's place."""
    if not CS.hiprtc_installed():
        pytest.skip("hipRTC is not installed")
    monkeypatch.delenv("IKGPU_CHAIN_HOT", raising=False)
    monkeypatch.setenv("IKGPU_CACHE_DIR", str(tmp_path))
    assert ik.precompile(PC.make_problem(c, PC.inputs(c).model)) == PC.kernel_name(c, "hot-rtc")
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].startswith("chain_hot_") and files[0].endswith(".hsaco"), files


_TWINS = """
import os, sys
sys.path[:0] = [%r, %r, %r]
import chain_shapes_common as CS, prismatic_common as PC, ik_amd
rev = next(k for k in CS.HOT_CASES if k.nj == 7 and k.reference == "universe")
pris = next(k for k in PC.HOT_CASES if k.robot == "arm8_j7")
print(ik_amd.precompile(CS.make_problem(rev, CS.inputs(rev).model)), len(os.listdir(os.environ["IKGPU_CACHE_DIR"])))
print(ik_amd.precompile(PC.make_problem(pris, PC.inputs(pris).model)), len(os.listdir(os.environ["IKGPU_CACHE_DIR"])))
"""


def test_the_revolute_chain_and_its_prismatic_twin_are_two_programs(ik, tmp_path):
    """The on-disk cache is keyed by the generated text, which names the mask of prismatic joints: arm8 / l7 and the same chain with j7
    sliding have one placement code and two cache entries.  In a process of its own: a program compiled once is kept in memory."""
    if not CS.hiprtc_installed():
        pytest.skip("hipRTC is not installed")
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, IKGPU_CACHE_DIR=str(tmp_path))
    env.pop("IKGPU_CHAIN_HOT", None)
    out = subprocess.check_output([sys.executable, "-c", _TWINS % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))], env=env, text=True)
    assert out.split() == ["dls_chain<NJ=7,full,hot-rtc>", "1", "dls_chain<NJ=7,full,hot-rtc>", "2"], out


def _tree_with_a_prismatic_joint(ik):
    """cassie (free-flyer) with the left knee made prismatic: the left-foot chain of a tree-kind problem has a sliding joint."""
    xml = open(urdf_path("cassie")).read()
    joint = next(j for j in re.findall(r'<joint name="([^"]+)" type="revolute">', xml) if "knee" in j.lower() and "left" in j.lower())
    return PC._prismatic(xml, joint), joint


def test_the_tree_kind_keeps_refusing_a_prismatic_joint(ik):
    xml, joint = _tree_with_a_prismatic_joint(ik)
    for model_xml, generic in ((open(urdf_path("cassie")).read(), False), (xml, True)):
        model = ik.Model.from_urdf_xml(model_xml, free_flyer=True)
        problem = ik.InverseKinematicsProblem(model)
        problem.add_frame_task("lf", ik.FrameTask.create(model, "LeftFootFront", ik.KinematicType.Full))
        problem.add_frame_task("rf", ik.FrameTask.create(model, "RightFootFront", ik.KinematicType.Full))
        name = ik.plan(problem)
        assert name.startswith("dls_generic<") if generic else name.startswith("dls_tree<"), (joint, name)


@pytest.mark.parametrize("c", [c for c in CS.CASES if (c.robot, c.frame) in (("arm8", "l7"), ("ur5", "wrist_1_link"), ("cassie_fixed", "rightknee"))][:6],
                         ids=CS.case_id)
def test_chains_of_revolute_joints_plan_what_they_planned(ik, monkeypatch, c):
    monkeypatch.delenv("IKGPU_CHAIN_HOT", raising=False)
    problem = CS.make_problem(c, CS.inputs(c).model)
    if c.build == "default":
        assert ik.plan(problem) == CS.kernel_name(c, CS.hiprtc_installed())
    monkeypatch.setenv("IKGPU_CHAIN_HOT", "0")
    assert ik.plan(problem) == "dls_chain<NJ=%d,%s,general>" % (c.nj, CS.TYPE_NAMES[c.ktype])


def test_the_cassie_leg_and_ur5_keep_their_prebuilt_programs(ik, monkeypatch):
    monkeypatch.delenv("IKGPU_CHAIN_HOT", raising=False)
    for name, frame, want in (("cassie_fixed", "LeftFootFront", "dls_chain<NJ=7,full,hot>"), ("ur5", "tool0", "dls_chain<NJ=6,full,hot>")):
        model = ik.Model.from_urdf_xml(open(urdf_path(name)).read())
        p = ik.InverseKinematicsProblem(model)
        p.add_frame_task("t", ik.FrameTask.create(model, frame, ik.KinematicType.Full))
        assert ik.plan(p) == want


@pytest.mark.parametrize("c", [PC.JOB_CASES[0], PC.JOB_CASES[1], PC.CASES[0]], ids=PC.case_id)
def test_generated_starts_draw_the_prismatic_entries_of_the_support(native_built, c):
    """ikgpu_multistart_starts' host rule (tests/lane_emu/prismatic_emu.cpp restates the kernel): a prismatic entry of the support is
    drawn inside [lo, hi] by the formula of tests/multistart_common.py and differs from q0; entries outside the support are q0's."""
    L = PC.compile_emulator()
    E = PC.Emu(L, c)
    x = E.x
    st, sup, draw = E.structure()
    assert np.array_equal(sup, x.support)
    assert np.array_equal(draw, x.support)                   # every joint of these chains is bounded
    assert (draw & x.prismatic).any()
    assert st[4] == sum(1 << k for k, i in enumerate(np.flatnonzero(x.support)) if x.prismatic[i])       # the chain's mask of prismatic joints
    assert st[5] >> 16 == st[4]                              # ... as the kernels receive it
    q0, K, seed = np.array(x.q0[:5]), 4, 12345
    starts = E.starts(q0, K, seed)
    for k in range(1, K):
        for b in range(5):
            for i in np.flatnonzero(draw):
                want = MC.draw(seed, b, k, int(i), float(x.lo[i]), float(x.hi[i]))
                assert abs(starts[k - 1, b, i] - want) <= 2 * np.spacing(max(abs(want), abs(starts[k - 1, b, i]))), (k, b, i)
    sl = draw & x.prismatic
    assert (starts[:, :, sl] >= x.lo[sl]).all() and (starts[:, :, sl] <= x.hi[sl]).all() and (starts[:, :, sl] != q0[:, sl]).all()
    assert np.array_equal(starts[:, :, ~draw], np.broadcast_to(q0[:, ~draw], (K - 1, 5, int((~draw).sum()))))
    assert np.array_equal(E.starts(q0, K, seed, layout=0), starts)
