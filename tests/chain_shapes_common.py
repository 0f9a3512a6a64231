"""What the chain-shape tests share (tests/test_chain_shapes_emulation.py on the CPU, tests/test_gpu_chain_shapes.py on the device): the
matrix of chain problems and their inputs.  No tests here.

The general chain kernel is instantiated for NJ = 1 .. 8 x Position / Orientation / Full (ik_amd/csrc/kernels.hip launch_dls_chain), and
the run-time specialised hot build takes every Full, unit-weight chain of NJ <= 7 (rtc.cpp).  The matrix runs every one of them:

  arm8       fixtures/models/arm7.kin.urdf with a revolute j8 between l7 and tool and a link `bench` fixed obliquely to the base (made by
             string edit in arm8_xml(); nothing is written to disk).  Task frames l1 .. l7 and tool are chains of 1 .. 8 joints; below
             NJ = 8 the entries j(NJ+1) .. j8 lie outside the support and pass through.  Per length and task type two variants:
             (unit weights, reference universe) and (weights WEIGHTS cut to the task's dimension, reference bench) -- 48 problems on the
             general build.  Every Full / unit / universe problem of NJ <= 7 again on the default build (hot-rtc), and Full / unit / bench
             on it for NJ = 3 and 7 (the hot body composes the target from its own place).
  cassie_fixed / rightknee   NJ = 4 with q indices 8 .. 11 (not from 0) and 12 entries outside the chain; Position and Full.
  ur5 / wrist_1_link         Orientation with reference `base`: NJ = 4 on a fixture-robot table with exact zeros.

Inputs (inputs(case), computed once per case and cached -- callers copy before they write): B = 197 (three waves and a five-lane tail);
starts uniform in the limits; the target of problem b is the task frame at q0 + U(-0.15, 0.15) expressed in the reference frame
(oMr^-1 oMf by the oracle's FK).  Where entries lie outside the chain, two of them are pushed beyond their limits in every third problem.
Ten problems are rewritten so that a chain joint starts ON a limit with the first step pointing outwards, decided by the oracle alone
(as tests/test_gpu_hot_task_frame.py _inputs does): its first iterate leaves the joint on the limit while the unclipped step (the same
model with the limits lifted) crosses it.  A one-joint chain may yield fewer than ten; Position on l1 yields none -- the frame origin
lies on the joint axis, the Jacobian is identically zero and no step exists (such a lane stops at iteration 0).

The line job (line_goals): the case's own target, and for every third problem a far goal, T = 8 waypoints under the default stop rule.

SEED was chosen on the CPU, once: the double oracle, the _Float128 oracle (O.dls_batch(..., ext="q")) and the lane emulator agree on
every success flag and iteration count of every case for 1, 2, 3 fixed iterations and for the default stop rule with 100
(tests/test_chain_shapes_emulation.py asserts it again on every run)."""
import collections
import functools
import os
import re

import numpy as np

from conftest import urdf_path

B = 197
SEED = 1
WEIGHTS = [2.0, 1.0, 0.25, 1.5, 1.0, 3.0]
TYPE_NAMES = ("position", "orientation", "full")
ARM_FRAMES = ["l1", "l2", "l3", "l4", "l5", "l6", "l7", "tool"]     # chains of 1 .. 8 joints of arm8
# (max_iterations, stop tolerance): 1, 2, 3 fixed iterations (never-stop) and the default rule
RULES = [(1, -1.0), (2, -1.0), (3, -1.0), (100, 1e-4)]

Case = collections.namedtuple("Case", "robot frame nj ktype weighted reference build")


def case_id(c):
    return "%s-%s-nj%d-%s-%s-%s-%s" % (c.robot, c.frame, c.nj, TYPE_NAMES[c.ktype], "weighted" if c.weighted else "unit", c.reference, c.build)


def _cases():
    out = []
    for nj, frame in enumerate(ARM_FRAMES, 1):
        for ktype in (0, 1, 2):
            out.append(Case("arm8", frame, nj, ktype, False, "universe", "general"))
            out.append(Case("arm8", frame, nj, ktype, True, "bench", "general"))
    for nj, frame in enumerate(ARM_FRAMES[:7], 1):
        out.append(Case("arm8", frame, nj, 2, False, "universe", "default"))
    for nj in (3, 7):
        out.append(Case("arm8", ARM_FRAMES[nj - 1], nj, 2, False, "bench", "default"))
    out.append(Case("cassie_fixed", "rightknee", 4, 0, False, "universe", "general"))
    out.append(Case("cassie_fixed", "rightknee", 4, 2, False, "universe", "general"))
    out.append(Case("ur5", "wrist_1_link", 4, 1, False, "base", "general"))
    return out


CASES = _cases()
GENERAL_ARM_CASES = [c for c in CASES if c.robot == "arm8" and c.build == "general"]
HOT_CASES = [c for c in CASES if c.build == "default"]


def kernel_name(c, hiprtc=True):
    """The name of the build the case must run on.  A default-build case is hot-rtc when hipRTC is installed."""
    build = "general" if c.build == "general" or not hiprtc else "hot-rtc"
    return "dls_chain<NJ=%d,%s,%s>" % (c.nj, TYPE_NAMES[c.ktype], build)


def hiprtc_installed():
    """Decided from the installation alone, before any work (as tests/test_gpu_pik.py does)."""
    return any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7"))


def arm8_xml():
    """arm7's URDF text with the fixed tool joint turned into the revolute j8 (its origin keeps its oblique rotation) and the link
    `bench` fixed obliquely to the base."""
    xml = open(urdf_path("arm7")).read()
    fixed = ('  <joint name="tool_joint" type="fixed">\n'
             '    <origin rpy="0.21 -0.12 0.33" xyz="0.03 0.02 0.14"/>\n'
             '    <parent link="l7"/>\n'
             '    <child link="tool"/>\n'
             '  </joint>\n')
    assert xml.count(fixed) == 1
    j8 = ('  <joint name="j8" type="revolute">\n'
          '    <origin rpy="0.21 -0.12 0.33" xyz="0.03 0.02 0.14"/>\n'
          '    <axis xyz="0.64 -0.48 0.6"/>\n'
          '    <parent link="l7"/>\n'
          '    <child link="tool"/>\n'
          '    <limit lower="-2.5" upper="2.4"/>\n'
          '  </joint>\n')
    bench = ('  <link name="bench"/>\n'
             '  <joint name="bench_joint" type="fixed">\n'
             '    <origin rpy="0.3 -0.7 1.1" xyz="0.2 -0.1 0.4"/>\n'
             '    <parent link="base"/>\n'
             '    <child link="bench"/>\n'
             '  </joint>\n')
    xml = xml.replace(fixed, j8 + bench).replace('<robot name="arm7">', '<robot name="arm8">')
    assert xml.count("</robot>") == 1
    return xml


def robot_xml(robot):
    return arm8_xml() if robot == "arm8" else open(urdf_path(robot)).read()


def weights(c):
    """The task's weights (its dimension long), or None for unit weights."""
    return WEIGHTS[:6 if c.ktype == 2 else 3] if c.weighted else None


def rows(c):
    return 6 if c.ktype == 2 else 3


def make_problem(c, model):
    """The ik_amd problem of the case on `model` (Model.from_urdf_xml(robot_xml(c.robot)))."""
    import ik_amd
    problem = ik_amd.InverseKinematicsProblem(model)
    task = problem.add_frame_task("t", ik_amd.FrameTask.create(model, c.frame, ik_amd.KinematicType(c.ktype), c.reference))
    if c.weighted:
        task.weighting()[:] = weights(c)
    return problem


def _T4(m12):
    M = np.eye(4)
    M[:3, :3] = np.asarray(m12[:9]).reshape(3, 3)
    M[:3, 3] = m12[9:]
    return M


def relative_targets(O, om, q, fid, rid):
    """[n, 1, 12]: the frame's placement at q [n, nq] expressed in the reference frame, oMr^-1 oMf by the oracle's FK."""
    fr = O.fk_batch(om, q, [fid, rid])
    out = np.empty((q.shape[0], 1, 12))
    for b in range(q.shape[0]):
        rel = np.linalg.inv(_T4(fr[b, 1])) @ _T4(fr[b, 0])
        out[b, 0] = np.concatenate([rel[:3, :3].ravel(), rel[:3, 3]])
    return out


Inputs = collections.namedtuple("Inputs", "xml model om om_free fid rid tasks support q0 qs tg on_limit pushed lo hi")


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The inputs of a case (see the module's docstring).  Cached: copy an array before writing to it.
    q0, qs [B, nq]; tg [B, 1, 12] = the frame at qs in the reference frame; om_free: the oracle's model with the limits lifted; on_limit: (problem, q index) pairs; pushed: (problems [n],
    the two q indices outside the chain) or None; support [nq] bool: the chain's entries."""
    import ik_amd
    import oracle as O
    xml = robot_xml(c.robot)
    model = ik_amd.Model.from_urdf_xml(xml)
    om = O.OracleModel(model.flat())
    fid, rid = model.getFrameId(c.frame), model.getFrameId(c.reference)
    assert fid < model.nframes and rid < model.nframes
    tasks = O.make_tasks([(fid, rid, c.ktype, 0, weights(c))])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    # the chain's entries of q, read off the model: the joints between the frame and the root (a Jacobian column can be structurally
    # zero inside the chain: Position on l1)
    flat = model.flat()
    support = np.zeros(model.nq, bool)
    j = int(flat["frame_parent"][fid])
    while j > 0:
        support[int(flat["idx_q"][j])] = True
        j = int(flat["parent"][j])
    assert support.sum() == c.nj, (case_id(c), support)
    rng = np.random.default_rng(SEED)
    q0 = rng.uniform(lo, hi, (B, lo.size))
    qs = q0 + rng.uniform(-0.15, 0.15, q0.shape)
    pushed = None
    outside = np.flatnonzero(~support)
    if outside.size:
        two = outside[[0, -1]] if outside.size > 1 else outside
        who = np.arange(0, B, 3)
        q0[np.ix_(who, two)] = np.where(np.arange(who.size)[:, None] % 2 == 0, hi[two] + 0.25, lo[two] - 0.4)
        pushed = (who, two)
    # the same model with the limits lifted: the oracle's unclipped first step, and FK at configurations beyond the limits
    free = ik_amd.Model.from_urdf_xml(re.sub(r'lower="[-0-9.e]+" upper="[-0-9.e]+"', 'lower="-100.0" upper="100.0"', xml))
    om_free = O.OracleModel(free.flat())
    one = O.params(1, 1e-2, 1.0, -1.0)
    chain = np.flatnonzero(support)
    on_limit = []
    for b in range(10):
        for try_ in range(2 * chain.size):
            j, lim, out = chain[(b + try_ // 2) % chain.size], (hi, lo)[(b + try_) % 2], (1.0, -1.0)[(b + try_) % 2]
            q, s = q0[b].copy(), qs[b].copy()
            q[j], s[j] = lim[j], lim[j] + out * 0.15
            tg = relative_targets(O, om_free, s[None], fid, rid)
            q1, _, _ = O.dls(om, tasks, tg[0], q, one)
            q1_free, _, _ = O.dls(om_free, tasks, tg[0], q, one)
            if q1[j] == lim[j] and out * (q1_free[j] - lim[j]) > 1e-3:
                q0[b], qs[b] = q, s
                on_limit.append((b, int(j)))
                break
    if c.nj == 1 and c.ktype == 0:
        assert not on_limit      # the Jacobian is identically zero: no step exists
    elif c.nj == 1:
        assert len(on_limit) >= 1, (case_id(c), on_limit)
    else:
        assert len(on_limit) == 10, (case_id(c), on_limit)
    tg = relative_targets(O, om_free, qs, fid, rid)
    for a in (q0, qs, tg):
        a.setflags(write=False)
    return Inputs(xml, model, om, om_free, fid, rid, tasks, support, q0, qs, tg, on_limit, pushed, lo, hi)


@functools.lru_cache(maxsize=None)
def waypoints(c):
    """[3, B, 1, 12]: a trajectory of three waypoints towards the case's target -- the frame a third and two thirds of the way from q0 to
    qs, then the target itself -- in the reference frame, for the tracking job."""
    import oracle as O
    x = inputs(c)
    way = np.stack([relative_targets(O, x.om_free, x.q0 + f * (x.qs - x.q0), x.fid, x.rid) for f in (1.0 / 3, 2.0 / 3)] + [x.tg])
    way.setflags(write=False)
    return way


LINE_T = 8                    # waypoints per line
LINE_RULE = (100, 1e-4)       # (max_iterations, stop tolerance) of the line job


@functools.lru_cache(maxsize=None)
def line_goals(c):
    """(goals [B, 1, 12], far [n]): one goal per problem for the line job, in the reference frame.  Every problem outside `far` takes the
    case's own target (a near line: the frame at q0 + U(-0.15, 0.15)).  Problem b of far = 1, 4, 7, .. (disjoint from the pushed
    problems 0, 3, 6, ..) takes the frame at q0[b] + s d[b], d = U(-1.2, 1.2) on the chain's entries, s = 1 halved until the rotation from
    the start pose to the goal is at most line_common.MAX_ROTATION (log3 near pi is the caller's to split): lines that leave the
    workspace or the limits and fail on the way.  tests/test_chain_shapes_emulation.py asserts what this draw has to contain."""
    import line_common
    import oracle as O
    x = inputs(c)
    far = np.arange(1, B, 3)
    d = np.random.default_rng(SEED + 2).uniform(-1.2, 1.2, (B, x.model.nq)) * x.support
    start = relative_targets(O, x.om_free, x.q0, x.fid, x.rid)
    goals = np.array(x.tg)
    s, todo = np.ones(B), far
    for _ in range(40):
        goals[todo] = relative_targets(O, x.om_free, x.q0[todo] + s[todo, None] * d[todo], x.fid, x.rid)
        angle = line_common.rotation_angle(start[todo, 0, :9].reshape(-1, 3, 3), goals[todo, 0, :9].reshape(-1, 3, 3))
        todo = todo[angle > line_common.MAX_ROTATION]
        if todo.size == 0:
            break
        s[todo] *= 0.5
    assert todo.size == 0, (case_id(c), todo)
    goals.setflags(write=False)
    far.setflags(write=False)
    return goals, far


@functools.lru_cache(maxsize=None)
def _twin_model(robot):
    import twin
    return twin.load_urdf(robot_xml(robot))


@functools.lru_cache(maxsize=None)
def line_twin_waypoints(c):
    """[LINE_T, B, 12]: the waypoints of the case's lines by oracle/twin.py (log3, exp3 and FK in numpy) with the case's reference frame."""
    import line_common
    x = inputs(c)
    W = line_common.twin_waypoints(_twin_model(c.robot), c.frame, x.q0, line_goals(c)[0][:, 0], LINE_T, reference=c.reference)
    W.setflags(write=False)
    return W


MS_K, MS_B = 4, 33     # multi-start / solutions: four supplied starts on 33 problems (132 lanes: two waves and a four-lane tail)


@functools.lru_cache(maxsize=None)
def multistart_inputs(c):
    """(starts [MS_K, MS_B, nq], first [MS_B]): the starts of the first MS_B problems for the multi-start and solutions jobs, and the
    lowest start index from which the ORACLE converges under the default rule (-1: none) -- the winner the definition then names.
    The case's own start (near its target) sits in slot b % MS_K of problem b and uniform draws in the other slots, so that the winner
    is not always lane 0 of the group."""
    import oracle as O
    x = inputs(c)
    rng = np.random.default_rng(SEED + 1)
    starts = rng.uniform(x.lo, x.hi, (MS_K, MS_B, x.model.nq))
    rows_ = np.arange(MS_B)
    starts[rows_ % MS_K, rows_] = x.q0[:MS_B]
    ok = np.stack([O.dls_batch(x.om, x.tasks, x.tg[:MS_B], starts[k], O.params(100, 1e-2, 1.0, 1e-4))[1] for k in range(MS_K)]).astype(bool)
    first = np.where(ok.any(axis=0), ok.argmax(axis=0), -1)
    if c.robot == "arm8" and c.nj >= 2:
        assert len(set(first[first >= 0].tolist())) >= 2, (case_id(c), first)      # the inputs put winners into more than one lane
    starts.setflags(write=False)
    return starts, first
