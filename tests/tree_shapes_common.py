"""What the tree-shape tests share (tests/test_tree_shapes_emulation.py on the CPU, tests/test_gpu_tree_shapes.py on the device): the
robots, the matrix of tree problems and their inputs.  No tests here.

The tree kernel is instantiated for (NJ, chains) in {(7,2), (7,1), (6,2), (6,1)}, and per shape the launcher picks one of up to
thirteen compile-time builds (ik_amd/csrc/problem.cpp select_tree_build; include/ikgpu.h ikgpu_dls_tree_build_plan reports it):
hot, hot under the never-stop visitor, mask, and the general build with the placement mask folded or not x {no extras, posture rows,
a FrameConstraint, posture rows next to the constraint, level 1 of a two-level ik::pik}.  The matrix holds one case per (shape,
build, folded, extras) cell the launcher can reach.

Robots (made by string edit from the committed fixtures; nothing is written to disk):
  floating_ur5        ur5 with a free flyer.  Chain frame tool0: NJ = 6, placement mask 0x05 = HotMask<6>.  Base frames base_link
                      (identity placement) and base (turned by pi).
  dual_ur5(rpy)       the UR5 body again with every link and joint name prefixed r_, its world_joint re-parented to link world at
                      xyz "0 -0.45 0.1" rpy `rpy`; nq = 19.  "0 0 0" (dual_ur5): both chains carry the mask, the folded builds run;
                      "0.3 -0.2 0.5" (dual_ur5_oblique): chain B loses bit 0, the unfolded builds run; a full turn about z
                      (dual_ur5_turn): the same robot to rounding, and unfolded.
  floating_arm7       arm7 with a free flyer; frames tool (NJ = 7) and l6 (NJ = 6); no identity placement: unfolded.
  dual_arm7           the arm again with prefix r_ on the same base link, its first joint origin moved to "0.05 -0.32 0.21"; nq = 21;
                      tool / r_tool is (7,2) unfolded, l6 / r_l6 is (6,2) unfolded.
  cassie              the folded NJ = 7 cells.
  with_tail(xml, n)   n extra revolute joints chained off the base link (as _tail in tests/test_gpu_generic.py): the joints outside
                      the chains that carry posture rows, up to the kernel's cap of 32.

How the builds are reached.  hot: Full unit-weight chain tasks and a Full unit-weight base task on a frame at a pure translation;
under the never-stop visitor (the fixed-iteration rules) the same problem is hot-never.  mask: the chain task weighted.  general
without extras: the chain task given in a frame on the floating base (a base-relative reference) where the chains carry the mask,
nothing at all where they do not.  posture: that plus PostureTask rows on every joint, with holes in the mask and uneven weights.
pik: the demo's shape (chain Position task in the base frame, Full base task, an alignment row one level down).  constraint and
posture+constraint (NCH = 2 kernels only): one task chain, the other limb's frame pinned to the universe -- their name says chains=1.

Unreachable cells: a constraint on a one-chain kernel (the constrained limb IS the second chain: select_tree_build reports such a
problem as not launchable and the analysis never produces it); hot, hot-never and mask without the mask folded (they are the folded
builds by definition); refill twins other than none at NJ = 6 or next to posture rows, a constraint or a pik level.

Inputs (inputs(case), computed once per case and cached -- callers copy before they write): B = 197 (three waves and a five-lane tail,
not a multiple of the 128-lane tree workgroup); the base pose perturbed about identity and the joints about a nominal posture
(ik_amd.workload.freeflyer_workload); the target of every task is its frame at a nearby q* expressed in the task's reference frame,
an alignment row asks for the axis at q*, a posture row for q*'s entry.  In every third problem two entries outside every chain are
pushed beyond their limits.  Ten problems are rewritten so that a chain joint starts ON a limit with the first step pointing
outwards, decided by the oracle alone (as tests/chain_shapes_common.py does; a start the double oracle itself does not answer to
ORACLE_AGREES of its _Float128 version is passed over: see there).

SEED was chosen on the CPU, once: the double oracle, the _Float128 oracle (ext="q") and the lane emulator agree on every success flag
and iteration count of every case and rule (tests/test_tree_shapes_emulation.py asserts it again on every run)."""
import collections
import functools
import os
import re

import numpy as np

from conftest import urdf_path

B = 197
SEED = 1
# (max_iterations, damping, step length, stop tolerance): 1, 2, 3 fixed iterations (never-stop) and the default rule
RULES = [(1, 1e-2, 1.0, -1.0), (2, 1e-2, 1.0, -1.0), (3, 1e-2, 1.0, -1.0), (100, 1e-2, 1.0, 1e-4)]
# ... of a case with an alignment row (full steps are chaotic there beyond a few iterations: the note in tests/test_gpu_generic.py)
ALIGN_STOP_RULE = (100, 1e-1, 0.5, 1e-4)
# ik::pik cells: (max_iterations, lambda_0, step length, stop tolerance, lambda_1)
PIK_RULES = [(1, 1.0, 1.0, -1.0, 1.0), (2, 0.1, 1.0, -1.0, 0.1), (3, 0.1, 1.0, -1.0, 0.1), (30, 0.05, 0.5, 1e-8, 0.1)]
# An on-limit start is taken only where the double oracle's first iterate agrees with its own _Float128 version this closely.  Some
# limits are kinematic singularities (the UR5's elbow at +-pi, its wrist_2 at +-2 pi): with a Full task on all six joints of the other
# arm the null-space projector of a two-level ik::pik is decided by rounding there, the double oracle parts from the _Float128 one by
# 1.4e-7 rad after one step (3e-5 after two) and cannot arbitrate a 1e-8 bar -- the lane program agrees with the _Float128 oracle to
# 3e-16 on those very starts.  Decided by the oracle alone, as the rest of the rewrite.
ORACLE_AGREES = 1e-10
POSTURE_CAP = 32     # ikdev::kMaxPostOut: posture rows on joints outside the chains

MOUNT_STRAIGHT, MOUNT_OBLIQUE = "0 0 0", "0.3 -0.2 0.5"
# a full turn about z: the rotation's sine is -2.4e-16, not zero -- the same robot to rounding, but chain B's first placement is no
# longer an exact identity rotation, so the mask bit goes and the unfolded builds run (tests/test_gpu_tree_shapes.py, folded against unfolded)
MOUNT_FULL_TURN = "0 0 6.283185307179586"


# ---- robots --------------------------------------------------------------------------------------------------------------------------
def _prefixed(body, keep):
    """Every name="X" / link="X" of the URDF fragment prefixed r_, except the links in `keep`."""
    def sub(m):
        return m.group(0) if m.group(2) in keep else '%s="r_%s"' % (m.group(1), m.group(2))
    return re.sub(r'\b(name|link)="([^"]+)"', sub, body)


def _robot_body(xml, name):
    head = '<robot name="%s">' % name
    assert xml.count(head) == 1 and xml.count("</robot>") == 1
    return xml[xml.index(head) + len(head):xml.index("</robot>")]


def dual_ur5_xml(mount_rpy):
    xml = open(urdf_path("ur5")).read()
    body = _robot_body(xml, "ur5")
    world = '  <link name="world"/>\n'
    assert body.count(world) == 1
    twin = _prefixed(body.replace(world, ""), {"world"})
    joint = ('  <joint name="r_world_joint" type="fixed">\n'
             '    <origin rpy="0.0 0.0 0.0" xyz="0.0 0.0 0.0"/>\n')
    assert twin.count(joint) == 1
    twin = twin.replace(joint, '  <joint name="r_world_joint" type="fixed">\n    <origin rpy="%s" xyz="0 -0.45 0.1"/>\n' % mount_rpy)
    return xml.replace("</robot>", twin + "</robot>").replace('<robot name="ur5">', '<robot name="dual_ur5">')


def dual_arm7_xml():
    xml = open(urdf_path("arm7")).read()
    body = _robot_body(xml, "arm7")
    base = body[body.index('  <link name="base">'):body.index('  <link name="l1">')]
    twin = _prefixed(body.replace(base, ""), {"base"})
    first = '<origin rpy="0.11 -0.23 0.37" xyz="0.05 -0.02 0.31"/>'
    assert twin.count(first) == 1
    twin = twin.replace(first, '<origin rpy="0.11 -0.23 0.37" xyz="0.05 -0.32 0.21"/>')
    return xml.replace("</robot>", twin + "</robot>").replace('<robot name="arm7">', '<robot name="dual_arm7">')


def with_tail(xml, n, base_link):
    """n extra revolute joints chained off `base_link`, after every other joint (so that they are the last n entries of q)."""
    extra, parent = [], base_link
    for k in range(n):
        link = "tail%d" % k
        extra.append('  <link name="%s"><inertial><mass value="0.%d"/><origin rpy="0 0 0" xyz="0.01 0 0.02"/></inertial></link>' % (link, k % 9 + 1))
        extra.append('  <joint name="tail-joint%d" type="revolute"><parent link="%s"/><child link="%s"/><origin rpy="0 0 0" xyz="0.05 0 %s"/>'
                     '<axis xyz="%s"/><limit lower="-1.5" upper="1.5"/></joint>' % (k, parent, link, "0.03" if k % 2 else "-0.02", ("0 0 1", "0 1 0", "1 0 0")[k % 3]))
        parent = link
    assert xml.count("</robot>") == 1
    return xml.replace("</robot>", "\n".join(extra) + "\n</robot>")


# robot -> (xml maker, free flyer, chain frame A, chain frame B or None, base frame at an identity placement, base frame turned,
#           link the tail hangs off, nominal posture: "zero" | "ur5" | "cassie")
Robot = collections.namedtuple("Robot", "xml ff A B base_id base_turned tail_link nominal")
ROBOTS = {
    "floating_ur5": Robot(lambda: open(urdf_path("ur5")).read(), True, "tool0", None, "base_link", "base", "base_link", "ur5"),
    "dual_ur5": Robot(lambda: dual_ur5_xml(MOUNT_STRAIGHT), True, "tool0", "r_tool0", "base_link", "base", "base_link", "ur5"),
    "dual_ur5_oblique": Robot(lambda: dual_ur5_xml(MOUNT_OBLIQUE), True, "tool0", "r_tool0", "base_link", "base", "base_link", "ur5"),
    "dual_ur5_turn": Robot(lambda: dual_ur5_xml(MOUNT_FULL_TURN), True, "tool0", "r_tool0", "base_link", "base", "base_link", "ur5"),
    "floating_arm7": Robot(lambda: open(urdf_path("arm7")).read(), True, "tool", None, "base", None, "base", "zero"),
    "floating_arm7_l6": Robot(lambda: open(urdf_path("arm7")).read(), True, "l6", None, "base", None, "base", "zero"),
    "dual_arm7": Robot(dual_arm7_xml, True, "tool", "r_tool", "base", None, "base", "zero"),
    "dual_arm7_l6": Robot(dual_arm7_xml, True, "l6", "r_l6", "base", None, "base", "zero"),
    "cassie": Robot(lambda: open(urdf_path("cassie")).read(), True, "LeftFootFront", "RightFootFront", "pelvis", None, "pelvis", "cassie"),
    "cassie_fixed": Robot(lambda: open(urdf_path("cassie_fixed")).read(), False, "LeftFootFront", "RightFootFront", None, None, None, "cassie"),
}
# (NJ, folded) -> robot, per number of chains the kernel is instantiated for
SHAPE_ROBOT = {(7, 1, True): "cassie", (7, 2, True): "cassie", (7, 1, False): "floating_arm7", (7, 2, False): "dual_arm7",
               (6, 1, True): "floating_ur5", (6, 2, True): "dual_ur5", (6, 1, False): "floating_arm7_l6", (6, 2, False): "dual_ur5_oblique"}


@functools.lru_cache(maxsize=None)
def robot_xml(robot, tail=0):
    r = ROBOTS[robot]
    xml = r.xml()
    return with_tail(xml, tail, r.tail_link) if tail else xml


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
# specs: (kind 'frame' | 'align' | 'posture', frame | nj, reference, type | axis, priority, weights | (weights, mask)) as tests/test_gpu_generic.py
# build(); cons: ((frame, type, reference),) or (); pik: the case is solved by ik::pik with two levels.
# nj, nch: the kernel instantiation that runs (a constraint cell's name says chains=1 and runs the two-chain kernel).
Case = collections.namedtuple("Case", "id robot tail nj nch specs cons pik kernel build build_never")

WEIGHTS = (2.0, 1.0, 0.25, 1.5, 1.0, 3.0)


def posture_spec(n, priority):
    """PostureTask rows on the last n joints: uneven weights, a mask with holes (as posture_regulariser in tests/test_gpu_generic.py)."""
    return ("posture", n, None, None, priority, (tuple(0.1 + 0.05 * (k % 9) for k in range(n)), tuple(0.0 if k % 7 == 3 else 1.0 for k in range(n))))


def build_string(nj, build, folded, extras):
    """The name ikgpu_dls_tree_build_plan must give the cell: "<build>,<folded|unfolded>,<extras>,refill=<twin>".  The twin: NJ = 7
    only, and only without posture rows, a constraint or a pik level."""
    twin = "none"
    if nj == 7 and extras == "none":
        twin = {"hot": "hot", "hot-never": "hot", "mask": "mask"}.get(build, "fold" if folded else "general")
    return "%s,%s,%s,refill=%s" % (build, "folded" if folded else "unfolded", extras, twin)


def _joints(robot):
    return {"floating_ur5": 6, "dual_ur5": 12, "dual_ur5_oblique": 12, "dual_ur5_turn": 12, "floating_arm7": 7, "floating_arm7_l6": 7, "dual_arm7": 14,
            "dual_arm7_l6": 14, "cassie": 16, "cassie_fixed": 16}[robot]


def _cases():
    out = []
    for (nj, nch, folded), robot in sorted(SHAPE_ROBOT.items(), reverse=True):
        r = ROBOTS[robot]
        shape = "nj%d-ch%d-%s" % (nj, nch, "folded" if folded else "unfolded")
        second = [("frame", r.B, "universe", 2, 0, None)] if nch == 2 else []
        head = "dls_tree<NJ=%d,chains=%d" % (nj, nch)

        def case(tag, specs, kernel, build, extras, cons=(), pik=False, tail=0, build_never=None):
            b = build_string(nj, build, folded, extras)
            out.append(Case("%s-%s-%s" % (shape, robot, tag), robot, tail, nj, nch, tuple(specs), tuple(cons), pik, kernel, b,
                            build_string(nj, build_never, folded, extras) if build_never else b))

        if folded:
            hot = [("frame", r.A, "universe", 2, 0, None)] + second + [("frame", r.base_id, "universe", 2, 0, None)]
            case("hot", hot, head + ",base_task>", "hot", "none", build_never="hot-never")
            mask = [("frame", r.A, "universe", 0, 0, WEIGHTS[:3])] + second + [("frame", r.base_id, "universe", 2, 0, None)]
            case("mask", mask, head + ",base_task>", "mask", "none")
            if r.base_turned:   # ... and through the base task on a frame whose placement is no pure translation
                turned = [("frame", r.A, "universe", 2, 0, None)] + second + [("frame", r.base_turned, "universe", 2, 0, None)]
                case("mask-base-turned", turned, head + ",base_task>", "mask", "none")
        # general, no extras: where the chains carry the mask a base-relative reference keeps the problem off hot / mask
        if folded:
            none, none_kernel = [("frame", r.A, r.base_id, 2, 0, None)], head + ",base_task,base_reference"
        else:
            none, none_kernel = [("frame", r.A, "universe", 2, 0, None)], head + ",base_task"
        none = none + second + [("frame", r.base_id, "universe", 2, 0, None)]
        case("general-none", none, none_kernel + ">", "general", "none")
        case("general-posture", none + [posture_spec(_joints(robot), 1)], none_kernel + ",posture>", "general", "posture")
        pik = [("frame", r.A, r.base_id, 0, 0, None)] + second + [("frame", r.base_id, "universe", 2, 0, None), ("align", r.A, "universe", 1, 1, None)]
        case("general-pik", pik, head + ",base_task,base_reference,align_axis>", "general", "pik", pik=True)
        if nch == 2:   # the other limb pinned to the universe: one task chain, the two-chain kernel
            one = "dls_tree<NJ=%d,chains=1" % nj
            cons = [("frame", r.A, "universe", 2, 0, None), ("frame", r.base_id, "universe", 2, 0, None)]
            case("general-constraint", cons, one + ",base_task,constraint_rows=3>", "general", "constraint", cons=[(r.B, 0, "universe")])
            case("general-posture+constraint", cons + [posture_spec(_joints(robot), 0)], one + ",base_task,posture,constraint_rows=3>", "general",
                 "posture+constraint", cons=[(r.B, 0, "universe")])
    return out


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}


def _edge_cases():
    """Posture rows outside the chains near the cap (POSTURE_CAP = 32).  One chain: the launcher asks for 1024 (2 post_n + NJ) bytes of
    dynamic LDS, 64 KiB at post_n = 29 for NJ = 6.  The other limb pinned: the outside joints live in the idle park buffer while
    2 post_n + NJ <= 63 entries (post_n = 28), else in the q_out column (29)."""
    out = []
    for n in (28, 29, 30, 32):
        specs = [("frame", "tool0", "base_link", 2, 0, None), ("frame", "base_link", "universe", 2, 0, None), posture_spec(n + 6, 1)]
        out.append(Case("edge-floating_ur5-tail%d-posture" % n, "floating_ur5", n, 6, 1, tuple(specs), (), False,
                        "dls_tree<NJ=6,chains=1,base_task,base_reference,posture>", build_string(6, "general", True, "posture"),
                        build_string(6, "general", True, "posture")))
    for n in (28, 29):
        specs = [("frame", "tool0", "universe", 2, 0, None), ("frame", "base_link", "universe", 2, 0, None), posture_spec(n + 12, 0)]
        out.append(Case("edge-dual_ur5-tail%d-posture+constraint" % n, "dual_ur5", n, 6, 2, tuple(specs), (("r_tool0", 0, "universe"),), False,
                        "dls_tree<NJ=6,chains=1,base_task,posture,constraint_rows=3>", build_string(6, "general", True, "posture+constraint"),
                        build_string(6, "general", True, "posture+constraint")))
    return out


EDGE_CASES = _edge_cases()
# one row too many: the problem must plan onto the generic kernel
BEYOND_THE_CAP = Case("edge-floating_ur5-tail33-posture", "floating_ur5", 33, 6, 1,
                      (("frame", "tool0", "base_link", 2, 0, None), ("frame", "base_link", "universe", 2, 0, None), posture_spec(39, 1)), (), False,
                      "dls_generic<", "", "")

# Refill cells (NJ = 7 only): every twin on both numbers of chains, as (case id, twin)
REFILL_CASES = [("nj7-ch1-folded-cassie-hot", "hot"), ("nj7-ch2-folded-cassie-hot", "hot"),
                ("nj7-ch1-folded-cassie-mask", "mask"), ("nj7-ch2-folded-cassie-mask", "mask"),
                ("nj7-ch1-folded-cassie-general-none", "fold"), ("nj7-ch2-folded-cassie-general-none", "fold"),
                ("nj7-ch1-unfolded-floating_arm7-general-none", "general"), ("nj7-ch2-unfolded-dual_arm7-general-none", "general")]


def every_build_string():
    """What select_tree_build can return for the four instantiated shapes, written out from its rules: hot / hot-never / mask are folded
    and carry no extras; general is folded or not with any of the extras, the constraint ones on two-chain kernels only (so every
    string a one-chain kernel can give a two-chain kernel gives too)."""
    out = set()
    for nj in (6, 7):
        for b in ("hot", "hot-never", "mask"):
            out.add(build_string(nj, b, True, "none"))
        for folded in (True, False):
            for extras in ("none", "posture", "pik", "constraint", "posture+constraint"):
                out.add(build_string(nj, "general", folded, extras))
    return out


def rules(c):
    """The (max_iterations, damping | lambda_0, step length, stop tolerance[, lambda_1]) rules of a case."""
    if c.pik:
        return PIK_RULES
    if any(s[0] == "align" for s in c.specs):
        return RULES[:3] + [ALIGN_STOP_RULE]
    return RULES


# ---- problems and inputs -------------------------------------------------------------------------------------------------------------
def make_problem(c, model):
    """The ik_amd problem of the case on `model` (Model.from_urdf_xml(robot_xml(c.robot, c.tail), free_flyer=ROBOTS[c.robot].ff))."""
    import ik_amd
    problem = ik_amd.InverseKinematicsProblem(model, max(s[4] for s in c.specs))
    for i, (kind, f, r, t, p, w) in enumerate(c.specs):
        if kind == "posture":
            task = problem.add_posture_task("t%d" % i, ik_amd.PostureTask.create(model, f), p)
            task.weighting()[:], task.mask[:] = w
            continue
        if kind == "align":
            task = problem.add_align_axis_task("t%d" % i, ik_amd.AlignAxisTask.create(model, f, ik_amd.AlignAxisType(t), r), p)
        else:
            task = problem.add_frame_task("t%d" % i, ik_amd.FrameTask.create(model, f, ik_amd.KinematicType(t), r), p)
        if w is not None:
            task.weighting()[:] = w
    for i, (f, t, r) in enumerate(c.cons):
        problem.add_frame_constraint("c%d" % i, ik_amd.FrameConstraint.create(model, f, ik_amd.KinematicType(t), r))
    return problem


def oracle_spec(model, problem):
    """The oracle's task records in stacking order: (frame, reference, type, priority, weights); a posture row is (tangent column,
    q index, 6, priority, [weight, mask])."""
    import ik_amd
    ospec = []
    for t, prio in problem.ordered_tasks():
        if isinstance(t, ik_amd.PostureTask):
            ospec += [(model.nv - t.nj + k, model.nq - t.nj + k, 6, prio, [t.weighting()[k], t.mask[k]]) for k in range(t.nj)]
            continue
        w = None if np.all(t.weighting() == 1) else list(t.weighting())
        ospec.append((t._frame_id, t._ref_id, 3 + int(t.axis) if isinstance(t, ik_amd.AlignAxisTask) else int(t.type), prio, w))
    return ospec


def targets_at(O, om, ospec, qs):
    """[n, ntasks, 12]: every task's target such that its error vanishes at qs [n, nq] -- the frame in the reference frame (oMr^-1 oMf),
    the direction of the frame's axis in the reference frame (alignment row), the entry of q (posture row)."""
    n = qs.shape[0]
    frames = sorted({s[0] for s in ospec if s[2] != 6} | {s[1] for s in ospec if s[2] != 6})
    poses = O.fk_batch(om, qs, frames)
    at = {f: k for k, f in enumerate(frames)}
    tg = np.zeros((n, len(ospec), 12))
    for i, (fid, rid, typ, _, _) in enumerate(ospec):
        if typ == 6:
            tg[:, i, 9] = qs[:, rid]
            continue
        Rf, pf = poses[:, at[fid], :9].reshape(n, 3, 3), poses[:, at[fid], 9:]
        Rr, pr = poses[:, at[rid], :9].reshape(n, 3, 3), poses[:, at[rid], 9:]
        if typ >= 3:
            tg[:, i, :9] = np.eye(3).ravel()
            tg[:, i, 9:] = np.einsum("bki,bk->bi", Rr, Rf[:, :, typ - 3])
        else:
            tg[:, i, :9] = np.einsum("bki,bkj->bij", Rr, Rf).reshape(n, 9)
            tg[:, i, 9:] = np.einsum("bki,bk->bi", Rr, pf - pr)
    return tg


def oracle_solve(O, x, tg, q0, rule, ext=None, om=None):
    """The case's solve by the oracle under `rule` (rules(case)): ik::dls, ik::dls with the constraint, or ik::pik with two levels."""
    om = om or x.om
    threads = min(16, os.cpu_count() or 1) if q0.shape[0] > 1 else 1
    if x.case.pik:
        iters, lam0, step, tol, lam1 = rule
        return O.pik_batch(om, x.tasks, tg, q0, O.pik_params(iters, step, tol, [lam0, lam1]), threads, ext)
    iters, damping, step, tol = rule
    if x.cons is not None:
        return O.dls_batch_constrained(om, x.tasks, x.cons, tg, q0, O.params(iters, damping, step, tol), threads, ext)
    return O.dls_batch(om, x.tasks, tg, q0, O.params(iters, damping, step, tol), threads, ext)


Inputs = collections.namedtuple("Inputs", "case xml model problem om om_free ospec tasks cons chain q0 qs tg on_limit pushed lo hi")


def _chain_entries(model, frames):
    """[nq] bool: the entries of q of the joints between the frames and the root (the free flyer's seven left out)."""
    flat = model.flat()
    support = np.zeros(model.nq, bool)
    for f in frames:
        j = int(flat["frame_parent"][f])
        while j > 0:
            support[int(flat["idx_q"][j])] = True     # (the free flyer's first entry too: the caller clears its seven)
            j = int(flat["parent"][j])
    return support


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The inputs of a case (see the module's docstring).  Cached: copy an array before writing to it.  q0, qs [B, nq]; tg [B, ntasks, 12];
    om_free: the oracle's model with the limits lifted; chain [nq] bool: the entries of the chains' joints; on_limit: (problem, q index)
    pairs; pushed: (problems [n], the two q indices outside every chain) or None."""
    import ik_amd
    import oracle as O
    from ik_amd import workload
    r = ROBOTS[c.robot]
    xml = robot_xml(c.robot, c.tail)
    model = ik_amd.Model.from_urdf_xml(xml, free_flyer=r.ff)
    problem = make_problem(c, model)
    om = O.OracleModel(model.flat())
    ospec = oracle_spec(model, problem)
    tasks = O.make_tasks(ospec)
    cons = O.make_tasks([(model.getFrameId(f), model.getFrameId(ref), t, 0, None) for f, t, ref in c.cons]) if c.cons else None
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    off = 7 if r.ff else 0
    frames = [s[0] for s in ospec if s[2] < 3] + [model.getFrameId(f) for f, _, _ in c.cons]
    chain = _chain_entries(model, frames)
    chain[:off] = False
    assert chain.sum() == c.nj * c.nch, (c.id, chain.sum())
    nj_all = model.nq - off
    nominal = np.zeros(nj_all)
    if r.nominal == "cassie":
        nominal = np.asarray(workload.cassie_nominal(model.names), float)
    elif r.nominal == "ur5":
        arm = np.asarray(workload.UR5_NOMINAL, float)
        nominal[:6] = arm
        if r.B:
            nominal[6:12] = arm
    idx = np.arange(B)
    if r.ff:
        q0, qs = workload.freeflyer_workload(lo, hi, nominal, idx, seed=SEED)
    else:
        q0, qs = workload.chain_workload(lo, hi, nominal, idx, SEED, "near")
    q0, qs = np.array(q0), np.array(qs)
    pushed = None
    outside = np.flatnonzero(~chain)
    outside = outside[outside >= off]
    if outside.size:
        two = outside[[0, -1]] if outside.size > 1 else outside
        who = np.arange(0, B, 3)
        q0[np.ix_(who, two)] = np.where(np.arange(who.size)[:, None] % 2 == 0, hi[two] + 0.25, lo[two] - 0.4)
        pushed = (who, two)
    # the same model with the limits lifted: the oracle's unclipped first step, and FK at configurations beyond the limits
    free = ik_amd.Model.from_urdf_xml(re.sub(r'lower="[-0-9.e]+" upper="[-0-9.e]+"', 'lower="-100.0" upper="100.0"', xml), free_flyer=r.ff)
    om_free = O.OracleModel(free.flat())
    x = Inputs(c, xml, model, problem, om, om_free, ospec, tasks, cons, chain, None, None, None, None, None, lo, hi)
    one = rules(c)[0]
    joints = np.flatnonzero(chain)
    on_limit = []
    for b in range(10):
        for try_ in range(2 * joints.size):
            j, lim, out = joints[(b + try_ // 2) % joints.size], (hi, lo)[(b + try_) % 2], (1.0, -1.0)[(b + try_) % 2]
            q, s = q0[b].copy(), qs[b].copy()
            q[j], s[j] = lim[j], lim[j] + out * 0.15
            tg = targets_at(O, om_free, ospec, s[None])
            q1 = oracle_solve(O, x, tg, q[None], one)[0][0]
            q1_free = oracle_solve(O, x, tg, q[None], one, om=om_free)[0][0]
            q1_quad = oracle_solve(O, x, tg, q[None], one, ext="q")[0][0]
            if q1[j] == lim[j] and out * (q1_free[j] - lim[j]) > 1e-3 and np.abs(q1 - q1_quad).max() <= ORACLE_AGREES:
                q0[b], qs[b] = q, s
                on_limit.append((b, int(j)))
                break
    assert len(on_limit) == 10, (c.id, on_limit)
    tg = targets_at(O, om_free, ospec, qs)
    for a in (q0, qs, tg):
        a.setflags(write=False)
    return x._replace(q0=q0, qs=qs, tg=tg, on_limit=on_limit, pushed=pushed)


def plan_names(c, rule):
    """(kernel name, build string) of the case under `rule` by the host analysis alone (ikgpu_problem_plan_constrained,
    ikgpu_dls_tree_build_plan): no device."""
    import ik_amd
    x_model = ik_amd.Model.from_urdf_xml(robot_xml(c.robot, c.tail), free_flyer=ROBOTS[c.robot].ff)
    problem = make_problem(c, x_model)
    p = ik_amd.dls_parameters(max_iterations=rule[0], damping=rule[1], step_length=rule[2])
    return ik_amd.plan(problem), ik_amd.tree_build(problem, ik_amd.inverse_kinematics_visitor(rule[3]), p, pik_levels=2 if c.pik else 0)
