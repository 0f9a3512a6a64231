"""What the prismatic-chain tests share (tests/test_prismatic_chain_host.py and tests/test_prismatic_chain_emulation.py on the CPU,
tests/test_gpu_prismatic_chain.py on the device): the matrix of chain problems with sliding joints, their inputs, and the ctypes
wrappers of tests/lane_emu/prismatic_emu.cpp.  No tests here.

Models are made by string edit; nothing is written to disk.  Prismatic limits are -0.20 .. 0.25 m unless stated:

  arm8 {j3, j6}       frames l3, l5, tool (NJ 3, 5, 8) x Position / Orientation / Full, (unit, universe) and (WEIGHTS, bench), general
                      build; l7 Full unit on the default build (hot-rtc) and the general one.  A prismatic joint last in the chain, inside
                      it, twice in it; NJ = 8; oblique axes and all-general placements.
  arm8 {j1}           l1 (NJ 1) Position and Full: a chain that is one sliding joint; l7 Full default: prismatic joint 0 of the hot walk.
  arm8 {j7}           l7 Full default: the prismatic joint at the tip of the hot walk.
  arm8 {j1, j2, j3}   l3 Orientation: the Jacobian is identically zero.  Every second target is turned by 0.3 rad about a fixed axis: those
                      lanes run all 100 iterations with dq = 0 and fail with q = clip(q0); the others stop at iteration 0 with q0 untouched.
  ur5 rail            world_joint made prismatic along x, -0.8 .. 1.2 (NJ = 7): tool0 Full default and general, Position general.
                      Structural placements (exact 0 / +-1) next to a prismatic joint, an identity placement on the rail.
  ur5 elbow           elbow_joint prismatic, +-0.2: tool0 Full default and general with reference `base` (world-fixed, so the problem is
                      a chain).  A prismatic joint inside UR5's run of parallel axes; the placement code is the pre-built UR5 program's.

Inputs follow tests/chain_shapes_common.py inputs(): B = 197, seed 1, q0 uniform in the limits, target = the frame at
clip(q0 + U(-0.15, 0.15) s, lo, hi) with s = 1/3 on prismatic entries; two entries outside the chain pushed beyond their limits in
every third problem; ten problems start with a chain joint ON a limit and the first step pointing outwards, decided by the oracle alone,
at least three of them on a prismatic joint wherever the chain has one and the task has position rows (an Orientation task never
steps a prismatic joint)."""
import collections
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import chain_shapes_common as CS
from conftest import ROOT, urdf_path

B, SEED = CS.B, CS.SEED
STEP_BAR, TOL = 1e-9, 1e-6      # tests/test_gpu_full_size.py: per synchronised step, and for the default rule
PRIS_LIMITS = (-0.20, 0.25)
PRIS_SCALE = 1.0 / 3
TRACK_T, LINE_T, PATH_PT, PATH_STEP = 3, 8, (3, 6), 0.25
MS_K, MS_B, GS_G, SEP = CS.MS_K, CS.MS_B, 2, 0.5

# robot: the model's key in MODELS; the other fields as chain_shapes_common.Case
Case = collections.namedtuple("Case", "robot frame nj ktype weighted reference build")


def case_id(c):
    return "%s-%s-nj%d-%s-%s-%s-%s" % (c.robot, c.frame, c.nj, CS.TYPE_NAMES[c.ktype], "weighted" if c.weighted else "unit", c.reference, c.build)


def _prismatic(xml, joint, limits=PRIS_LIMITS, axis=None):
    """The URDF text with `joint` (revolute, or fixed when `axis` is given) turned into a prismatic joint with the given limits."""
    m = re.search(r'<joint name="%s" type="(revolute|fixed)">(.*?)</joint>' % re.escape(joint), xml, re.S)
    assert m, joint
    body = m.group(2)
    limit = '<limit lower="%r" upper="%r"/>' % limits
    if m.group(1) == "revolute":
        body, n = re.subn(r'<limit lower="[-0-9.e]+" upper="[-0-9.e]+"/>', limit, body)
        assert n == 1 and axis is None
    else:
        body = body.rstrip() + '\n    <axis xyz="%s"/>\n    %s\n  ' % (axis, limit)
    return xml[:m.start()] + '<joint name="%s" type="prismatic">%s</joint>' % (joint, body) + xml[m.end():]


@functools.lru_cache(maxsize=None)
def robot_xml(robot):
    if robot.startswith("arm8"):
        xml = CS.arm8_xml()
        for j in robot.split("_")[1:]:
            xml = _prismatic(xml, j)
        return xml
    ur5 = open(urdf_path("ur5")).read()
    if robot == "ur5_rail":
        return _prismatic(ur5, "world_joint", (-0.8, 1.2), axis="1 0 0")
    if robot == "ur5_elbow":
        return _prismatic(ur5, "elbow_joint", (-0.2, 0.2))
    return CS.robot_xml(robot)


def _cases():
    out = []
    for nj, frame in ((3, "l3"), (5, "l5"), (8, "tool")):
        for ktype in (0, 1, 2):
            out.append(Case("arm8_j3_j6", frame, nj, ktype, False, "universe", "general"))
            out.append(Case("arm8_j3_j6", frame, nj, ktype, True, "bench", "general"))
    out.append(Case("arm8_j3_j6", "l7", 7, 2, False, "universe", "default"))
    out.append(Case("arm8_j1", "l1", 1, 0, False, "universe", "general"))
    out.append(Case("arm8_j1", "l1", 1, 2, False, "universe", "general"))
    out.append(Case("arm8_j1", "l7", 7, 2, False, "universe", "default"))
    out.append(Case("arm8_j7", "l7", 7, 2, False, "universe", "default"))
    out.append(Case("arm8_j1_j2_j3", "l3", 3, 1, False, "universe", "general"))
    out.append(Case("ur5_rail", "tool0", 7, 2, False, "universe", "default"))
    out.append(Case("ur5_rail", "tool0", 7, 0, False, "universe", "general"))
    out.append(Case("ur5_elbow", "tool0", 6, 2, False, "base", "default"))
    return out


CASES = _cases()
ZERO_JACOBIAN = Case("arm8_j1_j2_j3", "l3", 3, 1, False, "universe", "general")
HOT_CASES = [c for c in CASES if c.build == "default"]
# the jobs run on both builds of these two (the issue's choice), and on the general build of one short weighted chain
JOB_CASES = [Case("arm8_j3_j6", "l7", 7, 2, False, "universe", "default"), Case("ur5_rail", "tool0", 7, 2, False, "universe", "default")]


def kernel_name(c, build):
    return "dls_chain<NJ=%d,%s,%s>" % (c.nj, CS.TYPE_NAMES[c.ktype], build)


def builds(c, hiprtc=True):
    """The names of the builds a case runs on: a default-build case on hot-rtc (where hipRTC is installed) and on the general build."""
    return (["hot-rtc"] if c.build == "default" and hiprtc else []) + ["general"]


def make_problem(c, model):
    return CS.make_problem(c, model)


Inputs = collections.namedtuple("Inputs", "xml model om om_free fid rid tasks support prismatic q0 qs tg on_limit pushed lo hi")


def _turn(tg, angle, axis):
    """The targets [n, 1, 12] with their rotation turned by `angle` about `axis` (in the target's own frame)."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    out = tg.copy()
    out[:, 0, :9] = (tg[:, 0, :9].reshape(-1, 3, 3) @ R).reshape(-1, 9)
    return out


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The inputs of a case (the module's docstring).  Cached: copy an array before writing to it.  prismatic [nq] bool: the entries of
    q that belong to a prismatic joint; the other fields as chain_shapes_common.inputs."""
    import ik_amd
    import oracle as O
    xml = robot_xml(c.robot)
    model = ik_amd.Model.from_urdf_xml(xml)
    om = O.OracleModel(model.flat())
    fid, rid = model.getFrameId(c.frame), model.getFrameId(c.reference)
    assert fid < model.nframes and rid < model.nframes
    tasks = O.make_tasks([(fid, rid, c.ktype, 0, CS.weights(c))])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    flat = model.flat()
    support, prismatic = np.zeros(model.nq, bool), np.zeros(model.nq, bool)
    for j in range(1, len(flat["jtype"])):
        if int(flat["jtype"][j]) == 2:      # IKGPU_JOINT_PRISMATIC
            prismatic[int(flat["idx_q"][j])] = True
    j = int(flat["frame_parent"][fid])
    while j > 0:
        support[int(flat["idx_q"][j])] = True
        j = int(flat["parent"][j])
    assert support.sum() == c.nj, (case_id(c), support)
    scale = np.where(prismatic, PRIS_SCALE, 1.0)
    rng = np.random.default_rng(SEED)
    q0 = rng.uniform(lo, hi, (B, lo.size))
    qs = np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape) * scale, lo, hi)
    pushed = None
    outside = np.flatnonzero(~support)
    if outside.size:
        two = outside[[0, -1]] if outside.size > 1 else outside
        who = np.arange(0, B, 3)
        q0[np.ix_(who, two)] = np.where(np.arange(who.size)[:, None] % 2 == 0, hi[two] + 0.25, lo[two] - 0.4)
        pushed = (who, two)
    free = ik_amd.Model.from_urdf_xml(re.sub(r'lower="[-0-9.e]+" upper="[-0-9.e]+"', 'lower="-100.0" upper="100.0"', xml))
    om_free = O.OracleModel(free.flat())
    on_limit = []
    if c != ZERO_JACOBIAN:      # (no step exists there)
        one = O.params(1, 1e-2, 1.0, -1.0)
        chain = np.flatnonzero(support)
        sliding = np.flatnonzero(support & prismatic)
        for b in range(10):
            # the first three problems try the chain's prismatic joints first
            order = (list(sliding) if b < 3 else []) + [chain[(b + k) % chain.size] for k in range(chain.size)]
            found = False
            for t, j in enumerate(order):
                for side in ((b + t) % 2, (b + t + 1) % 2):
                    lim, out = (hi, lo)[side], (1.0, -1.0)[side]
                    q, s = q0[b].copy(), qs[b].copy()
                    q[j], s[j] = lim[j], lim[j] + out * 0.15 * scale[j]
                    tg = CS.relative_targets(O, om_free, s[None], fid, rid)
                    q1, _, _ = O.dls(om, tasks, tg[0], q, one)
                    q1_free, _, _ = O.dls(om_free, tasks, tg[0], q, one)
                    if q1[j] == lim[j] and out * (q1_free[j] - lim[j]) > 1e-3 * scale[j]:
                        q0[b], qs[b] = q, s
                        on_limit.append((b, int(j)))
                        found = True
                        break
                if found:
                    break
        if c.nj == 1 and c.ktype == 0 and not sliding.size:
            assert not on_limit
        elif c.nj == 1:
            assert len(on_limit) >= 1, (case_id(c), on_limit)
        else:
            assert len(on_limit) == 10, (case_id(c), on_limit)
        # (an Orientation task has no row a prismatic joint moves: its column is zero and no step of it exists)
        if sliding.size and c.ktype != 1:
            assert sum(1 for _, j in on_limit if prismatic[j]) >= min(3, len(on_limit)), (case_id(c), on_limit)
        if c.ktype == 1:
            assert not any(prismatic[j] for _, j in on_limit)
    tg = CS.relative_targets(O, om_free, qs, fid, rid)
    if c == ZERO_JACOBIAN:
        tg[1::2] = _turn(tg[1::2], 0.3, (0.36, 0.48, 0.8))
    for a in (q0, qs, tg):
        a.setflags(write=False)
    return Inputs(xml, model, om, om_free, fid, rid, tasks, support, prismatic, q0, qs, tg, on_limit, pushed, lo, hi)


@functools.lru_cache(maxsize=None)
def waypoints(c):
    """[TRACK_T, B, 1, 12]: the frame a third and two thirds of the way from q0 to qs, then the target itself (chain_shapes_common)."""
    import oracle as O
    x = inputs(c)
    way = np.stack([CS.relative_targets(O, x.om_free, x.q0 + f * (x.qs - x.q0), x.fid, x.rid) for f in (1.0 / 3, 2.0 / 3)] + [x.tg])
    way.setflags(write=False)
    return way


@functools.lru_cache(maxsize=None)
def far_goals(c, P=1, seed_offset=2):
    """[P, B, 1, 12]: goals / vias for the line and path jobs, in the reference frame.  Segment s ends at the frame at q_s = q_{s-1} + d
    with d = U(-0.3, 0.3) on the chain's entries (x 1/3 on prismatic ones), and U(-1.2, 1.2) for every third problem (offset by s): lines
    that leave the workspace or the limits and fail on the way, and waypoints reached only through a jump.  d is halved until the
    segment turns by at most line_common.MAX_ROTATION."""
    import line_common
    import oracle as O
    x = inputs(c)
    rng = np.random.default_rng(SEED + seed_offset)
    scale = np.where(x.prismatic, PRIS_SCALE, 1.0) * x.support
    q, prev, out = np.array(x.q0), CS.relative_targets(O, x.om_free, x.q0, x.fid, x.rid), []
    for s in range(P):
        d = rng.uniform(-0.3, 0.3, q.shape)
        far = rng.uniform(-1.2, 1.2, q.shape)
        d[(s + 1) % 3::3] = far[(s + 1) % 3::3]
        d *= scale
        f, todo, via = np.ones(B), np.arange(B), prev.copy()
        for _ in range(40):
            via[todo] = CS.relative_targets(O, x.om_free, q[todo] + f[todo, None] * d[todo], x.fid, x.rid)
            angle = line_common.rotation_angle(prev[todo, 0, :9].reshape(-1, 3, 3), via[todo, 0, :9].reshape(-1, 3, 3))
            todo = todo[angle > line_common.MAX_ROTATION]
            if todo.size == 0:
                break
            f[todo] *= 0.5
        assert todo.size == 0, (case_id(c), s, todo)
        q = q + f[:, None] * d
        out.append(via)
        prev = via
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def multistart_inputs(c):
    """(starts [MS_K, MS_B, nq], first [MS_B]) as chain_shapes_common.multistart_inputs: the case's own start in slot b % MS_K, uniform
    draws elsewhere; first: the lowest start from which the oracle converges (-1: none)."""
    import oracle as O
    x = inputs(c)
    rng = np.random.default_rng(SEED + 1)
    starts = rng.uniform(x.lo, x.hi, (MS_K, MS_B, x.model.nq))
    rows_ = np.arange(MS_B)
    starts[rows_ % MS_K, rows_] = x.q0[:MS_B]
    ok = np.stack([O.dls_batch(x.om, x.tasks, x.tg[:MS_B], starts[k], O.params(100, 1e-2, 1.0, 1e-4))[1] for k in range(MS_K)]).astype(bool)
    first = np.where(ok.any(axis=0), ok.argmax(axis=0), -1)
    starts.setflags(write=False)
    return starts, first


@functools.lru_cache(maxsize=None)
def goalset_goals(c):
    """[GS_G, MS_B, 1, 12]: goal 0 a far pose (the frame at a uniform configuration), goal 1 the case's own target, swapped for every
    second problem -- so both goals win somewhere."""
    import oracle as O
    x = inputs(c)
    rng = np.random.default_rng(SEED + 3)
    far = CS.relative_targets(O, x.om_free, rng.uniform(x.lo, x.hi, (MS_B, x.model.nq)), x.fid, x.rid)
    own = np.array(x.tg[:MS_B])
    goals = np.stack([far, own])
    goals[:, 1::2] = goals[::-1, 1::2]
    goals.setflags(write=False)
    return goals


# ---- tests/lane_emu/prismatic_emu.cpp through ctypes -----------------------------------------------------------------------------------
PROGRAM = {"runtime": 0, "general": 1, "hot": 2}
_p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None


def compile_emulator():
    src = os.path.join(ROOT, "tests", "lane_emu", "prismatic_emu.cpp")
    out = os.path.join(ROOT, "tests", "lane_emu", "libprismatic_emu.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp",
                                                    "device/multistart.hpp", "device/solutions.hpp", "device/goalset.hpp", "device/line.hpp",
                                                    "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.prismatic_emu_last_error.restype = C.c_char_p
    return L


def task_of(c, x):
    from ik_amd import capi
    w = CS.weights(c)
    w = list(w) + [1.0] * (6 - len(w)) if w is not None else [1.0] * 6
    return capi.Task(x.fid, x.rid, c.ktype, 0, (C.c_double * 6)(*w))


class Emu:
    """One case on the emulator: every call takes and returns AoS arrays ([n, nq], [n, 12]) whatever layout it runs in."""

    def __init__(self, L, c):
        self.L, self.c, self.x = L, c, inputs(c)
        self.urdf, self.task = self.x.xml.encode(), task_of(c, self.x)
        self.nq, self.nv, self.M = self.x.model.nq, self.x.model.nv, CS.rows(c)

    def _head(self):
        return self.urdf, C.c_size_t(len(self.urdf)), C.byref(self.task)

    def _check(self, rc):
        assert rc == 0, self.L.prismatic_emu_last_error()

    def structure(self):
        out, sup, draw = np.zeros(6, np.uint64), np.zeros(self.nq, np.uint8), np.zeros(self.nq, np.uint8)
        self._check(self.L.prismatic_emu_structure(*self._head(), _p(out), _p(sup), _p(draw)))
        return [int(v) for v in out], sup.astype(bool), draw.astype(bool)

    def starts(self, q0, K, seed, layout=1):
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        out = np.full((K - 1,) + qi.shape, np.nan)
        self._check(self.L.prismatic_emu_starts(*self._head(), C.c_int64(n), K, _p(qi), C.c_uint64(seed), _p(out), layout))
        return out if layout == 1 else np.ascontiguousarray(out.transpose(0, 2, 1))

    def run(self, program, mode, q0, tg, prm=None, layout=1):
        """mode 0: (q, success, iters); 1: (e [n, M], J [n, M, nv]); 2: oMf [n, 1, 12]."""
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        ti = np.ascontiguousarray(tg.reshape(n, 12) if layout == 1 else tg.reshape(n, 12).T)
        qo, ok, it = np.full(qi.shape, np.nan), np.full(n, 7, np.uint8), np.full(n, -7, np.int32)
        e, J, oMf = np.empty((n, self.M)), np.empty((n, self.M, self.nv)), np.empty((n, 1, 12))
        assert layout == 1 or mode == 0
        self._check(self.L.prismatic_emu_run(*self._head(), PROGRAM[program], mode, C.c_int64(n), _p(qi), _p(ti), C.byref(prm) if prm is not None else None,
                                             _p(qo), _p(ok), _p(it), _p(e), _p(J), _p(oMf), layout))
        if mode == 0:
            return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it
        return (e, J) if mode == 1 else oMf

    def track(self, program, q0, way, prm, layout=1):
        """way [T, n, 12] -> q [T, n, nq], success, iters [T, n]."""
        T, n = way.shape[:2]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        wi = np.ascontiguousarray(way if layout == 1 else way.transpose(0, 2, 1))
        qt = np.full((T,) + qi.shape, np.nan)
        ok, it = np.full((T, n), 7, np.uint8), np.full((T, n), -7, np.int32)
        self._check(self.L.prismatic_emu_track(*self._head(), PROGRAM[program], C.c_int64(n), T, _p(qi), _p(wi), C.byref(prm), _p(qt), _p(ok), _p(it), layout))
        return (qt if layout == 1 else np.ascontiguousarray(qt.transpose(0, 2, 1))), ok, it

    def line_waypoints(self, q0, goals, T, layout=1):
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        gi = np.ascontiguousarray(goals if layout == 1 else goals.T)
        W = np.full((T, n, 12) if layout == 1 else (T, 12, n), np.nan)
        self._check(self.L.prismatic_emu_line(*self._head(), 1, C.c_int64(n), T, _p(qi), _p(gi), None, None, None, None, None, None, _p(W), layout))
        return W if layout == 1 else np.ascontiguousarray(W.transpose(0, 2, 1))

    def line(self, program, q0, goals, T, prm, layout=1):
        """goals [n, 12] -> q [T, n, nq] (NaN where not written), success, iters [T, n] (7 / -7), reached [n], visited [n]."""
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        gi = np.ascontiguousarray(goals if layout == 1 else goals.T)
        qt = np.full((T,) + qi.shape, np.nan)
        ok, it, reached, visited = np.full((T, n), 7, np.uint8), np.full((T, n), -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
        self._check(self.L.prismatic_emu_line(*self._head(), PROGRAM[program], C.c_int64(n), T, _p(qi), _p(gi), C.byref(prm), _p(qt), _p(ok), _p(it),
                                              _p(reached), _p(visited), None, layout))
        return (qt if layout == 1 else np.ascontiguousarray(qt.transpose(0, 2, 1))), ok, it, reached, visited

    def path_waypoints(self, q0, vias, T, layout=1):
        P, n = vias.shape[:2]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        vi = np.ascontiguousarray(vias if layout == 1 else vias.transpose(0, 2, 1))
        W = np.full((P * T, n, 12) if layout == 1 else (P * T, 12, n), np.nan)
        self._check(self.L.prismatic_emu_path(*self._head(), 1, C.c_int64(n), P, T, _p(qi), _p(vi), None, C.c_double(0.0), None, None, None, None, None,
                                              _p(W), layout))
        return W if layout == 1 else np.ascontiguousarray(W.transpose(0, 2, 1))

    def path(self, program, q0, vias, T, prm, step, layout=1):
        """vias [P, n, 12] -> q [P T, n, nq], success, iters [P T, n], reached [n], visited [n] (sentinels as line())."""
        P, n = vias.shape[:2]
        N = P * T
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        vi = np.ascontiguousarray(vias if layout == 1 else vias.transpose(0, 2, 1))
        qt = np.full((N,) + qi.shape, np.nan)
        ok, it, reached, visited = np.full((N, n), 7, np.uint8), np.full((N, n), -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
        self._check(self.L.prismatic_emu_path(*self._head(), PROGRAM[program], C.c_int64(n), P, T, _p(qi), _p(vi), C.byref(prm), C.c_double(step), _p(qt),
                                              _p(ok), _p(it), _p(reached), _p(visited), None, layout))
        return (qt if layout == 1 else np.ascontiguousarray(qt.transpose(0, 2, 1))), ok, it, reached, visited

    def multistart(self, program, q0, starts, seed, tg, prm, K, layout=1):
        """(q, success, iters, winner, err_sq) of ikgpu_dls_multistart_batch; starts None or [K-1, n, nq]."""
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
        ti = np.ascontiguousarray(tg.reshape(n, 12) if layout == 1 else tg.reshape(n, 12).T)
        qo, ok, it, win, err = np.full(qi.shape, np.nan), np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, np.nan)
        self._check(self.L.prismatic_emu_multistart(*self._head(), PROGRAM[program], C.c_int64(n), K, _p(qi), _p(si), C.c_uint64(seed), _p(ti), C.byref(prm),
                                                    _p(qo), _p(ok), _p(it), _p(win), _p(err), layout))
        return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, win, err

    def goalset(self, program, q0, starts, seed, goals, prm, K, layout=1):
        """(q, success, iters, goal, start, err_sq, reachable [G, n]) of ikgpu_dls_goalset_batch; goals [G, n, 1, 12]."""
        G, n = goals.shape[:2]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
        gi = np.ascontiguousarray(goals.reshape(G, n, 12) if layout == 1 else goals.reshape(G, n, 12).transpose(0, 2, 1))
        qo = np.full(qi.shape, np.nan)
        ok, it, gl, st, err, reach = (np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32),
                                      np.full(n, np.nan), np.full((G, n), 7, np.uint8))
        self._check(self.L.prismatic_emu_goalset(*self._head(), PROGRAM[program], C.c_int64(n), G, K, _p(qi), _p(si), C.c_uint64(seed), _p(gi), C.byref(prm),
                                                 _p(qo), _p(ok), _p(it), _p(gl), _p(st), _p(err), _p(reach), layout))
        return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, gl, st, err, reach

    def solutions(self, program, q0, starts, seed, tg, prm, K, N, sep, layout=1):
        """(q_sols [N, n, nq], count, which, iters) of ikgpu_dls_solutions_batch with the prefill of tests/solutions_common.py."""
        import solutions_common as SC
        n = q0.shape[0]
        qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
        si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
        ti = np.ascontiguousarray(tg.reshape(n, 12) if layout == 1 else tg.reshape(n, 12).T)
        qo = np.full((N,) + qi.shape, SC.NAN_FILL)
        count, which, it = np.full(n, SC.INT_FILL, np.int32), np.full((N, n), SC.INT_FILL, np.int32), np.full((N, n), SC.INT_FILL, np.int32)
        self._check(self.L.prismatic_emu_solutions(*self._head(), PROGRAM[program], C.c_int64(n), K, N, _p(qi), _p(si), C.c_uint64(seed), _p(ti), C.byref(prm),
                                                   C.c_double(sep), _p(qo), _p(count), _p(which), _p(it), layout))
        return (qo if layout == 1 else np.ascontiguousarray(qo.transpose(0, 2, 1))), count, which, it
