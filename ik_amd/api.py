"""Host-side mirror of the reference's API for the DLS path, over the C ABI (include/ikgpu.h).

Names, argument meaning and outcome reporting follow dazzmo/ik so that the parity tests read
like the reference's own (commented-out) tests (ik/test/dls.cpp:10-76):

    reference (C++)                                   here (Python over libikgpu.so)
    ------------------------------------------------  -----------------------------------------
    pinocchio::urdf::buildModelFromXML  cassie.cpp:34  Model.from_urdf_xml(xml, free_flyer)
    ik::InverseKinematicsProblem        problem.hpp:9  InverseKinematicsProblem(model, max_priority_level)
    ik::FrameTask::create               frame.hpp:123  FrameTask.create(model, frame, type, reference_frame)
    ik::KinematicType                   frame.hpp:20   KinematicType
    ik::dls_parameters                  dls.hpp:24     dls_parameters
    ik::AlignAxisTask::create           frame.hpp:245  AlignAxisTask.create(model, frame, axis, reference_frame)
    ik::inverse_kinematics_visitor      visitor.hpp:7  inverse_kinematics_visitor (one-parameter family)
    ik::dls_data                        dls.hpp:34     dls_data(problem)  (owns the device handle)
    ik::dls(problem, q0, data, v, p)    dls.hpp:111    dls(problem, q0, data, visitor, p)
    --                                                 dls_batch(problem, Q0, targets, data, visitor, p)

The C++ mirror of the same classes lives in ik_amd/csrc/host/ik/.  No arithmetic happens here.
"""
import collections
import ctypes as C
import enum
import math

import numpy as np

from . import capi


class KinematicType(enum.IntEnum):  # reference ik/ik/frame.hpp:20
    Position = 0
    Orientation = 1
    Full = 2


class AlignAxisType(enum.IntEnum):  # reference ik/ik/frame.hpp:202
    AxisX = 0
    AxisY = 1
    AxisZ = 2


class SE3:
    """pinocchio::SE3 as the path uses it: a rotation matrix and a translation."""

    def __init__(self, rotation=None, translation=None):
        self.rotation = np.eye(3) if rotation is None else np.array(rotation, dtype=np.float64).reshape(3, 3)
        self.translation = np.zeros(3) if translation is None else np.array(translation, dtype=np.float64).reshape(3)

    @staticmethod
    def Identity():
        return SE3()

    @staticmethod
    def from12(v):
        v = np.asarray(v, dtype=np.float64).reshape(12)
        return SE3(v[:9].reshape(3, 3), v[9:])

    def to12(self):
        return np.concatenate([self.rotation.reshape(9), self.translation])


class Model:
    """What the path reads of pinocchio::Model (reference ik/ik/common.hpp:16)."""

    def __init__(self, handle):
        self._h = handle
        L = capi.lib()
        f = capi.FlatModel()
        capi.check(L.ikgpu_model_get_flat(self._h, C.byref(f)))
        self.njoints, self.nq, self.nv, self.nframes = f.njoints, f.nq, f.nv, f.nframes
        self.names = [f.joint_names[i].decode() for i in range(f.njoints)]
        self.frame_names = [f.frame_names[i].decode() for i in range(f.nframes)]
        self.lowerPositionLimit = np.array(f.lower[:f.nq], dtype=np.float64)
        self.upperPositionLimit = np.array(f.upper[:f.nq], dtype=np.float64)
        self._flat = f

    @staticmethod
    def from_urdf_xml(xml, free_flyer=False):
        """pinocchio::urdf::buildModelFromXML(xml, [JointModelFreeFlyer(),] model)."""
        if isinstance(xml, str):
            xml = xml.encode("utf-8")
        h = C.c_void_p()
        capi.check(capi.lib().ikgpu_model_from_urdf(xml, len(xml), capi.ROOT_FREEFLYER if free_flyer else capi.ROOT_FIXED,
                                                    C.byref(h)))
        return Model(h)

    @staticmethod
    def from_urdf_file(path, free_flyer=False):
        with open(path, "rb") as fh:
            return Model.from_urdf_xml(fh.read(), free_flyer)

    def getFrameId(self, name):
        return int(capi.lib().ikgpu_model_frame_id(self._h, name.encode()))

    def getJointId(self, name):
        return int(capi.lib().ikgpu_model_joint_id(self._h, name.encode()))

    def existFrame(self, name):
        return self.getFrameId(name) < self.nframes

    def flat(self):
        """numpy copies of the flat arrays (same keys as the oracle's model dict)."""
        f, nj, nf = self._flat, self.njoints, self.nframes
        return dict(
            nq=self.nq, nv=self.nv,
            jtype=np.array(f.joint_type[:nj], np.int32), parent=np.array(f.joint_parent[:nj], np.int32),
            idx_q=np.array(f.joint_idx_q[:nj], np.int32), idx_v=np.array(f.joint_idx_v[:nj], np.int32),
            placement=np.array(f.joint_placement[:12 * nj]).reshape(nj, 12),
            axis=np.array(f.joint_axis[:3 * nj]).reshape(nj, 3),
            mass=np.array(f.joint_mass[:nj]), lever=np.array(f.joint_com[:3 * nj]).reshape(nj, 3),
            lower=self.lowerPositionLimit.copy(), upper=self.upperPositionLimit.copy(),
            frame_parent=np.array(f.frame_parent[:nf], np.int32),
            frame_placement=np.array(f.frame_placement[:12 * nf]).reshape(nf, 12),
            frame_names=list(self.frame_names), joint_names=list(self.names))

    def __del__(self):
        try:
            if self._h:
                capi.lib().ikgpu_model_destroy(self._h)
                self._h = None
        except Exception:
            pass


class FrameTask:
    """ik::FrameTask (reference ik/ik/frame.hpp:78-200)."""

    def __init__(self, model, frame, type=KinematicType.Full, reference_frame="universe"):
        self.frame, self.reference_frame, self.type = frame, reference_frame, KinematicType(type)
        self._frame_id, self._ref_id = model.getFrameId(frame), model.getFrameId(reference_frame)
        if self._frame_id >= model.nframes:
            raise ValueError("frame %r not found in model" % frame)
        if self._ref_id >= model.nframes:
            raise ValueError("reference frame %r not found in model" % reference_frame)
        self._dimension = 6 if self.type == KinematicType.Full else 3  # frame.hpp:102-108
        self._weighting = np.ones(self._dimension)                      # task.hpp:48-51
        self.target = SE3.Identity()                                    # frame.hpp:189

    @staticmethod
    def create(model, frame, type=KinematicType.Full, reference_frame="universe"):
        return FrameTask(model, frame, type, reference_frame)

    def dimension(self):
        return self._dimension

    def weighting(self):
        return self._weighting


class AlignAxisTask:
    """ik::AlignAxisTask (reference ik/ik/frame.hpp:210-319): one row, e = 1 - axis . target/|target| with the
    frame's chosen axis expressed in the reference frame.  Runs on the generic kernel."""

    def __init__(self, model, frame, axis, reference_frame="universe"):
        self.frame, self.reference_frame, self.axis = frame, reference_frame, AlignAxisType(axis)
        self._frame_id, self._ref_id = model.getFrameId(frame), model.getFrameId(reference_frame)
        if self._frame_id >= model.nframes:
            raise ValueError("frame %r not found in model" % frame)
        if self._ref_id >= model.nframes:
            raise ValueError("reference frame %r not found in model" % reference_frame)
        self._weighting = np.ones(1)
        self.target = np.array([1.0, 0.0, 0.0])  # frame.hpp:307 (uninitialised in the reference)

    @staticmethod
    def create(model, frame, axis, reference_frame="universe"):
        return AlignAxisTask(model, frame, axis, reference_frame)

    def dimension(self):
        return 1

    def weighting(self):
        return self._weighting


class PostureTask:
    """ik::PostureTask (reference ik/ik/posture.hpp:17-85): e = (q.tail(nj) - target) * mask, J.rightCols(nj) = I
    (the reference does not apply the mask to J).  Crosses the ABI as nj one-row tasks (IKGPU_POSTURE_ROW) and
    runs on the generic kernel."""

    def __init__(self, model, nj):
        if not 0 < nj <= min(model.nq, model.nv):
            raise ValueError("PostureTask over %d joints on a model with nv = %d" % (nj, model.nv))
        self.nj = int(nj)
        self._q0, self._v0 = model.nq - self.nj, model.nv - self.nj
        self.target = np.zeros(self.nj)   # posture.hpp:75
        self.mask = np.ones(self.nj)      # posture.hpp:82
        self._weighting = np.ones(self.nj)

    @staticmethod
    def create(model, nj):
        return PostureTask(model, nj)

    def dimension(self):
        return self.nj

    def weighting(self):
        return self._weighting


class FrameConstraint:
    """ik::FrameConstraint (reference ik/ik/frame.hpp:325-449): the frame may not move relative to its reference frame in
    the selected coordinates.  ik::dls keeps its step in the null space of the constraint Jacobian (reference
    ik/ik/dls.cpp:26-34,43-53); `target` is carried for source compatibility -- the loop never reads it."""

    def __init__(self, model, frame, type=KinematicType.Full, reference_frame="universe"):
        self.frame, self.reference_frame, self.type = frame, reference_frame, KinematicType(type)
        self._frame_id, self._ref_id = model.getFrameId(frame), model.getFrameId(reference_frame)
        if self._frame_id >= model.nframes:
            raise ValueError("Frame not found in model: %s" % frame)
        if self._ref_id >= model.nframes:
            raise ValueError("Reference frame not found in model: %s" % reference_frame)
        self.target = SE3.Identity()

    @staticmethod
    def create(model, frame, type=KinematicType.Full, reference_frame="universe"):
        return FrameConstraint(model, frame, type, reference_frame)

    def dimension(self):
        return 6 if self.type == KinematicType.Full else 3


def _constraint_table(problem):
    cons = problem.get_all_constraints()
    arr = (capi.Task * max(1, len(cons)))()
    for i, c in enumerate(cons):
        arr[i].frame, arr[i].reference, arr[i].type, arr[i].priority = c._frame_id, c._ref_id, int(c.type), 0
        for k in range(6):
            arr[i].weight[k] = 1.0
    return arr, len(cons)


class CentreOfMassTask:
    """ik::CentreOfMassTask (reference ik/ik/centre_of_mass.hpp:14-62): e = oMr^-1 com(q) - target (three rows),
    J = R(oMr)^T Jcom.  Needs link masses in the model (URDF <inertial>).  Runs on the generic kernel."""

    def __init__(self, model, reference_frame="universe"):
        self.reference_frame = reference_frame
        self._ref_id = model.getFrameId(reference_frame)
        if self._ref_id >= model.nframes:
            raise ValueError("Reference frame not found in model: %s" % reference_frame)
        self.target = np.zeros(3)   # the reference leaves it uninitialised; a caller sets it (cassie.cpp:101)
        self._weighting = np.ones(3)

    @staticmethod
    def create(model, reference_frame="universe"):
        return CentreOfMassTask(model, reference_frame)

    def dimension(self):
        return 3

    def weighting(self):
        return self._weighting


def _abi_rows(task, prio):
    """The rows a task contributes to the ABI's task table: (frame, reference, type, priority, weight[6])."""
    if isinstance(task, CentreOfMassTask):
        return [(0, task._ref_id, capi.CENTRE_OF_MASS, prio, [float(x) for x in task._weighting] + [1.0] * 3)]
    if isinstance(task, PostureTask):
        return [(task._v0 + k, task._q0 + k, capi.POSTURE_ROW, prio, [float(task._weighting[k]), float(task.mask[k]), 1, 1, 1, 1])
                for k in range(task.nj)]
    w = list(np.asarray(task.weighting(), dtype=np.float64)) + [1.0] * 6
    typ = 3 + int(task.axis) if isinstance(task, AlignAxisTask) else int(task.type)
    return [(task._frame_id, task._ref_id, typ, prio, w[:6])]


def _target_slots(task):
    """The 12-double target slots of a task, one per ABI row."""
    if isinstance(task, PostureTask):
        out = np.zeros((task.nj, 12))
        out[:, 9] = np.asarray(task.target, dtype=np.float64)
        return out
    if isinstance(task, (AlignAxisTask, CentreOfMassTask)):
        return np.concatenate([np.eye(3).reshape(9), np.asarray(task.target, dtype=np.float64).reshape(3)])[None, :]
    return task.target.to12()[None, :]


def _task_table(problem):
    rows = [r for t, prio in problem.ordered_tasks() for r in _abi_rows(t, prio)]
    arr = (capi.Task * len(rows))()
    for i, (f, r, typ, prio, w) in enumerate(rows):
        arr[i].frame, arr[i].reference, arr[i].type, arr[i].priority = f, r, typ, prio
        for k in range(6):
            arr[i].weight[k] = w[k]
    return arr


class InverseKinematicsProblem:
    """ik::InverseKinematicsProblem (reference ik/ik/problem.hpp:9-206), frame tasks only --
    the other task kinds are outside the accelerated path."""

    def __init__(self, model, max_priority_level=0):
        self._model = model
        self._max_priority_level = int(max_priority_level)
        self._tasks = [[] for _ in range(self._max_priority_level + 1)]
        self._frame_tasks = []
        self._frame_tasks_map = {}
        self._axis_tasks = []
        self._axis_tasks_map = {}
        self._posture_tasks = []
        self._posture_tasks_map = {}
        self._frame_constraints = []
        self._frame_constraints_map = {}
        self._com_task = None
        self._generation = 0

    def max_priority_level(self):
        return self._max_priority_level

    def model(self):
        return self._model

    def add_frame_task(self, name, task, priority=0):
        if not 0 <= priority <= self._max_priority_level:
            raise ValueError("Maximum priority level exceeded!")
        self._frame_tasks_map.setdefault(name, len(self._frame_tasks))
        self._frame_tasks.append(task)
        self._tasks[priority].append(task)
        self._generation += 1
        return task

    def get_frame_task(self, name):
        return self._frame_tasks[self._frame_tasks_map[name]]

    def add_align_axis_task(self, name, task, priority=0):  # reference ik/ik/problem.hpp:94-105
        if not 0 <= priority <= self._max_priority_level:
            raise ValueError("Maximum priority level exceeded!")
        self._axis_tasks_map.setdefault(name, len(self._axis_tasks))
        self._axis_tasks.append(task)
        self._tasks[priority].append(task)
        self._generation += 1
        return task

    def get_align_axis_task(self, name):
        return self._axis_tasks[self._axis_tasks_map[name]]

    def get_all_tasks(self, priority):
        return self._tasks[priority]

    def add_frame_constraint(self, name, constraint):  # reference ik/ik/problem.hpp:68-77
        self._frame_constraints_map.setdefault(name, len(self._frame_constraints))
        self._frame_constraints.append(constraint)
        self._generation += 1
        return constraint

    def get_frame_constraint(self, name):
        return self._frame_constraints[self._frame_constraints_map[name]]

    def get_all_constraints(self):  # reference ik/ik/problem.hpp:167-173
        return list(self._frame_constraints)

    def e_size(self, priority):
        return sum(t.dimension() for t in self._tasks[priority])

    def c_size(self):  # reference ik/ik/problem.hpp:47-53
        return sum(c.dimension() for c in self._frame_constraints)

    def ordered_tasks(self):
        """(task, priority) in the row order of the stacked system (reference ik/ik/dls.cpp:20-24)."""
        return [(t, p) for p in range(self._max_priority_level + 1) for t in self._tasks[p]]

    def target_slots(self):
        """Number of 12-double target slots a batch call takes per problem: one per frame / axis task, one per
        joint of a posture task (value in double 9 of its slot)."""
        return sum(t.nj if isinstance(t, PostureTask) else 1 for t, _ in self.ordered_tasks())

    def add_posture_task(self, name, task, priority=0):  # reference ik/ik/problem.hpp:134-145
        if not 0 <= priority <= self._max_priority_level:
            raise ValueError("Maximum priority level exceeded!")
        self._posture_tasks_map.setdefault(name, len(self._posture_tasks))
        self._posture_tasks.append(task)
        self._tasks[priority].append(task)
        self._generation += 1
        return task

    def get_posture_task(self, name):
        return self._posture_tasks[self._posture_tasks_map[name]]

    def add_centre_of_mass_task(self, task, priority=0):  # reference ik/ik/problem.hpp:121-128
        if not 0 <= priority <= self._max_priority_level:
            raise ValueError("Maximum priority level exceeded!")
        if self._com_task is not None:
            raise ValueError("a problem holds one centre-of-mass task")
        self._com_task = task
        self._tasks[priority].append(task)
        self._generation += 1
        return task

    def get_centre_of_mass_task(self):  # reference ik/ik/problem.hpp:130-132
        return self._com_task


Problem = InverseKinematicsProblem   # the name BASELINE.json's north_star uses for reference ik/ik/problem.hpp:9's class


class dls_parameters:
    """ik::dls_parameters (reference ik/ik/dls.hpp:24-28, ik/ik/common.hpp:59-66)."""

    def __init__(self, max_iterations=100, step_length=1.0, damping=1e-2, max_time=1.0, random_restart=False):
        self.max_iterations = max_iterations
        self.max_time = max_time              # unused by the reference loop
        self.step_length = step_length
        self.damping = damping
        self.random_restart = random_restart  # unused by the reference loop


class inverse_kinematics_visitor:
    """ik::inverse_kinematics_visitor (reference ik/ik/visitor.hpp:7-22).  A C++ visitor cannot run
    inside the kernel; the one-parameter family `||e[0]||^2 < tolerance` is what crosses the ABI.
    tolerance < 0 is a visitor whose should_stop() always returns false."""

    def __init__(self, tolerance=1e-4, step_tolerance=0.0, level_tolerances=()):
        self.tolerance = tolerance
        # the rest of what should_stop(ik, e, dq) is handed (reference ik/ik/visitor.hpp:15-21): also stop when ||dq||^2 <
        # step_tolerance (<= 0: off); test ||e[l]||^2 < level_tolerances[l] on every level instead of level 0 alone (empty: off)
        self.step_tolerance = step_tolerance
        self.level_tolerances = tuple(level_tolerances)


class never_stop_visitor(inverse_kinematics_visitor):
    def __init__(self):
        super().__init__(-1.0)


class dls_data:
    """ik::dls_data (reference ik/ik/dls.hpp:34-65): the reusable workspace.  Here it owns the
    device-side problem handle (constant tables in HBM) and reports the outcome of the last call."""

    def __init__(self, problem, device=0):
        self.success = False
        self.iterations = 0
        self.q = None
        self._device = int(device)
        self._h = None
        self._generation = -1
        self._bind(problem)

    def _bind(self, problem):
        # everything ikgpu_problem_create_constrained reads: the model, every ABI row (frame, reference, type, priority,
        # weight[6]) and every constraint row -- the comparison the C++ mirror makes (ik_gpu.hpp dls_data::same)
        key = (id(problem.model()), int(problem.model()._h.value or 0),
               tuple((f, r, typ, prio, tuple(w)) for t, p in problem.ordered_tasks() for f, r, typ, prio, w in _abi_rows(t, p)),
               tuple((c._frame_id, c._ref_id, int(c.type)) for c in problem.get_all_constraints()))
        if self._h is not None and key == self._generation:
            return
        self._release()
        arr = _task_table(problem)
        cons, ncons = _constraint_table(problem)
        h = C.c_void_p()
        capi.check(capi.lib().ikgpu_problem_create_constrained(problem.model()._h, arr, len(arr), cons, ncons, self._device, C.byref(h)))
        self._h = h
        self._generation = key
        self.rows = int(capi.lib().ikgpu_problem_rows(h))
        self.kernel = capi.lib().ikgpu_problem_kernel(h).decode()
        sup = (C.c_uint8 * problem.model().nq)()
        capi.check(capi.lib().ikgpu_problem_support(h, sup))
        self.support = np.frombuffer(sup, dtype=np.uint8).astype(bool)   # [nq]: entries of q a solve can move (the rest is only clipped)

    def _release(self):
        if self._h is not None:
            capi.lib().ikgpu_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def _params(visitor, p):
    lt = tuple(getattr(visitor, "level_tolerances", ()))
    if len(lt) > capi.MAX_VISITOR_LEVELS:
        raise ValueError("at most %d level tolerances" % capi.MAX_VISITOR_LEVELS)
    return capi.DlsParams(int(p.max_iterations), float(p.damping), float(p.step_length), float(visitor.tolerance),
                          float(getattr(visitor, "step_tolerance", 0.0)), len(lt),
                          (C.c_double * capi.MAX_VISITOR_LEVELS)(*(list(lt) + [0.0] * (capi.MAX_VISITOR_LEVELS - len(lt)))))


def _describe(fn, problem, *extra):
    """The string a host-only C entry writes about (model, task table, constraint table, *extra)."""
    arr = _task_table(problem)
    cons, ncons = _constraint_table(problem)
    buf = C.create_string_buffer(160)
    capi.check(fn(problem.model()._h, arr, len(arr), cons, ncons, *extra, buf, len(buf)))
    return buf.value.decode()


def plan(problem):
    """Name of the kernel specialisation the problem maps to (host-only; raises IkgpuError when the
    shape has no device kernel)."""
    return _describe(capi.lib().ikgpu_problem_plan_constrained, problem)


def tree_build(problem, visitor=None, p=None, pik_levels=0):
    """Which compile-time build of the tree kernel a solve of the problem launches (host-only, include/ikgpu.h
    ikgpu_dls_tree_build_plan): "<build>,<folded|unfolded>,<extras>,refill=<twin>", or "" when the solve does not run on the tree
    kernel.  pik_levels: 0 for dls / dls_batch, 1 or 2 for pik with that many levels."""
    prm = _params(visitor or inverse_kinematics_visitor(), p or dls_parameters())
    return _describe(capi.lib().ikgpu_dls_tree_build_plan, problem, C.byref(prm), pik_levels)


def precompile(problem):
    """Compile ahead of time (host-only, no device) what dls_data(problem) would compile at run time -- the structure-specialised
    chain kernel of a chain without a pre-built instantiation -- into the on-disk cache; returns the kernel name.  Raises
    IkgpuError (UNSUPPORTED) with the compiler's log when the compilation fails (the problem then runs on the general build)."""
    return _describe(capi.lib().ikgpu_problem_precompile, problem)


# ---- the device-tensor entry points.  Each reads top to bottom: _prologue, the scalar checks, _batch, _check_slots
# and _check_shape, _check_inputs, _outputs, data._bind, _launch.  A call with a wrong scalar, shape or container is refused before `data` is
# looked at (tests/test_api_refusals_host.py).

def _layout(layout):
    return {"soa": capi.SOA, "aos": capi.AOS}[layout]   # (KeyError for an unknown name)


def _prologue(problem, layout, visitor, p, params=_params):
    """(model, ntasks, lay, prm) of a solve, with the defaults for the visitor and the parameters."""
    lay = _layout(layout)
    return problem.model(), problem.target_slots(), lay, params(visitor or inverse_kinematics_visitor(), p or dls_parameters())


def _check_shape(name, t, shape):
    """ValueError unless t (None: not given) has the shape; needs no device, and a wrong one would make the kernel read or write out
    of bounds."""
    if t is not None and tuple(getattr(t, "shape", ())) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(getattr(t, "shape", ())), tuple(shape)))


def _check_dims(name, t, n):
    if len(t.shape) != n:
        raise ValueError("%s has shape %s, expected %d dimensions" % (name, tuple(t.shape), n))


def _batch(lay, nq, name, Q0):
    """(B, shape) of the configurations Q0: [nq, B] | [B, nq]."""
    _check_dims(name, Q0, 2)
    B = Q0.shape[1] if lay == capi.SOA else Q0.shape[0]
    _check_shape(name, Q0, (nq, B) if lay == capi.SOA else (B, nq))
    return B, tuple(Q0.shape)


def _check_slots(lay, ntasks, B, name, X, lead=0):
    """The targets-like X is `lead` leading axes (waypoints, vias, goals: outermost) in front of [ntasks, 12, B] | [B, ntasks, 12].
    Returns the leading extents."""
    _check_dims(name, X, 3 + lead)
    extents = tuple(X.shape[:lead])
    _check_shape(name, X, extents + ((ntasks, 12, B) if lay == capi.SOA else (B, ntasks, 12)))
    return extents


def _check_tensors(items, data):
    """Device buffers handed to the C ABI as raw pointers, as (name, tensor, dtype): every one a CUDA tensor of its dtype (TypeError),
    then every one on the problem's device and contiguous (ValueError).  With a wrong one the kernel would read or write out of
    bounds, or through a pointer of another device."""
    import torch
    for name, t, dtype in items:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError("%s must be a CUDA tensor" % name)
        if t.dtype != dtype:
            raise TypeError("%s has dtype %s, expected %s" % (name, t.dtype, dtype))
    for name, t, _ in items:
        if t.device.index != data._device:
            raise ValueError("%s lives on cuda:%s but the problem was created on device %d" % (name, t.device.index, data._device))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)


def _check_inputs(data, **tensors):
    """_check_tensors on the float64 inputs of a call, by argument name; an optional one that is None is skipped."""
    import torch
    _check_tensors([(name, t, torch.float64) for name, t in tensors.items() if t is not None], data)


def _outputs(specs, like, data, out, label="out[{i}] ({name})", unused=0):
    """The outputs of a call, specs = [(name, shape, dtype)]: allocated on like's device, or the caller's own tensors checked against
    the specs.  The last `unused` entries of `out` are neither allocated nor checked (None when allocated, the caller's otherwise)."""
    import torch
    if out is None:
        return [torch.empty(shape, dtype=dtype, device=like.device) for _, shape, dtype in specs] + [None] * unused
    out = list(out)
    if len(out) != len(specs) + unused:
        raise ValueError("out holds %d entries, expected %d" % (len(out), len(specs) + unused))
    for i, (t, (name, shape, dtype)) in enumerate(zip(out, specs)):   # (one output after the other, its shape last)
        _check_tensors([(label.format(i=i, name=name), t, dtype)], data)
        _check_shape(label.format(i=i, name=name), t, shape)
    return out


def _solve_outputs(qs, B, extra=()):
    """The specs every solve shares -- Q like Q0, success and iterations per problem -- followed by `extra`."""
    import torch
    return [("Q", qs, torch.float64), ("success", (B,), torch.uint8), ("iterations", (B,), torch.int32)] + list(extra)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _seed(seed):
    return seed & 0xFFFFFFFFFFFFFFFF


def _launch(like, stream, fn, *args, workspace=None):
    """capi.check(fn(*args[, workspace pointer, its size], stream)) on `stream`, or (None) on torch's current stream of like's device.
    workspace = (size function, *its arguments): allocated for the call when the size is not 0 (0 for a single launch)."""
    import torch
    if workspace is not None:
        nbytes = workspace[0](*workspace[1:])
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=like.device) if nbytes else None
        args += (_ptr(ws), nbytes)
    s = torch.cuda.current_stream(like.device).cuda_stream if stream is None else stream
    capi.check(fn(*args, C.c_void_p(s)))


def _kernel_name(fn, data, visitor, p, *extra):
    prm = _params(visitor or inverse_kinematics_visitor(), p or dls_parameters())
    return fn(data._h, C.byref(prm), *extra).decode()


def dls(problem, q0, data, visitor=None, p=None):
    """ik::dls (reference ik/ik/dls.hpp:111-114): one problem, targets taken from each task's
    `target`; returns q and sets data.success exactly as reference ik/ik/dls.cpp:62-63,76-77.
    Runs as a batch of one on the device."""
    visitor = visitor or inverse_kinematics_visitor()
    p = p or dls_parameters()
    data._bind(problem)
    model = problem.model()
    q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(model.nq)
    tg = np.ascontiguousarray(np.concatenate([_target_slots(t) for t, _ in problem.ordered_tasks()]))
    q = np.empty(model.nq)
    ok = np.zeros(1, np.uint8)
    it = np.zeros(1, np.int32)
    prm = _params(visitor, p)
    capi.check(capi.lib().ikgpu_dls_solve_batch_host(
        data._h, 1, q0.ctypes.data, tg.ctypes.data, C.byref(prm), q.ctypes.data, ok.ctypes.data, it.ctypes.data, capi.AOS))
    data.success, data.iterations, data.q = bool(ok[0]), int(it[0]), q
    return q


def dls_batch(problem, Q0, targets, data, visitor=None, p=None, layout="soa", out=None, stream=None):
    """B independent ik::dls() calls in lockstep on the device.

    torch CUDA tensors (float64, contiguous) go straight through as device pointers on the current
    stream; numpy arrays take the host-pointer entry point (copy in / solve / copy out).
      layout "soa": Q0 [nq, B], targets [ntasks, 12, B]   |   "aos": Q0 [B, nq], targets [B, ntasks, 12]
    Returns (Q, success uint8 [B], iterations int32 [B]) in the same container type as Q0.
    """
    L = capi.lib()
    return _solve_batch(problem, Q0, targets, data, visitor, p, _params, layout, out, stream, L.ikgpu_dls_solve_batch_host, L.ikgpu_dls_solve_batch)


def _solve_batch(problem, Q0, targets, data, visitor, p, params, layout, out, stream, host_fn, device_fn):
    """dls_batch and pik_batch.  Unlike the later entries these bind first and test the container before the shapes: numpy arrays
    are a container they take."""
    data._bind(problem)
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p, params)
    if isinstance(Q0, np.ndarray):
        Q0 = np.ascontiguousarray(Q0, dtype=np.float64)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        B, _ = _batch(lay, model.nq, "Q0", Q0)
        _check_slots(lay, ntasks, B, "targets", targets)
        Q = np.empty_like(Q0)
        ok = np.zeros(B, np.uint8)
        it = np.zeros(B, np.int32)
        capi.check(host_fn(data._h, B, Q0.ctypes.data, targets.ctypes.data, C.byref(prm), Q.ctypes.data, ok.ctypes.data, it.ctypes.data, lay))
        return Q, ok, it
    _check_inputs(data, Q0=Q0, targets=targets)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "targets", targets)
    Q, ok, it = _outputs(_solve_outputs(qs, B), Q0, data, out)
    _launch(Q0, stream, device_fn, data._h, B, _ptr(Q0), _ptr(targets), C.byref(prm), _ptr(Q), _ptr(ok), _ptr(it), lay)
    return Q, ok, it


def dls_track_kernel(data, visitor=None, p=None):
    """Name of what dls_track_batch runs for these parameters: "dls_chain_track<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_track_kernel, data, visitor, p)


def dls_track_batch(problem, Q0, targets, data, visitor=None, p=None, layout="soa", out=None, stream=None):
    """B trajectories of T waypoints: waypoint k of every problem is solved from the result of waypoint k - 1 (waypoint 0 from Q0) --
    the reference caller's tick loop (ik_ros/src/cassie.cpp:92-113) as a horizon.  Bit-identical to T chained dls_batch calls; a
    chain problem runs the whole sequence in one launch with q on-chip between waypoints.

    float64 CUDA tensors, contiguous, waypoints outermost:
      layout "soa": Q0 [nq, B], targets [T, ntasks, 12, B]   |   "aos": Q0 [B, nq], targets [T, B, ntasks, 12]
    out: (Q [T, nq, B] | [T, B, nq], success uint8 [T, B], iterations int32 [T, B]) preallocated, or None.
    Returns (Q, success, iterations)."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    T, = _check_slots(lay, ntasks, B, "targets", targets, lead=1)
    _check_inputs(data, Q0=Q0, targets=targets)
    Q, ok, it = _outputs([("Q", (T,) + qs, torch.float64), ("success", (T, B), torch.uint8), ("iterations", (T, B), torch.int32)], Q0, data, out)
    data._bind(problem)
    _launch(Q0, stream, capi.lib().ikgpu_dls_track_batch, data._h, B, T, _ptr(Q0), _ptr(targets), C.byref(prm), _ptr(Q), _ptr(ok), _ptr(it), lay)
    return Q, ok, it


def _check_waypoints(T):
    if not isinstance(T, int) or T < 0:
        raise ValueError("T must be a non-negative integer, got %r" % (T,))


def _check_vias(P):
    if P < 1:
        raise ValueError("vias holds no via pose (P must be at least 1)")


def _check_joint_step(max_joint_step):
    if not isinstance(max_joint_step, (int, float)) or not math.isfinite(max_joint_step) or max_joint_step < 0:
        raise ValueError("max_joint_step must be finite and not negative (0: no joint-step rule), got %r" % (max_joint_step,))


def _trajectory_outputs(N, qs, B):
    """The specs of a job that writes N slabs of Q / success / iterations and how many of them each problem reached."""
    import torch
    return [("Q", (N,) + qs, torch.float64), ("success", (N, B), torch.uint8), ("iterations", (N, B), torch.int32), ("reached", (B,), torch.int32)]


def line_targets(problem, Q0, goals, data, T, layout="soa"):
    """The T waypoints of the straight Cartesian line from the pose of every task frame at Q0 to its goal (include/ikgpu.h
    ikgpu_line_targets): waypoint k has s = (k + 1) / T, R = R0 exp3(s log3(R0^T R1)), p = p0 + s (p1 - p0); waypoint T - 1 is the goal
    itself.  Every target slot must be a FrameTask's, with a reference frame fixed in the world.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], goals [ntasks, 12, B]   |   "aos": Q0 [B, nq], goals [B, ntasks, 12].
    Returns W [T, ntasks, 12, B] | [T, B, ntasks, 12], the shape of dls_track_batch's targets."""
    import torch
    model, ntasks, lay = problem.model(), problem.target_slots(), _layout(layout)
    _check_waypoints(T)
    B, _ = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "goals", goals)
    _check_inputs(data, Q0=Q0, goals=goals)
    W = torch.empty((T,) + tuple(goals.shape), dtype=torch.float64, device=Q0.device)
    data._bind(problem)
    _launch(Q0, None, capi.lib().ikgpu_line_targets, data._h, B, T, _ptr(Q0), _ptr(goals), _ptr(W), lay)
    return W


def dls_line_kernel(data, visitor=None, p=None):
    """Name of what dls_line_batch runs for these parameters: "dls_chain_line<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_line_kernel, data, visitor, p)


def dls_line_batch(problem, Q0, goals, data, T, visitor=None, p=None, layout="soa", out=None, stream=None):
    """Can the task frame travel in a straight line from where it is at Q0 to its goal, and along which joint trajectory?
    dls_track_batch on line_targets(problem, Q0, goals, data, T), a problem taking part in waypoint k only while all its earlier
    waypoints met the stop rule.  reached[b] counts the waypoints met before the first failure (T: the goal was reached); slabs
    k <= min(reached[b], T - 1) of problem b are written and bit-identical to dls_track_batch on those waypoints, later slabs are
    unspecified.  A chain problem runs one launch that reads the goal alone and leaves a failed line at once.  A relative rotation near
    pi has an ill-conditioned axis: split such a move.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], goals [ntasks, 12, B]   |   "aos": Q0 [B, nq], goals [B, ntasks, 12].
    out: (Q [T, nq, B] | [T, B, nq], success uint8 [T, B], iterations int32 [T, B], reached int32 [B]) preallocated, or None.
    Returns (Q, success, iterations, reached)."""
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_waypoints(T)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "goals", goals)
    _check_inputs(data, Q0=Q0, goals=goals)
    Q, ok, it, reached = _outputs(_trajectory_outputs(T, qs, B), Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_line_batch, data._h, B, T, _ptr(Q0), _ptr(goals), C.byref(prm), _ptr(Q), _ptr(ok), _ptr(it), _ptr(reached), lay,
            workspace=(L.ikgpu_dls_line_workspace_bytes, data._h, B, T, C.byref(prm)))
    return Q, ok, it, reached


def path_targets(problem, Q0, vias, data, T, layout="soa"):
    """The P x T waypoints of the Cartesian path through P via poses per problem (include/ikgpu.h ikgpu_path_targets): segment 0 is
    line_targets(problem, Q0, vias[0], data, T); segment s >= 1 runs from via s - 1's own twelve values to via s; waypoint s T + T - 1 is
    via s itself.  The slot restrictions are line_targets'.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], vias [P, ntasks, 12, B]   |   "aos": Q0 [B, nq], vias [P, B, ntasks, 12].
    Returns W [P T, ntasks, 12, B] | [P T, B, ntasks, 12], the shape of dls_track_batch's targets."""
    import torch
    model, ntasks, lay = problem.model(), problem.target_slots(), _layout(layout)
    _check_waypoints(T)
    B, _ = _batch(lay, model.nq, "Q0", Q0)
    P, = _check_slots(lay, ntasks, B, "vias", vias, lead=1)
    _check_vias(P)
    _check_inputs(data, Q0=Q0, vias=vias)
    W = torch.empty((P * T,) + tuple(vias.shape[1:]), dtype=torch.float64, device=Q0.device)
    data._bind(problem)
    _launch(Q0, None, capi.lib().ikgpu_path_targets, data._h, B, P, T, _ptr(Q0), _ptr(vias), _ptr(W), lay)
    return W


def dls_path_kernel(data, visitor=None, p=None):
    """Name of what dls_path_batch runs for these parameters: "dls_chain_path<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_path_kernel, data, visitor, p)


def dls_path_batch(problem, Q0, vias, data, T, max_joint_step=0.0, visitor=None, p=None, layout="soa", out=None, stream=None):
    """Can the task frame travel from where it is at Q0 through its P via poses, T waypoints per segment, without a joint-space jump --
    and along which joint trajectory?  dls_track_batch on path_targets(problem, Q0, vias, data, T), a problem taking part in waypoint n
    only while all its earlier waypoints were met: the solve met the stop rule and, with max_joint_step > 0, no entry of the task
    support moved by more than max_joint_step (rad, or m for a prismatic joint's entry: one bound over both; plain entries) from the
    configuration the solve started from.  reached[b] counts
    the waypoints met before the first one that was not (P T: the whole path); slabs n <= min(reached[b], P T - 1) of problem b are
    written and bit-identical to dls_track_batch on those waypoints, later slabs are unspecified; success = 1 in the failing slab says
    the waypoint was reached through a jump.  A chain problem runs one launch that reads the P vias alone.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], vias [P, ntasks, 12, B]   |   "aos": Q0 [B, nq], vias [P, B, ntasks, 12].
    out: (Q [P T, nq, B] | [P T, B, nq], success uint8 [P T, B], iterations int32 [P T, B], reached int32 [B]) preallocated, or None.
    Returns (Q, success, iterations, reached)."""
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_waypoints(T)
    _check_joint_step(max_joint_step)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    P, = _check_slots(lay, ntasks, B, "vias", vias, lead=1)
    _check_vias(P)
    _check_inputs(data, Q0=Q0, vias=vias)
    Q, ok, it, reached = _outputs(_trajectory_outputs(P * T, qs, B), Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_path_batch, data._h, B, P, T, _ptr(Q0), _ptr(vias), C.byref(prm), float(max_joint_step), _ptr(Q), _ptr(ok), _ptr(it),
            _ptr(reached), lay, workspace=(L.ikgpu_dls_path_workspace_bytes, data._h, B, P, T, C.byref(prm)))
    return Q, ok, it, reached


def dls_multistart_kernel(data, visitor=None, p=None, num_starts=8):
    """Name of what dls_multistart_batch runs for these parameters: "dls_chain_multistart<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_multistart_kernel, data, visitor, p, num_starts)


def _check_starts(num_starts):
    if not isinstance(num_starts, int) or not 1 <= num_starts <= 64:
        raise ValueError("num_starts must be an integer in 1 .. 64, got %r" % (num_starts,))


def multistart_starts(data, Q0, num_starts, seed=0, layout="soa"):
    """The generated starts 1 .. num_starts-1 of dls_multistart_batch for (seed, Q0): [num_starts-1, nq, B] ("soa") or
    [num_starts-1, B, nq] ("aos").  An entry is drawn uniformly between its limits when it lies in the task support, belongs to a revolute
    or prismatic joint and both limits are finite; every other entry is Q0's.  A function of (seed, problem index, start index, entry)
    only (include/ikgpu.h ikgpu_multistart_starts)."""
    import torch
    _check_starts(num_starts)
    lay = _layout(layout)
    _check_dims("Q0", Q0, 2)
    _check_inputs(data, Q0=Q0)   # (before the shape: nq is read from data)
    B, qs = _batch(lay, len(data.support), "Q0", Q0)
    out = torch.empty((num_starts - 1,) + qs, dtype=torch.float64, device=Q0.device)
    _launch(Q0, None, capi.lib().ikgpu_multistart_starts, data._h, B, num_starts, _ptr(Q0), _seed(seed), _ptr(out), lay)
    return out


def dls_multistart_batch(problem, Q0, targets, data, visitor=None, p=None, num_starts=8, seed=0, starts=None, layout="soa", out=None, stream=None):
    """The best of num_starts solves per problem (ik::dls is a local method: reference ik/ik/dls.cpp:10, :73; the random_restart flag of
    ik/ik/dls.hpp:27 stays inert).  Start 0 is Q0; starts 1 .. num_starts-1 are `starts` ([num_starts-1, nq, B] | [num_starts-1, B, nq])
    or, when None, generated from `seed` (multistart_starts).  The winner is the lowest-index start that met the stop rule, else the one
    with the smallest squared weighted error; Q / success / iterations are bit-identical to dls_batch from that start.  A chain problem
    with num_starts in {2, 4, ..., 64} runs one launch with the starts of a problem in neighbouring lanes.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], targets [ntasks, 12, B]   |   "aos": Q0 [B, nq], targets [B, ntasks, 12]
    out: (Q, success uint8 [B], iterations int32 [B], winner int32 [B], err_sq float64 [B]) preallocated, or None.
    Returns (Q, success, iterations, winner, err_sq)."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_starts(num_starts)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "targets", targets)
    _check_shape("starts", starts, (num_starts - 1,) + qs)
    _check_inputs(data, Q0=Q0, targets=targets, starts=starts)
    Q, ok, it, win, err = _outputs(_solve_outputs(qs, B, [("winner", (B,), torch.int32), ("err_sq", (B,), torch.float64)]), Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_multistart_batch, data._h, B, num_starts, _ptr(Q0), _ptr(starts), _seed(seed), _ptr(targets), C.byref(prm), _ptr(Q),
            _ptr(ok), _ptr(it), _ptr(win), _ptr(err), lay, workspace=(L.ikgpu_dls_multistart_workspace_bytes, data._h, B, num_starts, C.byref(prm)))
    return Q, ok, it, win, err


PathMultistartResult = collections.namedtuple(
    "PathMultistartResult", "q_entry entry_success entry_iterations winner err_sq reached reached_all q success iterations")


def dls_path_multistart_kernel(data, visitor=None, p=None, num_starts=8):
    """Name of what dls_path_multistart_batch runs for these parameters: "dls_chain_path_multistart<...>" (the scout launch, followed by
    "dls_chain_path<...>" for the trajectory) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_path_multistart_kernel, data, visitor, p, num_starts)


def dls_path_multistart_batch(problem, Q0, vias, data, T, max_joint_step=0.0, visitor=None, p=None, num_starts=8, seed=0, starts=None,
                              layout="soa", trajectory=True, out=None, stream=None):
    """Which IK branch at the path's first pose carries the whole path?  vias[0] is that pose; the robot may move freely in joint space
    to it.  Each of num_starts starts (dls_multistart_batch's: Q0, then `starts` or generated from `seed`) solves vias[0]; every start
    that met the stop rule is followed along dls_path_batch(Q0 = its result, vias[1:], T, max_joint_step); the start that gets furthest
    wins, a tie goes to the lowest index, and when no start entered the smallest error wins (include/ikgpu.h
    ikgpu_dls_path_multistart_batch).  q_entry / entry_success / entry_iterations are dls_batch from the winning start, bit for bit;
    reached_all[k] is start k's count, -1 where its entry failed; with trajectory=True, q / success / iterations are dls_path_batch from
    q_entry (for the problems with entry_success = 1).  A chain problem with num_starts in {2, 4, ..., 64} runs two launches: a scout
    that stores no trajectory, then the winner's path -- one trajectory buffer, not num_starts.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], vias [P, ntasks, 12, B]   |   "aos": Q0 [B, nq], vias [P, B, ntasks, 12].
    out: a PathMultistartResult of preallocated tensors (q / success / iterations None with trajectory=False), or None.
    Returns PathMultistartResult(q_entry, entry_success, entry_iterations, winner, err_sq, reached int32 [B], reached_all int32 [K, B],
    q [(P-1) T, nq, B] | [(P-1) T, B, nq], success uint8 [(P-1) T, B], iterations int32 [(P-1) T, B])."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_starts(num_starts)
    _check_waypoints(T)
    _check_joint_step(max_joint_step)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    P, = _check_slots(lay, ntasks, B, "vias", vias, lead=1)
    _check_vias(P)
    _check_shape("starts", starts, (num_starts - 1,) + qs)
    _check_inputs(data, Q0=Q0, vias=vias, starts=starts)
    N, K = (P - 1) * T, num_starts
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    specs = list(zip(PathMultistartResult._fields, (qs, (B,), (B,), (B,), (B,), (B,), (K, B), (N,) + qs, (N, B), (N, B)),
                     (f64, u8, i32, i32, f64, i32, i32, f64, u8, i32)))
    kept = 10 if trajectory else 7    # trajectory=False: q / success / iterations are neither allocated nor checked
    r = PathMultistartResult(*_outputs(specs[:kept], Q0, data, out, "out.{name}", unused=10 - kept))
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_path_multistart_batch, data._h, B, K, P, T, _ptr(Q0), _ptr(starts), _seed(seed), _ptr(vias), C.byref(prm),
            float(max_joint_step), _ptr(r.q_entry), _ptr(r.entry_success), _ptr(r.entry_iterations), _ptr(r.winner), _ptr(r.err_sq), _ptr(r.reached),
            _ptr(r.reached_all), *(_ptr(t) if trajectory else None for t in (r.q, r.success, r.iterations)), lay,
            workspace=(L.ikgpu_dls_path_multistart_workspace_bytes, data._h, B, K, P, T, C.byref(prm), 1 if trajectory else 0))
    return r


class PickRule(enum.IntEnum):
    """How dls_pick_batch ranks the starts that met the stop rule (include/ikgpu.h ikgpu_pick_rule); the smallest cost wins."""
    DISTANCE = 0         # sum of w (q - q_ref)^2 over the task support
    MAX_DISTANCE = 1     # max of w |q - q_ref| over the task support
    LIMIT_MARGIN = 2     # 0.5 - the smallest relative distance to a joint limit
    MANIPULABILITY = 3   # 1 / sqrt(det(J J^T + damping^2 I))


def dls_pick_kernel(data, visitor=None, p=None, num_starts=8, rule=PickRule.DISTANCE):
    """Name of what dls_pick_batch runs for these parameters: "dls_chain_pick<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_pick_kernel, data, visitor, p, num_starts, int(PickRule(rule)))


def dls_pick_batch(problem, Q0, targets, data, visitor=None, p=None, num_starts=8, rule=PickRule.DISTANCE, q_ref=None, weights=None, seed=0,
                   starts=None, layout="soa", out=None, stream=None):
    """Among num_starts solves per problem (dls_multistart_batch's starts), the one that met the stop rule with the smallest cost under
    `rule`: the configuration closest to q_ref (default Q0), the one furthest from its joint limits, or the best-conditioned one
    (TRAC-IK's Distance / Manip solve types; ik::dls is a local method: reference ik/ik/dls.cpp:10, :73).  A cost tie goes to the lowest
    start index; when no start converged, the one with the smallest squared weighted error.  Q / success / iterations are bit-identical
    to dls_batch from the winning start.  A chain problem with num_starts in {2, 4, ..., 64} runs one launch.

    float64 CUDA tensors, contiguous: layout "soa": Q0, q_ref [nq, B], targets [ntasks, 12, B]   |   "aos": Q0, q_ref [B, nq], targets [B, ntasks, 12]
    weights: nq non-negative floats (host), or None: ones.  Read by DISTANCE and MAX_DISTANCE only, as q_ref.
    out: (Q, success uint8 [B], iterations int32 [B], winner int32 [B], cost float64 [B], err_sq float64 [B]) preallocated, or None.
    Returns (Q, success, iterations, winner, cost, err_sq)."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_starts(num_starts)
    rule = int(PickRule(rule))
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "targets", targets)
    _check_shape("starts", starts, (num_starts - 1,) + qs)
    _check_shape("q_ref", q_ref, qs)
    w = None
    if weights is not None:
        w = [float(x) for x in weights]
        if len(w) != model.nq:
            raise ValueError("weights has %d entries, the model has nq = %d" % (len(w), model.nq))
        w = (C.c_double * model.nq)(*w)
    _check_inputs(data, Q0=Q0, targets=targets, starts=starts, q_ref=q_ref)
    Q, ok, it, win, cost, err = _outputs(_solve_outputs(qs, B, [("winner", (B,), torch.int32), ("cost", (B,), torch.float64),
                                                               ("err_sq", (B,), torch.float64)]), Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_pick_batch, data._h, B, num_starts, _ptr(Q0), _ptr(starts), _seed(seed), _ptr(targets), C.byref(prm), rule,
            _ptr(q_ref), w, _ptr(Q), _ptr(ok), _ptr(it), _ptr(win), _ptr(cost), _ptr(err), lay,
            workspace=(L.ikgpu_dls_pick_workspace_bytes, data._h, B, num_starts, C.byref(prm)))
    return Q, ok, it, win, cost, err


def dls_solutions_kernel(data, visitor=None, p=None, num_starts=8):
    """Name of what dls_solutions_batch runs for these parameters: "dls_chain_solutions<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_solutions_kernel, data, visitor, p, num_starts)


def dls_solutions_batch(problem, Q0, targets, data, visitor=None, p=None, num_starts=8, max_solutions=None, separation=0.1, seed=0, starts=None,
                        layout="soa", out=None, stream=None):
    """The distinct solutions among num_starts solves per problem (an IK target rarely has one; ik::dls is a local method: reference
    ik/ik/dls.cpp:10, :73; the random_restart flag of ik/ik/dls.hpp:27 stays inert).  The starts are dls_multistart_batch's.  In increasing
    start index, a start is kept when it met the stop rule, fewer than max_solutions (default: num_starts) are kept, and some entry of the
    task support differs by `separation` (rad or m, plain entries: a full turn apart is a different configuration) or more from every
    start kept before it.  Each kept Q is bit-identical to dls_batch from that start.  A chain problem with num_starts in {2, 4, ..., 64}
    runs one launch with the starts of a problem in neighbouring lanes.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], targets [ntasks, 12, B]   |   "aos": Q0 [B, nq], targets [B, ntasks, 12]
    out: (Q [N, nq, B] | [N, B, nq], count int32 [B], which int32 [N, B], iterations int32 [N, B]) preallocated, or None.
    Returns (Q, count, which, iterations); slots n >= count[b] of problem b are not written."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    _check_starts(num_starts)
    N = num_starts if max_solutions is None else max_solutions
    if not isinstance(N, int) or not 1 <= N <= num_starts:
        raise ValueError("max_solutions must be an integer in 1 .. num_starts, got %r" % (max_solutions,))
    separation = float(separation)
    if not (math.isfinite(separation) and separation >= 0.0):
        raise ValueError("separation must be finite and not negative, got %r" % (separation,))
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    _check_slots(lay, ntasks, B, "targets", targets)
    _check_shape("starts", starts, (num_starts - 1,) + qs)
    _check_inputs(data, Q0=Q0, targets=targets, starts=starts)
    Q, count, which, it = _outputs([("Q", (N,) + qs, torch.float64), ("count", (B,), torch.int32), ("which", (N, B), torch.int32),
                                    ("iterations", (N, B), torch.int32)], Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_solutions_batch, data._h, B, num_starts, N, _ptr(Q0), _ptr(starts), _seed(seed), _ptr(targets), C.byref(prm), separation,
            _ptr(Q), _ptr(count), _ptr(which), _ptr(it), lay, workspace=(L.ikgpu_dls_solutions_workspace_bytes, data._h, B, num_starts, N, C.byref(prm)))
    return Q, count, which, it


def _check_goalset_size(num_goals, num_starts):
    _check_starts(num_starts)
    if not isinstance(num_goals, int) or num_goals < 1 or num_goals * num_starts > 64:
        raise ValueError("the number of goals must be an integer >= 1 with goals x starts <= 64, got %r goals and %r starts" % (num_goals, num_starts))


def dls_goalset_kernel(data, visitor=None, p=None, num_goals=4, num_starts=1):
    """Name of what dls_goalset_batch runs for these parameters: "dls_chain_goalset<...>" (one launch) or "loop(<data.kernel>)"."""
    return _kernel_name(capi.lib().ikgpu_dls_goalset_kernel, data, visitor, p, num_goals, num_starts)


def dls_goalset_batch(problem, Q0, goals, data, visitor=None, p=None, num_starts=1, seed=0, starts=None, layout="soa", out=None, stream=None):
    """Reach any of G alternative goals per problem from num_starts starts (G grasp candidates, footholds, docking poses; G =
    goals.shape[0], G x num_starts <= 64).  Candidate g * num_starts + k is dls_batch from start k (dls_multistart_batch's starts: they do
    not depend on the goal) against goals[g].  The winner is the first candidate, in that order, that met the stop rule -- the lowest goal
    index, and within it the lowest start -- else the one with the smallest squared weighted error; Q / success / iterations are
    bit-identical to dls_batch for that candidate.  reachable[g, b] = 1 where some start of goal g met the stop rule.  A chain problem
    with G and num_starts powers of two (and G x num_starts >= 2) runs one launch with a problem's candidates in neighbouring lanes.

    float64 CUDA tensors, contiguous: layout "soa": Q0 [nq, B], goals [G, ntasks, 12, B]   |   "aos": Q0 [B, nq], goals [G, B, ntasks, 12]
    out: (Q, success uint8 [B], iterations int32 [B], goal int32 [B], start int32 [B], err_sq float64 [B], reachable uint8 [G, B])
    preallocated, or None.  Returns (Q, success, iterations, goal, start, err_sq, reachable)."""
    import torch
    model, ntasks, lay, prm = _prologue(problem, layout, visitor, p)
    B, qs = _batch(lay, model.nq, "Q0", Q0)
    G, = _check_slots(lay, ntasks, B, "goals", goals, lead=1)
    _check_goalset_size(G, num_starts)
    _check_shape("starts", starts, (num_starts - 1,) + qs)
    _check_inputs(data, Q0=Q0, goals=goals, starts=starts)
    Q, ok, it, goal, start, err, reach = _outputs(_solve_outputs(qs, B, [("goal", (B,), torch.int32), ("start", (B,), torch.int32),
                                                                        ("err_sq", (B,), torch.float64), ("reachable", (G, B), torch.uint8)]), Q0, data, out)
    data._bind(problem)
    L = capi.lib()
    _launch(Q0, stream, L.ikgpu_dls_goalset_batch, data._h, B, G, num_starts, _ptr(Q0), _ptr(starts), _seed(seed), _ptr(goals), C.byref(prm), _ptr(Q), _ptr(ok),
            _ptr(it), _ptr(goal), _ptr(start), _ptr(err), _ptr(reach), lay,
            workspace=(L.ikgpu_dls_goalset_workspace_bytes, data._h, B, G, num_starts, C.byref(prm)))
    return Q, ok, it, goal, start, err, reach


class pik_parameters:
    """ik::pik_parameters (reference ik/ik/pik.hpp:11-16).  `damping` and `max_time` are carried for source
    compatibility: the reference loop reads neither (the damping factors live in pik_data.lambda_)."""

    def __init__(self, max_iterations=100, damping=1e-2, step_length=1.0, max_time=1.0):
        self.max_iterations = max_iterations
        self.damping = damping
        self.step_length = step_length
        self.max_time = max_time


class pik_data(dls_data):
    """ik::pik_data (reference ik/ik/pik.hpp:21-50): the workspace of ik::pik.  `lambda_` holds the damping factor of
    each priority level (`lambda` in the reference, 1.0 each) and `da` the secondary step projected into the null
    space of all levels (zero); both are read at every call."""

    def __init__(self, problem, device=0):
        super().__init__(problem, device)
        self.lambda_ = [1.0] * (problem.max_priority_level() + 1)
        self.da = np.zeros(problem.model().nv)

    @property
    def kernel(self):
        """Name of the kernel the next call runs with the current `lambda_` / `da`: the problem's DLS kernel when there is one
        priority level and no secondary step (ik::pik is then the DLS iteration, include/ikgpu.h), the PIK kernel otherwise."""
        if self._h is None or len(self.lambda_) > capi.MAX_PIK_LEVELS:
            return ""
        prm = self._params(inverse_kinematics_visitor(), pik_parameters())
        return capi.lib().ikgpu_pik_kernel(self._h, C.byref(prm)).decode()

    @kernel.setter
    def kernel(self, _):
        pass  # dls_data._bind records the DLS kernel's name; this class derives its name from the handle at every read

    def _params(self, visitor, p):
        prm = capi.PikParams()
        prm.max_iterations, prm.step_length, prm.stop_sq_tol = int(p.max_iterations), float(p.step_length), float(visitor.tolerance)
        prm.num_levels = len(self.lambda_)
        if prm.num_levels > capi.MAX_PIK_LEVELS:
            raise ValueError("ik::pik on the device takes at most %d priority levels" % capi.MAX_PIK_LEVELS)
        for i, l in enumerate(self.lambda_):
            prm.lam[i] = float(l)
        da = np.ascontiguousarray(self.da, dtype=np.float64)
        if da.any():
            prm._da_keepalive = da
            prm.da = da.ctypes.data_as(C.POINTER(C.c_double))
        return prm


def plan_generic(problem):
    """Name of the generic kernel instance of the problem (what ik::pik runs on)."""
    name = plan(problem)
    if name.startswith("dls_generic<"):
        return name
    rows = sum(t.dimension() for t, _ in problem.ordered_tasks())
    m = problem.model()
    return "dls_generic<M=%d,nv=%d,joints=%d>" % (rows, m.nv, m.njoints - 1)


def pik(problem, q0, data, visitor=None, p=None):
    """ik::pik (reference ik/ik/pik.hpp:56-59, ik/ik/pik.cpp:31-103): one problem, targets from each task's `target`;
    returns q and sets data.success as the reference does.  A batch of one on the device."""
    visitor = visitor or inverse_kinematics_visitor()
    p = p or pik_parameters()
    data._bind(problem)
    model = problem.model()
    q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(model.nq)
    tg = np.ascontiguousarray(np.concatenate([_target_slots(t) for t, _ in problem.ordered_tasks()]))
    q = np.empty(model.nq)
    ok = np.zeros(1, np.uint8)
    it = np.zeros(1, np.int32)
    prm = data._params(visitor, p)
    capi.check(capi.lib().ikgpu_pik_solve_batch_host(
        data._h, 1, q0.ctypes.data, tg.ctypes.data, C.byref(prm), q.ctypes.data, ok.ctypes.data, it.ctypes.data, capi.AOS))
    data.success, data.iterations, data.q = bool(ok[0]), int(it[0]), q
    return q


def pik_batch(problem, Q0, targets, data, visitor=None, p=None, layout="soa", out=None, stream=None):
    """B independent ik::pik() calls in lockstep on the device; arguments and return value as dls_batch."""
    L = capi.lib()
    return _solve_batch(problem, Q0, targets, data, visitor, p or pik_parameters(), data._params, layout, out, stream, L.ikgpu_pik_solve_batch_host,
                        L.ikgpu_pik_solve_batch)


def evaluate_batch(problem, Q, targets, data, layout="soa", jacobian=True):
    """evaluate_problem_data + stacking (reference ik/ik/data.cpp:25-58, ik/ik/dls.cpp:18-24) for a
    batch, on the device: returns (e [M, B], J [M, nv, B]) for "soa" ([B, M], [B, M, nv] for "aos")."""
    import torch
    data._bind(problem)
    model, nt, lay = problem.model(), problem.target_slots(), _layout(layout)
    _check_inputs(data, Q=Q)   # (one argument after the other, its shape last)
    B, _ = _batch(lay, model.nq, "Q", Q)
    _check_inputs(data, targets=targets)
    _check_slots(lay, nt, B, "targets", targets)
    M = data.rows
    e = torch.empty((M, B) if lay == capi.SOA else (B, M), dtype=torch.float64, device=Q.device)
    J = torch.empty((M, model.nv, B) if lay == capi.SOA else (B, M, model.nv), dtype=torch.float64, device=Q.device) if jacobian else None
    _launch(Q, None, capi.lib().ikgpu_evaluate_batch, data._h, B, _ptr(Q), _ptr(targets), _ptr(e), _ptr(J), lay)
    return e, J


def task_frames_fk_batch(problem, Q, data, layout="soa"):
    """World placements of the task frames (one entry of data.oMf per task, reference
    ik/ik/data.cpp:28-29): [ntasks, 12, B] ("soa") or [B, ntasks, 12] ("aos")."""
    import torch
    data._bind(problem)
    model, nt, lay = problem.model(), problem.target_slots(), _layout(layout)
    _check_inputs(data, Q=Q)
    B, _ = _batch(lay, model.nq, "Q", Q)
    out = torch.empty((nt, 12, B) if lay == capi.SOA else (B, nt, 12), dtype=torch.float64, device=Q.device)
    _launch(Q, None, capi.lib().ikgpu_task_frames_fk_batch, data._h, B, _ptr(Q), _ptr(out), lay)
    return out
