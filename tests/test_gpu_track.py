"""ikgpu_dls_track_batch on the device: a sequence of T targets per problem, every waypoint started from the result of the one before
(the reference caller's tick loop, ik_ros/src/cassie.cpp:92-113, as a horizon).  The call is DEFINED as T chained calls of the single
solve, so the reference here is T calls of ik_amd.dls_batch on the same stream and the assertion is np.array_equal on all three
outputs -- for every build of the chain kernel (one launch: dls_chain_track<...>), both layouts, batch sizes around the wave and
machine boundaries, stop rule and never-stop, with and without the optional arrays; for a tree, a static-program and a derived-visitor
problem through the loop of existing launches; under a captured graph; and against the chained oracle.  The trajectory
(tests/track_common.py) puts lanes into every branch of the lane program."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import urdf_path
import track_common

pytestmark = pytest.mark.gpu

STOP = (12, 1e-4)      # (max_iterations, tolerance): more than the two-phase hand-over point, so a large chained batch runs two-phase
NEVER = (5, -1.0)


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# the chain cases of tests/test_gpu_refill.py
CASES = [
    ("cassie_fixed", "LeftFootFront", 2, "default"),   # hot
    ("cassie_fixed", "LeftFootFront", 2, "general"),
    ("cassie_fixed", "LeftFootFront", 0, "default"),   # a Position task: general builds only
    ("ur5", "tool0", 2, "default"),                    # nq == nj: no entries outside the chain
    ("arm7", "tool", 2, "default"),                    # hot-rtc (general when hipRTC is absent)
    ("arm7", "tool", 2, "general"),
]
_problems = {}


def _problem(case):
    import ik_amd
    if case not in _problems:
        name, frame, ktype, build = case
        model = ik_amd.Model.from_urdf_file(urdf_path(name))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType(ktype)))
        with env(IKGPU_CHAIN_HOT="0" if build == "general" else None):
            data = ik_amd.dls_data(problem, device=0)
        # the waypoints are poses of the frame: a Full task on the same frame computes them whatever the case's own task type
        pose = ik_amd.InverseKinematicsProblem(model)
        pose.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        _problems[case] = (model, problem, data, pose, ik_amd.dls_data(pose, device=0))
    return _problems[case]


def _trajectory(torch, case, B, T, jump=True):
    """(start [nq, B], waypoints [T, 1, 12, B]) on the device, SoA."""
    import ik_amd
    model, problem, data, pose, pose_data = _problem(case)
    q0, confs = track_common.configurations(model, case[0], B, T, jump)
    way = [ik_amd.task_frames_fk_batch(pose, torch.from_numpy(np.ascontiguousarray(q.T)).cuda(), pose_data) for q in confs]
    return torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.stack(way)


def _in_layout(Q0, TG, layout):
    return (Q0, TG) if layout == "soa" else (Q0.t().contiguous(), TG.permute(0, 3, 1, 2).contiguous())


def _visitor(ik_amd, rule):
    return (ik_amd.inverse_kinematics_visitor(rule[1]) if rule[1] >= 0 else ik_amd.never_stop_visitor()), ik_amd.dls_parameters(max_iterations=rule[0])


def _chained(ik_amd, problem, data, Q0, TG, rule, layout, visitor=None):
    """The definition: T calls of dls_batch, each from the result of the one before, on the current stream."""
    v, p = _visitor(ik_amd, rule)
    v = visitor or v
    q, Qs, oks, its = Q0, [], [], []
    for k in range(TG.shape[0]):
        q, ok, it = ik_amd.dls_batch(problem, q, TG[k], data, v, p, layout=layout)
        Qs.append(q), oks.append(ok), its.append(it)
    import torch
    return torch.stack(Qs).cpu().numpy(), torch.stack(oks).cpu().numpy(), torch.stack(its).cpu().numpy()


def _tracked(ik_amd, problem, data, Q0, TG, rule, layout, visitor=None, out=None):
    v, p = _visitor(ik_amd, rule)
    Q, ok, it = ik_amd.dls_track_batch(problem, Q0, TG, data, visitor or v, p, layout=layout, out=out)
    return Q.cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_track" + data.kernel[len("dls_chain"):]


def _check_name(ik_amd, data, rule):
    v, p = _visitor(ik_amd, rule)
    name = ik_amd.dls_track_kernel(data, v, p)
    fused, loop = _expected_name(data), "loop(%s)" % data.kernel
    # every stop-rule call on a chain problem is the single launch; a never-stop call may be routed through the loop of launches
    assert name == fused or (rule[1] < 0 and name == loop), (name, data.kernel)
    return name


@pytest.mark.parametrize("B,T", [(1, 24), (63, 24), (64, 24), (65, 24), (4097, 24), (65536, 24), (300017, 8)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_track_is_bit_identical_to_chained_solves(torch_cuda, case, B, T):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, TG = _trajectory(torch, case, B, T)
    for layout in ("soa", "aos"):
        q0, tg = _in_layout(Q0, TG, layout)
        for rule in (STOP, NEVER):
            name = _check_name(ik_amd, data, rule)
            ref = _chained(ik_amd, problem, data, q0, tg, rule, layout)
            got = _tracked(ik_amd, problem, data, q0, tg, rule, layout)
            for x, y, what in zip(got, ref, ("q", "success", "iterations")):
                assert np.array_equal(x, y), (case, B, layout, rule, name, what)
            if rule is STOP and case[0] == "cassie_fixed" and case[2] == 2 and B >= 4097:
                q, ok, it = (ref[0] if layout == "aos" else ref[0].transpose(0, 2, 1)), ref[1], ref[2]
                hi = float(np.asarray(model.upperPositionLimit)[-1])
                start = (q0 if layout == "aos" else q0.t()).cpu().numpy()[:, -1]
                assert (it[0] == 0).all() and (it[T // 2] == 0).all() and (ok[T - 1] == 0).any() and (ok[T - 1] == 1).any()
                assert np.array_equal(q[0][:, -1], start) and (start > hi).all() and (q[1][it[1] > 0, -1] == hi).all() and (it[1] > 0).any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_track_without_the_optional_arrays(torch_cuda, case):
    """success == NULL and iters == NULL, straight through the C ABI (the Python entry always passes them)."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, T = 4097, 24
    Q0, TG = _trajectory(torch, case, B, T)
    for rule in (STOP, NEVER):
        ref = _chained(ik_amd, problem, data, Q0, TG, rule, "soa")
        v, p = _visitor(ik_amd, rule)
        prm = api._params(v, p)
        Q = torch.full((T, model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        capi.check(capi.lib().ikgpu_dls_track_batch(data._h, B, T, Q0.data_ptr(), TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, capi.SOA, C.c_void_p(s)))
        assert np.array_equal(Q.cpu().numpy(), ref[0]), (case, rule)
        # ... and only one of them
        it = torch.full((T, B), -7, dtype=torch.int32, device="cuda")
        capi.check(capi.lib().ikgpu_dls_track_batch(data._h, B, T, Q0.data_ptr(), TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, it.data_ptr(), capi.SOA, C.c_void_p(s)))
        assert np.array_equal(Q.cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[2]), (case, rule)


def _fallback_trajectory(torch, name, ff, specs, B, T, rows=None):
    """A problem of tests/test_gpu_generic.py's builder with T target sets (its workload under T seeds) around one start."""
    from test_gpu_generic import build
    with env(IKGPU_TREE_STATIC_ROWS=rows):
        ik, O, model, problem, data, om, ot, q0, tg = build(name, ff, specs, B, seed=0)
    tgs = [tg] + [build(name, ff, specs, B, seed=k, device=False)[8] for k in range(1, T)]
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
    TG = torch.from_numpy(np.ascontiguousarray(np.stack(tgs).transpose(0, 2, 3, 1))).cuda()
    return ik, problem, data, Q0, TG


FULL_BODY = [("frame", "LeftFootFront", "universe", 2, 0, None), ("frame", "RightFootFront", "universe", 2, 0, None), ("frame", "pelvis", "universe", 2, 0, None)]
DEMO = [("frame", "LeftFootFront", "pelvis", 0, 0, None), ("frame", "pelvis", "universe", 2, 0, None), ("align", "LeftFootFront", "universe", 1, 0, None)]


@pytest.mark.parametrize("kind", ["tree", "static_program", "derived_visitor"])
def test_other_problem_kinds_run_the_chained_launches_inside_the_call(torch_cuda, kind):
    torch = torch_cuda
    import ik_amd
    B, T = 4097, 6
    visitor = None
    if kind == "tree":
        ik, problem, data, Q0, TG = _fallback_trajectory(torch, "cassie", True, FULL_BODY, B, T, rows="0")
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
    elif kind == "static_program":
        ik, problem, data, Q0, TG = _fallback_trajectory(torch, "cassie", True, DEMO, B, T, rows="12")
        assert data.kernel.startswith("dls_generic<") and data.kernel.endswith(",static>") or data.kernel.startswith("dls_tree<"), data.kernel   # (the tree kernel when hipRTC is absent)
    else:
        model, problem, data, _, _ = _problem(CASES[0])
        Q0, TG = _trajectory(torch, CASES[0], B, T)
        visitor = ik_amd.inverse_kinematics_visitor(1e-4, step_tolerance=1e-3)
    rules = [(30, 1e-4)] if kind == "derived_visitor" else [(1, -1.0), (3, -1.0), (30, 1e-4)]
    for rule in rules:
        for layout in ("soa", "aos"):
            q0, tg = _in_layout(Q0, TG, layout)
            v, p = _visitor(ik_amd, rule)
            name = ik_amd.dls_track_kernel(data, visitor or v, p)
            assert name == "loop(%s)" % data.kernel, name
            ref = _chained(ik_amd, problem, data, q0, tg, rule, layout, visitor)
            got = _tracked(ik_amd, problem, data, q0, tg, rule, layout, visitor)
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), (kind, rule, layout)
            assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_track_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist and no allocation: captured on a side stream (outputs preallocated through
    out=) and replayed twice it gives the eager call's bits."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, T = 4097, 24
    Q0, TG = _trajectory(torch, case, B, T)
    name = _check_name(ik_amd, data, STOP)
    assert name == _expected_name(data)
    eager = _tracked(ik_amd, problem, data, Q0, TG, STOP, "soa")
    out = (torch.empty((T, model.nq, B), dtype=torch.float64, device="cuda"), torch.empty((T, B), dtype=torch.uint8, device="cuda"),
           torch.empty((T, B), dtype=torch.int32, device="cuda"))
    v, p = _visitor(ik_amd, STOP)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_track_batch(problem, Q0, TG, data, v, p, out=out)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_track_batch(problem, Q0, TG, data, v, p, out=out)
    for _ in range(2):
        out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert np.array_equal(x.cpu().numpy(), y), case


def test_track_against_the_chained_oracle(torch_cuda):
    """The CPU test's rule on the device: the oracle chained the same way agrees on flags and iteration counts on every waypoint,
    max |dq| < 1e-9 (Cassie leg, hot and general builds)."""
    torch = torch_cuda
    import ik_amd
    import oracle as O
    B, T = 4097, 24
    for case in (CASES[0], CASES[1]):
        model, problem, data, _, _ = _problem(case)
        Q0, TG = _trajectory(torch, case, B, T)
        om = O.OracleModel(model.flat())
        ot = O.make_tasks([(model.getFrameId(case[1]), 0, 2, 0, None)])
        tg = TG.permute(0, 3, 1, 2).contiguous().cpu().numpy()          # [T, B, 1, 12]
        for rule in (STOP, NEVER):
            q, ok, it = _tracked(ik_amd, problem, data, Q0, TG, rule, "soa")
            qo, worst = Q0.t().contiguous().cpu().numpy(), 0.0
            for k in range(T):
                qo, ok_ref, it_ref = O.dls_batch(om, ot, tg[k], qo, O.params(rule[0], 1e-2, 1.0, rule[1]))
                assert np.array_equal(ok[k], ok_ref) and np.array_equal(it[k], it_ref), (case, rule, k)
                worst = max(worst, float(np.abs(q[k].T - qo).max()))
            print("%s %s: max |q_track - q_oracle| over %d waypoints = %.3g" % (data.kernel, rule, T, worst))
            assert worst < 1e-9, (case, rule, worst)
