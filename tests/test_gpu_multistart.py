"""ikgpu_dls_multistart_batch on the device: the best of K starts per problem (ik::dls is a local method -- reference ik/ik/dls.cpp:10,
:73; the random_restart flag of ik/ik/dls.hpp:27 is read by nothing).  The call is DEFINED through K single solves (include/ikgpu.h),
so the reference here is K calls of ik_amd.dls_batch from the columns of ik_amd.multistart_starts, with the errors from
evaluate_batch(jacobian=False), and the assertions are tests/multistart_common.py check_selection's: q / success / iterations are the
single solve's from start winner[b] by np.array_equal; the winner has the minimal key; err_sq is the winner's error to 5e-11 in the
norm.  For every build of the chain kernel (one launch: dls_chain_multistart<...>), group sizes 2 / 8 / 64 with batch sizes that put a
group alone in a wave, a wave boundary between groups and B K off a multiple of 64, both layouts, both rules, generated and caller's
starts, with and without the optional arrays; through the loop of existing launches for K = 1, K = 3, a tree problem and a derived
visitor; under a captured graph; and the effect on an arm with uniform targets."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import urdf_path
import multistart_common as MC

pytestmark = pytest.mark.gpu

STOP = (100, 1e-4)
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


# the chain cases of tests/test_gpu_track.py
CASES = [
    ("cassie_fixed", "LeftFootFront", 2, "default"),   # hot
    ("cassie_fixed", "LeftFootFront", 2, "general"),
    ("cassie_fixed", "LeftFootFront", 0, "default"),   # a Position task: general builds only
    ("ur5", "tool0", 2, "default"),                    # nq == nj: no entries outside the chain
    ("arm7", "tool", 2, "default"),                    # hot-rtc (general when hipRTC is absent)
    ("arm7", "tool", 2, "general"),
]
_problems, _workloads = {}, {}


def _problem(case):
    import ik_amd
    if case not in _problems:
        name, frame, ktype, build = case
        model = ik_amd.Model.from_urdf_file(urdf_path(name))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType(ktype)))
        with env(IKGPU_CHAIN_HOT="0" if build == "general" else None):
            data = ik_amd.dls_data(problem, device=0)
        # the targets are poses of the frame: a Full task on the same frame computes them whatever the case's own task type
        pose = ik_amd.InverseKinematicsProblem(model)
        pose.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        _problems[case] = (model, problem, data, pose, ik_amd.dls_data(pose, device=0))
    return _problems[case]


def _workload(torch, case, B):
    """(start [nq, B], targets [1, 12, B]) on the device, SoA: uniform between the limits (tests/multistart_common.py)."""
    import ik_amd
    if (case[0], case[1], B) not in _workloads:
        model, problem, data, pose, pose_data = _problem(case)
        q0, qt = MC.uniform_configurations(model, B, 0)
        tg = ik_amd.task_frames_fk_batch(pose, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), pose_data)
        _workloads[(case[0], case[1], B)] = (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), tg)
    return _workloads[(case[0], case[1], B)]


def _visitor(ik_amd, rule):
    return (ik_amd.inverse_kinematics_visitor(rule[1]) if rule[1] >= 0 else ik_amd.never_stop_visitor()), ik_amd.dls_parameters(max_iterations=rule[0])


def _norms(ik_amd, problem, data, Q, TG):
    e = ik_amd.evaluate_batch(problem, Q, TG, data, jacobian=False)
    e = e[0] if isinstance(e, tuple) else e
    return np.linalg.norm(e.cpu().numpy(), axis=0)           # [B]


def _reference(ik_amd, problem, data, Q0, gen, TG, v, p):
    """The definition: the single solve from every start (SoA), and the error at its result."""
    singles, errs = [], []
    for k in range(gen.shape[0] + 1):
        q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], TG, data, v, p)
        singles.append((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()))
        errs.append(_norms(ik_amd, problem, data, q, TG) ** 2)
    return singles, errs


def _run(ik_amd, problem, data, Q0, TG, v, p, K, seed, starts, layout, out=None):
    """One multi-start call in `layout` from SoA inputs; AoS numpy views back."""
    if layout == "aos":
        Q0, TG = Q0.t().contiguous(), TG.permute(2, 0, 1).contiguous()
        starts = None if starts is None else starts.permute(0, 2, 1).contiguous()
    Q, ok, it, win, err = ik_amd.dls_multistart_batch(problem, Q0, TG, data, v, p, num_starts=K, seed=seed, starts=starts, layout=layout, out=out)
    q = Q.cpu().numpy()
    return (q.T if layout == "soa" else q), ok.cpu().numpy(), it.cpu().numpy(), win.cpu().numpy(), err.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_multistart" + data.kernel[len("dls_chain"):]


def _check_call(torch, ik_amd, problem, data, Q0, TG, rule, K, seed, label, visitor=None, supplied=True):
    """Every way to make the call against the definition; returns the SoA-generated result."""
    v, p = _visitor(ik_amd, rule)
    v = visitor or v
    gen = ik_amd.multistart_starts(data, Q0, K, seed)
    assert tuple(gen.shape) == (K - 1,) + tuple(Q0.shape)
    singles, errs = _reference(ik_amd, problem, data, Q0, gen, TG, v, p)
    got = _run(ik_amd, problem, data, Q0, TG, v, p, K, seed, None, "soa")
    at_result = _norms(ik_amd, problem, data, torch.from_numpy(np.ascontiguousarray(got[0].T)).cuda(), TG)
    worst = MC.check_selection(got, singles, errs, at_result, label)
    ways = [(None, "aos")] + ([(gen, "soa"), (gen, "aos")] if supplied and K > 1 else [])
    for starts, layout in ways:
        again = _run(ik_amd, problem, data, Q0, TG, v, p, K, seed, starts, layout)
        for x, y, what in zip(again, got, ("q", "success", "iterations", "winner", "err_sq")):
            assert np.array_equal(x, y), (label, layout, starts is None, what)
    # the generated starts are the same in both layouts
    assert torch.equal(ik_amd.multistart_starts(data, Q0.t().contiguous(), K, seed, layout="aos").permute(0, 2, 1), gen)
    return got, singles, worst


SHAPES = [(2, 33), (2, 130)] + [(8, b) for b in (1, 7, 8, 9, 4097)] + [(64, b) for b in (1, 3, 130)]


@pytest.mark.parametrize("K,B", SHAPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_multistart_returns_the_best_single_solve(torch_cuda, case, K, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, TG = _workload(torch, case, B)
    for rule in (STOP, NEVER):
        v, p = _visitor(ik_amd, rule)
        assert ik_amd.dls_multistart_kernel(data, v, p, K) == _expected_name(data)
        got, singles, worst = _check_call(torch, ik_amd, problem, data, Q0, TG, rule, K, 5, (case, K, B, rule))
        print("%s K=%d B=%d %s: converged %d from start 0, %d with the best of %d; max |sqrt(err_sq) - ||e||| = %.3g"
              % (data.kernel, K, B, rule, int(singles[0][1].sum()), int(got[1].sum()), K, worst))
        if rule is NEVER:
            assert not got[1].any()
        elif B >= 130:
            assert got[1].sum() > singles[0][1].sum() and (got[3] > 0).any() and (got[3] == 0).any()


def _fallback_problem(torch, kind, B):
    import ik_amd
    if kind == "tree":
        from test_gpu_generic import build
        full_body = [("frame", "LeftFootFront", "universe", 2, 0, None), ("frame", "RightFootFront", "universe", 2, 0, None),
                     ("frame", "pelvis", "universe", 2, 0, None)]
        with env(IKGPU_TREE_STATIC_ROWS="0"):
            ik, O, model, problem, data, om, ot, q0, tg = build("cassie", True, full_body, B, seed=0)
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        TG = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
        return problem, data, Q0, TG, None
    model, problem, data, _, _ = _problem(CASES[0])
    Q0, TG = _workload(torch, CASES[0], B)
    return problem, data, Q0, TG, (ik_amd.inverse_kinematics_visitor(1e-4, step_tolerance=1e-3) if kind == "derived_visitor" else None)


@pytest.mark.parametrize("kind,K", [("chain", 1), ("chain", 3), ("tree", 4), ("derived_visitor", 4)])
def test_other_cases_run_the_definition_inside_the_call(torch_cuda, kind, K):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    B = 130
    problem, data, Q0, TG, visitor = _fallback_problem(torch, kind, B)
    rules = [(30, 1e-4)] if kind == "derived_visitor" else [(30, 1e-4), NEVER]
    for rule in rules:
        v, p = _visitor(ik_amd, rule)
        v = visitor or v
        assert ik_amd.dls_multistart_kernel(data, v, p, K) == "loop(%s)" % data.kernel
        got, singles, worst = _check_call(torch, ik_amd, problem, data, Q0, TG, rule, K, 9, (kind, K, rule), visitor=visitor)
        assert np.isfinite(got[0]).all()
        if K == 1:
            assert (got[3] == 0).all()
        # a workspace one byte short is refused, with a message
        prm = api._params(v, p)
        L = capi.lib()
        need = L.ikgpu_dls_multistart_workspace_bytes(data._h, B, K, C.byref(prm))
        assert need > 0
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        Q = torch.empty_like(Q0)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.ikgpu_dls_multistart_batch(data._h, B, K, Q0.data_ptr(), None, 9, TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, None, None, capi.SOA,
                                          ws.data_ptr(), need - 1, s)
        assert rc == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
        # ... and the exact size works, without the optional arrays
        capi.check(L.ikgpu_dls_multistart_batch(data._h, B, K, Q0.data_ptr(), None, 9, TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, None, None,
                                                capi.SOA, ws.data_ptr(), need, s))
        assert np.array_equal(Q.t().cpu().numpy(), got[0]), (kind, K, rule)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_multistart_without_the_optional_arrays(torch_cuda, case):
    """success, iters, winner and err_sq NULL, straight through the C ABI (the Python entry always passes them)."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, K = 130, 8
    Q0, TG = _workload(torch, case, B)
    L = capi.lib()
    for rule in (STOP, NEVER):
        v, p = _visitor(ik_amd, rule)
        ref = _run(ik_amd, problem, data, Q0, TG, v, p, K, 5, None, "soa")
        prm = api._params(v, p)
        assert L.ikgpu_dls_multistart_workspace_bytes(data._h, B, K, C.byref(prm)) == 0
        Q = torch.full((model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capi.check(L.ikgpu_dls_multistart_batch(data._h, B, K, Q0.data_ptr(), None, 5, TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, None, None,
                                                capi.SOA, None, 0, s))
        assert np.array_equal(Q.t().cpu().numpy(), ref[0]), (case, rule)
        # ... and only some of them
        it = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        err = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
        capi.check(L.ikgpu_dls_multistart_batch(data._h, B, K, Q0.data_ptr(), None, 5, TG.data_ptr(), C.byref(prm), Q.data_ptr(), None, it.data_ptr(), None,
                                                err.data_ptr(), capi.SOA, None, 0, s))
        assert np.array_equal(Q.t().cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[2]) and np.array_equal(err.cpu().numpy(), ref[4])


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_multistart_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist and no allocation: captured on a side stream (outputs preallocated through
    out=) and replayed twice it gives the eager call's bits."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, K = 4097, 8
    Q0, TG = _workload(torch, case, B)
    v, p = _visitor(ik_amd, STOP)
    assert ik_amd.dls_multistart_kernel(data, v, p, K) == _expected_name(data)
    eager = [x.clone() for x in ik_amd.dls_multistart_batch(problem, Q0, TG, data, v, p, num_starts=K, seed=5)]
    out = tuple(torch.empty_like(x) for x in eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_multistart_batch(problem, Q0, TG, data, v, p, num_starts=K, seed=5, out=out)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_multistart_batch(problem, Q0, TG, data, v, p, num_starts=K, seed=5, out=out)
    for _ in range(2):
        out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7), out[3].fill_(-7), out[4].fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y), case


def test_more_starts_solve_more_uniform_targets(torch_cuda):
    """arm7, 512 uniform targets from uniform starts, default parameters.  Start 0 is shared, so eight starts never solve fewer problems
    than one; the oracle measured 209 -> 467 of 512 (2.2 x) with eight uniform starts, and 1.5 x leaves room for another draw of starts
    while it still fails if the restarts do nothing."""
    torch = torch_cuda
    import ik_amd
    case = CASES[4]
    model, problem, data, _, _ = _problem(case)
    Q0, TG = _workload(torch, case, 512)
    one = ik_amd.dls_multistart_batch(problem, Q0, TG, data, num_starts=1)
    ref = ik_amd.dls_batch(problem, Q0, TG, data)
    assert torch.equal(one[0], ref[0]) and torch.equal(one[1], ref[1]) and torch.equal(one[2], ref[2]) and int(one[3].abs().sum()) == 0
    eight = ik_amd.dls_multistart_batch(problem, Q0, TG, data, num_starts=8)
    n1, n8 = int(one[1].sum()), int(eight[1].sum())
    print("arm7, B = 512, uniform targets and starts: %d converge from one start, %d with the best of eight" % (n1, n8))
    assert n8 >= n1 and (eight[1] >= one[1]).all()
    assert n8 >= 1.5 * n1, (n1, n8)
