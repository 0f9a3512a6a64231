"""ikgpu_dls_pick_batch on the device: among K starts per problem, the one that met the stop rule with the smallest cost under one of
four rules (distance to a reference configuration, its max-norm, margin to the joint limits, manipulability).  The call is DEFINED
through K single solves (include/ikgpu.h), so the reference here is K calls of ik_amd.dls_batch from the columns of
ik_amd.multistart_starts, with the cost recomputed in numpy on those results (J and e from ik_amd.evaluate_batch, which the header names
as the Jacobian's definition), and the assertions are tests/pick_common.py check_pick's: q / success / iterations are the single
solve's from start winner[b] by np.array_equal; the winner attains the minimal key (problems whose two best reference keys differ by
less than 1e-12 relative without being equal are left out, at most 2 %; an exact tie must go to the lower index); cost[b] is the recomputation within 1e-12 relative (MANIPULABILITY: within
8 kappa(G) 2^-53).  B = 130 with K in {2, 8, 64}: whole waves, a tail group and a shadow of the last problem; B = 1 with K = 8."""
import ctypes as C

import numpy as np
import pytest

from conftest import urdf_path
import multistart_common as MC
import pick_common as PK
from test_gpu_multistart import env, _fallback_problem

pytestmark = pytest.mark.gpu

STOP = (100, 1e-4)
DAMPING = 1e-2


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# (model, frame, task type, build): the builds of the chain kernel
CASES = [
    ("ur5", "tool0", 2, "default"),                    # hot
    ("cassie_fixed", "LeftFootFront", 2, "default"),   # hot, entries outside the chain
    ("arm7", "tool", 2, "default"),                    # hot-rtc (general when hipRTC is absent)
    ("ur5", "tool0", 0, "default"),                    # a Position task: general
    ("ur5_rail", "tool0", 2, "default"),               # a prismatic joint: hot-rtc with the joint-kind mask
    ("ur5_rail", "tool0", 2, "general"),               # ... and the general build that reads it
]
_cache = {}


def _problem(case):
    import ik_amd
    import prismatic_common as PC
    if case not in _cache:
        name, frame, ktype, build = case
        model = ik_amd.Model.from_urdf_xml(PC.robot_xml(name).encode()) if name == "ur5_rail" else ik_amd.Model.from_urdf_file(urdf_path(name))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType(ktype)))
        with env(IKGPU_CHAIN_HOT="0" if build == "general" else None):
            data = ik_amd.dls_data(problem, device=0)
        pose = ik_amd.InverseKinematicsProblem(model)
        pose.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        _cache[case] = (model, problem, data, pose, ik_amd.dls_data(pose, device=0))
    return _cache[case]


def _workload(torch, case, B, K):
    """SoA on the device: start [nq, B], targets [1, 12, B], q_ref [nq, B]; the weights [nq] (host); the caller's starts [K-1, nq, B] or
    None: generated (tests/pick_common.py workload)."""
    import ik_amd
    key = (case[0], case[1], B, K)
    if key not in _cache:
        model, problem, data, pose, pose_data = _problem(case)
        q0, qt, near = PK.workload(model, case[0], B, K)
        tg = ik_amd.task_frames_fk_batch(pose, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), pose_data)
        rng = np.random.default_rng(11)
        q_ref = rng.uniform(np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit), (B, model.nq))
        _cache[key] = (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), tg, torch.from_numpy(np.ascontiguousarray(q_ref.T)).cuda(),
                       rng.uniform(0.25, 2.0, model.nq), None if near is None else torch.from_numpy(np.ascontiguousarray(near.transpose(0, 2, 1))).cuda())
    return _cache[key]


def _vp(ik_amd, rule=STOP):
    return ik_amd.inverse_kinematics_visitor(rule[1]), ik_amd.dls_parameters(max_iterations=rule[0], damping=DAMPING)


def _device_evaluation(torch, ik_amd, problem, data, TG):
    def evaluate(q):                                          # q [B, nq] -> e [B, M], J [B, M, nv]
        e, J = ik_amd.evaluate_batch(problem, torch.from_numpy(np.ascontiguousarray(q.T)).cuda(), TG, data)
        return e.t().cpu().numpy(), J.permute(2, 0, 1).cpu().numpy()
    return evaluate


def _reference(torch, ik_amd, problem, data, Q0, gen, TG, QR, w, v, p):
    """The definition: the single solve from every start, and every rule's cost at its result."""
    singles = []
    for k in range(gen.shape[0] + 1):
        q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], TG, data, v, p)
        singles.append((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()))
    model = problem.model()
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    refs, err = PK.all_reference_costs(_device_evaluation(torch, ik_amd, problem, data, TG), singles, np.asarray(data.support, bool), lo, hi,
                                       QR.t().cpu().numpy(), np.asarray(w, float), DAMPING)
    return singles, refs, err


def _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, QR, w, seed, starts=None, layout="soa", out=None):
    """One pick call in `layout` from SoA inputs; AoS numpy views back."""
    if layout == "aos":
        Q0, TG = Q0.t().contiguous(), TG.permute(2, 0, 1).contiguous()
        QR = None if QR is None else QR.t().contiguous()
        starts = None if starts is None else starts.permute(0, 2, 1).contiguous()
    Q, ok, it, win, cost, err = ik_amd.dls_pick_batch(problem, Q0, TG, data, v, p, num_starts=K, rule=rule, q_ref=QR, weights=w, seed=seed, starts=starts,
                                                      layout=layout, out=out)
    q = Q.cpu().numpy()
    return (q.T if layout == "soa" else q), ok.cpu().numpy(), it.cpu().numpy(), win.cpu().numpy(), cost.cpu().numpy(), err.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_pick" + data.kernel[len("dls_chain"):]


def _check_all_rules(torch, ik_amd, problem, data, Q0, TG, QR, w, v, p, K, seed, label, ways=True, near=None):
    """near: the caller's starts of the main call, or None: generated from `seed`."""
    gen = ik_amd.multistart_starts(data, Q0, K, seed) if near is None else near
    singles, refs, err = _reference(torch, ik_amd, problem, data, Q0, gen, TG, QR, w, v, p)
    counts = {}
    for rule in PK.RULES:
        got = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, QR, w, seed, near)
        counts[rule] = PK.check_pick(got, singles, rule, refs[rule][0], refs[rule][1], err, label + (PK.RULE_NAMES[rule],))
        print("%s %s K=%d B=%d %-14s: %d problems with >= 2 converged starts, winner not the first converged one in %d, left out %d"
              % ((data.kernel, label, K, Q0.shape[1], PK.RULE_NAMES[rule]) + counts[rule]))
        for starts, layout in ([(near, "aos")] + ([(gen, "soa")] if K > 1 else []) if ways else []):
            again = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, QR, w, seed, starts, layout)
            for x, y, what in zip(again, got, ("q", "success", "iterations", "winner", "cost", "err_sq")):
                assert np.array_equal(x, y), (label, rule, layout, starts is None, what)
    return singles, counts


@pytest.mark.parametrize("K,B", [(2, 130), (8, 130), (64, 130), (8, 1)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_pick_returns_the_cheapest_converged_single_solve(torch_cuda, case, K, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[0] in ("ur5", "cassie_fixed") and case[2] == 2:
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, TG, QR, w, near = _workload(torch, case, B, K)
    v, p = _vp(ik_amd)
    for rule in PK.RULES:
        assert ik_amd.dls_pick_kernel(data, v, p, K, rule) == _expected_name(data)
    singles, counts = _check_all_rules(torch, ik_amd, problem, data, Q0, TG, QR, w, v, p, K, PK.DRAW_SEED[(case[0], case[2])], (case, K, B), near=near)
    if case[:3] == ("ur5", "tool0", 2) and K == 8 and B == 130:     # not vacuous: the rule has something to choose from, and chooses
        for rule in PK.RULES:
            assert counts[rule][0] >= B / 2 and counts[rule][1] >= B / 5, (rule, counts[rule])


@pytest.mark.parametrize("kind,K", [("chain", 1), ("chain", 3), ("tree", 4), ("derived_visitor", 4)])
def test_other_cases_run_the_definition_inside_the_call(torch_cuda, kind, K):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    B = 130
    problem, data, Q0, TG, visitor = _fallback_problem(torch, kind, B)
    v, p = ik_amd.inverse_kinematics_visitor(1e-4), ik_amd.dls_parameters(max_iterations=30, damping=DAMPING)
    v = visitor or v
    rng = np.random.default_rng(11)
    QR = Q0 + torch.from_numpy(rng.normal(0.0, 0.3, tuple(Q0.shape))).cuda()
    w = rng.uniform(0.25, 2.0, Q0.shape[0])
    for rule in PK.RULES:
        assert ik_amd.dls_pick_kernel(data, v, p, K, rule) == "loop(%s)" % data.kernel
    singles, counts = _check_all_rules(torch, ik_amd, problem, data, Q0, TG, QR, w, v, p, K, 9, (kind, K), ways=kind != "tree")
    # a workspace one byte short is refused, with a message; the exact size works, without the optional arrays
    prm = api._params(v, p)
    L = capi.lib()
    need = L.ikgpu_dls_pick_workspace_bytes(data._h, B, K, C.byref(prm))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    Q = torch.empty_like(Q0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wc = (C.c_double * len(w))(*w)
    args = (data._h, B, K, Q0.data_ptr(), None, 9, TG.data_ptr(), C.byref(prm), PK.DISTANCE, QR.data_ptr(), wc, Q.data_ptr(), None, None, None, None, None, capi.SOA)
    assert L.ikgpu_dls_pick_batch(*args, ws.data_ptr(), need - 1, s) == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
    assert L.ikgpu_dls_pick_batch(*args, None, need, s) == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
    capi.check(L.ikgpu_dls_pick_batch(*args, ws.data_ptr(), need, s))
    ref = _run(ik_amd, problem, data, Q0, TG, v, p, K, PK.DISTANCE, QR, w, 9)
    assert np.array_equal(Q.t().cpu().numpy(), ref[0]), (kind, K)
    # q_ref = NULL is q0, w = NULL is ones
    a = _run(ik_amd, problem, data, Q0, TG, v, p, K, PK.DISTANCE, None, None, 9)
    b = _run(ik_amd, problem, data, Q0, TG, v, p, K, PK.DISTANCE, Q0, np.ones(Q0.shape[0]), 9)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), (kind, K)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[3]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_pick_optional_arguments_and_refusals(torch_cuda, case):
    """success, iters, winner, cost and err_sq NULL straight through the C ABI; q_ref = NULL equals q_ref = q0 and w = NULL equals ones,
    bit for bit; a negative or non-finite weight is refused; every start equal to q0 under DISTANCE from q0 is the multi-start call."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, K = 130, 8
    Q0, TG, QR, w, _ = _workload(torch, case, B, K)
    v, p = _vp(ik_amd)
    prm = api._params(v, p)
    L = capi.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.ikgpu_dls_pick_workspace_bytes(data._h, B, K, C.byref(prm)) == 0
    wc = (C.c_double * model.nq)(*w)
    for rule in PK.RULES:
        ref = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, QR, w, 5)
        Q = torch.full((model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
        head = (data._h, B, K, Q0.data_ptr(), None, 5, TG.data_ptr(), C.byref(prm), rule, QR.data_ptr(), wc, Q.data_ptr())
        capi.check(L.ikgpu_dls_pick_batch(*head, None, None, None, None, None, capi.SOA, None, 0, s))
        assert np.array_equal(Q.t().cpu().numpy(), ref[0]), (case, rule)
        # ... and only some of them
        it = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        cost = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
        capi.check(L.ikgpu_dls_pick_batch(*head, None, it.data_ptr(), None, cost.data_ptr(), None, capi.SOA, None, 0, s))
        assert np.array_equal(Q.t().cpu().numpy(), ref[0]) and np.array_equal(it.cpu().numpy(), ref[2]) and np.array_equal(cost.cpu().numpy(), ref[4])
    for rule in (PK.DISTANCE, PK.MAX_DISTANCE):
        a = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, None, None, 5)
        b = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, Q0, np.ones(model.nq), 5)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (case, rule)
        weighted = _run(ik_amd, problem, data, Q0, TG, v, p, K, rule, None, w, 5)
        assert not np.array_equal(weighted[4], a[4])                 # the weights reach the kernel
    # refusals that need a problem: a weight that is negative or not finite
    Q = torch.empty_like(Q0)
    for bad in (-1.0, float("nan"), float("inf")):
        wb = (C.c_double * model.nq)(*w)
        wb[model.nq - 1] = bad
        rc = L.ikgpu_dls_pick_batch(data._h, B, K, Q0.data_ptr(), None, 5, TG.data_ptr(), C.byref(prm), PK.DISTANCE, None, wb, Q.data_ptr(), None, None, None,
                                    None, None, capi.SOA, None, 0, s)
        assert rc == capi.ERR_INVALID and "w[" in L.ikgpu_last_error().decode(), bad
    # every start equal to q0, DISTANCE from q0: every key of a group ties, the lowest index wins -- the multi-start call's result
    same = Q0.unsqueeze(0).repeat(K - 1, 1, 1).contiguous()
    tie = _run(ik_amd, problem, data, Q0, TG, v, p, K, PK.DISTANCE, None, None, 5, starts=same)
    ms = ik_amd.dls_multistart_batch(problem, Q0, TG, data, v, p, num_starts=K, seed=5, starts=same)
    assert np.array_equal(tie[0], ms[0].t().cpu().numpy()) and np.array_equal(tie[1], ms[1].cpu().numpy()) and np.array_equal(tie[2], ms[2].cpu().numpy())
    assert np.array_equal(tie[3], ms[3].cpu().numpy()) and (tie[3] == 0).all() and np.array_equal(tie[5], ms[4].cpu().numpy())


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_pick_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist and no allocation: captured on a side stream (outputs preallocated through
    out=) and replayed twice it gives the eager call's bits."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, K = 130, 8
    Q0, TG, QR, w, _ = _workload(torch, case, B, K)
    v, p = _vp(ik_amd)
    for rule in (PK.DISTANCE, PK.MANIPULABILITY):
        assert ik_amd.dls_pick_kernel(data, v, p, K, rule) == _expected_name(data)
        call = lambda out=None: ik_amd.dls_pick_batch(problem, Q0, TG, data, v, p, num_starts=K, rule=rule, q_ref=QR, weights=w, seed=5, out=out)
        eager = [x.clone() for x in call()]
        out = tuple(torch.empty_like(x) for x in eager)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(out)                                                # (warm-up outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call(out)
        for _ in range(2):
            out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7), out[3].fill_(-7), out[4].fill_(float("nan")), out[5].fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for x, y in zip(out, eager):
                assert torch.equal(x, y), (case, rule)
