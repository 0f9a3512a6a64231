"""ikgpu_dls_goalset_batch on the device: any of G alternative goals per problem from K starts.  The call is DEFINED through G x K single
solves (include/ikgpu.h), so the reference here is G x K calls of ik_amd.dls_batch -- start k (a column of ik_amd.multistart_starts)
against goal g -- with the errors from evaluate_batch(jacobian=False), and the assertions are tests/goalset_common.py check_goalset's:
q / success / iterations are candidate goal K + start's single solve by np.array_equal; that candidate has the minimal key; err_sq is its
error to 5e-11 in the norm; reachable[g] is exactly "some start of goal g met the stop rule".  For every build of the chain kernel (one
launch: dls_chain_goalset<...>), group sizes 2 / 8 / 16 / 64 with batch sizes that leave a partial last wave, put one problem in a wave
and cross a wave boundary, both layouts, both rules, generated and caller's starts, with and without the optional arrays; through the
loop of existing launches for G or K not a power of two, a tree problem and a derived visitor; and under a captured graph.

A candidate's single solve depends on (problem, B, rule, g, k) only -- the starts are a function of (seed, b, k) and goal g of a problem
is drawn from seed + 1000 g -- so every shape of one batch size shares one table of single solves."""
import ctypes as C

import numpy as np
import pytest

import goalset_common as GC
from test_gpu_multistart import NEVER, STOP, _norms, _problem, _visitor, env

pytestmark = pytest.mark.gpu

CASES = [
    ("ur5", "tool0", 2, "default"),                    # hot
    ("arm7", "tool", 2, "default"),                    # hot-rtc (general when hipRTC is absent)
    ("cassie_fixed", "LeftFootFront", 0, "default"),   # a Position task: general
    ("ur5", "tool0", 2, "general"),                    # IKGPU_CHAIN_HOT=0
]
BATCHES = [1, 3, 33, 63, 64, 65, 130, 4097]
SHAPES = [(2, 1), (4, 2), (2, 8), (64, 1), (8, 8)]
SEED = 5
_ids = lambda c: "%s-%s-%d-%s" % c
_goals, _singles = {}, {}


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _workload(torch, case, B, G):
    """(start [nq, B], goals [G, 1, 12, B]) on the device, SoA: uniform between the limits (tests/goalset_common.py).  Goal g of a
    problem does not depend on G."""
    import ik_amd
    model, problem, data, pose, pose_data = _problem(case)
    key = (case[0], case[1], B)
    if key not in _goals:
        _goals[key] = (torch.from_numpy(np.ascontiguousarray(GC.goal_configurations(model, B, 1, 0)[0].T)).cuda(), [])
    Q0, slabs = _goals[key]
    for g in range(len(slabs), G):
        qt = GC.MC.uniform_configurations(model, B, 1000 * g)[1]   # (goal g of goalset_common.goal_configurations(model, B, G, 0))
        slabs.append(ik_amd.task_frames_fk_batch(pose, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), pose_data))
    return Q0, torch.stack(slabs[:G]).contiguous()


def _reference(ik_amd, key, problem, data, Q0, gen, GL, v, p, K):
    """The definition: the single solve of every candidate (SoA) and the error at its result, j = g K + k.  Cached under `key`."""
    singles, errs = [], []
    for g in range(GL.shape[0]):
        for k in range(K):
            at = None if key is None else key + (g, k)
            if at is None or at not in _singles:
                q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], GL[g], data, v, p)
                res = ((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()), _norms(ik_amd, problem, data, q, GL[g]) ** 2)
                if at is None:
                    singles.append(res[0]), errs.append(res[1])
                    continue
                _singles[at] = res
            singles.append(_singles[at][0]), errs.append(_singles[at][1])
    return singles, errs


def _run(ik_amd, problem, data, Q0, GL, v, p, K, seed, starts, layout, out=None):
    """One goal-set call in `layout` from SoA inputs; AoS numpy views back."""
    if layout == "aos":
        Q0, GL = Q0.t().contiguous(), GL.permute(0, 3, 1, 2).contiguous()
        starts = None if starts is None else starts.permute(0, 2, 1).contiguous()
    res = ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=seed, starts=starts, layout=layout, out=out)
    q = res[0].cpu().numpy()
    return ((q.T if layout == "soa" else q),) + tuple(x.cpu().numpy() for x in res[1:])


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_goalset" + data.kernel[len("dls_chain"):]


def _check_call(torch, ik_amd, problem, data, Q0, GL, rule, K, label, visitor=None, key=None):
    """Every way to make the call against the definition; returns the SoA-generated result."""
    v, p = _visitor(ik_amd, rule)
    v = visitor or v
    G, B = GL.shape[0], Q0.shape[1]
    gen = ik_amd.multistart_starts(data, Q0, K, SEED)
    singles, errs = _reference(ik_amd, key, problem, data, Q0, gen, GL, v, p, K)
    got = _run(ik_amd, problem, data, Q0, GL, v, p, K, SEED, None, "soa")
    won = GL[torch.from_numpy(got[3].astype(np.int64)).cuda(), :, :, torch.arange(B, device="cuda")].permute(1, 2, 0).contiguous()   # [ntasks, 12, B]
    at_result = _norms(ik_amd, problem, data, torch.from_numpy(np.ascontiguousarray(got[0].T)).cuda(), won)
    worst = GC.check_goalset(got, singles, errs, at_result, K, label)
    for starts, layout in [(None, "aos")] + ([(gen, "soa")] if K > 1 else []):
        again = _run(ik_amd, problem, data, Q0, GL, v, p, K, SEED, starts, layout)
        for x, y, what in zip(again, got, ("q", "success", "iterations", "goal", "start", "err_sq", "reachable")):
            assert np.array_equal(x, y), (label, layout, starts is None, what)
    return got, singles, worst


@pytest.mark.parametrize("G,K", SHAPES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_goalset_returns_the_best_candidate(torch_cuda, case, B, G, K):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case == CASES[0]:
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, GL = _workload(torch, case, B, G)
    for rule in (STOP, NEVER):
        v, p = _visitor(ik_amd, rule)
        assert ik_amd.dls_goalset_kernel(data, v, p, G, K) == _expected_name(data)
        got, singles, worst = _check_call(torch, ik_amd, problem, data, Q0, GL, rule, K, (case, B, G, K, rule), key=(case, B, rule))
        print("%s G=%d K=%d B=%d %s: %d reached a goal, goals %s; max |sqrt(err_sq) - ||e||| = %.3g"
              % (data.kernel, G, K, B, rule, int(got[1].sum()), np.bincount(got[3], minlength=G)[:8].tolist(), worst))
        if rule is NEVER:
            assert not got[1].any() and not got[6].any()
        elif B >= 130 and case[2] == 2:
            assert got[1].sum() >= singles[0][1].sum() and (got[3] > 0).any() and (got[3] == 0).any() and (got[6] == 0).any() and (got[6] == 1).any()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_one_goal_is_the_multistart_call(torch_cuda, case):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, K = 130, 8
    Q0, GL = _workload(torch, case, B, 1)
    for rule in (STOP, NEVER):
        v, p = _visitor(ik_amd, rule)
        assert ik_amd.dls_goalset_kernel(data, v, p, 1, K) == _expected_name(data)
        got = ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=SEED)
        ms = ik_amd.dls_multistart_batch(problem, Q0, GL[0], data, v, p, num_starts=K, seed=SEED)
        for x, y, what in zip(ms, (got[0], got[1], got[2], got[4], got[5]), ("q", "success", "iterations", "winner", "err_sq")):
            assert torch.equal(x, y), (case, rule, what)
        assert not got[3].any() and torch.equal(got[6][0], got[1])


def _fallback_problem(torch, kind, B, G):
    import ik_amd
    if kind == "tree":
        from test_gpu_track import FULL_BODY, _fallback_trajectory
        ik, problem, data, Q0, TG = _fallback_trajectory(torch, "cassie", True, FULL_BODY, B, G, rows="0")   # G target sets: [G, 3, 12, B]
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
        return problem, data, Q0, TG, None
    case = ("cassie_fixed", "LeftFootFront", 2, "default")
    model, problem, data, _, _ = _problem(case)
    Q0, GL = _workload(torch, case, B, G)
    return problem, data, Q0, GL, (ik_amd.inverse_kinematics_visitor(1e-4, step_tolerance=1e-3) if kind == "derived_visitor" else None)


@pytest.mark.parametrize("kind,G,K", [("chain", 3, 1), ("chain", 4, 3), ("chain", 1, 1), ("derived_visitor", 2, 2), ("tree", 2, 2)])
def test_other_cases_run_the_definition_inside_the_call(torch_cuda, kind, G, K):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    B = 130
    problem, data, Q0, GL, visitor = _fallback_problem(torch, kind, B, G)
    rules = [(30, 1e-4)] if kind == "derived_visitor" else [(30, 1e-4), NEVER]
    for rule in rules:
        v, p = _visitor(ik_amd, rule)
        v = visitor or v
        assert ik_amd.dls_goalset_kernel(data, v, p, G, K) == "loop(%s)" % data.kernel
        got, singles, worst = _check_call(torch, ik_amd, problem, data, Q0, GL, rule, K, (kind, G, K, rule), visitor=visitor)
        assert np.isfinite(got[0]).all()
        if rule is NEVER:
            assert not got[6].any()
        # a workspace one byte short is refused, with a message, and so is none at all
        prm = api._params(v, p)
        L = capi.lib()
        need = L.ikgpu_dls_goalset_workspace_bytes(data._h, B, G, K, C.byref(prm))
        assert need > 0
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        Q = torch.empty_like(Q0)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda w, n, *opt: L.ikgpu_dls_goalset_batch(data._h, B, G, K, Q0.data_ptr(), None, SEED, GL.data_ptr(), C.byref(prm), Q.data_ptr(),
                                                            *(opt or (None,) * 6), capi.SOA, w, n, s)
        assert call(ws.data_ptr(), need - 1) == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
        assert call(None, need) == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
        # ... and the exact size works, without the optional arrays, and with `start` alone (the loop keeps its winner there)
        capi.check(call(ws.data_ptr(), need))
        assert np.array_equal(Q.t().cpu().numpy(), got[0]), (kind, G, K, rule)
        st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        capi.check(call(ws.data_ptr(), need, None, None, None, st.data_ptr(), None, None))
        assert np.array_equal(Q.t().cpu().numpy(), got[0]) and np.array_equal(st.cpu().numpy(), got[4]), (kind, G, K, rule)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_goalset_without_the_optional_arrays(torch_cuda, case):
    """Every optional output NULL, and each one alone, straight through the C ABI (the Python entry always passes them); the outputs lie
    inside larger sentinel-filled buffers: all of [B] and [G][B] is overwritten and nothing beyond."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, G, K = 65, 4, 2
    Q0, GL = _workload(torch, case, B, G)
    L = capi.lib()
    PAD = 64
    kinds = [(torch.uint8, 1, 7), (torch.int32, 1, -7), (torch.int32, 1, -7), (torch.int32, 1, -7), (torch.float64, 1, float("nan")), (torch.uint8, G, 7)]
    names = ("success", "iterations", "goal", "start", "err_sq", "reachable")
    for rule in (STOP, NEVER):
        v, p = _visitor(ik_amd, rule)
        ref = ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=SEED)
        prm = api._params(v, p)
        assert L.ikgpu_dls_goalset_workspace_bytes(data._h, B, G, K, C.byref(prm)) == 0
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for only in (None, 0, 1, 2, 3, 4, 5):
            Q = torch.full((PAD + model.nq * B + PAD,), float("nan"), dtype=torch.float64, device="cuda")
            bufs = [torch.full((PAD + n * B + PAD,), fill, dtype=dt, device="cuda") for dt, n, fill in kinds]
            ptr = lambda t: t.data_ptr() + PAD * t.element_size()
            opt = [ptr(b) if only == i else None for i, b in enumerate(bufs)]
            capi.check(L.ikgpu_dls_goalset_batch(data._h, B, G, K, Q0.data_ptr(), None, SEED, GL.data_ptr(), C.byref(prm), ptr(Q), *opt, capi.SOA, None, 0, s))
            torch.cuda.synchronize()
            assert torch.equal(Q[PAD:-PAD].view(model.nq, B), ref[0]) and torch.isnan(Q[:PAD]).all() and torch.isnan(Q[-PAD:]).all(), (case, rule, only)
            for i, (b, (dt, n, fill)) in enumerate(zip(bufs, kinds)):
                untouched = (lambda x: torch.isnan(x).all()) if dt == torch.float64 else (lambda x: (x == fill).all())
                assert untouched(b[:PAD]) and untouched(b[-PAD:]), (case, rule, only, names[i])
                if only == i:
                    assert torch.equal(b[PAD:-PAD].view(ref[1 + i].shape), ref[1 + i]), (case, rule, names[i])
                else:
                    assert untouched(b), (case, rule, only, names[i])


@pytest.mark.parametrize("case", CASES[:3], ids=_ids)
def test_goalset_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist and no allocation: captured on a side stream (outputs preallocated through
    out=) and replayed twice it gives the eager call's bits."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, G, K = 4097, 4, 2
    Q0, GL = _workload(torch, case, B, G)
    v, p = _visitor(ik_amd, STOP)
    assert ik_amd.dls_goalset_kernel(data, v, p, G, K) == _expected_name(data)
    eager = [x.clone() for x in ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=SEED)]
    out = tuple(torch.empty_like(x) for x in eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=SEED, out=out)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_goalset_batch(problem, Q0, GL, data, v, p, num_starts=K, seed=SEED, out=out)
    for _ in range(2):
        out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7), out[3].fill_(-7), out[4].fill_(-7), out[5].fill_(float("nan")), out[6].fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y), case
