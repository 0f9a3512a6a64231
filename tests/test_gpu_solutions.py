"""ikgpu_dls_solutions_batch on the device: the distinct converged starts among K starts per problem, up to N of them.  The call is
DEFINED through K single solves and a greedy rule over their results (include/ikgpu.h), so the reference here is K calls of
ik_amd.dls_batch from the columns of ik_amd.multistart_starts with the rule restated in numpy (tests/solutions_common.py), and the
assertions are: count and which are equal; every written slab is the single solve from which[n][b] by np.array_equal over all nq entries;
unwritten slots keep their prefill.  For every build of the chain kernel (one launch: dls_chain_solutions<...>) with the shapes at which
the lane mapping can go wrong, N in {1, 3, K}, both layouts, generated and caller's starts, with and without the optional arrays;
through the loop of existing launches for K = 1, K = 6, a tree problem and a derived visitor; and under a captured graph."""
import ctypes as C

import numpy as np
import pytest

import solutions_common as SC
from test_gpu_multistart import CASES, _fallback_problem, _problem, _visitor, _workload

pytestmark = pytest.mark.gpu

STOP = (100, 1e-4)
SEED = 5
SEP = {"ur5": 0.1, "cassie_fixed": 0.5, "arm7": 0.5, "cassie": 0.5}


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_references = {}


def _reference(ik_amd, key, problem, data, Q0, TG, v, p, K):
    """The definition's K single solves (SoA), computed once per workload and shared: (generated starts, singles, support)."""
    if key not in _references:
        gen = ik_amd.multistart_starts(data, Q0, K, SEED)
        singles = []
        for k in range(K):
            q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], TG, data, v, p)
            singles.append((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()))
        _references[key] = (gen, singles, np.asarray(data.support, dtype=bool))
    return _references[key]


def _prefilled(torch, N, q_shape, B):
    return (torch.full((N,) + tuple(q_shape), SC.NAN_FILL, dtype=torch.float64, device="cuda"),
            torch.full((B,), SC.INT_FILL, dtype=torch.int32, device="cuda"),
            torch.full((N, B), SC.INT_FILL, dtype=torch.int32, device="cuda"),
            torch.full((N, B), SC.INT_FILL, dtype=torch.int32, device="cuda"))


def _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, starts, layout):
    """One call in `layout` from SoA inputs into prefilled outputs; AoS numpy views back: (Q [N, B, nq], count, which, iters)."""
    if layout == "aos":
        Q0, TG = Q0.t().contiguous(), TG.permute(2, 0, 1).contiguous()
        starts = None if starts is None else starts.permute(0, 2, 1).contiguous()
    B = Q0.shape[1] if layout == "soa" else Q0.shape[0]
    out = _prefilled(torch, N, Q0.shape, B)
    Q, count, which, it = ik_amd.dls_solutions_batch(problem, Q0, TG, data, v, p, num_starts=K, max_solutions=N, separation=sep, seed=SEED,
                                                     starts=starts, layout=layout, out=out)
    q = Q.cpu().numpy()
    return (q.transpose(0, 2, 1) if layout == "soa" else q), count.cpu().numpy(), which.cpu().numpy(), it.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_solutions" + data.kernel[len("dls_chain"):]


# B x K: one live group with seven shadow groups in its wave; across a wave; group = wave; K = 2; the grid
SHAPES = [(8, 1), (8, 9), (64, 1), (64, 2), (2, 33), (8, 4097)]


@pytest.mark.parametrize("K,B", SHAPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_solutions_are_the_greedy_set_of_single_solves(torch_cuda, case, K, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, TG = _workload(torch, case, B)
    v, p = _visitor(ik_amd, STOP)
    assert ik_amd.dls_solutions_kernel(data, v, p, K) == _expected_name(data)
    gen, singles, support = _reference(ik_amd, (case, K, B), problem, data, Q0, TG, v, p, K)
    sep = SEP[case[0]]
    for N in sorted({1, min(3, K), K}):
        got = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, None, "soa")
        count, which = SC.check_set(got, singles, support, sep, N, (case, K, B, N))
        for starts, layout in ((None, "aos"), (gen, "soa"), (gen, "aos")):
            again = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, starts, layout)
            for x, y, what in zip(again, got, ("q", "count", "which", "iterations")):
                assert np.array_equal(x, y, equal_nan=True), (case, K, B, N, layout, starts is None, what)
    if B >= 4097:
        print("%s K=%d B=%d sep=%g: problems by count %s" % (data.kernel, K, B, sep, np.bincount(count, minlength=K + 1).tolist()))
        assert (count >= 2).any() and (count <= 1).any()


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_solutions_without_the_optional_arrays(torch_cuda, case):
    """which and iters NULL, straight through the C ABI (the Python entry always passes them); caller's starts that differ from Q0
    outside the support; sep = 0."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, K, N = 130, 8, 3
    Q0, TG = _workload(torch, case, B)
    v, p = _visitor(ik_amd, STOP)
    sep = SEP[case[0]]
    gen, singles, support = _reference(ik_amd, (case, K, B), problem, data, Q0, TG, v, p, K)
    ref = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, None, "soa")
    SC.check_set(ref, singles, support, sep, N, (case, "python entry"))
    L = capi.lib()
    prm = api._params(v, p)
    assert L.ikgpu_dls_solutions_workspace_bytes(data._h, B, K, N, C.byref(prm)) == 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_which, with_iters in ((False, False), (True, False), (False, True)):
        Q, count, which, it = _prefilled(torch, N, Q0.shape, B)
        capi.check(L.ikgpu_dls_solutions_batch(data._h, B, K, N, Q0.data_ptr(), None, SEED, TG.data_ptr(), C.byref(prm), sep, Q.data_ptr(), count.data_ptr(),
                                               which.data_ptr() if with_which else None, it.data_ptr() if with_iters else None, capi.SOA, None, 0, s))
        got = (Q.cpu().numpy().transpose(0, 2, 1), count.cpu().numpy(), which.cpu().numpy() if with_which else None, it.cpu().numpy() if with_iters else None)
        SC.check_set(got, singles, support, sep, N, (case, with_which, with_iters))
        if not with_which:
            assert (which == SC.INT_FILL).all()
        if not with_iters:
            assert (it == SC.INT_FILL).all()
    # sep = 0: every converged start, up to N
    got = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, 0.0, None, "soa")
    SC.check_set(got, singles, support, 0.0, N, (case, "sep = 0"))
    assert np.array_equal(got[1], np.minimum(np.stack([x[1] for x in singles]).astype(bool).sum(axis=0), N))
    # the caller's starts with entries outside the support of their own (only the Cassie leg has such entries)
    if not support.all():
        outside = int(np.flatnonzero(~support)[-1])
        mine = gen.clone()
        mine[:, outside, :] += 0.01 * torch.arange(1, K, dtype=torch.float64, device="cuda")[:, None]
        own = []
        for k in range(K):
            q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else mine[k - 1], TG, data, v, p)
            own.append((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()))
        for layout in ("soa", "aos"):
            got = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, K, sep, mine, layout)
            count, which = SC.check_set(got, own, support, sep, K, (case, "own columns", layout))
            assert (which > 0).any()


@pytest.mark.parametrize("kind,K", [("chain", 1), ("chain", 6), ("tree", 4), ("derived_visitor", 4)])
def test_other_cases_run_the_definition_inside_the_call(torch_cuda, kind, K):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    B = 130
    problem, data, Q0, TG, visitor = _fallback_problem(torch, kind, B)
    v, p = _visitor(ik_amd, (30, 1e-4))
    v = visitor or v
    assert ik_amd.dls_solutions_kernel(data, v, p, K) == "loop(%s)" % data.kernel
    gen, singles, support = _reference(ik_amd, (kind, K, B), problem, data, Q0, TG, v, p, K)
    sep = 0.5
    for N in sorted({1, min(3, K), K}):
        got = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, None, "soa")
        count, which = SC.check_set(got, singles, support, sep, N, (kind, K, N))
        ways = [(None, "aos")] + ([(gen, "soa"), (gen, "aos")] if K > 1 else [])
        for starts, layout in ways:
            again = _run(torch, ik_amd, problem, data, Q0, TG, v, p, K, N, sep, starts, layout)
            for x, y, what in zip(again, got, ("q", "count", "which", "iterations")):
                assert np.array_equal(x, y, equal_nan=True), (kind, K, N, layout, starts is None, what)
    assert count.max() >= 1
    # a workspace one byte short is refused, with a message
    N = K
    prm = api._params(v, p)
    L = capi.lib()
    need = L.ikgpu_dls_solutions_workspace_bytes(data._h, B, K, N, C.byref(prm))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    Q, cnt, which, it = _prefilled(torch, N, Q0.shape, B)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.ikgpu_dls_solutions_batch(data._h, B, K, N, Q0.data_ptr(), None, SEED, TG.data_ptr(), C.byref(prm), sep, Q.data_ptr(), cnt.data_ptr(), None, None,
                                     capi.SOA, ws.data_ptr(), need - 1, s)
    assert rc == capi.ERR_INVALID and "workspace" in L.ikgpu_last_error().decode()
    # ... and the exact size works, without the optional arrays
    capi.check(L.ikgpu_dls_solutions_batch(data._h, B, K, N, Q0.data_ptr(), None, SEED, TG.data_ptr(), C.byref(prm), sep, Q.data_ptr(), cnt.data_ptr(), None,
                                           None, capi.SOA, ws.data_ptr(), need, s))
    assert np.array_equal(Q.cpu().numpy().transpose(0, 2, 1), got[0], equal_nan=True) and np.array_equal(cnt.cpu().numpy(), got[1])
    assert (which == SC.INT_FILL).all() and (it == SC.INT_FILL).all()


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_solutions_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist and no allocation: captured on a side stream (outputs preallocated through
    out=) and replayed twice, each time into refilled outputs, it gives the eager call's bits."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, K, N = 4097, 8, 3
    sep = SEP[case[0]]
    Q0, TG = _workload(torch, case, B)
    v, p = _visitor(ik_amd, STOP)
    assert ik_amd.dls_solutions_kernel(data, v, p, K) == _expected_name(data)
    kw = dict(num_starts=K, max_solutions=N, separation=sep, seed=SEED)
    eager = _prefilled(torch, N, Q0.shape, B)
    ik_amd.dls_solutions_batch(problem, Q0, TG, data, v, p, out=eager, **kw)
    out = _prefilled(torch, N, Q0.shape, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_solutions_batch(problem, Q0, TG, data, v, p, out=out, **kw)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_solutions_batch(problem, Q0, TG, data, v, p, out=out, **kw)
    assert int(eager[1].max()) == N and int(eager[1].min()) < N
    for _ in range(2):
        out[0].fill_(SC.NAN_FILL), out[1].fill_(SC.INT_FILL), out[2].fill_(SC.INT_FILL), out[3].fill_(SC.INT_FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), case
