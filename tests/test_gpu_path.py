"""ikgpu_dls_path_batch on the device: a Cartesian path through P via poses per problem, T waypoints per segment, solved waypoint after
waypoint, a problem leaving at its first waypoint that was not met -- the solve met the stop rule and no support entry moved by more
than max_joint_step.  The call is DEFINED as ikgpu_dls_track_batch on ikgpu_path_targets plus that rule, so the reference here is
ik_amd.dls_track_batch on ik_amd.path_targets, the rule in numpy (tests/path_common.py met_rule) on what tracking returned, and the
assertion is np.array_equal on the written slabs and on `reached` -- for every build of the chain kernel (one launch:
dls_chain_path<...>), both layouts, batch sizes around the wave boundary, with and without the bound; the slabs beyond the first
waypoint that was not met keep their sentinel; the waypoints match oracle/twin.py and the line's; one segment without a bound is
dls_line_batch; the optional arrays may be null; the launch can be captured; a tree problem and a derived-visitor problem run the
definition inside the call; a short workspace and what has no line are refused.  No reference uses the path call itself.

Inputs: tests/path_common.py (inputs_exact, seed 1).  Measured on the CPU with the emulated tracking program (tests/test_path_emulation.py,
B = 130, P = 3, T = 6): lanes ended by a jump with success = 1 / by the stop rule / complete -- ur5 65 / 9 / 56, arm7 64 / 17 / 49, Cassie
leg 7 / 122 / 1; the conditions are asserted below on the device's own reference at B = 130 before anything is compared."""
import ctypes as C

import numpy as np
import pytest

from conftest import urdf_path
import line_common
import path_common
from test_gpu_track import CASES, FULL_BODY, _problem, env

pytestmark = pytest.mark.gpu

SHAPES = [(1, 6), (3, 6), (2, 1)]
MAX_IT, TOL, SEED = 100, 1e-4, 1


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _rule(ik_amd, visitor=None):
    return visitor or ik_amd.inverse_kinematics_visitor(TOL), ik_amd.dls_parameters(max_iterations=MAX_IT)


_inputs = {}


def _path(torch, case, B, P):
    """(start [nq, B], vias [P, 1, 12, B]) on the device, SoA, and the host arrays [B, nq], [P, B, 12]: the first P segments of the
    three-segment draw."""
    key = (case[0], B)
    if key not in _inputs:
        model = _problem(case)[0]
        _inputs[key] = path_common.inputs_exact(model, case[1], B, 3, SEED)
    q0, vias = _inputs[key]
    vias = np.ascontiguousarray(vias[:P])
    return (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.from_numpy(np.ascontiguousarray(vias.transpose(0, 2, 3, 1))).cuda(), q0, vias[:, :, 0])


def _in_layout(Q0, V, layout):
    return (Q0, V) if layout == "soa" else (Q0.t().contiguous(), V.permute(0, 3, 1, 2).contiguous())


def _sentinels(torch, N, nq, B, layout):
    return (torch.full((N, nq, B) if layout == "soa" else (N, B, nq), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((N, B), 7, dtype=torch.uint8, device="cuda"), torch.full((N, B), -7, dtype=torch.int32, device="cuda"),
            torch.full((B,), -7, dtype=torch.int32, device="cuda"))


def _tracking(ik_amd, problem, data, q0, v, T, layout, visitor=None):
    """dls_track_batch on path_targets: (q [N, B, nq], success, iters [N, B], q0 [B, nq], W) -- the part of the definition that does not
    depend on the bound."""
    vis, p = _rule(ik_amd, visitor)
    W = ik_amd.path_targets(problem, q0, v, data, T, layout=layout)
    Q, ok, it = ik_amd.dls_track_batch(problem, q0, W, data, vis, p, layout=layout)
    q = Q.cpu().numpy() if layout == "aos" else Q.permute(0, 2, 1).cpu().numpy()
    return q, ok.cpu().numpy(), it.cpu().numpy(), (q0.cpu().numpy() if layout == "aos" else q0.t().cpu().numpy()), W


def _solved(ik_amd, problem, data, q0, v, T, step, layout, out, visitor=None):
    vis, p = _rule(ik_amd, visitor)
    Q, ok, it, reached = ik_amd.dls_path_batch(problem, q0, v, data, T, step, vis, p, layout=layout, out=out)
    q = Q.cpu().numpy() if layout == "aos" else Q.permute(0, 2, 1).cpu().numpy()
    return q, ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_path" + data.kernel[len("dls_chain"):]


def _compare(got, ref, want, N, what):
    q, ok, it, reached = got
    q_ref, ok_ref, it_ref = ref
    mask = line_common.written(want, N)
    assert np.array_equal(reached, want), what
    for x, y, name in ((q, q_ref, "q"), (ok, ok_ref, "success"), (it, it_ref, "iterations")):
        assert np.array_equal(x[mask], y[mask]), what + (name,)
    # the single launch stops at the first waypoint that was not met: later slabs keep what was there
    assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), what


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 4097])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_fused_launch_is_bit_identical_to_the_definition(torch_cuda, case, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    assert ik_amd.dls_path_kernel(data, *_rule(ik_amd)) == _expected_name(data)
    support = np.asarray(data.support, dtype=bool)
    robot_step = path_common.JOINT_STEP[case[0]]
    for P, T in SHAPES:
        N = P * T
        Q0, V, _, _ = _path(torch, case, B, P)
        for layout in ("soa", "aos"):
            q0, v = _in_layout(Q0, V, layout)
            q_ref, ok_ref, it_ref, q0_host, _ = _tracking(ik_amd, problem, data, q0, v, T, layout)
            for step in (0.0, robot_step):
                want, _ = path_common.met_rule(ok_ref, q_ref, q0_host, support, step)
                if B == 130 and (P, T) == (3, 6) and step > 0 and case[2] == 2:
                    counts = path_common.check_conditions(ok_ref, want, P, T)      # conditions on the reference, before anything is compared
                    print("%s: ended by a jump / by the stop rule / complete = %d / %d / %d" % ((data.kernel,) + counts))
                got = _solved(ik_amd, problem, data, q0, v, T, step, layout, _sentinels(torch, N, model.nq, B, layout))
                _compare(got, (q_ref, ok_ref, it_ref), want, N, (case, B, P, T, layout, step))
            if P == 1:   # one segment without a bound is the line job, all four outputs
                vis, p = _rule(ik_amd)
                line = ik_amd.dls_line_batch(problem, q0, v[0], data, T, vis, p, layout=layout, out=_sentinels(torch, N, model.nq, B, layout))
                free = ik_amd.dls_path_batch(problem, q0, v, data, T, 0.0, vis, p, layout=layout, out=_sentinels(torch, N, model.nq, B, layout))
                for x, y in zip(free, line):
                    assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=x.dtype == torch.float64), (case, B, layout)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_device_waypoints_match_the_line_the_vias_and_the_twin(torch_cuda, case):
    """ikgpu_path_targets: segment 0 is ikgpu_line_targets bit for bit, slab s T + T - 1 is via s bit for bit, every segment agrees with
    oracle/twin.py at line_common.WAYPOINT_BAR, both layouts give the same bits."""
    torch = torch_cuda
    import ik_amd
    import twin
    model, problem, data, _, _ = _problem(case)
    B, P, T = 130, 3, 6
    Q0, V, q0, vias = _path(torch, case, B, P)
    W = ik_amd.path_targets(problem, Q0, V, data, T)                               # [P T, 1, 12, B]
    got = W[:, 0].permute(0, 2, 1).cpu().numpy()
    assert np.array_equal(W[:T].cpu().numpy(), ik_amd.line_targets(problem, Q0, V[0], data, T).cpu().numpy())
    for s in range(P):
        assert np.array_equal(got[s * T + T - 1], vias[s]), s
    err = float(np.abs(got - path_common.twin_waypoints(twin.load_urdf(urdf_path(case[0])), case[1], q0, vias, T)).max())
    print("%s: max |W_device - W_twin| = %.3g" % (case[0], err))
    assert err <= line_common.WAYPOINT_BAR
    Wa = ik_amd.path_targets(problem, Q0.t().contiguous(), V.permute(0, 3, 1, 2).contiguous(), data, T, layout="aos")
    assert np.array_equal(Wa[:, :, 0].cpu().numpy(), got)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_path_without_the_optional_arrays(torch_cuda, case):
    """success == NULL, iters == NULL and reached == NULL, straight through the C ABI (the Python entry always passes them)."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, P, T = 4097, 3, 6
    N = P * T
    step = path_common.JOINT_STEP[case[0]]
    Q0, V, _, _ = _path(torch, case, B, P)
    q_ref, ok_ref, it_ref, q0_host, _ = _tracking(ik_amd, problem, data, Q0, V, T, "soa")
    want, _ = path_common.met_rule(ok_ref, q_ref, q0_host, np.asarray(data.support, dtype=bool), step)
    mask = line_common.written(want, N)
    prm = api._params(*_rule(ik_amd))
    s = torch.cuda.current_stream().cuda_stream
    Q = torch.full((N, model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
    call = lambda reached: capi.check(capi.lib().ikgpu_dls_path_batch(data._h, B, P, T, Q0.data_ptr(), V.data_ptr(), C.byref(prm), step, Q.data_ptr(), None, None,
                                                                      reached, capi.SOA, None, 0, C.c_void_p(s)))
    call(None)
    q = Q.permute(0, 2, 1).cpu().numpy()
    assert np.array_equal(q[mask], q_ref[mask]) and np.isnan(q[~mask]).all(), case
    # ... and only one of them
    reached = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    call(reached.data_ptr())
    assert np.array_equal(Q.permute(0, 2, 1).cpu().numpy()[mask], q_ref[mask]) and np.array_equal(reached.cpu().numpy(), want), case


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_path_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist, no allocation and no workspace: captured on a side stream (outputs
    preallocated through out=) and replayed twice it gives the eager call's bits.  One kernel, no branches."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B, P, T = 4097, 3, 6
    N = P * T
    step = path_common.JOINT_STEP[case[0]]
    Q0, V, _, _ = _path(torch, case, B, P)
    v, p = _rule(ik_amd)
    assert ik_amd.dls_path_kernel(data, v, p) == _expected_name(data)
    eager = _solved(ik_amd, problem, data, Q0, V, T, step, "soa", _sentinels(torch, N, model.nq, B, "soa"))
    out = _sentinels(torch, N, model.nq, B, "soa")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_path_batch(problem, Q0, V, data, T, step, v, p, out=out)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_path_batch(problem, Q0, V, data, T, step, v, p, out=out)
    for _ in range(2):
        out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7), out[3].fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (out[0].permute(0, 2, 1).cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy())
        for x, y in zip(got, eager):
            assert np.array_equal(x, y, equal_nan=x.dtype == np.float64), case


def _workspace_call(torch, ik_amd, data, Q0, V, T, step, visitor, short):
    """ikgpu_dls_path_batch through the C ABI with a workspace `short` bytes smaller than asked for.  Returns (rc, message)."""
    from ik_amd import api, capi
    prm = api._params(*_rule(ik_amd, visitor))
    L = capi.lib()
    P, B = V.shape[0], Q0.shape[1]
    need = L.ikgpu_dls_path_workspace_bytes(data._h, B, P, T, C.byref(prm))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    Q = torch.empty((P * T, Q0.shape[0], B), dtype=torch.float64, device="cuda")
    rc = L.ikgpu_dls_path_batch(data._h, B, P, T, Q0.data_ptr(), V.data_ptr(), C.byref(prm), step, Q.data_ptr(), None, None, None, capi.SOA, ws.data_ptr(),
                                need - short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, L.ikgpu_last_error().decode()


@pytest.mark.parametrize("kind", ["tree", "derived_visitor"])
def test_other_problem_kinds_run_the_definition_inside_the_call(torch_cuda, kind):
    """A tree problem (dls_tree<NJ=7,chains=2,base_task>) and a derived-visitor problem run loop(...) through the workspace and equal the
    same reference; a workspace one byte short is refused with the needed size."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import capi
    visitor = None
    if kind == "tree":
        from test_gpu_generic import build
        B, P, T, step = 130, 2, 3, 0.25
        with env(IKGPU_TREE_STATIC_ROWS="0"):
            _, _, model, problem, data, _, _, q0, tg = build("cassie", True, FULL_BODY, B, seed=0)
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
        _, _, _, _, _, _, _, _, tg2 = build("cassie", True, FULL_BODY, B, seed=1)
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        V = torch.from_numpy(np.ascontiguousarray(np.stack([tg, tg2]).transpose(0, 2, 3, 1))).cuda()     # [P, 3, 12, B]
        # the waypoints: segment 0 is the line's, the last slab of every segment its via
        W = ik_amd.path_targets(problem, Q0, V, data, T)
        assert np.array_equal(W[:T].cpu().numpy(), ik_amd.line_targets(problem, Q0, V[0], data, T).cpu().numpy())
        assert np.array_equal(W[T - 1].cpu().numpy(), V[0].cpu().numpy()) and np.array_equal(W[2 * T - 1].cpu().numpy(), V[1].cpu().numpy())
    else:
        B, P, T = 130, 3, 6
        step = path_common.JOINT_STEP["cassie_fixed"]
        model, problem, data, _, _ = _problem(CASES[0])
        Q0, V, _, _ = _path(torch, CASES[0], B, P)
        visitor = ik_amd.inverse_kinematics_visitor(TOL, step_tolerance=1e-3)
    N = P * T
    assert ik_amd.dls_path_kernel(data, *_rule(ik_amd, visitor)) == "loop(%s)" % data.kernel
    support = np.asarray(data.support, dtype=bool)
    for layout in ("soa", "aos"):
        q0_, v = _in_layout(Q0, V, layout)
        q_ref, ok_ref, it_ref, q0_host, _ = _tracking(ik_amd, problem, data, q0_, v, T, layout, visitor)
        for s in (0.0, step):
            want, _ = path_common.met_rule(ok_ref, q_ref, q0_host, support, s)
            q, ok, it, reached = _solved(ik_amd, problem, data, q0_, v, T, s, layout, _sentinels(torch, N, model.nq, B, layout), visitor)
            mask = line_common.written(want, N)
            assert np.array_equal(reached, want), (kind, layout, s)
            for x, y in ((q, q_ref), (ok, ok_ref), (it, it_ref)):
                assert np.array_equal(x[mask], y[mask]), (kind, layout, s)
    print("%s: reached %s" % (kind, np.bincount(want, minlength=N + 1).tolist()))
    # success == NULL: the flags live in the workspace; a workspace one byte short is refused, with a message
    rc, msg = _workspace_call(torch, ik_amd, data, Q0, V, T, step, visitor, 0)
    assert rc == capi.OK, msg
    rc, msg = _workspace_call(torch, ik_amd, data, Q0, V, T, step, visitor, 1)
    assert rc == capi.ERR_INVALID and "workspace too small" in msg and "ikgpu_dls_path_workspace_bytes" in msg, msg
    torch.cuda.synchronize()


def test_what_has_no_path_is_refused(torch_cuda):
    """IKGPU_ERR_UNSUPPORTED for the demo task set's pelvis-relative foot task (a reference frame that moves with q) and for a
    posture slot, from both entry points: the slot restrictions are the line's."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import capi
    from test_gpu_generic import build
    from test_gpu_track import DEMO
    posture = [("posture", 4, None, None, 0, ([1.0] * 4, [1.0] * 4)), ("frame", "tool0", "universe", 0, 0, None)]
    for name, ff, specs, word in (("cassie", True, DEMO, "moves with the configuration"), ("ur5", False, posture, "not a FrameTask")):
        B = 8
        _, _, model, problem, data, _, _, q0, tg = build(name, ff, specs, B, seed=0)
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        V = torch.from_numpy(np.ascontiguousarray(np.stack([tg, tg]).transpose(0, 2, 3, 1))).cuda()
        for call in (lambda: ik_amd.path_targets(problem, Q0, V, data, 4), lambda: ik_amd.dls_path_batch(problem, Q0, V, data, 4, 0.5)):
            with pytest.raises(capi.IkgpuError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED and word in e.value.message, (name, e.value.message)
