"""ikgpu_dls_line_batch on the device: a straight Cartesian line from the pose at q0 to one goal per problem, solved waypoint after
waypoint, a problem leaving at its first failed waypoint.  The call is DEFINED as ikgpu_dls_track_batch on ikgpu_line_targets, so the
reference here is ik_amd.dls_track_batch on ik_amd.line_targets and the assertion is np.array_equal on the written slabs and on
`reached` -- for every build of the chain kernel (one launch: dls_chain_line<...>), both layouts and batch sizes around the wave
boundary; the slabs beyond a failed waypoint keep their sentinel (the single launch stops there); the waypoints match oracle/twin.py;
the optional arrays may be null; the launch can be captured; the chained oracle agrees; a tree problem, a derived-visitor problem and
two-slot problems in a world-fixed reference frame other than the universe run the definition inside the call; what has no line is
refused.  Inputs: tests/line_common.py.  The other chain lengths, task types, weights and reference frames: tests/test_gpu_chain_shapes.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import urdf_path
import line_common
from test_gpu_track import CASES, DEMO, FULL_BODY, _problem, env

pytestmark = pytest.mark.gpu

T = 16
MAX_IT, TOL = 100, 1e-4


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _rule(ik_amd, visitor=None):
    return visitor or ik_amd.inverse_kinematics_visitor(TOL), ik_amd.dls_parameters(max_iterations=MAX_IT)


_inputs = {}


def _line(torch, case, B, seed=0):
    """(start [nq, B], goals [1, 12, B]) on the device, SoA, and the host arrays [B, nq], [B, 12]."""
    key = (case[0], B, seed)
    if key not in _inputs:
        model = _problem(case)[0]
        _inputs[key] = line_common.inputs_exact(model, case[1], B, seed)
    q0, goals = _inputs[key]
    return (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda(), q0, goals[:, 0])


def _in_layout(Q0, G, layout):
    return (Q0, G) if layout == "soa" else (Q0.t().contiguous(), G.permute(2, 0, 1).contiguous())


def _sentinels(torch, nT, nq, B, layout):
    return (torch.full((nT, nq, B) if layout == "soa" else (nT, B, nq), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((nT, B), 7, dtype=torch.uint8, device="cuda"), torch.full((nT, B), -7, dtype=torch.int32, device="cuda"),
            torch.full((B,), -7, dtype=torch.int32, device="cuda"))


def _definition(ik_amd, problem, data, q0, g, nT, layout, visitor=None):
    """dls_track_batch on line_targets: (q [nT, B, nq], success, iters [nT, B], reached [B], written [nT, B], W)."""
    v, p = _rule(ik_amd, visitor)
    W = ik_amd.line_targets(problem, q0, g, data, nT, layout=layout)
    Q, ok, it = ik_amd.dls_track_batch(problem, q0, W, data, v, p, layout=layout)
    q = Q.cpu().numpy() if layout == "aos" else Q.permute(0, 2, 1).cpu().numpy()
    ok, it = ok.cpu().numpy(), it.cpu().numpy()
    reached, _ = line_common.reached_from_flags(ok)
    return q, ok, it, reached, line_common.written(reached, nT), W


def _solved(ik_amd, problem, data, q0, g, nT, layout, out, visitor=None):
    v, p = _rule(ik_amd, visitor)
    Q, ok, it, reached = ik_amd.dls_line_batch(problem, q0, g, data, nT, v, p, layout=layout, out=out)
    q = Q.cpu().numpy() if layout == "aos" else Q.permute(0, 2, 1).cpu().numpy()
    return q, ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_line" + data.kernel[len("dls_chain"):]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_fused_launch_is_bit_identical_to_tracking_the_waypoints(torch_cuda, case, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    Q0, G, _, _ = _line(torch, case, B)
    assert ik_amd.dls_line_kernel(data, *_rule(ik_amd)) == _expected_name(data)
    for layout in ("soa", "aos"):
        q0, g = _in_layout(Q0, G, layout)
        q_ref, ok_ref, it_ref, want, mask, _ = _definition(ik_amd, problem, data, q0, g, T, layout)
        q, ok, it, reached = _solved(ik_amd, problem, data, q0, g, T, layout, _sentinels(torch, T, model.nq, B, layout))
        assert np.array_equal(reached, want), (case, B, layout)
        for x, y, what in ((q, q_ref, "q"), (ok, ok_ref, "success"), (it, it_ref, "iterations")):
            assert np.array_equal(x[mask], y[mask]), (case, B, layout, what)
        # the single launch stops at the failed waypoint: later slabs keep what was there
        assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), (case, B, layout)
        if B == 4097:   # the regimes: lines that reach the goal and lines that fail on the way
            assert (want == T).any() and (want < T).any(), np.bincount(want, minlength=T + 1)


def test_one_waypoint_is_the_single_solve(torch_cuda):
    torch = torch_cuda
    import ik_amd
    for case in (CASES[0], CASES[1]):
        model, problem, data, _, _ = _problem(case)
        B = 130
        Q0, G, _, _ = _line(torch, case, B)
        v, p = _rule(ik_amd)
        q1, ok1, it1 = ik_amd.dls_batch(problem, Q0, G, data, v, p)
        Q, ok, it, reached = ik_amd.dls_line_batch(problem, Q0, G, data, 1, v, p)
        assert np.array_equal(Q[0].cpu().numpy(), q1.cpu().numpy()) and np.array_equal(ok[0].cpu().numpy(), ok1.cpu().numpy())
        assert np.array_equal(it[0].cpu().numpy(), it1.cpu().numpy()) and np.array_equal(reached.cpu().numpy(), ok1.cpu().numpy().astype(np.int32))


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_device_waypoints_match_the_twin(torch_cuda, case):
    """ikgpu_line_targets against oracle/twin.py at the bar the emulator test asserts (line_common.WAYPOINT_BAR)."""
    torch = torch_cuda
    import ik_amd
    import twin
    model, problem, data, _, _ = _problem(case)
    B = 130
    Q0, G, q0, goals = _line(torch, case, B)
    W = ik_amd.line_targets(problem, Q0, G, data, T)                               # [T, 1, 12, B]
    ref = line_common.twin_waypoints(twin.load_urdf(urdf_path(case[0])), case[1], q0, goals, T)
    got = W[:, 0].permute(0, 2, 1).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print("%s: max |W_device - W_twin| = %.3g" % (case[0], err))
    assert err <= line_common.WAYPOINT_BAR
    assert np.array_equal(got[T - 1], goals)                                      # the goal itself, bit for bit
    Wa = ik_amd.line_targets(problem, Q0.t().contiguous(), G.permute(2, 0, 1).contiguous(), data, T, layout="aos")
    assert np.array_equal(Wa[:, :, 0].cpu().numpy(), got)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_line_without_the_optional_arrays(torch_cuda, case):
    """success == NULL, iters == NULL and reached == NULL, straight through the C ABI (the Python entry always passes them)."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B = 4097
    Q0, G, _, _ = _line(torch, case, B)
    q_ref, ok_ref, it_ref, want, mask, _ = _definition(ik_amd, problem, data, Q0, G, T, "soa")
    prm = api._params(*_rule(ik_amd))
    s = torch.cuda.current_stream().cuda_stream
    Q = torch.full((T, model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(capi.lib().ikgpu_dls_line_batch(data._h, B, T, Q0.data_ptr(), G.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, None, capi.SOA,
                                               None, 0, C.c_void_p(s)))
    q = Q.permute(0, 2, 1).cpu().numpy()
    assert np.array_equal(q[mask], q_ref[mask]) and np.isnan(q[~mask]).all(), case
    # ... and only one of them
    reached = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    capi.check(capi.lib().ikgpu_dls_line_batch(data._h, B, T, Q0.data_ptr(), G.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, reached.data_ptr(),
                                               capi.SOA, None, 0, C.c_void_p(s)))
    assert np.array_equal(Q.permute(0, 2, 1).cpu().numpy()[mask], q_ref[mask]) and np.array_equal(reached.cpu().numpy(), want), case


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "%s-%s-%d-%s" % c)
def test_line_launch_under_a_captured_graph(torch_cuda, case):
    """The single launch takes no queue slot, no worklist, no allocation and no workspace: captured on a side stream (outputs
    preallocated through out=) and replayed it gives the eager call's bits.  One kernel, no branches."""
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    B = 4097
    Q0, G, _, _ = _line(torch, case, B)
    v, p = _rule(ik_amd)
    assert ik_amd.dls_line_kernel(data, v, p) == _expected_name(data)
    eager = _solved(ik_amd, problem, data, Q0, G, T, "soa", _sentinels(torch, T, model.nq, B, "soa"))
    out = _sentinels(torch, T, model.nq, B, "soa")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ik_amd.dls_line_batch(problem, Q0, G, data, T, v, p, out=out)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ik_amd.dls_line_batch(problem, Q0, G, data, T, v, p, out=out)
    out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7), out[3].fill_(-7)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = (out[0].permute(0, 2, 1).cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy())
    for x, y in zip(got, eager):
        assert np.array_equal(x, y, equal_nan=x.dtype == np.float64), case


def test_line_against_the_chained_oracle(torch_cuda):
    """The CPU test's rule (c) on the device, Cassie leg on the hot and the general build: the oracle chained along the device's
    waypoints agrees on flags and iteration counts on every written waypoint and within 1e-9 on q on every waypoint met; the failed
    waypoint's q is an unconverged iterate and is not compared."""
    torch = torch_cuda
    import ik_amd
    import oracle as O
    B = 130
    for case in (CASES[0], CASES[1]):
        model, problem, data, _, _ = _problem(case)
        Q0, G, q0, _ = _line(torch, case, B)
        W = ik_amd.line_targets(problem, Q0, G, data, T).permute(0, 3, 1, 2).contiguous().cpu().numpy()          # [T, B, 1, 12]
        q, ok, it, reached = _solved(ik_amd, problem, data, Q0, G, T, "soa", _sentinels(torch, T, model.nq, B, "soa"))
        om = O.OracleModel(model.flat())
        ot = O.make_tasks([(model.getFrameId(case[1]), 0, 2, 0, None)])
        qo, alive, worst, count = q0, np.ones(B, bool), 0.0, np.zeros(B, np.int32)
        for k in range(T):
            qo, ok_ref, it_ref = O.dls_batch(om, ot, W[k], qo, O.params(MAX_IT, 1e-2, 1.0, TOL))
            assert np.array_equal(ok[k][alive], ok_ref[alive]) and np.array_equal(it[k][alive], it_ref[alive]), (case, k)
            met = alive & (ok_ref == 1)
            if met.any():
                worst = max(worst, float(np.abs(q[k][met] - qo[met]).max()))
            alive = met
            count += met
        assert np.array_equal(reached, count), case
        print("%s: reached %s, max |q_line - q_oracle| on met waypoints = %.3g" % (data.kernel, np.bincount(reached, minlength=T + 1).tolist(), worst))
        assert worst <= 1e-9, (case, worst)


def _workspace_call(torch, ik_amd, problem, data, Q0, G, nT, visitor, short):
    """ikgpu_dls_line_batch through the C ABI with a workspace `short` bytes smaller than asked for.  Returns (rc, message)."""
    from ik_amd import api, capi
    prm = api._params(*_rule(ik_amd, visitor))
    L = capi.lib()
    B = Q0.shape[1]
    need = L.ikgpu_dls_line_workspace_bytes(data._h, B, nT, C.byref(prm))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    Q = torch.empty((nT, Q0.shape[0], B), dtype=torch.float64, device="cuda")
    rc = L.ikgpu_dls_line_batch(data._h, B, nT, Q0.data_ptr(), G.data_ptr(), C.byref(prm), Q.data_ptr(), None, None, None, capi.SOA, ws.data_ptr(),
                                need - short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, L.ikgpu_last_error().decode()


# Two frame tasks in a world-fixed reference frame other than the universe (the waypoint kernel of the other problem kinds reads one
# reference placement per slot): (robot, URDF text or None for the fixture's, [(frame, type)], reference).  ur5's `base` is rotated by
# -pi about z against base_link -- far from the identity, yet a symmetric matrix; arm8's `bench` (tests/chain_shapes_common.py) is
# oblique and displaced, so its transpose is another placement.
REFERENCE_KINDS = {"reference_base": ("ur5", None, [("tool0", 2), ("wrist_1_link", 0)], "base"),
                   "reference_bench": ("arm7", "arm8", [("tool", 2), ("l3", 0)], "bench")}


@pytest.mark.parametrize("kind", ["tree", "derived_visitor"] + sorted(REFERENCE_KINDS))
def test_other_problem_kinds_run_the_definition_inside_the_call(torch_cuda, kind):
    torch = torch_cuda
    import ik_amd
    import twin
    from ik_amd import capi
    visitor = None
    if kind in REFERENCE_KINDS:
        from test_gpu_generic import build
        import chain_shapes_common as CS
        name, edited, frames, reference = REFERENCE_KINDS[kind]
        B, nT = 130, 4
        xml = CS.arm8_xml() if edited else open(urdf_path(name)).read()
        _, _, model, problem, data, _, _, q0, tg = build(name, False, [("frame", f, reference, t, 0, None) for f, t in frames], B, seed=0,
                                                         xml_edit=(lambda _: xml.encode()) if edited else None)
        assert not data.kernel.startswith("dls_chain"), data.kernel
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        G = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
        W = ik_amd.line_targets(problem, Q0, G, data, nT).permute(0, 3, 1, 2).cpu().numpy()                   # [nT, B, 2, 12]
        tm = twin.load_urdf(xml)
        for s, (f, _) in enumerate(frames):
            err = float(np.abs(W[:, :, s] - line_common.twin_waypoints(tm, f, q0, tg[:, s], nT, reference=reference)).max())
            print("%s slot %d (%s in %s): max |W_device - W_twin| = %.3g" % (data.kernel, s, f, reference, err))
            assert err <= line_common.WAYPOINT_BAR, (f, err)
            assert np.array_equal(W[nT - 1, :, s], tg[:, s])
    elif kind == "tree":
        from test_gpu_generic import build
        B, nT = 130, 4
        with env(IKGPU_TREE_STATIC_ROWS="0"):
            _, _, model, problem, data, _, _, q0, tg = build("cassie", True, FULL_BODY, B, seed=0)
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        G = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
        # the waypoints of every slot against the twin (the start pose comes from what ikgpu_task_frames_fk_batch launches)
        W = ik_amd.line_targets(problem, Q0, G, data, nT).permute(0, 3, 1, 2).cpu().numpy()                   # [nT, B, 3, 12]
        tm = twin.load_urdf(urdf_path("cassie"), free_flyer=True)
        for s, spec in enumerate(FULL_BODY):
            ref = line_common.twin_waypoints(tm, spec[1], q0[:32], tg[:32, s], nT)
            assert float(np.abs(W[:, :32, s] - ref).max()) <= line_common.WAYPOINT_BAR, spec[1]
    else:
        B, nT = 130, T
        model, problem, data, _, _ = _problem(CASES[0])
        Q0, G, _, _ = _line(torch, CASES[0], B)
        visitor = ik_amd.inverse_kinematics_visitor(TOL, step_tolerance=1e-3)
    assert ik_amd.dls_line_kernel(data, *_rule(ik_amd, visitor)) == "loop(%s)" % data.kernel
    for layout in ("soa", "aos"):
        q0_, g = _in_layout(Q0, G, layout)
        q_ref, ok_ref, it_ref, want, mask, _ = _definition(ik_amd, problem, data, q0_, g, nT, layout, visitor)
        q, ok, it, reached = _solved(ik_amd, problem, data, q0_, g, nT, layout, _sentinels(torch, nT, model.nq, B, layout), visitor)
        assert np.array_equal(reached, want), (kind, layout)
        for x, y in ((q, q_ref), (ok, ok_ref), (it, it_ref)):
            assert np.array_equal(x[mask], y[mask]), (kind, layout)
    assert (want == nT).any()
    # success == NULL: the flags live in the workspace; a workspace one byte short is refused, with a message
    rc, msg = _workspace_call(torch, ik_amd, problem, data, Q0, G, nT, visitor, 0)
    assert rc == capi.OK, msg
    rc, msg = _workspace_call(torch, ik_amd, problem, data, Q0, G, nT, visitor, 1)
    assert rc == capi.ERR_INVALID and "workspace too small" in msg and "ikgpu_dls_line_workspace_bytes" in msg, msg
    torch.cuda.synchronize()


def test_what_has_no_line_is_refused(torch_cuda):
    """IKGPU_ERR_UNSUPPORTED for the demo task set's pelvis-relative foot task (a reference frame that moves with q) and for a
    posture slot, from both entry points."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import capi
    from test_gpu_generic import build
    posture = [("posture", 4, None, None, 0, ([1.0] * 4, [1.0] * 4)), ("frame", "tool0", "universe", 0, 0, None)]
    for name, ff, specs, word in (("cassie", True, DEMO, "moves with the configuration"), ("ur5", False, posture, "not a FrameTask")):
        B = 8
        _, _, model, problem, data, _, _, q0, tg = build(name, ff, specs, B, seed=0)
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        G = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
        for call in (lambda: ik_amd.line_targets(problem, Q0, G, data, 4), lambda: ik_amd.dls_line_batch(problem, Q0, G, data, 4)):
            with pytest.raises(capi.IkgpuError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED and word in e.value.message, (name, e.value.message)
