"""Every instantiation of the chain kernels on the device: the 24 general shapes (NJ = 1 .. 8 x Position / Orientation / Full), unit and
non-unit weights, a world-fixed oblique reference frame, and the run-time specialised hot build at NJ = 1 .. 7 -- the matrix and inputs
of tests/chain_shapes_common.py (B = 197: three waves and a five-lane tail), which tests/test_chain_shapes_emulation.py runs through
the CPU lane emulator.  What the device does not share with the emulator is what is under test: the kernel-argument layout per NJ, the
table reads, the LDS staging of the stage kernels, the hot code generator at short lengths, and the wave exchanges of the multi-start
and solutions kernels of those instantiations.

Per case: (a) the kernel's name; (b) task_frames_fk_batch at 1e-13 and evaluate_batch (e and the dense J, zero outside the support) at
1e-10 against the oracle, both layouts; (c) step-synchronised, from the oracle's k-th iterate the device's next iterate within
STEP_BAR = 1e-9 rad on every lane, k = 0, 1, 2 (tests/test_gpu_full_size.py rule S1), the on-limit problems keep their joint on the
limit, entries outside the chain equal clip(q0) bit for bit; (d) the default stop rule with 100 iterations: flags and iteration counts
equal to the oracle's, q within TOL = 1e-6, an iteration-0 stop returns q0 untouched, IKGPU_REFILL=1 / 2 give the same bits; (e) track
(T = 3, stop rule and never-stop) equal to three chained dls_batch calls, multi-start and solutions (K = 4 supplied starts on B = 33,
the near start in slot b % 4 so that the winner moves through the lanes of a group) against their definitions in
tests/multistart_common.py / tests/solutions_common.py, all by np.array_equal, and the kernel-name queries report the fused kernels;
(f) the general build of a hot-rtc problem within STEP_BAR of the hot one.  The line job has a test function of its own,
test_line_job_of_every_chain_shape_on_the_device, so that a failure names the job.

A case takes 0.02 - 0.3 s on an MI355X; a hot-rtc case whose program is not in the on-disk cache yet adds its compile (1.2 - 2.3 s
measured, NJ = 1 .. 7)."""
import numpy as np
import pytest

import chain_shapes_common as CS
import multistart_common as MC
import solutions_common as SC
from test_gpu_full_size import STEP_BAR, TOL
from test_gpu_refill import env

pytestmark = pytest.mark.gpu

K, SMALL_B, SEP = CS.MS_K, CS.MS_B, 0.5     # multi-start / solutions: four supplied starts on two waves and a four-lane tail of lanes


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _data(problem, general):
    """The build is decided when the problem is created and is part of the kernel's name."""
    import ik_amd
    with env(IKGPU_CHAIN_HOT="0" if general else None):
        return ik_amd.dls_data(problem, device=0)


def _variant(data, suffix):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain" + suffix + data.kernel[len("dls_chain"):]


@pytest.mark.parametrize("c", CS.CASES, ids=CS.case_id)
def test_chain_shape_on_the_device(torch_cuda, c):
    torch = torch_cuda
    import ik_amd
    import oracle as O
    import test_gpu_multistart as TM
    import test_gpu_solutions as TS
    x = CS.inputs(c)
    model, om, tasks = x.model, x.om, x.tasks
    q0, tg = np.array(x.q0), np.array(x.tg)
    B, sup = CS.B, x.support
    problem = CS.make_problem(c, model)
    never, stop = ik_amd.never_stop_visitor(), ik_amd.inverse_kinematics_visitor()
    p1, p100 = ik_amd.dls_parameters(max_iterations=1), ik_amd.dls_parameters(max_iterations=100)
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()                         # [n, nq] -> SoA [nq, n]
    dev_t = lambda t: torch.from_numpy(np.ascontiguousarray(t.transpose(1, 2, 0))).cuda()      # [n, 1, 12] -> SoA [1, 12, n]

    # a. the kernel's name.  With hipRTC installed a default-build case that is not hot-rtc is a failure: the library would run the
    # general build in its place
    data = _data(problem, general=c.build == "general")
    assert data.kernel == CS.kernel_name(c, CS.hiprtc_installed()), data.kernel
    assert np.array_equal(data.support, sup)
    print("kernel %s" % data.kernel)
    builds = [data]
    if c.build == "default" and data.kernel.endswith(",hot-rtc>"):
        gen = _data(problem, general=True)
        assert gen.kernel == "dls_chain<NJ=%d,%s,general>" % (c.nj, CS.TYPE_NAMES[c.ktype]), gen.kernel
        builds.append(gen)
    Q0, T = dev(q0), dev_t(tg)

    # b. the stage kernels, both layouts
    fk_ref = O.fk_batch(om, q0, [x.fid])
    ev_ref = [O.evaluate(om, tasks, tg[b], q0[b]) for b in range(B)]
    e_ref, J_ref = np.stack([r[0] for r in ev_ref]), np.stack([r[1] for r in ev_ref])       # [B, M], [B, M, nv]
    for layout in ("soa", "aos"):
        Ql, Tl = (Q0, T) if layout == "soa" else (Q0.t().contiguous(), T.permute(2, 0, 1).contiguous())
        fk = ik_amd.task_frames_fk_batch(problem, Ql, data, layout=layout).cpu().numpy()
        e, J = ik_amd.evaluate_batch(problem, Ql, Tl, data, layout=layout)
        e, J = e.cpu().numpy(), J.cpu().numpy()
        if layout == "soa":
            fk, e, J = fk.transpose(2, 0, 1), e.T, J.transpose(2, 0, 1)
        d_fk, d_e, d_J = np.abs(fk - fk_ref).max(), np.abs(e - e_ref).max(), np.abs(J - J_ref).max()
        print("stages %s: max |oMf - oracle| %.2e, |e - oracle| %.2e, |J - oracle| %.2e" % (layout, d_fk, d_e, d_J))
        assert d_fk <= 1e-13 and d_e <= 1e-10 and d_J <= 1e-10, (layout, d_fk, d_e, d_J)
        assert (J[:, :, ~sup] == 0.0).all(), layout

    # c. step-synchronised along the oracle's trajectory (and f: the general build of a hot-rtc problem within the same bar of the hot one)
    one = O.params(1, 1e-2, 1.0, -1.0)
    q = q0
    for k in range(3):
        q_next, _, _ = O.dls_batch(om, tasks, tg, q, one)
        if k == 0:
            assert all(q_next[b, j] in (x.lo[j], x.hi[j]) and q_next[b, j] == q0[b, j] for b, j in x.on_limit)
        got = [ik_amd.dls_batch(problem, dev(q), T, d, never, p1)[0].cpu().numpy().T for d in builds]
        for d, q_dev in zip(builds, got):
            worst = np.abs(q_dev - q_next).max()
            print("%s step %d: max |dq| vs oracle %.2e" % (d.kernel, k + 1, worst))
            assert np.isfinite(q_dev).all() and worst <= STEP_BAR, (d.kernel, k, worst, int(np.argmax(np.abs(q_dev - q_next).max(axis=1))))
            assert np.array_equal(q_dev[:, ~sup], np.clip(q, x.lo, x.hi)[:, ~sup]), (d.kernel, k)
            if k == 0:
                assert all(q_dev[b, j] == q0[b, j] for b, j in x.on_limit), d.kernel
        if len(got) == 2:
            d_builds = np.abs(got[0] - got[1]).max()
            print("%s step %d: hot vs general %.2e" % (data.kernel, k + 1, d_builds))
            assert d_builds <= STEP_BAR, (k, d_builds)
        q = q_next

    # d. the default stop rule with 100 iterations; lock-step, refill and two-phase give the same bits
    q_ref, ok_ref, it_ref = O.dls_batch(om, tasks, tg, q0, O.params(100, 1e-2, 1.0, 1e-4))
    stopped0 = it_ref == 0
    for d in builds:
        res = {}
        for refill in (None, "1", "2"):
            with env(IKGPU_REFILL=refill):
                Q, ok, it = ik_amd.dls_batch(problem, Q0, T, d, stop, p100)
            res[refill] = (Q.cpu().numpy().T, ok.cpu().numpy(), it.cpu().numpy())
        q_dev, ok, it = res[None]
        for refill in ("1", "2"):
            for a, b_, what in zip(res[refill], res[None], ("q", "success", "iterations")):
                assert np.array_equal(a, b_), (d.kernel, "IKGPU_REFILL=" + refill, what)
        worst = np.abs(q_dev - q_ref).max()
        print("%s stop rule: max |dq| vs oracle %.2e, converged %d of %d, iteration counts %d .. %d" % (d.kernel, worst, int(ok_ref.sum()), B, it_ref.min(), it_ref.max()))
        assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), d.kernel
        assert worst <= TOL, (d.kernel, worst)
        assert np.array_equal(q_dev[stopped0], q0[stopped0]), d.kernel      # an iteration-0 stop returns the whole q0, unclipped
    if c.ktype == 0 and c.frame == "l1":      # the frame origin lies on the joint axis: every lane stops at iteration 0
        assert stopped0.all() and (q0 > x.hi).any() and (q0 < x.lo).any()
    if c.nj >= 3:
        assert len(set(it_ref[ok_ref != 0].tolist())) >= 2

    # e. the job kinds against their definitions, bit for bit
    TW = torch.from_numpy(np.ascontiguousarray(CS.waypoints(c).transpose(0, 2, 3, 1))).cuda()      # [3, B, 1, 12] -> SoA [3, 1, 12, B]
    ms, _ = CS.multistart_inputs(c)                                                               # [K, 33, nq]: slot 0 is the call's Q0
    Qs, starts = dev(ms[0]), torch.from_numpy(np.ascontiguousarray(ms[1:].transpose(0, 2, 1))).cuda()
    Ts = T[:, :, :SMALL_B].contiguous()
    for d in builds:
        for v, p in ((stop, p100), (never, ik_amd.dls_parameters(max_iterations=3))):
            assert ik_amd.dls_track_kernel(d, v, p) == _variant(d, "_track")
            qk, chained = Q0, []
            for t in range(3):
                qk, ok, it = ik_amd.dls_batch(problem, qk, TW[t], d, v, p)
                chained.append((qk, ok, it))
            tracked = ik_amd.dls_track_batch(problem, Q0, TW, d, v, p)
            for i, what in enumerate(("q", "success", "iterations")):
                assert np.array_equal(tracked[i].cpu().numpy(), torch.stack([s[i] for s in chained]).cpu().numpy()), (d.kernel, "track", what, v.tolerance)
        # multi-start: the best single solve by the rule of tests/multistart_common.py
        assert ik_amd.dls_multistart_kernel(d, stop, p100, K) == _variant(d, "_multistart")
        singles, errs = TM._reference(ik_amd, problem, d, Qs, starts, Ts, stop, p100)
        got = TM._run(ik_amd, problem, d, Qs, Ts, stop, p100, K, 0, starts, "soa")
        at_result = TM._norms(ik_amd, problem, d, dev(got[0]), Ts)
        MC.check_selection(got, singles, errs, at_result, (d.kernel, "multistart"))
        # solutions: the greedy set of tests/solutions_common.py over the same single solves
        assert ik_amd.dls_solutions_kernel(d, stop, p100, K) == _variant(d, "_solutions")
        sols = TS._run(torch, ik_amd, problem, d, Qs, Ts, stop, p100, K, K, SEP, starts, "soa")
        count, _ = SC.check_set(sols, singles, sup, SEP, K, (d.kernel, "solutions"))
        print("%s jobs: multi-start winners %s, solutions by count %s" % (d.kernel, np.bincount(got[3], minlength=K).tolist(), np.bincount(count, minlength=K + 1).tolist()))


def _chained_oracle(O, x, W, near, ext=None):
    """The oracle chained along the waypoints W [T, B, 12] on the lines `near`, a line leaving at its first failed waypoint: per waypoint
    (alive [n], q, success, iterations)."""
    prm = O.params(CS.LINE_RULE[0], 1e-2, 1.0, CS.LINE_RULE[1])
    qo, alive, out = x.q0[near], np.ones(near.size, bool), []
    for k in range(W.shape[0]):
        qo, ok_ref, it_ref = O.dls_batch(x.om, x.tasks, np.ascontiguousarray(W[k][near][:, None, :]), qo, prm, ext=ext)
        out.append((alive, qo, ok_ref, it_ref))
        alive = alive & (ok_ref == 1)
    return out


@pytest.mark.parametrize("c", CS.CASES, ids=CS.case_id)
def test_line_job_of_every_chain_shape_on_the_device(torch_cuda, c):
    """The line job (dls_chain_job_kernel<NJ, KT, SMASK>(a, LineArgs), and the entry ikgpu_hot_line_stop of the run-time compiled module at
    NJ = 1 .. 7) on every build of every case: CS.LINE_T waypoints towards CS.line_goals in the case's reference frame under the default
    stop rule.  Per build: the kernel's name; line_targets against oracle/twin.py with the case's reference at line_common.WAYPOINT_BAR,
    both layouts giving the same bits and the last waypoint the goal's; dls_line_batch into sentinel-filled outputs np.array_equal to
    dls_track_batch on line_targets on the written slabs and on `reached`, the sentinels kept elsewhere, both layouts; T = 1 equal to
    dls_batch to the goal; on the near lines the chained double oracle's flags and iteration counts on every written waypoint and q
    within 1e-9 on every waypoint met (tests/test_line_emulation.py rule (c)).  A flag or a count that differs from the double oracle
    is reported with the _Float128 oracle's answer on that line and fails the test: no line is excluded."""
    torch = torch_cuda
    import ik_amd
    import line_common
    import oracle as O
    from test_gpu_line import _in_layout, _sentinels
    x = CS.inputs(c)
    goals, far = CS.line_goals(c)
    goals = np.array(goals)
    q0, B, T, nq = np.array(x.q0), CS.B, CS.LINE_T, x.model.nq
    near = np.setdiff1d(np.arange(B), far)
    problem = CS.make_problem(c, x.model)
    stop, p100 = ik_amd.inverse_kinematics_visitor(CS.LINE_RULE[1]), ik_amd.dls_parameters(max_iterations=CS.LINE_RULE[0])
    data = _data(problem, general=c.build == "general")
    assert data.kernel == CS.kernel_name(c, CS.hiprtc_installed()), data.kernel
    builds = [data]
    if c.build == "default" and data.kernel.endswith(",hot-rtc>"):
        builds.append(_data(problem, general=True))
        assert builds[1].kernel == "dls_chain<NJ=%d,%s,general>" % (c.nj, CS.TYPE_NAMES[c.ktype]), builds[1].kernel
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()                          # SoA [nq, B]
    G = torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda()       # SoA [1, 12, B]
    W_twin = CS.line_twin_waypoints(c)
    oracle_at = None
    for d in builds:
        assert ik_amd.dls_line_kernel(d, stop, p100) == _variant(d, "_line")
        W_host = {}
        for layout in ("soa", "aos"):
            ql, gl = _in_layout(Q0, G, layout)
            # the waypoints
            W = ik_amd.line_targets(problem, ql, gl, d, T, layout=layout)               # [T, 1, 12, B] | [T, B, 1, 12]
            W_host[layout] = (W[:, 0].permute(0, 2, 1) if layout == "soa" else W[:, :, 0]).cpu().numpy()
            err = float(np.abs(W_host[layout] - W_twin).max())
            print("%s %s: max |W_device - W_twin| = %.3g (reference %s)" % (d.kernel, layout, err, c.reference))
            assert err <= line_common.WAYPOINT_BAR, (d.kernel, layout, err)
            assert np.array_equal(W_host[layout][T - 1], goals[:, 0]), (d.kernel, layout)
            # the definition: track on those waypoints
            Qt, okt, itt = ik_amd.dls_track_batch(problem, ql, W, d, stop, p100, layout=layout)
            qt = (Qt if layout == "aos" else Qt.permute(0, 2, 1)).cpu().numpy()
            okt, itt = okt.cpu().numpy(), itt.cpu().numpy()
            want, _ = line_common.reached_from_flags(okt)
            mask = line_common.written(want, T)
            Ql, ok, it, reached = ik_amd.dls_line_batch(problem, ql, gl, d, T, stop, p100, layout=layout, out=_sentinels(torch, T, nq, B, layout))
            q = (Ql if layout == "aos" else Ql.permute(0, 2, 1)).cpu().numpy()
            ok, it, reached = ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()
            assert np.array_equal(reached, want), (d.kernel, layout)
            for a, b_, what in ((q, qt, "q"), (ok, okt, "success"), (it, itt, "iterations")):
                assert np.array_equal(a[mask], b_[mask]), (d.kernel, layout, what)
            assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), (d.kernel, layout)
            # T = 1: the single solve to the goal
            q1, ok1, it1 = ik_amd.dls_batch(problem, ql, gl, d, stop, p100, layout=layout)
            L1 = ik_amd.dls_line_batch(problem, ql, gl, d, 1, stop, p100, layout=layout)
            for a, b_, what in zip((L1[0][0], L1[1][0], L1[2][0]), (q1, ok1, it1), ("q", "success", "iterations")):
                assert np.array_equal(a.cpu().numpy(), b_.cpu().numpy()), (d.kernel, layout, "T = 1", what)
            assert np.array_equal(L1[3].cpu().numpy(), ok1.cpu().numpy().astype(np.int32)), (d.kernel, layout, "T = 1")
        assert np.array_equal(W_host["aos"], W_host["soa"]), d.kernel
        # the near lines against the chained oracle (the last layout's q, ok, it: equal to the other's through the definition)
        if oracle_at is None or not np.array_equal(oracle_at[0], W_host["soa"]):
            oracle_at = (W_host["soa"], _chained_oracle(O, x, W_host["soa"], near))
        worst, count, differs = 0.0, np.zeros(near.size, np.int32), np.zeros(near.size, bool)
        for k, (alive, qo, ok_ref, it_ref) in enumerate(oracle_at[1]):
            differs |= alive & ((ok[k][near] != ok_ref) | (it[k][near] != it_ref))
            met = alive & (ok_ref == 1)
            if met.any():
                worst = max(worst, float(np.abs(q[k][near][met] - qo[met]).max()))
            count += met
        if differs.any():      # a finding: what the _Float128 oracle says on those lines goes into the failure
            ext = _chained_oracle(O, x, W_host["soa"], near, ext="q")
            lanes = np.flatnonzero(differs)
            report = [(int(near[i]), [(int(ok[k][near[i]]), int(it[k][near[i]]), int(oracle_at[1][k][2][i]), int(oracle_at[1][k][3][i]), int(ext[k][2][i]), int(ext[k][3][i]))
                                      for k in range(T)]) for i in lanes]
            pytest.fail("%s: near lines differing from the double oracle -- (problem, per waypoint (device ok, it, double ok, it, _Float128 ok, it)): %r" % (d.kernel, report))
        assert np.array_equal(want[near], count), d.kernel
        print("%s: reached %s (far lines %s), near lines max |q_line - q_oracle| on met waypoints = %.3g"
              % (d.kernel, np.bincount(want, minlength=T + 1).tolist(), np.bincount(want[far], minlength=T + 1).tolist(), worst))
        assert worst <= 1e-9, (d.kernel, worst)
