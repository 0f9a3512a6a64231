"""Chains with prismatic joints on the device: the matrix and inputs of tests/prismatic_common.py (B = 197: three waves and a five-lane
tail), which tests/test_prismatic_chain_emulation.py runs through the CPU lane emulator.  Mirrors tests/test_gpu_chain_shapes.py.

Per case: (a) data.kernel, data.support and the seven dls_*_kernel queries report the fused chain kernels -- before the chain kernels
took prismatic joints they reported dls_generic<...> and loop(dls_generic<...>); (b) the stage kernels, both layouts, at 1e-13 / 1e-10
against the oracle; (c) step-synchronised, three iterates within STEP_BAR = 1e-9 (rad or m) of the oracle on every lane of every build,
the on-limit problems keep their joint on the limit, entries outside the chain equal clip(q0) bit for bit; (d) the default rule with
100 iterations: flags and iteration counts equal, q within TOL = 1e-6, an iteration-0 stop returns q0 untouched, IKGPU_REFILL=1 / 2 give
the same bits; (e) track, multi-start, solutions, goal set, line and path equal to their definitions by np.array_equal; (f) the same
problem under IKGPU_DLS_KERNEL=generic -- the route it took before -- within STEP_BAR per step.

test_chains_of_revolute_joints_compute_the_recorded_bits guards the other side: arm8 / l7 Full on its default build and the Cassie
leg give, for one fixed batch, the bits recorded from the library as it was before this change (tests/golden/make_revolute_chain_bits.py).

A case takes a fraction of a second on an MI355X; a hot-rtc case whose program is not in the on-disk cache adds its compile once."""
import os

import numpy as np
import pytest

import chain_shapes_common as CS
import goalset_common as GC
import line_common
import multistart_common as MC
import path_common
import prismatic_common as PC
import solutions_common as SC
from test_gpu_refill import env

pytestmark = pytest.mark.gpu

K, SMALL_B = PC.MS_K, PC.MS_B


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _data(problem, general=False, generic=False):
    """The build is decided when the problem is created and is part of the kernel's name."""
    import ik_amd
    # (the generic route without its run-time compiled form: one compile per case would be most of the test's time)
    with env(IKGPU_CHAIN_HOT="0" if general else None, IKGPU_DLS_KERNEL="generic" if generic else None, IKGPU_RTC="0" if generic else None):
        return ik_amd.dls_data(problem, device=0)


def _variant(data, suffix):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain" + suffix + data.kernel[len("dls_chain"):]


def _builds(c, problem):
    data = _data(problem, general=c.build == "general")
    hot = c.build == "default" and CS.hiprtc_installed()
    assert data.kernel == PC.kernel_name(c, "hot-rtc" if hot else "general"), data.kernel
    out = [data]
    if hot:
        out.append(_data(problem, general=True))
        assert out[1].kernel == PC.kernel_name(c, "general"), out[1].kernel
    return out


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_prismatic_chain_on_the_device(torch_cuda, c):
    torch = torch_cuda
    import ik_amd
    import oracle as O
    x = PC.inputs(c)
    model, om, tasks = x.model, x.om, x.tasks
    q0, tg = np.array(x.q0), np.array(x.tg)
    B, sup = PC.B, x.support
    problem = PC.make_problem(c, model)
    never, stop = ik_amd.never_stop_visitor(), ik_amd.inverse_kinematics_visitor()
    p1, p100 = ik_amd.dls_parameters(max_iterations=1), ik_amd.dls_parameters(max_iterations=100)
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()                         # [n, nq] -> SoA [nq, n]
    dev_t = lambda t: torch.from_numpy(np.ascontiguousarray(t.transpose(1, 2, 0))).cuda()      # [n, 1, 12] -> SoA [1, 12, n]

    # a. the kernels' names
    builds = _builds(c, problem)
    data = builds[0]
    assert np.array_equal(data.support, sup)
    for d in builds:
        assert ik_amd.dls_track_kernel(d, stop, p100) == _variant(d, "_track")
        assert ik_amd.dls_multistart_kernel(d, stop, p100, K) == _variant(d, "_multistart")
        assert ik_amd.dls_solutions_kernel(d, stop, p100, K) == _variant(d, "_solutions")
        assert ik_amd.dls_line_kernel(d, stop, p100) == _variant(d, "_line")
        assert ik_amd.dls_path_kernel(d, stop, p100) == _variant(d, "_path")
        assert ik_amd.dls_goalset_kernel(d, stop, p100, PC.GS_G, K) == _variant(d, "_goalset")
    print("kernels %s" % [d.kernel for d in builds])
    Q0, T = dev(q0), dev_t(tg)

    # b. the stage kernels, both layouts
    fk_ref = O.fk_batch(om, q0, [x.fid])
    ev_ref = [O.evaluate(om, tasks, tg[b], q0[b]) for b in range(B)]
    e_ref, J_ref = np.stack([r[0] for r in ev_ref]), np.stack([r[1] for r in ev_ref])
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
        if c.ktype != 0:
            assert (J[:, (3 if c.ktype == 2 else 0):, sup & x.prismatic] == 0.0).all(), layout

    # c. step-synchronised along the oracle's trajectory, every build; f. the generic lane program on the same problem
    generic = _data(problem, generic=True)
    assert generic.kernel.startswith("dls_generic<"), generic.kernel
    one = O.params(1, 1e-2, 1.0, -1.0)
    q = q0
    for k in range(3):
        q_next, _, _ = O.dls_batch(om, tasks, tg, q, one)
        got = [ik_amd.dls_batch(problem, dev(q), T, d, never, p1)[0].cpu().numpy().T for d in builds]
        old = ik_amd.dls_batch(problem, dev(q), T, generic, never, p1)[0].cpu().numpy().T
        for d, q_dev in zip(builds, got):
            worst = np.abs(q_dev - q_next).max()
            print("%s step %d: max |dq| vs oracle %.2e, vs the generic program %.2e" % (d.kernel, k + 1, worst, np.abs(q_dev - old).max()))
            assert np.isfinite(q_dev).all() and worst <= PC.STEP_BAR, (d.kernel, k, worst, int(np.argmax(np.abs(q_dev - q_next).max(axis=1))))
            assert np.abs(q_dev - old).max() <= PC.STEP_BAR, (d.kernel, k)
            assert np.array_equal(q_dev[:, ~sup], np.clip(q, x.lo, x.hi)[:, ~sup]), (d.kernel, k)
            if k == 0:
                assert all(q_dev[b, j] == q0[b, j] and q0[b, j] in (x.lo[j], x.hi[j]) for b, j in x.on_limit), d.kernel
        if len(got) == 2:
            assert np.abs(got[0] - got[1]).max() <= PC.STEP_BAR, k
        q = q_next

    # d. the default rule with 100 iterations; lock-step, refill and two-phase give the same bits
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
        print("%s stop rule: max |dq| vs oracle %.2e, converged %d of %d" % (d.kernel, worst, int(ok_ref.sum()), B))
        assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), d.kernel
        assert worst <= PC.TOL, (d.kernel, worst)
        assert np.array_equal(q_dev[stopped0], q0[stopped0]), d.kernel
        if c == PC.ZERO_JACOBIAN:
            turned = np.arange(B) % 2 == 1
            assert (it[turned] == 100).all() and not ok[turned].any() and np.array_equal(q_dev[turned], np.clip(q0, x.lo, x.hi)[turned])
            assert (it[~turned] == 0).all() and ok[~turned].all()

    # e. track, multi-start, solutions and goal set against their definitions, bit for bit (line and path: the next test)
    import test_gpu_multistart as TM
    import test_gpu_solutions as TS
    TW = torch.from_numpy(np.ascontiguousarray(PC.waypoints(c).transpose(0, 2, 3, 1))).cuda()      # [3, B, 1, 12] -> SoA [3, 1, 12, B]
    ms, _ = PC.multistart_inputs(c)
    Qs, starts = dev(ms[0]), torch.from_numpy(np.ascontiguousarray(ms[1:].transpose(0, 2, 1))).cuda()
    Ts = T[:, :, :SMALL_B].contiguous()
    goals = np.array(PC.goalset_goals(c))                                                          # [G, n, 1, 12]
    Gs = torch.from_numpy(np.ascontiguousarray(goals.transpose(0, 2, 3, 1))).cuda()                # SoA [G, 1, 12, n]
    for d in builds:
        for v, p in ((stop, p100), (never, ik_amd.dls_parameters(max_iterations=3))):
            qk, chained = Q0, []
            for t in range(PC.TRACK_T):
                qk, ok, it = ik_amd.dls_batch(problem, qk, TW[t], d, v, p)
                chained.append((qk, ok, it))
            tracked = ik_amd.dls_track_batch(problem, Q0, TW, d, v, p)
            for i, what in enumerate(("q", "success", "iterations")):
                assert np.array_equal(tracked[i].cpu().numpy(), torch.stack([s[i] for s in chained]).cpu().numpy()), (d.kernel, "track", what, v.tolerance)
        singles, errs = TM._reference(ik_amd, problem, d, Qs, starts, Ts, stop, p100)
        got = TM._run(ik_amd, problem, d, Qs, Ts, stop, p100, K, 0, starts, "soa")
        MC.check_selection(got, singles, errs, TM._norms(ik_amd, problem, d, dev(got[0]), Ts), (d.kernel, "multistart"))
        sols = TS._run(torch, ik_amd, problem, d, Qs, Ts, stop, p100, K, K, PC.SEP, starts, "soa")
        count, _ = SC.check_set(sols, singles, sup, PC.SEP, K, (d.kernel, "solutions"))
        # goal set: candidate j = g K + k is the single solve of start k against goal g
        cands = []
        for g in range(PC.GS_G):
            for k in range(K):
                Qk = Qs if k == 0 else starts[k - 1]
                Q, ok, it = ik_amd.dls_batch(problem, Qk, Gs[g], d, stop, p100)
                cands.append((Q.cpu().numpy().T, ok.cpu().numpy(), it.cpu().numpy()))
        import test_gpu_goalset as TG
        gs = list(TG._run(ik_amd, problem, d, Qs, Gs, stop, p100, K, 0, starts, "soa"))
        norm = lambda qq, t: np.array([np.linalg.norm(O.evaluate(om, tasks, t[b], qq[b])[0]) for b in range(SMALL_B)])
        unsolved = ~np.stack([s[1] for s in cands]).astype(bool).any(axis=0)
        errs_g = [np.where(unsolved, norm(cands[j][0], goals[j // K]), 0.0) ** 2 for j in range(len(cands))]
        GC.check_goalset(tuple(gs), cands, errs_g, norm(gs[0], goals[gs[3], np.arange(SMALL_B)]), K, (d.kernel, "goalset"))
        print("%s jobs: multi-start winners %s, solutions by count %s, goal-set goals %s"
              % (d.kernel, np.bincount(got[3], minlength=K).tolist(), np.bincount(count, minlength=K + 1).tolist(), np.bincount(gs[3], minlength=PC.GS_G).tolist()))


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_line_and_path_jobs_of_a_prismatic_chain_on_the_device(torch_cuda, c):
    """dls_line_batch (T = 8) and dls_path_batch ((P, T) = (3, 6), max_joint_step = 0.25 over radians and metres alike) on every build:
    np.array_equal to dls_track_batch on line_targets / path_targets on the written slabs and on `reached`, the sentinels kept
    elsewhere, both layouts."""
    torch = torch_cuda
    import ik_amd
    from test_gpu_line import _in_layout, _sentinels
    x = PC.inputs(c)
    q0, B, nq, sup = np.array(x.q0), PC.B, x.model.nq, x.support
    problem = PC.make_problem(c, x.model)
    stop, p100 = ik_amd.inverse_kinematics_visitor(1e-4), ik_amd.dls_parameters(max_iterations=100)
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
    P, PT = PC.PATH_PT
    vias = np.array(PC.far_goals(c, P))                                                    # [P, B, 1, 12]
    G = torch.from_numpy(np.ascontiguousarray(vias[0].transpose(1, 2, 0))).cuda()          # SoA [1, 12, B]
    V = torch.from_numpy(np.ascontiguousarray(vias.transpose(0, 2, 3, 1))).cuda()          # SoA [P, 1, 12, B]
    for d in _builds(c, problem):
        for layout in ("soa", "aos"):
            ql, gl = _in_layout(Q0, G, layout)
            vl = V if layout == "soa" else V.permute(0, 3, 1, 2).contiguous()
            # line
            T = PC.LINE_T
            W = ik_amd.line_targets(problem, ql, gl, d, T, layout=layout)
            Qt, okt, itt = ik_amd.dls_track_batch(problem, ql, W, d, stop, p100, layout=layout)
            qt = (Qt if layout == "aos" else Qt.permute(0, 2, 1)).cpu().numpy()
            okt, itt = okt.cpu().numpy(), itt.cpu().numpy()
            want, _ = line_common.reached_from_flags(okt)
            mask = line_common.written(want, T)
            Ql, ok, it, reached = ik_amd.dls_line_batch(problem, ql, gl, d, T, stop, p100, layout=layout, out=_sentinels(torch, T, nq, B, layout))
            q = (Ql if layout == "aos" else Ql.permute(0, 2, 1)).cpu().numpy()
            ok, it, reached = ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()
            assert np.array_equal(reached, want), (d.kernel, layout, "line")
            for a, b_, what in ((q, qt, "q"), (ok, okt, "success"), (it, itt, "iterations")):
                assert np.array_equal(a[mask], b_[mask]), (d.kernel, layout, "line", what)
            assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), (d.kernel, layout, "line")
            line_hist = np.bincount(want, minlength=T + 1)
            # path
            N = P * PT
            W = ik_amd.path_targets(problem, ql, vl, d, PT, layout=layout)
            Qt, okt, itt = ik_amd.dls_track_batch(problem, ql, W, d, stop, p100, layout=layout)
            qt = (Qt if layout == "aos" else Qt.permute(0, 2, 1)).cpu().numpy()
            okt, itt = okt.cpu().numpy(), itt.cpu().numpy()
            want, _ = path_common.met_rule(okt, qt, q0, sup, PC.PATH_STEP)
            mask = line_common.written(want, N)
            Ql, ok, it, reached = ik_amd.dls_path_batch(problem, ql, vl, d, PT, PC.PATH_STEP, stop, p100, layout=layout,
                                                         out=_sentinels(torch, N, nq, B, layout))
            q = (Ql if layout == "aos" else Ql.permute(0, 2, 1)).cpu().numpy()
            ok, it, reached = ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()
            assert np.array_equal(reached, want), (d.kernel, layout, "path")
            for a, b_, what in ((q, qt, "q"), (ok, okt, "success"), (it, itt, "iterations")):
                assert np.array_equal(a[mask], b_[mask]), (d.kernel, layout, "path", what)
            assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), (d.kernel, layout, "path")
            jump, stopped, complete = path_common.endings(okt, want, N)
        print("%s: line reached %s; path ended by a jump / by the stop rule / complete = %d / %d / %d"
              % (d.kernel, line_hist.tolist(), int(jump.sum()), int(stopped.sum()), int(complete.sum())))
        if c in PC.JOB_CASES:
            assert jump.sum() >= 1 and stopped.sum() >= 1 and line_hist[PC.LINE_T] > 0 and line_hist[:PC.LINE_T].sum() > 0


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "revolute_chain_bits.npy")


def test_chains_of_revolute_joints_compute_the_recorded_bits(torch_cuda):
    """Three step-synchronised iterates and the default rule of arm8 / l7 Full (default build) and the Cassie leg (the pre-built hot
    program) and of their general builds, B = 197: the bits tests/golden/make_revolute_chain_bits.py recorded from the library as it
    was before the chain kernels took prismatic joints, on the same kind of device."""
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    import make_revolute_chain_bits as G
    want = np.load(GOLDEN)
    got = G.compute()
    assert got.shape == want.shape
    for i, label in enumerate(G.LABELS):
        for k, what in enumerate(G.SLOTS):
            assert np.array_equal(got[i, k], want[i, k]), (label, what)
