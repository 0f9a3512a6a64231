"""Folded runs of parallel joints in the hot chain kernels (ik_amd/csrc/device/chain_hot.hpp hot_evaluate: a run is walked in the frame
it is entered with) on the device at B = 197 -- three full waves and a five-lane tail -- for the chains of tests/hot_fold_common.py
(a folded run at the tip with the leader at joint 0, in the middle before a general placement, twice in one chain, beside unfolded
joints, none at all) on the kernel compiled for their structure code at run time ("hot-rtc"; hipRTC is required, not skipped), and for
Cassie's leg and UR5 on the kernels compiled into the library ("hot").  The model is tests/test_gpu_hot_task_frame.py.

Inputs: starts uniform in the limits, the target of problem b the frame at clamp-free q0 + U(-0.15, 0.15).  The first lanes are
rewritten per run: every member on its upper limit, on its lower limit (run sums of +-6.6 rad for a run of two, +-9.9 for the run of
three: beyond 2 pi) and alternating.  The last nine lanes get a target a rotation of pi - 1e-9 / 1e-6 / 1e-2 away from the start pose.

Asserted: the kernel's name; step-synchronised along the oracle's trajectory, the first three steps: from the oracle's k-th iterate the
device's next iterate is within STEP_BAR = 1e-9 rad of the oracle's on every lane, and the general build (device/chain_solver.hpp,
the independently formulated second build) within the same bar of the hot one; 50 fixed iterations within tests/test_gpu_full_size.py's
TOL = 1e-6 of the oracle's, flags and counts equal; the default stop rule with 100 iterations: flags and counts equal to the oracle's.
A lane whose error rotation the ORACLE puts within 1e-2 rad of pi at the iterate a step starts from -- the band in which log3 takes its
theta -> pi formula: the nine far lanes at k = 0 -- is held to 1e-6 for that step, the bar of tests/test_gpu_rotation_by_pi.py: the
oracle's own double arithmetic is 1e-8 from its _Float128 build there (the lane program on the host is 2.7e-8 from it,
tests/test_hot_fold_host.py).  Just outside the band the bar is STEP_BAR max(1, 1e-3 / sin^2 theta), the conditioning of the regular
formula derived in tests/hot_fold_common.py (conditioned): 1e-9 up to pi - 0.032, 1e-8 at pi - 1e-2.  The nine far lanes are left out
of the comparisons over many steps, which have no lane-wise answer for a far target (tests/test_gpu_full_size.py).
On run2_middle the other jobs that share hot_evaluate, each through the stop rule: lane refill alone and two-phase give the bits of
the lock-step launch, track equals chained solves, multi-start equals its definition (tests/multistart_common.py)."""
import functools
import re

import numpy as np
import pytest

import hot_fold_common as HF
import multistart_common as MC
from chain_shapes_common import hiprtc_installed
from test_gpu_full_size import STEP_BAR, TOL
from test_gpu_refill import env
from test_hot_evaluate import PI_AXES, PI_GAPS, _rot

pytestmark = pytest.mark.gpu

B = 197
NEAR_PI_BAR = 1e-6
FAR = np.arange(B - len(PI_GAPS) * len(PI_AXES), B)      # the lanes with a target a rotation of almost pi away


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _inputs(name):
    import ik_amd
    import oracle as O
    c = HF.BY_NAME[name]
    xml = HF.chain_xml(c)
    model = ik_amd.Model.from_urdf_xml(xml)
    om = O.OracleModel(model.flat())
    free = ik_amd.Model.from_urdf_xml(re.sub(r'lower="[-0-9.e]+" upper="[-0-9.e]+"', 'lower="-100.0" upper="100.0"', xml))
    om_free = O.OracleModel(free.flat())
    fid = model.getFrameId(c.frame)
    flat = model.flat()
    qidx, j = [], int(flat["frame_parent"][fid])
    while j > 0:
        qidx.insert(0, int(flat["idx_q"][j]))
        j = int(flat["parent"][j])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(197)
    q0 = rng.uniform(lo, hi, (B, lo.size))
    rows = HF.run_rows(c, lo, hi, qidx, q0)
    q0[:len(rows)] = rows
    qs = q0 + rng.uniform(-0.15, 0.15, q0.shape)
    tg = O.fk_batch(om_free, qs, [fid])
    here = O.fk_batch(om, q0[FAR], [fid])
    for i, b in enumerate(FAR):
        gap, axis = PI_GAPS[i // len(PI_AXES)], PI_AXES[i % len(PI_AXES)]
        tg[b, 0] = here[i, 0]
        tg[b, 0, :9] = (here[i, 0, :9].reshape(3, 3) @ _rot(axis, np.pi - gap)).ravel()
    way = np.stack([O.fk_batch(om_free, q0 + f * (qs - q0), [fid]) for f in (1.0 / 3, 2.0 / 3)] + [tg])       # [3, B, 1, 12]
    return dict(chain=c, xml=xml, model=model, om=om, fid=fid, qidx=qidx, lo=lo, hi=hi, q0=q0, tg=tg, way=way, nrows=len(rows),
                tasks=O.make_tasks([(fid, 0, 2, 0, None)]))


def _builds(x):
    import ik_amd
    problem = ik_amd.InverseKinematicsProblem(x["model"])
    problem.add_frame_task("t", ik_amd.FrameTask.create(x["model"], x["chain"].frame, ik_amd.KinematicType.Full))
    hot = ik_amd.dls_data(problem, device=0)
    with env(IKGPU_CHAIN_HOT="0"):
        gen = ik_amd.dls_data(problem, device=0)
    return problem, hot, gen


def _bars(O, x, q):
    """Per lane: STEP_BAR, widened by the conditioning of log3 towards pi, NEAR_PI_BAR inside its theta -> pi band (HF.conditioned); theta
    is the oracle's error rotation at q."""
    theta = np.array([np.linalg.norm(O.evaluate(x["om"], x["tasks"], x["tg"][b], q[b])[0][3:]) for b in range(B)])
    return HF.conditioned(theta, STEP_BAR, NEAR_PI_BAR), theta


@pytest.mark.parametrize("name", [c.name for c in HF.CHAINS])
def test_folded_runs_against_oracle_and_general_build(torch_cuda, name):
    torch = torch_cuda
    import ik_amd
    import oracle as O
    assert hiprtc_installed(), "the run-time specialised build needs hipRTC"
    x = _inputs(name)
    c, om, tasks, q0, tg = x["chain"], x["om"], x["tasks"], x["q0"], x["tg"]
    problem, hot, gen = _builds(x)
    nj = len(c.leader)
    assert hot.kernel == "dls_chain<NJ=%d,full,%s>" % (nj, "hot-rtc" if c.joints is not None else "hot"), hot.kernel
    assert gen.kernel == "dls_chain<NJ=%d,full,general>" % nj, gen.kernel
    # the inputs are what the docstring says: every run with all members on either limit, sums beyond 2 pi on the made-up chains
    for m in HF.runs(c):
        idx = [x["qidx"][j] for j in m]
        head = q0[:x["nrows"]][:, idx]
        assert (head == x["hi"][idx]).all(axis=1).any() and (head == x["lo"][idx]).all(axis=1).any()
        if c.joints is not None:
            assert head.sum(axis=1).max() > 2 * np.pi and head.sum(axis=1).min() < -2 * np.pi
    T = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
    never, stop = ik_amd.never_stop_visitor(), ik_amd.inverse_kinematics_visitor()
    near = np.setdiff1d(np.arange(B), FAR)

    # step-synchronised: from the oracle's k-th iterate, the device's next iterate -- every lane, the first three steps
    one, p1 = O.params(1, 1e-2, 1.0, -1.0), ik_amd.dls_parameters(max_iterations=1)
    q = q0
    for k in range(3):
        bars, theta = _bars(O, x, q)
        if k == 0:
            assert (np.abs(theta[FAR] - (np.pi - np.repeat(PI_GAPS, len(PI_AXES)))) < 1e-6).all()      # the far lanes are where they claim to be
            assert (bars[near] == STEP_BAR).all()
            bars[FAR] = NEAR_PI_BAR      # (the three lanes AT pi - 1e-2 sit on the edge of the band: they belong to the far group whichever side theta rounds to)
        q_next, _, _ = O.dls_batch(om, tasks, tg, q, one)
        q_hot = ik_amd.dls_batch(problem, dev(q), T, hot, never, p1)[0].cpu().numpy().T
        q_gen = ik_amd.dls_batch(problem, dev(q), T, gen, never, p1)[0].cpu().numpy().T
        d_hot, d_builds = np.abs(q_hot - q_next).max(axis=1), np.abs(q_hot - q_gen).max(axis=1)
        tight = bars == STEP_BAR
        print("%s step %d: max |dq| hot vs oracle %.2e (%d lanes with a wider bar: %.2e), hot vs general %.2e (wider bar: %.2e)"
              % (hot.kernel, k + 1, d_hot[tight].max(), (~tight).sum(), d_hot[~tight].max(initial=0.0), d_builds[tight].max(), d_builds[~tight].max(initial=0.0)))
        assert np.isfinite(q_hot).all() and np.isfinite(q_gen).all()
        assert (d_hot <= bars).all(), (hot.kernel, k, int(np.argmax(d_hot / bars)), d_hot.max())
        assert (d_builds <= bars).all(), (hot.kernel, gen.kernel, k, int(np.argmax(d_builds / bars)), d_builds.max())
        q = q_next

    # 50 fixed iterations, and the default stop rule with 100
    Q0 = dev(q0)
    for iters, visitor, tol in ((50, never, -1.0), (100, stop, 1e-4)):
        q_ref, ok_ref, it_ref = O.dls_batch(om, tasks, tg, q0, O.params(iters, 1e-2, 1.0, tol))
        Q, ok, it = ik_amd.dls_batch(problem, Q0, T, hot, visitor, ik_amd.dls_parameters(max_iterations=iters))
        q_dev, ok, it = Q.cpu().numpy().T, ok.cpu().numpy(), it.cpu().numpy()
        worst = np.abs(q_dev - q_ref)[near].max()
        print("%s iters %d tol %g: max |dq| vs oracle %.2e (far lanes %.2e), converged %d of %d" % (hot.kernel, iters, tol, worst, np.abs(q_dev - q_ref)[FAR].max(),
                                                                                              int(ok_ref[near].sum()), near.size))
        assert np.isfinite(q_dev).all()
        assert np.array_equal(ok[near], ok_ref[near]) and np.array_equal(it[near], it_ref[near]), (hot.kernel, iters)
        assert worst <= TOL, (hot.kernel, iters, worst)
        if iters == 100:
            assert ok_ref[near].sum() >= near.size // 2      # the stop rule was exercised


def test_the_other_jobs_on_a_chain_with_a_folded_run(torch_cuda):
    """Refill, track and multi-start call the same hot_evaluate: run2_middle through the stop rule, each against its definition."""
    torch = torch_cuda
    import ik_amd
    import test_gpu_multistart as TM
    assert hiprtc_installed(), "the run-time specialised build needs hipRTC"
    x = _inputs("run2_middle")
    problem, hot, _ = _builds(x)
    assert hot.kernel.endswith(",hot-rtc>"), hot.kernel
    q0, tg = x["q0"], x["tg"]
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
    Q0, T = dev(q0), torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
    stop, p100 = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(max_iterations=100)

    # lane refill: the refill kernel alone ("1") and the two-phase solve ("2") give the bits of the lock-step launch
    res = {}
    for refill in (None, "1", "2"):
        with env(IKGPU_REFILL=refill):
            res[refill] = [a.cpu().numpy() for a in ik_amd.dls_batch(problem, Q0, T, hot, stop, p100)]
    assert len(set(res[None][2][res[None][1] != 0].tolist())) >= 2      # lanes finish at different iterations: refill has something to do
    for refill in ("1", "2"):
        for a, b_, what in zip(res[refill], res[None], ("q", "success", "iterations")):
            assert np.array_equal(a, b_), ("IKGPU_REFILL=" + refill, what)

    # track: three waypoints in one launch equal three chained solves
    TW = torch.from_numpy(np.ascontiguousarray(x["way"].transpose(0, 2, 3, 1))).cuda()      # [3, B, 1, 12] -> SoA [3, 1, 12, B]
    assert ik_amd.dls_track_kernel(hot, stop, p100) == "dls_chain_track" + hot.kernel[len("dls_chain"):]
    qk, chained = Q0, []
    for t in range(3):
        qk, ok, it = ik_amd.dls_batch(problem, qk, TW[t], hot, stop, p100)
        chained.append((qk, ok, it))
    tracked = ik_amd.dls_track_batch(problem, Q0, TW, hot, stop, p100)
    for i, what in enumerate(("q", "success", "iterations")):
        assert np.array_equal(tracked[i].cpu().numpy(), torch.stack([s[i] for s in chained]).cpu().numpy()), ("track", what)

    # multi-start: four supplied starts on 33 problems, the problem's own (near) start in slot b % 4
    K, SB = 4, 33
    rng = np.random.default_rng(198)
    starts = rng.uniform(x["lo"], x["hi"], (K, SB, x["lo"].size))
    rows = np.arange(SB)
    starts[rows % K, rows] = q0[:SB]
    Qs, gen = dev(starts[0]), torch.from_numpy(np.ascontiguousarray(starts[1:].transpose(0, 2, 1))).cuda()
    Ts = T[:, :, :SB].contiguous()
    assert ik_amd.dls_multistart_kernel(hot, stop, p100, K) == "dls_chain_multistart" + hot.kernel[len("dls_chain"):]
    singles, errs = TM._reference(ik_amd, problem, hot, Qs, gen, Ts, stop, p100)
    got = TM._run(ik_amd, problem, hot, Qs, Ts, stop, p100, K, 0, gen, "soa")
    MC.check_selection(got, singles, errs, TM._norms(ik_amd, problem, hot, dev(got[0]), Ts), (hot.kernel, "multistart"))
    print("%s multi-start winners %s" % (hot.kernel, np.bincount(got[3], minlength=K).tolist()))
