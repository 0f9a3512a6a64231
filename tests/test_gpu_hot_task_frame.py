"""The structure-specialised chain kernels with the task Jacobian built in the task frame, tip to base (device/chain_hot.hpp
hot_evaluate), on the device at B = 197 -- three full waves and a five-lane tail -- against the oracle and against the general build
(device/chain_solver.hpp: base to tip in the world frame, the independently formulated second build): the Cassie leg and UR5 on the
kernels compiled into the library ("hot"), arm7 on the kernel compiled for its structure code at run time ("hot-rtc").

Inputs: start configurations uniform in the joint limits; the target of problem b is the frame at clamp-free q0 + U(-0.15, 0.15) (the
project's "near" offset: a step towards a far target is chaotic and has no lane-wise answer, tests/test_gpu_full_size.py).  Ten problems
are rewritten so that a chain joint STARTS ON A LIMIT with the first step pointing outwards -- decided by the oracle alone: its first
iterate leaves that joint on the limit while the unclipped step (the same problem with the limits lifted) crosses it.

Asserted: success flags and iteration counts equal to the oracle's for 1, 2 and 3 fixed iterations and for the default stop rule with
100; the project's step-synchronised bar (tests/test_gpu_full_size.py rule S1) on each of the first three steps: from the oracle's k-th
iterate the device's next iterate is within 1e-9 rad of the oracle's on every lane; and the general build within the same bar of the hot
build on the same inputs."""
import os
import re

import numpy as np
import pytest

from conftest import urdf_path

pytestmark = pytest.mark.gpu

B = 197
STEP_BAR = 1e-9      # rad: one DLS step, every lane (tests/test_gpu_full_size.py STEP_BAR)
CASES = [("cassie_fixed", "LeftFootFront", ",hot>"), ("ur5", "tool0", ",hot>"), ("arm7", "tool", ",hot-rtc>")]


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _hiprtc():
    """Decided from the installation alone, before any work (as tests/test_gpu_pik.py does)."""
    return any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7"))


def _data(problem, general):
    """The build is decided when the problem is created (ikgpu_problem_create) and is part of the kernel's name."""
    import ik_amd
    prev = os.environ.get("IKGPU_CHAIN_HOT")
    if general:
        os.environ["IKGPU_CHAIN_HOT"] = "0"
    try:
        return ik_amd.dls_data(problem, device=0)
    finally:
        if general:
            if prev is None:
                del os.environ["IKGPU_CHAIN_HOT"]
            else:
                os.environ["IKGPU_CHAIN_HOT"] = prev


def _inputs(O, model, xml, frame, support):
    """q0 [B, nq], targets [B, 1, 12], and the (problem, joint) pairs that start on a limit with the first step pointing outwards."""
    import ik_amd
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    tasks = O.make_tasks([(fid, 0, 2, 0, None)])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(197)
    q0 = rng.uniform(lo, hi, (B, lo.size))
    qs = q0 + rng.uniform(-0.15, 0.15, q0.shape)
    # the same model with the limits lifted: the oracle's unclipped first step
    free = ik_amd.Model.from_urdf_xml(re.sub(r'lower="[-0-9.e]+" upper="[-0-9.e]+"', 'lower="-100.0" upper="100.0"', xml))
    om_free = O.OracleModel(free.flat())
    one = O.params(1, 1e-2, 1.0, -1.0)
    chain = np.flatnonzero(support)
    on_limit = []
    for b in range(10):
        for try_ in range(2 * chain.size):
            j, lim, out = chain[(b + try_ // 2) % chain.size], (hi, lo)[(b + try_) % 2], (1.0, -1.0)[(b + try_) % 2]
            q, s = q0[b].copy(), qs[b].copy()
            q[j], s[j] = lim[j], lim[j] + out * 0.15
            tg = O.fk_batch(om_free, s[None], [fid])
            q1, _, _ = O.dls(om, tasks, tg[0], q, one)
            q1_free, _, _ = O.dls(om_free, tasks, tg[0], q, one)
            if q1[j] == lim[j] and out * (q1_free[j] - lim[j]) > 1e-3:
                q0[b], qs[b] = q, s
                on_limit.append((b, int(j)))
                break
    assert len(on_limit) == 10, on_limit
    return om, tasks, q0, O.fk_batch(om_free, qs, [fid]), on_limit


@pytest.mark.parametrize("name,frame,want", CASES)
def test_hot_build_against_oracle_and_general_build(torch_cuda, name, frame, want):
    torch = torch_cuda
    if want == ",hot-rtc>" and not _hiprtc():
        pytest.skip("hipRTC is not installed")
    import ik_amd
    import oracle as O
    xml = open(urdf_path(name)).read()
    model = ik_amd.Model.from_urdf_xml(xml)
    problem = ik_amd.InverseKinematicsProblem(model)
    problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
    hot = _data(problem, general=False)
    # with hipRTC present a kernel that does not compile for the chain's structure code is an error here, not a reason to skip: the
    # library would run the general build in its place
    assert hot.kernel.endswith(want), hot.kernel
    gen = _data(problem, general=True)
    assert gen.kernel.endswith(",general>"), gen.kernel
    om, tasks, q0, tg, on_limit = _inputs(O, model, xml, frame, hot.support)
    T = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
    cores = os.cpu_count() or 1

    # flags and iteration counts: 1, 2, 3 fixed iterations and the default stop rule with 100
    Q0 = dev(q0)
    for iters, visitor, tol in ((1, ik_amd.never_stop_visitor(), -1.0), (2, ik_amd.never_stop_visitor(), -1.0),
                                (3, ik_amd.never_stop_visitor(), -1.0), (100, ik_amd.inverse_kinematics_visitor(), 1e-4)):
        q_ref, ok_ref, it_ref = O.dls_batch(om, tasks, tg, q0, O.params(iters, 1e-2, 1.0, tol), cores)
        for data in (hot, gen):
            Q, ok, it = ik_amd.dls_batch(problem, Q0, T, data, visitor, ik_amd.dls_parameters(max_iterations=iters))
            q_dev = Q.cpu().numpy().T
            print("%s iters %d tol %g: max |dq| vs oracle %.2e, converged %d of %d" % (data.kernel, iters, tol, np.abs(q_dev - q_ref).max(), int(ok_ref.sum()), B))
            assert np.isfinite(q_dev).all()
            assert np.array_equal(ok.cpu().numpy(), ok_ref) and np.array_equal(it.cpu().numpy(), it_ref), (data.kernel, iters)
        if iters == 100:
            assert ok_ref.sum() >= B // 2       # the stop rule was exercised: most problems converge, at different iterations
            assert len(set(it_ref[ok_ref != 0].tolist())) > 1

    # step-synchronised: from the oracle's k-th iterate, the device's next iterate -- every lane, the first three steps
    one, p1 = O.params(1, 1e-2, 1.0, -1.0), ik_amd.dls_parameters(max_iterations=1)
    q = q0
    for k in range(3):
        q_next, _, _ = O.dls_batch(om, tasks, tg, q, one, cores)
        if k == 0:   # the ten rewritten problems: the oracle's first iterate leaves the joint on its limit
            lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
            assert all(q_next[b, j] in (lo[j], hi[j]) and q_next[b, j] == q0[b, j] for b, j in on_limit)
        q_hot = ik_amd.dls_batch(problem, dev(q), T, hot, ik_amd.never_stop_visitor(), p1)[0].cpu().numpy().T
        q_gen = ik_amd.dls_batch(problem, dev(q), T, gen, ik_amd.never_stop_visitor(), p1)[0].cpu().numpy().T
        d_hot, d_gen, d_builds = np.abs(q_hot - q_next).max(), np.abs(q_gen - q_next).max(), np.abs(q_hot - q_gen).max()
        print("%s step %d: max |dq| hot vs oracle %.2e, general vs oracle %.2e, hot vs general %.2e" % (hot.kernel, k + 1, d_hot, d_gen, d_builds))
        assert d_hot <= STEP_BAR, (hot.kernel, k, d_hot, int(np.argmax(np.abs(q_hot - q_next).max(axis=1))))
        assert d_builds <= STEP_BAR, (hot.kernel, gen.kernel, k, d_builds)
        q = q_next
