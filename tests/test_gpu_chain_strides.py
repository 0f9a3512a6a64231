"""Addressing of the chain kernels (device/chain_kernel_body.hpp chain_strides / at: the layout resolved once into an element stride and
a problem stride) on the device: the Cassie leg on the kernel compiled into the library ("hot") and on the general build, UR5 on
"hot", arm7 on the kernel compiled for its structure code at run time ("hot-rtc") -- at B = 1, 63, 64, 65 and 197 (a lone lane, one
lane short of a wave, a full wave, one lane into a second wave, three waves and a five-lane tail), in both layouts, with and without
the success / iters outputs, under the never-stop rule and the default stop rule, for max_iterations = 0, 1 and 7.

Inputs: start configurations uniform in the joint limits, the target of problem b the frame at clip(q0 + U(-0.15, 0.15)) (the
project's "near" offset).  Where the model has entries of q outside the chain (the Cassie leg: nine of sixteen), every third problem
starts with two of them beyond their limits, one above and one below.  Problem b is the same whatever B is: the oracle solves the 197
once per stop rule and iteration count, and a batch of B is held to its first B.

Asserted, on EVERY entry of q_out: within 1e-9 rad of the oracle's (tests/test_gpu_hot_task_frame.py STEP_BAR; the entries outside
the chain are clipped copies, or -- when no step is taken: max_iterations = 0, or a stop at iteration 0 -- untouched ones, and equal
the oracle's to the bit); success flags and iteration counts equal to the oracle's; AOS and SOA, and the runs with and without the
success / iters outputs, the same bits.

Observed (one MI355X): max |dq| against the oracle 1.6e-14 (Cassie leg, hot and general), 3.5e-13 (UR5), 2.5e-14 (arm7)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import urdf_path

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 197)
BMAX = max(BS)
BAR = 1e-9           # rad (tests/test_gpu_hot_task_frame.py STEP_BAR)
CASES = [("cassie_fixed", "LeftFootFront", ",hot>"), ("cassie_fixed", "LeftFootFront", ",general>"), ("ur5", "tool0", ",hot>"),
         ("arm7", "tool", ",hot-rtc>")]
RULES = [("never_stop", -1.0), ("default", 1e-4)]
ITERS = (0, 1, 7)


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


def _solve(torch, data, prm, q0, tg, layout, with_flags):
    """One ikgpu_dls_solve_batch on device pointers; q0 [B, nq], tg [B, 1, 12] on the host, in and out.  Returns q [B, nq], ok, it."""
    from ik_amd import capi
    B = q0.shape[0]
    soa = layout == "soa"
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T if soa else q0)).cuda()
    T = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0) if soa else tg)).cuda()
    Q = torch.full_like(Q0, float("nan"))
    ok = torch.full((B,), 77, dtype=torch.uint8, device=Q0.device)
    it = torch.full((B,), -77, dtype=torch.int32, device=Q0.device)
    s = torch.cuda.current_stream(Q0.device).cuda_stream
    capi.check(capi.lib().ikgpu_dls_solve_batch(data._h, B, Q0.data_ptr(), T.data_ptr(), C.byref(prm), Q.data_ptr(),
                                               ok.data_ptr() if with_flags else None, it.data_ptr() if with_flags else None,
                                               capi.SOA if soa else capi.AOS, C.c_void_p(s)))
    torch.cuda.synchronize()
    q = Q.cpu().numpy()
    return (q.T if soa else q), ok.cpu().numpy(), it.cpu().numpy()


@pytest.mark.parametrize("name,frame,want", CASES, ids=[c[0] + c[2].strip(",>") for c in CASES])
def test_every_entry_in_both_layouts_at_wave_boundaries(torch_cuda, name, frame, want):
    torch = torch_cuda
    if want == ",hot-rtc>" and not _hiprtc():
        pytest.skip("hipRTC is not installed")
    import ik_amd
    from ik_amd import api
    import oracle as O
    model = ik_amd.Model.from_urdf_xml(open(urdf_path(name)).read())
    problem = ik_amd.InverseKinematicsProblem(model)
    problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
    data = _data(problem, general=want == ",general>")
    assert data.kernel.endswith(want), data.kernel
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    tasks = O.make_tasks([(fid, 0, 2, 0, None)])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(1970)
    q0 = rng.uniform(lo, hi, (BMAX, lo.size))
    tg = O.fk_batch(om, np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape), lo, hi), [fid])
    outside = np.flatnonzero(~data.support)
    if name == "cassie_fixed":
        assert outside.size == 9
    if outside.size >= 2:
        q0[::3, outside[0]] = hi[outside[0]] + 9.0
        q0[::3, outside[-1]] = lo[outside[-1]] - 9.0
    cores = os.cpu_count() or 1
    worst = 0.0
    for rule, tol in RULES:
        visitor = ik_amd.never_stop_visitor() if tol < 0 else ik_amd.inverse_kinematics_visitor()
        for iters in ITERS:
            q_ref, ok_ref, it_ref = O.dls_batch(om, tasks, tg, q0, O.params(iters, 1e-2, 1.0, tol), cores)
            prm = api._params(visitor, ik_amd.dls_parameters(max_iterations=iters))
            if iters == 0:
                assert np.array_equal(q_ref, q0)        # no step: nothing is clipped, inside the chain or outside it
            elif outside.size >= 2 and tol < 0:
                assert np.array_equal(q_ref[::3, outside[0]], hi[outside[0]] + 0 * q_ref[::3, outside[0]])
                assert np.array_equal(q_ref[::3, outside[-1]], lo[outside[-1]] + 0 * q_ref[::3, outside[-1]])
            for B in BS:
                got = {}
                for layout in ("soa", "aos"):
                    for with_flags in (True, False):
                        q, ok, it = _solve(torch, data, prm, q0[:B], tg[:B], layout, with_flags)
                        where = (data.kernel, rule, iters, B, layout, with_flags)
                        assert np.isfinite(q).all(), where
                        d = np.abs(q - q_ref[:B]).max()
                        worst = max(worst, d)
                        assert d <= BAR, where + (d,)
                        if outside.size:
                            assert np.array_equal(q[:, outside], q_ref[:B][:, outside]), where
                        if with_flags:
                            assert np.array_equal(ok, ok_ref[:B]) and np.array_equal(it, it_ref[:B]), where
                        else:   # the outputs that were not asked for were not written
                            assert (ok == 77).all() and (it == -77).all(), where
                        got[(layout, with_flags)] = q
                first = got[("soa", True)]
                for key, q in got.items():
                    assert np.array_equal(q.view(np.uint64), first.view(np.uint64)), (data.kernel, rule, iters, B, key)
    print("%s: max |dq| vs oracle %.2e over %d launches" % (data.kernel, worst, len(RULES) * len(ITERS) * len(BS) * 4))
