"""The pass-through plan on the device (ik_amd/csrc/device/chain_kernel_body.hpp PassPlan): the entries of q outside the chain come from
a plan in the kernel arguments, and every output must keep the bits it has without one.

Models (tests/pass_plan_common.py): the Cassie leg (9 entries outside the chain), the 6-joint chain to lefttarsus (10), UR5 (none: a plan
without entries) and `wide` (17: more than the plan holds, so the bodies walk the tables in HBM).  Builds: hot (the Cassie leg and UR5,
compiled into the library), hot-rtc (lefttarsus and wide, compiled for their structure code at run time; the general build where hipRTC
is not installed) and general (IKGPU_CHAIN_HOT=0) -- each model on its two.  Every (model, build) runs both layouts, B = 1, 63, 64, 65,
197 (one lane, a wave less one, a wave, a wave and one, more than one block of either block size with a ragged tail), an iteration
limit of 0 and of 3, the never-stop visitor and a stop rule under which every fifth problem, started at its target, stops at iteration 0.
The starts' entries outside the chain lie partly outside the limits, some exactly on them.

Asserted: the rows outside the chain equal min(hi, max(q0, lo)) where iterations > 0 and q0 where none was taken, bit for bit; q,
success and iterations are bitwise equal between a problem created and solved normally and one created and solved under
IKGPU_PASS_PLAN=0; the same comparison for one tracking call (T = 3) and one multi-start call (K = 2)."""
import os

import numpy as np
import pytest

import chain_shapes_common as CS
import pass_plan_common as PP

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 197)
LIMITS = (0, 3)
TOL = 1e-4
# (model, build): each model on the pre-built or run-time compiled hot program, whichever its chain takes, and on the general one
RUNS = [("cassie_leg", "hot"), ("cassie_leg", "general"), ("tarsus", "hot-rtc"), ("tarsus", "general"), ("ur5", "hot"), ("ur5", "general"),
        ("wide", "hot-rtc"), ("wide", "general")]


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_made = {}


def _setup(torch, name, build):
    """The model, the problem created normally and the one created under IKGPU_PASS_PLAN=0, and the inputs of the largest batch (the
    smaller ones are its leading problems) in both layouts -- made once per (model, build) and left unchanged."""
    import ik_amd
    if (name, build) not in _made:
        c = PP.BY_NAME[name]
        model = ik_amd.Model.from_urdf_xml(c.urdf().encode())
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, c.frame, ik_amd.KinematicType.Full))
        hot = "0" if build == "general" else None
        with env(IKGPU_CHAIN_HOT=hot, IKGPU_PASS_PLAN=None):
            data = ik_amd.dls_data(problem, device=0)
        with env(IKGPU_CHAIN_HOT=hot, IKGPU_PASS_PLAN="0"):
            data_off = ik_amd.dls_data(problem, device=0)
        want = ",%s>" % (build if build != "hot-rtc" or CS.hiprtc_installed() else "general")
        assert data.kernel.endswith(want) and data_off.kernel == data.kernel, (data.kernel, data_off.kernel, want)
        q0, q_near, inside = PP.starts(model, c.frame, max(SIZES), seed=7)
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        TG = ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(q_near.T)).cuda(), data)      # [1, 12, B]
        lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
        _made[name, build] = dict(c=c, model=model, problem=problem, data=data, data_off=data_off, q0=q0, inside=inside, lo=lo, hi=hi, Q0=Q0, TG=TG)
    return _made[name, build]


def _inputs(k, B, layout):
    Q0, TG = k["Q0"][:, :B].contiguous(), k["TG"][:, :, :B].contiguous()
    return (Q0, TG) if layout == "soa" else (Q0.t().contiguous(), TG.permute(2, 0, 1).contiguous())


def _rules(ik_amd):
    for limit in LIMITS:
        yield (limit, "never"), ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=limit)
        yield (limit, "stop"), ik_amd.inverse_kinematics_visitor(TOL), ik_amd.dls_parameters(max_iterations=limit)


def _both(k, call):
    """call(data) on the problem with the plan and on the one without, each under the environment it was created in."""
    with env(IKGPU_PASS_PLAN=None):
        on = [x.cpu().numpy() for x in call(k["data"])]
    with env(IKGPU_PASS_PLAN="0"):
        off = [x.cpu().numpy() for x in call(k["data_off"])]
    return on, off


def _same_bits(on, off, what):
    assert len(on) == len(off)
    for i, (x, y) in enumerate(zip(on, off)):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, i)


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-%s" % r)
def test_single_solves_keep_their_bits_and_follow_the_rule(torch_cuda, run, layout):
    import ik_amd
    k = _setup(torch_cuda, *run)
    out = ~k["inside"]
    assert out.sum() == k["c"].outside
    for B in SIZES:
        q0, tg = _inputs(k, B, layout)
        for rule, visitor, p in _rules(ik_amd):
            on, off = _both(k, lambda data: ik_amd.dls_batch(k["problem"], q0, tg, data, visitor, p, layout=layout))
            _same_bits(on, off, (run, layout, B, rule))
            q, ok, it = on
            q = q if layout == "aos" else q.T
            want = PP.outside_rule(k["q0"][:B], k["lo"], k["hi"], it > 0)
            assert np.array_equal(PP.bits(q[:, out]), PP.bits(want[:, out])), (run, layout, B, rule)
            if rule[1] == "never":
                assert (it == rule[0]).all()
            elif rule[0] > 0 and B >= 63:
                assert (it[::5] == 0).all() and ok[::5].all() and (it > 0).any(), (run, layout, B, rule)      # both rules in one batch
            if rule[0] == 0:
                assert np.array_equal(PP.bits(q), PP.bits(k["q0"][:B]))                                       # no step: nothing is clamped
    if out.any():      # the starts show the clamp: entries outside the chain beyond their limits, on both sides
        assert (k["q0"][:, out] < k["lo"][out]).any() and (k["q0"][:, out] > k["hi"][out]).any()


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-%s" % r)
def test_a_tracking_call_keeps_its_bits(torch_cuda, run):
    torch = torch_cuda
    import ik_amd
    k = _setup(torch, *run)
    B, T = 197, 3
    q0, tg = _inputs(k, B, "soa")
    # waypoint 0 is the single solve's target; the later ones are the same poses rolled by one and two problems
    TG = torch.stack([torch.roll(tg, s, dims=2) for s in range(T)]).contiguous()      # [T, 1, 12, B]
    out = ~k["inside"]
    for rule, visitor, p in _rules(ik_amd):
        if rule[0] == 0:
            continue
        on, off = _both(k, lambda data: ik_amd.dls_track_batch(k["problem"], q0, TG, data, visitor, p))
        _same_bits(on, off, (run, "track", rule))
        q, ok, it = on
        stepped = np.cumsum(it > 0, axis=0) > 0      # slab k: clamped once some waypoint <= k took a step
        for w in range(T):
            want = PP.outside_rule(k["q0"][:B], k["lo"], k["hi"], stepped[w])
            assert np.array_equal(PP.bits(q[w].T[:, out]), PP.bits(want[:, out])), (run, rule, w)


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-%s" % r)
def test_a_multi_start_call_keeps_its_bits(torch_cuda, run):
    import ik_amd
    k = _setup(torch_cuda, *run)
    B = 197
    q0, tg = _inputs(k, B, "soa")
    out = ~k["inside"]
    for rule, visitor, p in _rules(ik_amd):
        if rule[0] == 0:
            continue
        on, off = _both(k, lambda data: ik_amd.dls_multistart_batch(k["problem"], q0, tg, data, visitor, p, num_starts=2, seed=3))
        _same_bits(on, off, (run, "multistart", rule))
        q, ok, it, winner, err = on
        # a generated start draws the chain's entries only: the entries outside the chain are q0's whichever start won
        want = PP.outside_rule(k["q0"][:B], k["lo"], k["hi"], it > 0)
        assert np.array_equal(PP.bits(q.T[:, out]), PP.bits(want[:, out])), (run, rule)
