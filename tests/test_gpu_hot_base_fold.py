"""The base placement folded into the target (ik_amd/csrc/device/chain_hot.hpp hot_fold_base, hot_evaluate<.., BASE_FOLDED>: hot_dls
carries the target into joint 0's frame at entry, the refill loop where a lane takes a target), on the device.

Builds: the Cassie leg and UR5 on the kernels compiled into the library ("hot"), arm7 and run2_whole of tests/hot_fold_common.py -- the
leader of a folded run is joint 0 -- on the kernel compiled for their structure code at run time ("hot-rtc"; hipRTC is required, not
skipped), and the Cassie leg on the general build (device/chain_solver.hpp, which folds nothing).

Inputs: starts uniform in the limits, the target of problem b the frame at clip(q0 + U(-0.15, 0.15)), the project's "near" offset;
where the model has entries of q outside the chain every third problem starts with two of them beyond their limits.  Problem b is the
same whatever B is: the oracle solves the 197 once per iteration count and a batch of B is held to its first B.

Asserted.  Never-stop solves of 0, 1, 2, 7 and 50 iterations at B = 1, 63, 64, 65 and 197 (a lone lane, one short of a wave, a full
wave, one lane into a second wave, three waves and a five-lane tail), AOS and SOA: EVERY entry of q_out,
written over NaN, within 1e-9 rad of the oracle's; the two layouts the same bits.
On the hot builds the jobs of one build give the same bits (B = 65 and 197): single solve = track with T = 1 = multi-start with K = 1
(and with K = 2 from two copies of the start, the launch of the multi-start kernel itself), never-stop and under the default visitor;
lock-step = lane refill = two-phase under the default visitor; a goal set of G x K = 2 x 2 returns the bits of the single solve of
its winning candidate."""
import numpy as np
import pytest

import hot_fold_common as HF
from conftest import urdf_path
from test_gpu_chain_strides import _data, _hiprtc, _solve
from test_gpu_refill import env

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 197)
BMAX = max(BS)
BAR = 1e-9           # rad
ITERS = (0, 1, 2, 7, 50)
CASES = [("cassie_fixed", "LeftFootFront", ",hot>"), ("ur5", "tool0", ",hot>"), ("arm7", "tool", ",hot-rtc>"), ("run2_whole", "tool", ",hot-rtc>"),
         ("cassie_fixed", "LeftFootFront", ",general>")]
IDS = [c[0] + c[2].strip(",>") for c in CASES]


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_cache = {}


def _case(name, frame, want):
    """Model, problem, build and inputs of one case, made once."""
    import ik_amd
    import oracle as O
    key = (name, want)
    if key not in _cache:
        assert want != ",hot-rtc>" or _hiprtc(), "the run-time specialised build needs hipRTC"
        xml = HF.chain_xml(HF.BY_NAME[name]) if name in HF.MADE_UP else open(urdf_path(name)).read()
        model = ik_amd.Model.from_urdf_xml(xml)
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = _data(problem, general=want == ",general>")
        assert data.kernel.endswith(want), data.kernel
        om = O.OracleModel(model.flat())
        fid = model.getFrameId(frame)
        lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
        rng = np.random.default_rng(1971)
        q0 = rng.uniform(lo, hi, (BMAX, lo.size))
        tg = O.fk_batch(om, np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape), lo, hi), [fid])
        outside = np.flatnonzero(~data.support)
        if outside.size >= 2:
            q0[::3, outside[0]] = hi[outside[0]] + 9.0
            q0[::3, outside[-1]] = lo[outside[-1]] - 9.0
        _cache[key] = dict(model=model, problem=problem, data=data, om=om, tasks=O.make_tasks([(fid, 0, 2, 0, None)]), q0=q0, tg=tg, outside=outside)
    return _cache[key]


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
def test_every_entry_against_the_oracle(torch_cuda, name, frame, want):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api
    import oracle as O
    x = _case(name, frame, want)
    data, q0, tg, outside = x["data"], x["q0"], x["tg"], x["outside"]
    worst = {}
    for iters in ITERS:
        q_ref, ok_ref, it_ref = O.dls_batch(x["om"], x["tasks"], tg, q0, O.params(iters, 1e-2, 1.0, -1.0))
        prm = api._params(ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=iters))
        worst[iters] = 0.0
        for B in BS:
            got = {}
            for layout in ("soa", "aos"):
                q, ok, it = _solve(torch, data, prm, q0[:B], tg[:B], layout, True)
                where = (data.kernel, iters, B, layout)
                assert np.isfinite(q).all(), where      # (q_out was NaN: every entry was written)
                d = np.abs(q - q_ref[:B]).max()
                worst[iters] = max(worst[iters], d)
                assert d <= BAR, where + (d,)
                if outside.size:
                    assert np.array_equal(q[:, outside], q_ref[:B][:, outside]), where
                assert np.array_equal(ok, ok_ref[:B]) and np.array_equal(it, it_ref[:B]), where
                got[layout] = q
            assert np.array_equal(got["soa"].view(np.uint64), got["aos"].view(np.uint64)), (data.kernel, iters, B)
    print("%s: max |dq| vs oracle by iteration count: %s" % (data.kernel, "  ".join("%d: %.2e" % kv for kv in worst.items())))


def _same(a, b, where):
    for x, y, what in zip(a, b, ("q", "success", "iterations")):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.shape == y.shape, where + (what, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), where + (what,)


@pytest.mark.parametrize("name,frame,want", CASES[:4], ids=IDS[:4])
@pytest.mark.parametrize("B", [65, 197])
def test_the_jobs_of_one_hot_build_give_the_same_bits(torch_cuda, name, frame, want, B):
    torch = torch_cuda
    import ik_amd
    x = _case(name, frame, want)
    problem, data = x["problem"], x["data"]
    Q0 = torch.from_numpy(np.ascontiguousarray(x["q0"][:B].T)).cuda()
    T = torch.from_numpy(np.ascontiguousarray(x["tg"][:B].transpose(1, 2, 0))).cuda()      # [1, 12, B]
    rules = [("never_stop", ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=7)),
             ("default", ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(max_iterations=100))]
    for rule, v, p in rules:
        where = (data.kernel, rule, B)
        single = ik_amd.dls_batch(problem, Q0, T, data, v, p)
        tracked = ik_amd.dls_track_batch(problem, Q0, T[None].contiguous(), data, v, p)
        _same([t[0] for t in tracked], single, where + ("track T=1",))
        _same(ik_amd.dls_multistart_batch(problem, Q0, T, data, v, p, num_starts=1)[:3], single, where + ("multistart K=1",))
        twice = ik_amd.dls_multistart_batch(problem, Q0, T, data, v, p, num_starts=2, starts=Q0[None].contiguous())
        _same(twice[:3], single, where + ("multistart K=2, the same start twice",))
        assert (twice[3].cpu().numpy() == 0).all(), where
        if rule == "default":
            ok, it = single[1].cpu().numpy(), single[2].cpu().numpy()
            assert ok.sum() >= B // 2 and len(set(it[ok != 0].tolist())) >= 2, where      # the stop rule fired, at different iterations
            for refill in ("1", "2"):
                with env(IKGPU_REFILL=refill):
                    _same(ik_amd.dls_batch(problem, Q0, T, data, v, p), single, where + ("IKGPU_REFILL=" + refill,))
    # a goal set of 2 goals x 2 starts: the bits of the single solve of the winning candidate
    rule, v, p = rules[1]
    G, K = 2, 2
    other = torch.from_numpy(np.ascontiguousarray(np.roll(x["tg"][:B], 1, axis=0).transpose(1, 2, 0))).cuda()
    goals = torch.stack([other, T]).contiguous()                                            # [G, 1, 12, B]; goal 1 is the near one
    starts = ik_amd.multistart_starts(data, Q0, K, seed=5)
    Q, ok, it, goal, start, err, reach = ik_amd.dls_goalset_batch(problem, Q0, goals, data, v, p, num_starts=K, seed=5)
    goal, start = goal.cpu().numpy(), start.cpu().numpy()
    want_q, want_ok, want_it = np.empty_like(Q.cpu().numpy()), np.empty(B, np.uint8), np.empty(B, np.int32)
    for g in range(G):
        for k in range(K):
            sq, sok, sit = ik_amd.dls_batch(problem, Q0 if k == 0 else starts[k - 1].contiguous(), goals[g].contiguous(), data, v, p)
            pick = (goal == g) & (start == k)
            want_q[:, pick], want_ok[pick], want_it[pick] = sq.cpu().numpy()[:, pick], sok.cpu().numpy()[pick], sit.cpu().numpy()[pick]
    assert ((goal >= 0) & (goal < G) & (start >= 0) & (start < K)).all()
    assert np.array_equal(Q.cpu().numpy().view(np.uint64), want_q.view(np.uint64)), (data.kernel, B, "goalset q")
    assert np.array_equal(ok.cpu().numpy(), want_ok) and np.array_equal(it.cpu().numpy(), want_it), (data.kernel, B, "goalset flags")
    print("%s B=%d goal set: winners by candidate %s" % (data.kernel, B, np.bincount(goal * K + start, minlength=G * K).tolist()))
