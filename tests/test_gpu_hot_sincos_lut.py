"""sin / cos of the hot chain kernels from the 1024-entry table in LDS (ik_amd/csrc/device/lane_math.hpp dsincos_lut,
device/chain_hot.hpp HotTableLds: every hot entry stages the table and hot_evaluate reads it), on the device.

Builds: the Cassie leg and UR5 on the kernels compiled into the library ("hot"), arm7 on the kernel compiled for its structure code at
run time ("hot-rtc"; skipped without hipRTC).  Inputs as tests/test_gpu_hot_base_fold.py: starts uniform in the limits, the target of
problem b the frame at clip(q0 + U(-0.15, 0.15)); problem b is the same whatever B is.

Asserted.
 * Never-stop solves of 0, 1, 2, 7 and 50 iterations at B = 1, 63, 64, 65 and 197: every entry of q_out within 1e-9 rad of the oracle's.
 * B = 65 and 197: single solve = track with T = 1 = multi-start with K = 1, never-stop and under the default visitor; under the default
   visitor IKGPU_REFILL=0 (lock-step) = IKGPU_REFILL=1 (lane refill): every job stages and reads the same table.
 * Index wrap: starts +-50 rad and +-3000 rad away from the limits on every chain joint.  A multi-start call with K = 1 and no iteration
   returns |e|^2 of the evaluation at that unclipped q0: held to the oracle's e there within E_BAR = 1e-11 (the host tests' bar for e,
   with tests/hot_fold_common.py's allowance towards a rotation by pi) plus the reduction term: dsincos_lut's angle is off by up to
   4e-17 |x| per joint, and a joint's angle moves e by at most 1 rad/rad in its rotation part and REACH = 2 m/rad in its translation
   part (the fixture chains are shorter than that), NJ joints.  One never-stop iteration from there is held to the oracle's q as well
   (1e-9 rad: the step lands on the limits).
 * NaN isolation: a lane whose q0 holds a NaN leaves the bits of its 63 neighbours unchanged.
 * HIP graph: one capture and two replays of the single solve return the eager bits (static LDS: nothing to allocate)."""
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
E_BAR, E_BAR_NEAR_PI = 1e-11, 1e-6
REDUCTION, REACH = 4e-17, 2.0
ITERS = (0, 1, 2, 7, 50)
CASES = [("cassie_fixed", "LeftFootFront", ",hot>"), ("ur5", "tool0", ",hot>"), ("arm7", "tool", ",hot-rtc>")]
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
        if want == ",hot-rtc>" and not _hiprtc():
            pytest.skip("hipRTC is not installed")
        model = ik_amd.Model.from_urdf_xml(open(urdf_path(name)).read())
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = _data(problem, general=False)
        assert data.kernel.endswith(want), data.kernel
        om = O.OracleModel(model.flat())
        fid = model.getFrameId(frame)
        lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
        rng = np.random.default_rng(1024)
        q0 = rng.uniform(lo, hi, (BMAX, lo.size))
        tg = O.fk_batch(om, np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape), lo, hi), [fid])
        _cache[key] = dict(model=model, problem=problem, data=data, om=om, tasks=O.make_tasks([(fid, 0, 2, 0, None)]), q0=q0, tg=tg, lo=lo, hi=hi,
                           chain=np.flatnonzero(data.support))
    return _cache[key]


def _dev(torch, q0, tg):
    return (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda())


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
def test_every_entry_against_the_oracle(torch_cuda, name, frame, want):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api
    import oracle as O
    x = _case(name, frame, want)
    data, q0, tg = x["data"], x["q0"], x["tg"]
    worst = {}
    for iters in ITERS:
        q_ref, ok_ref, it_ref = O.dls_batch(x["om"], x["tasks"], tg, q0, O.params(iters, 1e-2, 1.0, -1.0))
        prm = api._params(ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=iters))
        worst[iters] = 0.0
        for B in BS:
            q, ok, it = _solve(torch, data, prm, q0[:B], tg[:B], "soa", True)
            where = (data.kernel, iters, B)
            assert np.isfinite(q).all(), where      # (q_out was NaN: every entry was written)
            d = np.abs(q - q_ref[:B]).max()
            worst[iters] = max(worst[iters], d)
            assert d <= BAR, where + (d,)
            assert np.array_equal(ok, ok_ref[:B]) and np.array_equal(it, it_ref[:B]), where
    print("%s: max |dq| vs oracle by iteration count: %s" % (data.kernel, "  ".join("%d: %.2e" % kv for kv in worst.items())))


def _same(a, b, where):
    for x, y, what in zip(a, b, ("q", "success", "iterations")):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.shape == y.shape, where + (what, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), where + (what,)


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
@pytest.mark.parametrize("B", [65, 197])
def test_the_jobs_of_one_build_give_the_same_bits(torch_cuda, name, frame, want, B):
    torch = torch_cuda
    import ik_amd
    x = _case(name, frame, want)
    problem, data = x["problem"], x["data"]
    Q0, T = _dev(torch, x["q0"][:B], x["tg"][:B])
    rules = [("never_stop", ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=7)),
             ("default", ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(max_iterations=100))]
    for rule, v, p in rules:
        where = (data.kernel, rule, B)
        single = ik_amd.dls_batch(problem, Q0, T, data, v, p)
        tracked = ik_amd.dls_track_batch(problem, Q0, T[None].contiguous(), data, v, p)
        _same([t[0] for t in tracked], single, where + ("track T=1",))
        _same(ik_amd.dls_multistart_batch(problem, Q0, T, data, v, p, num_starts=1)[:3], single, where + ("multistart K=1",))
        if rule == "default":
            ok, it = single[1].cpu().numpy(), single[2].cpu().numpy()
            assert ok.sum() >= B // 2 and len(set(it[ok != 0].tolist())) >= 2, where      # the stop rule fired, at different iterations
            got = {}
            for refill in ("0", "1"):
                with env(IKGPU_REFILL=refill):
                    got[refill] = ik_amd.dls_batch(problem, Q0, T, data, v, p)
            _same(got["0"], got["1"], where + ("IKGPU_REFILL=0 against 1",))
            _same(got["0"], single, where + ("IKGPU_REFILL=0",))


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
def test_starts_far_outside_the_limits_wrap_the_index(torch_cuda, name, frame, want):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api
    import oracle as O
    x = _case(name, frame, want)
    problem, data, lo, hi, chain = x["problem"], x["data"], x["lo"], x["hi"], x["chain"]
    B = 64
    q0, tg = x["q0"][:B].copy(), x["tg"][:B]
    far = np.empty(B)
    for b in range(B):   # +50, -50, +3000, -3000 by problem, every chain joint alike; the in-limits draw stays on top
        far[b] = (50.0, -50.0, 3000.0, -3000.0)[b % 4]
        q0[b, chain] += far[b]
    assert (q0[:, chain] > hi[chain]).all(axis=1)[far > 0].all() and (q0[:, chain] < lo[chain]).all(axis=1)[far < 0].all()
    Q0, T = _dev(torch, q0, tg)
    v = ik_amd.never_stop_visitor()
    err = ik_amd.dls_multistart_batch(problem, Q0, T, data, v, ik_amd.dls_parameters(max_iterations=0), num_starts=1)[4].cpu().numpy()
    eo = np.array([O.evaluate(x["om"], x["tasks"], tg[b], q0[b])[0] for b in range(B)])
    en = np.linalg.norm(eo, axis=1)
    reduction = chain.size * REDUCTION * (np.abs(far) + 2 * np.pi) * (1.0 + REACH)
    de = HF.conditioned(np.linalg.norm(eo[:, 3:], axis=1), E_BAR + reduction, E_BAR_NEAR_PI, E_BAR)      # per entry of e
    bar = 2.0 * en * np.sqrt(6.0) * de + 6.0 * de * de                                                    # of |e|^2
    d = np.abs(err - en * en)
    print("%s: |e|^2 at starts +-50 / +-3000 rad outside: worst share of its bar %.3f (max |d| %.2e, bars %.1e .. %.1e)"
          % (data.kernel, (d / bar).max(), d.max(), bar.min(), bar.max()))
    assert np.isfinite(err).all() and (d <= bar).all(), (int(np.argmax(d / bar)), d.max())
    # and one iteration from there
    q_ref, _, _ = O.dls_batch(x["om"], x["tasks"], tg, q0, O.params(1, 1e-2, 1.0, -1.0))
    q, _, _ = _solve(torch, data, api._params(v, ik_amd.dls_parameters(max_iterations=1)), q0, tg, "soa", True)
    assert np.isfinite(q).all() and np.abs(q - q_ref).max() <= BAR + chain.size * reduction.max(), np.abs(q - q_ref).max()


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
def test_a_nan_start_stays_in_its_lane(torch_cuda, name, frame, want):
    torch = torch_cuda
    import ik_amd
    from ik_amd import api
    x = _case(name, frame, want)
    data, chain = x["data"], x["chain"]
    q0, tg = x["q0"][:64].copy(), x["tg"][:64]
    prm = api._params(ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=7))
    clean, _, _ = _solve(torch, data, prm, q0, tg, "soa", True)
    for lane, joint in ((0, chain[0]), (37, chain[-1])):
        bad = q0.copy()
        bad[lane, joint] = np.nan
        q, _, _ = _solve(torch, data, prm, bad, tg, "soa", True)
        others = np.arange(64) != lane
        assert np.array_equal(q[others].view(np.uint64), clean[others].view(np.uint64)), (data.kernel, lane)


@pytest.mark.parametrize("name,frame,want", CASES, ids=IDS)
def test_hip_graph_capture_and_two_replays(torch_cuda, name, frame, want):
    torch = torch_cuda
    import ik_amd
    x = _case(name, frame, want)
    problem, data, B = x["problem"], x["data"], 197
    Q0, T = _dev(torch, x["q0"][:B], x["tg"][:B])
    v, p = ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=7)
    ref = ik_amd.dls_batch(problem, Q0, T, data, v, p)
    out = (torch.empty_like(Q0), torch.empty(B, dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ik_amd.dls_batch(problem, Q0, T, data, v, p, out=out)
    for _ in range(2):
        out[0].fill_(float("nan")), out[1].fill_(7), out[2].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        _same(out, ref, (data.kernel, "graph replay"))
