"""The `out=` argument of the eleven solve entries of ik_amd/api.py: a call into preallocated tensors returns
those very tensors, and every element the job writes carries the bits of the same call with out=None; what a job leaves unwritten
(line and path: slabs beyond min(reached, N - 1); solutions: slots from count on) is not compared.  One small problem -- the ur5 chain,
one Full frame task, B = 5 (no multiple of the wave or of K), K = 4 starts, T = 2 waypoints, P = 2 via poses, G = 2 goals with K = 2 --
in both layouts.  The targets are the frame's poses at configurations near Q0 (task_frames_fk_batch), so that every lane converges and
the line / path comparisons cover whole trajectories: that is asserted, on the device's own `reached`."""
import numpy as np
import pytest

from conftest import urdf_path

pytestmark = pytest.mark.gpu

B, K, T, P, G, KG = 5, 4, 2, 2, 2, 2
OFFSET = 0.05     # rad, per joint and per pose, from Q0 to the configurations the targets are taken from
STEP = 1.0        # max_joint_step of the path entries: well above what a waypoint OFFSET / T away asks for
SENTINEL = {"torch.float64": float("nan"), "torch.uint8": 7, "torch.int32": -7}


@pytest.fixture(scope="module")
def ctx(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ik_amd as ik
    model = ik.Model.from_urdf_file(urdf_path("ur5"))
    problem = ik.InverseKinematicsProblem(model)
    problem.add_frame_task("t", ik.FrameTask.create(model, "tool0", ik.KinematicType.Full))
    data = ik.dls_data(problem, device=0)
    # an elbow-bent posture away from the singular ones, a little different for every problem
    q0 = np.array([0.4, -1.1, 1.3, -0.9, 0.8, 0.3])[None, :] + 0.07 * np.arange(B)[:, None] + 0.03 * np.arange(model.nq)[None, :]
    inputs = {}
    for layout in ("soa", "aos"):
        def dev(q):
            return torch.from_numpy(np.ascontiguousarray(q.T if layout == "soa" else q)).cuda()

        def pose(k):
            return ik.task_frames_fk_batch(problem, dev(q0 + k * OFFSET), data, layout=layout)

        inputs[layout] = dict(Q0=dev(q0), one=pose(1), seq=torch.stack([pose(k) for k in (1, 2)]))
    return dict(torch=torch, ik=ik, model=model, problem=problem, data=data, pik=ik.pik_data(problem, device=0), inputs=inputs)


def _filled(torch, like):
    return torch.full(like.shape, SENTINEL[str(like.dtype)], dtype=like.dtype, device=like.device)


def _per_problem(t, layout, lead):
    """numpy view of an output with the problem axis last and `lead` leading axes kept: [lead..., (nq,) B]."""
    a = t.cpu().numpy()
    return np.moveaxis(a, lead, -1) if layout == "aos" and a.ndim == lead + 2 else a


def _slabs(reached, N):
    return np.arange(N)[:, None] <= np.minimum(reached, N - 1)[None, :]   # [N, B]: slab k <= min(reached, N - 1) is written


def _same(free, kept, layout, written=None, lead=0):
    """Bit-equality of one output of the two calls: all of it, or (written [N, B]) the slabs / slots the job writes."""
    a, b = _per_problem(free, layout, lead), _per_problem(kept, layout, lead)
    assert a.shape == b.shape and a.dtype == b.dtype
    if written is not None:
        m = written if a.ndim == 2 else np.broadcast_to(written[:, None, :], a.shape)
        a, b = a[m], b[m]
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _both(torch, call):
    """call(out) with out=None, then into sentinel-filled tensors of the same shapes: (free, kept), after checking identity."""
    free = call(None)
    out = type(free)(*[None if t is None else _filled(torch, t) for t in free]) if hasattr(free, "_fields") else tuple(_filled(torch, t) for t in free)
    kept = call(out)
    assert len(kept) == len(out) and all(k is o for k, o in zip(kept, out))
    return free, kept


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_out_is_returned_and_holds_the_bits_of_the_allocating_call(ctx, layout):
    torch, ik, problem, data = ctx["torch"], ctx["ik"], ctx["problem"], ctx["data"]
    Q0, one, seq = (ctx["inputs"][layout][k] for k in ("Q0", "one", "seq"))
    v, p = ik.inverse_kinematics_visitor(1e-4), ik.dls_parameters(max_iterations=100)
    kw = dict(layout=layout)
    whole = {
        "dls_batch": lambda out: ik.dls_batch(problem, Q0, one, data, v, p, out=out, **kw),
        "pik_batch": lambda out: ik.pik_batch(problem, Q0, one, ctx["pik"], v, ik.pik_parameters(), out=out, **kw),
        "dls_track_batch": lambda out: ik.dls_track_batch(problem, Q0, seq, data, v, p, out=out, **kw),
        "dls_multistart_batch": lambda out: ik.dls_multistart_batch(problem, Q0, one, data, v, p, num_starts=K, seed=3, out=out, **kw),
        "dls_pick_batch": lambda out: ik.dls_pick_batch(problem, Q0, one, data, v, p, num_starts=K, seed=3, out=out, **kw),
        "dls_goalset_batch": lambda out: ik.dls_goalset_batch(problem, Q0, seq, data, v, p, num_starts=KG, seed=3, out=out, **kw),
    }
    assert seq.shape[0] == T == P == G
    for name, call in whole.items():
        free, kept = _both(torch, call)
        for i, (a, b) in enumerate(zip(free, kept)):
            assert _same(a, b, layout, lead=1 if name == "dls_track_batch" and i == 0 else 0), (name, i)
    assert bool(whole["dls_batch"](None)[1].all()) and bool(whole["dls_track_batch"](None)[1].all())   # every lane converges

    # line and path: reached whole, the other three on the written slabs; at least 4 of the 5 problems travel the whole way
    partial = {
        "dls_line_batch": (T, lambda out: ik.dls_line_batch(problem, Q0, one, data, T, v, p, out=out, **kw)),
        "dls_path_batch": (P * T, lambda out: ik.dls_path_batch(problem, Q0, seq, data, T, STEP, v, p, out=out, **kw)),
    }
    for name, (N, call) in partial.items():
        free, kept = _both(torch, call)
        reached = free[3].cpu().numpy()
        assert (reached == N).sum() >= 4, (name, reached)
        assert _same(free[3], kept[3], layout), name
        for i in range(3):
            assert _same(free[i], kept[i], layout, _slabs(reached, N), lead=1), (name, i)

    # solutions: count whole, Q / which / iterations on the slots below count
    free, kept = _both(torch, lambda out: ik.dls_solutions_batch(problem, Q0, one, data, v, p, num_starts=K, seed=3, out=out, **kw))
    count = free[1].cpu().numpy()
    assert (count >= 1).all() and _same(free[1], kept[1], layout)
    slots = np.arange(K)[:, None] < count[None, :]
    for i in (0, 2, 3):
        assert _same(free[i], kept[i], layout, slots, lead=1), ("dls_solutions_batch", i)

    # path multi-start: the seven scout outputs whole; the trajectory on the written slabs of the problems that entered
    N = (P - 1) * T
    run = lambda out, trajectory=True: ik.dls_path_multistart_batch(problem, Q0, seq, data, T, STEP, v, p, num_starts=K, seed=3, trajectory=trajectory,
                                                                    out=out, **kw)
    free, kept = _both(torch, run)
    assert isinstance(kept, ik.api.PathMultistartResult)
    for name in free._fields[:7]:
        assert _same(getattr(free, name), getattr(kept, name), layout, lead=1 if name == "reached_all" else 0), name
    entered = free.entry_success.cpu().numpy() == 1
    reached = free.reached.cpu().numpy()
    assert (entered & (reached == N)).sum() >= 4, (entered, reached)
    written = _slabs(reached, N) & entered[None, :]
    for name in free._fields[7:]:
        assert _same(getattr(free, name), getattr(kept, name), layout, written, lead=1), name
    bare, bare_kept = _both(torch, lambda out: run(out, trajectory=False))
    for r in (bare, bare_kept):
        assert r.q is None and r.success is None and r.iterations is None
    for name in free._fields[:7]:
        assert _same(getattr(free, name), getattr(bare, name), layout, lead=1 if name == "reached_all" else 0), name
        assert _same(getattr(free, name), getattr(bare_kept, name), layout, lead=1 if name == "reached_all" else 0), name


def test_targets_on_another_device_are_refused(ctx):
    torch, ik = ctx["torch"], ctx["ik"]
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    Q0, one = ctx["inputs"]["soa"]["Q0"], ctx["inputs"]["soa"]["one"]
    with pytest.raises(ValueError):
        ik.dls_batch(ctx["problem"], Q0, one.to("cuda:1"), ctx["data"])
