"""Which exception each device-tensor entry point of ik_amd/api.py raises for a wrong call, and WHICH of two simultaneous mistakes is
reported, is part of the Python layer's contract: scalar arguments first, then dimensions and shapes
(ValueError), then an argument that is no float64 CUDA tensor (TypeError) -- all before `data` is looked at, which is why most rows
pass data=None.  dls_batch, pik_batch, evaluate_batch and task_frames_fk_batch bind `data` first and test the type before the shape
(dls_batch / pik_batch also take numpy arrays, whose shapes are then tested); multistart_starts reads nq from `data`, so without
one it can test only the count of dimensions (ValueError, first) and the type.  One table, one row per entry point; the same bad calls go to every row that has the argument, each as
numpy arrays and as CPU tensors, so every wrong shape is also a combined case (wrong shape in the wrong container).  No device is
touched: nothing here is a CUDA tensor, and the one call that reaches the C ABI carries a null problem, which it refuses first."""
import numpy as np
import pytest

from conftest import urdf_path

B, T, P, G, K = 8, 5, 3, 4, 4


@pytest.fixture(scope="module")
def rows(native_built):
    import ik_amd as ik
    from ik_amd import capi
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))

    class Unbound(ik.pik_data):
        """Stands in for a workspace in the entries that bind it before they look at their arguments: no handle, no device."""
        def __init__(self):
            self._h, self._device, self.rows, self.lambda_, self.da = None, 0, 6, [1.0], np.zeros(m.nv)

        def _bind(self, problem):
            pass

    u = Unbound()
    VE, TE = ValueError, TypeError
    # name: (call(q, x, layout, **kw), leading extents of x (None: the entry takes q alone), order, keywords it has, bad scalars)
    #   order "shape": a wrong shape is reported before a wrong container; "type": the other way round; "dims": as "type", but a Q0
    #   that has not 2 dimensions comes before the container; "host": as "type", and numpy arrays are a valid container (their
    #   shapes are tested, right ones reach the C ABI's refusal of a null problem)
    starts = [dict(num_starts=k) for k in (0, 65, -3, 2.0, None)]
    steps = [dict(max_joint_step=s) for s in (float("nan"), float("inf"), -0.1, "0.5")]
    waypoints = [dict(T=-1), dict(T=2.0)]
    table = {
        "dls_batch": (lambda q, x, layout, **kw: ik.dls_batch(p, q, x, u, layout=layout, **kw), (), "host", (), []),
        "pik_batch": (lambda q, x, layout, **kw: ik.pik_batch(p, q, x, u, layout=layout, **kw), (), "host", (), []),
        "dls_track_batch": (lambda q, x, layout, **kw: ik.dls_track_batch(p, q, x, None, layout=layout, **kw), (T,), "shape", (), []),
        "line_targets": (lambda q, x, layout, T=T: ik.line_targets(p, q, x, None, T, layout=layout), (), "shape", (), waypoints),
        "dls_line_batch": (lambda q, x, layout, T=T, **kw: ik.dls_line_batch(p, q, x, None, T, layout=layout, **kw), (), "shape", (), waypoints),
        "path_targets": (lambda q, x, layout, T=T: ik.path_targets(p, q, x, None, T, layout=layout), (P,), "shape", (), waypoints),
        "dls_path_batch": (lambda q, x, layout, T=T, max_joint_step=0.5, **kw: ik.dls_path_batch(p, q, x, None, T, max_joint_step, layout=layout, **kw),
                           (P,), "shape", (), waypoints + steps),
        "dls_multistart_batch": (lambda q, x, layout, num_starts=K, **kw: ik.dls_multistart_batch(p, q, x, None, num_starts=num_starts, layout=layout, **kw),
                                 (), "shape", ("starts",), starts),
        "dls_path_multistart_batch": (lambda q, x, layout, T=T, max_joint_step=0.5, num_starts=K, **kw: ik.dls_path_multistart_batch(
            p, q, x, None, T, max_joint_step, num_starts=num_starts, layout=layout, **kw), (P,), "shape", ("starts",), starts + waypoints + steps),
        "dls_pick_batch": (lambda q, x, layout, num_starts=K, **kw: ik.dls_pick_batch(p, q, x, None, num_starts=num_starts, layout=layout, **kw),
                           (), "shape", ("starts", "q_ref", "weights"), starts + [dict(rule=r) for r in (4, -1, "closest")]),
        "dls_solutions_batch": (lambda q, x, layout, num_starts=K, **kw: ik.dls_solutions_batch(p, q, x, None, num_starts=num_starts, layout=layout, **kw),
                                (), "shape", ("starts",), starts + [dict(max_solutions=n) for n in (0, K + 1, -1, 2.0)]
                                + [dict(separation=s) for s in (-0.5, float("inf"), float("nan"))]),
        "dls_goalset_batch": (lambda q, x, layout, num_starts=K, **kw: ik.dls_goalset_batch(p, q, x, None, num_starts=num_starts, layout=layout, **kw),
                              (G,), "shape", ("starts",), starts + [dict(num_starts=17)]),   # (17 x 4 goals > 64 candidates)
        "multistart_starts": (lambda q, x, layout, num_starts=K: ik.multistart_starts(None, q, num_starts, layout=layout), None, "dims", (), starts),
        "evaluate_batch": (lambda q, x, layout, **kw: ik.evaluate_batch(p, q, x, u, layout=layout, **kw), (), "type", (), []),
        "task_frames_fk_batch": (lambda q, x, layout: ik.task_frames_fk_batch(p, q, u, layout=layout), None, "type", (), []),
    }
    return dict(table=table, nq=m.nq, VE=VE, TE=TE, null_problem=capi.IkgpuError)


ENTRIES = ("dls_batch", "pik_batch", "dls_track_batch", "line_targets", "dls_line_batch", "path_targets", "dls_path_batch", "dls_multistart_batch",
           "dls_path_multistart_batch", "dls_pick_batch", "dls_solutions_batch", "dls_goalset_batch", "multistart_starts", "evaluate_batch",
           "task_frames_fk_batch")


def _numpy(shape):
    return np.zeros(shape)


def _cpu(shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64)


def _right(nq, lead, layout):
    lead = lead or ()
    return ((nq, B), lead + (1, 12, B)) if layout == "soa" else ((B, nq), lead + (B, 1, 12))


def _wrong_shapes(nq, lead, name):
    """(layout, shape of q, shape of x), each wrong in one way."""
    q, x = _right(nq, lead, "soa")
    qa, xa = _right(nq, lead, "aos")
    wrong = [("soa", (nq + 1, B), x),        # nq
             ("aos", q, xa), ("aos", (B,), xa)]   # Q0 in the other layout; a 1-D Q0
    if lead is None:
        return wrong
    wrong += [("soa", q, lead + (1, 12, B + 1)),   # batch extent of the second argument
              ("soa", q, lead + (2, 12, B)),       # target slots
              ("soa", q, lead + (1, 7, B)),        # doubles per slot
              ("aos", qa, x),                      # the second argument in the other layout
              ("soa", q, (T,) + x),                # one leading axis too many
              ("soa", q, x[1:])]                   # one axis too few
    if name in ("path_targets", "dls_path_batch", "dls_path_multistart_batch", "dls_goalset_batch"):
        wrong.append(("soa", q, (0,) + x[1:]))     # no via pose / no goal
    if name == "dls_goalset_batch":
        wrong.append(("soa", q, (65,) + x[1:]))    # more goals than candidates
    return wrong


@pytest.mark.parametrize("name", ENTRIES)
def test_wrong_shapes_and_containers(rows, name):
    call, lead, order, _, _ = rows["table"][name]
    nq, VE, TE = rows["nq"], rows["VE"], rows["TE"]
    for make in (_numpy, _cpu):
        host = order == "host" and make is _numpy
        for layout in ("soa", "aos"):   # right shapes, wrong container
            q, x = _right(nq, lead, layout)
            with pytest.raises(rows["null_problem"] if host else TE):
                call(make(q), make(x), layout)
        for layout, q, x in _wrong_shapes(nq, lead, name):
            with pytest.raises(VE if order == "shape" or host or (order == "dims" and len(q) != 2) else TE):
                call(make(q), make(x), layout)
        # mixed containers: the one that is no tensor decides
        if lead is not None and order != "host":
            q, x = _right(nq, lead, "soa")
            for a, b in ((_numpy, _cpu), (_cpu, _numpy)):
                with pytest.raises(TE):
                    call(a(q), b(x), "soa")
    q, x = _right(nq, lead, "soa")
    with pytest.raises(KeyError):
        call(_numpy(q), _numpy(x), "rows")
    with pytest.raises(KeyError):
        call(_cpu(q), _cpu(x), "rows")


@pytest.mark.parametrize("name", [n for n in ENTRIES if n not in ("dls_batch", "pik_batch", "dls_track_batch", "evaluate_batch", "task_frames_fk_batch")])
def test_bad_scalars_come_first(rows, name):
    call, lead, _, _, scalars = rows["table"][name]
    q, x = _right(rows["nq"], lead, "soa")
    assert scalars
    for kw in scalars:
        for make in (_numpy, _cpu):   # right shapes in the wrong container: the scalar is reported, not the container
            with pytest.raises(rows["VE"]):
                call(make(q), make(x), "soa", **kw)
        with pytest.raises(rows["VE"]):   # ... and with a wrong shape as well
            call(_cpu((rows["nq"] + 1, B)), _cpu(x), "soa", **kw)


@pytest.mark.parametrize("name", ["dls_multistart_batch", "dls_path_multistart_batch", "dls_pick_batch", "dls_solutions_batch", "dls_goalset_batch"])
def test_optional_arguments_of_the_wrong_shape(rows, name):
    call, lead, _, has, _ = rows["table"][name]
    nq, VE, TE = rows["nq"], rows["VE"], rows["TE"]
    for layout in ("soa", "aos"):
        q, x = _right(nq, lead, layout)
        for make in (_numpy, _cpu):
            for shape in ((K,) + q, (K - 1,) + q[::-1], q, (K - 1,) + q + (1,)):
                for others in (_numpy, _cpu):   # a shape error whatever the arrays are
                    with pytest.raises(VE):
                        call(others(q), others(x), layout, starts=make(shape))
            with pytest.raises(TE):   # the right shape: the container is reported
                call(make(q), make(x), layout, starts=make((K - 1,) + q))
            if "q_ref" in has:
                for shape in (q[::-1], (1,) + q, q[:1]):
                    with pytest.raises(VE):
                        call(make(q), make(x), layout, q_ref=make(shape))
                with pytest.raises(TE):
                    call(make(q), make(x), layout, q_ref=make(q))
            if "weights" in has:
                for n in (nq - 1, nq + 1, 0):
                    with pytest.raises(VE):
                        call(make(q), make(x), layout, weights=[1.0] * n)
                with pytest.raises(TE):
                    call(make(q), make(x), layout, weights=[1.0] * nq)
