"""The path job on every chain shape of tests/chain_shapes_common.py: lengths 1 .. 8 x Position / Orientation / Full on the general build,
unit and non-unit weights, a world-fixed oblique reference frame, and the run-time specialised hot build at lengths 1 .. 7
(dls_chain_job_kernel<NJ, KT, SMASK>(a, PathArgs), and the entry ikgpu_hot_path_stop of the run-time compiled module) -- as
tests/test_gpu_chain_shapes.py runs the line job.  B = 65 (a wave and one lane), P = 2, T = 3: via 0 is the case's own target (a near
line from the pose at q0), via 1 the case's line goal (every third one far: paths that leave the workspace or the limits, or get there
through a jump), in the case's reference frame.

Per build and layout: the kernel's name; path_targets -- segment 0 equal to line_targets bit for bit, the last slab of each segment the
via's; dls_path_batch into sentinel-filled outputs np.array_equal to dls_track_batch on path_targets on the written slabs, `reached` equal
to the numpy rule (tests/path_common.py met_rule) on what tracking returned, the sentinels kept elsewhere -- without a bound and with
max_joint_step = 0.5 rad; P = 1 without a bound equal to dls_line_batch."""
import numpy as np
import pytest

import chain_shapes_common as CS
import line_common
import path_common
from test_gpu_chain_shapes import _data, _variant

pytestmark = pytest.mark.gpu

B, P, T, STEP = 65, 2, 3, 0.5


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("c", CS.CASES, ids=CS.case_id)
def test_path_job_of_every_chain_shape_on_the_device(torch_cuda, c):
    torch = torch_cuda
    import ik_amd
    from test_gpu_path import _in_layout, _sentinels
    x = CS.inputs(c)
    goals, _ = CS.line_goals(c)
    q0, nq, N = np.array(x.q0)[:B], x.model.nq, P * T
    vias = np.stack([np.array(x.tg)[:B], np.array(goals)[:B]])                        # [P, B, 1, 12]
    problem = CS.make_problem(c, x.model)
    stop, p100 = ik_amd.inverse_kinematics_visitor(CS.LINE_RULE[1]), ik_amd.dls_parameters(max_iterations=CS.LINE_RULE[0])
    data = _data(problem, general=c.build == "general")
    assert data.kernel == CS.kernel_name(c, CS.hiprtc_installed()), data.kernel
    builds = [data]
    if c.build == "default" and data.kernel.endswith(",hot-rtc>"):
        builds.append(_data(problem, general=True))
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()                          # SoA [nq, B]
    V = torch.from_numpy(np.ascontiguousarray(vias.transpose(0, 2, 3, 1))).cuda()     # SoA [P, 1, 12, B]
    for d in builds:
        assert ik_amd.dls_path_kernel(d, stop, p100) == _variant(d, "_path")
        for layout in ("soa", "aos"):
            ql, vl = _in_layout(Q0, V, layout)
            W = ik_amd.path_targets(problem, ql, vl, d, T, layout=layout)
            assert np.array_equal(W[:T].cpu().numpy(), ik_amd.line_targets(problem, ql, vl[0], d, T, layout=layout).cpu().numpy()), (d.kernel, layout)
            for s in range(P):
                assert np.array_equal(W[s * T + T - 1].cpu().numpy(), vl[s].cpu().numpy()), (d.kernel, layout, s)
            Qt, okt, itt = ik_amd.dls_track_batch(problem, ql, W, d, stop, p100, layout=layout)
            qt = (Qt if layout == "aos" else Qt.permute(0, 2, 1)).cpu().numpy()
            okt, itt = okt.cpu().numpy(), itt.cpu().numpy()
            for step in (0.0, STEP):
                want, _ = path_common.met_rule(okt, qt, q0, x.support, step)
                mask = line_common.written(want, N)
                Ql, ok, it, reached = ik_amd.dls_path_batch(problem, ql, vl, d, T, step, stop, p100, layout=layout, out=_sentinels(torch, N, nq, B, layout))
                q = (Ql if layout == "aos" else Ql.permute(0, 2, 1)).cpu().numpy()
                ok, it, reached = ok.cpu().numpy(), it.cpu().numpy(), reached.cpu().numpy()
                assert np.array_equal(reached, want), (d.kernel, layout, step)
                for a, b_, what in ((q, qt, "q"), (ok, okt, "success"), (it, itt, "iterations")):
                    assert np.array_equal(a[mask], b_[mask]), (d.kernel, layout, step, what)
                assert np.isnan(q[~mask]).all() and (ok[~mask] == 7).all() and (it[~mask] == -7).all(), (d.kernel, layout, step)
            # one segment without a bound: the line job
            line = ik_amd.dls_line_batch(problem, ql, vl[0], d, T, stop, p100, layout=layout, out=_sentinels(torch, T, nq, B, layout))
            one = ik_amd.dls_path_batch(problem, ql, vl[:1].contiguous(), d, T, 0.0, stop, p100, layout=layout, out=_sentinels(torch, T, nq, B, layout))
            for a, b_ in zip(one, line):
                assert np.array_equal(a.cpu().numpy(), b_.cpu().numpy(), equal_nan=a.dtype == torch.float64), (d.kernel, layout, "P = 1")
        print("%s: reached without a bound %s, with %.2f rad %s" % (d.kernel, np.bincount(path_common.met_rule(okt, qt, q0, x.support, 0.0)[0], minlength=N + 1).tolist(),
                                                                    STEP, np.bincount(want, minlength=N + 1).tolist()))
