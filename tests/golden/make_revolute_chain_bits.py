"""Records what the chain kernels compute for two chains of revolute joints, for tests/test_gpu_prismatic_chain.py
(test_chains_of_revolute_joints_compute_the_recorded_bits): run ONCE on an MI355X with the library as it was before the chain kernels
took prismatic joints (IKGPU_LIB points the package at another libikgpu.so):

    IKGPU_LIB=<the earlier build>/libikgpu.so python tests/golden/make_revolute_chain_bits.py tests/golden/revolute_chain_bits.npy

Cases: arm8 / l7 Full (tests/chain_shapes_common.py; run-time compiled hot build) and the Cassie leg (cassie_fixed / LeftFootFront;
pre-built hot build), each also on its general build.  B = 197.  Per case and build four slots [B, NQ_MAX + 2]: the device's iterates
1, 2, 3 from the ORACLE's iterates 0, 1, 2 (one never-stop iteration each), and the default rule with 100 iterations; columns: q padded
with zeros, then the success flag and the iteration count."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE)), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

NQ_MAX = 16
LABELS = ("arm8/l7 default", "arm8/l7 general", "cassie leg default", "cassie leg general")
SLOTS = ("step 1", "step 2", "step 3", "default rule")


def _problems():
    import ik_amd
    import chain_shapes_common as CS
    from ik_amd import workload
    import oracle as O
    c = next(k for k in CS.HOT_CASES if k.nj == 7 and k.reference == "universe")
    x = CS.inputs(c)
    yield CS.make_problem(c, x.model), x.om, x.tasks, np.array(x.q0), np.array(x.tg)
    model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, "cassie_fixed.kin.urdf"))
    problem = ik_amd.InverseKinematicsProblem(model)
    problem.add_frame_task("lf", ik_amd.FrameTask.create(model, "LeftFootFront", ik_amd.KinematicType.Full))
    q0, qs = workload.chain_workload(model.lowerPositionLimit, model.upperPositionLimit, workload.cassie_nominal(model.names), np.arange(CS.B), seed=0, mode="near")
    om = O.OracleModel(model.flat())
    fid = model.getFrameId("LeftFootFront")
    yield problem, om, O.make_tasks([(fid, 0, 2, 0, None)]), q0, O.fk_batch(om, qs, [fid])


def compute():
    """[len(LABELS), len(SLOTS), B, NQ_MAX + 2] from the library the package loads, on cuda:0."""
    import torch
    import ik_amd
    import oracle as O
    from test_gpu_refill import env
    out = []
    never, stop = ik_amd.never_stop_visitor(), ik_amd.inverse_kinematics_visitor()
    p1, p100 = ik_amd.dls_parameters(max_iterations=1), ik_amd.dls_parameters(max_iterations=100)
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
    for problem, om, tasks, q0, tg in _problems():
        T = torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()
        for general in (False, True):
            with env(IKGPU_CHAIN_HOT="0" if general else None):
                data = ik_amd.dls_data(problem, device=0)
            assert data.kernel.endswith(",general>") == general, data.kernel
            slots, q = [], q0
            for k in range(3):
                Q, ok, it = ik_amd.dls_batch(problem, dev(q), T, data, never, p1)
                slots.append((Q, ok, it))
                q, _, _ = O.dls_batch(om, tasks, tg, q, O.params(1, 1e-2, 1.0, -1.0))
            slots.append(ik_amd.dls_batch(problem, dev(q0), T, data, stop, p100))
            rows = np.zeros((len(SLOTS), q0.shape[0], NQ_MAX + 2))
            for i, (Q, ok, it) in enumerate(slots):
                rows[i, :, :q0.shape[1]] = Q.cpu().numpy().T
                rows[i, :, NQ_MAX], rows[i, :, NQ_MAX + 1] = ok.cpu().numpy(), it.cpu().numpy()
            out.append(rows)
    return np.stack(out)


if __name__ == "__main__":
    np.save(sys.argv[1], compute())
    print("wrote %s" % sys.argv[1])
