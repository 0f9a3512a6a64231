"""What fusing a tracked sequence into one launch buys: ikgpu_dls_track_batch (ik_amd.dls_track_batch) against the T chained
ik_amd.dls_batch calls it replaces, on the same stream, in one process.

    python tools/track_timing.py [--T 64] [--reps 5] > profiles/track_timing.txt

Cassie leg (dls_chain<NJ=7,full,hot>) and arm7 (hot-rtc where hipRTC is available), the smooth trajectory of tests/track_common.py
(no jump: waypoint 0 is the start pose, then a steady motion, one repeated waypoint), three cells per robot:
  B = 65536, the default stop rule (100 iterations, 1e-4)      -- the planner's horizon
  B = 65536, never-stop, 10 iterations per waypoint            -- fixed work per waypoint
  B = 1,     the default stop rule                             -- the demo's own tick loop
Device events around `reps` trajectories that end in a synchronise, after a warm-up; the two versions alternate and every cell is
measured twice (the two figures show the run-to-run spread).  Both versions write into preallocated outputs.  Prints ms per
trajectory, microseconds per waypoint and the mean iteration count per waypoint."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import workload
    import track_common

    T = args.T
    print("# device: %s; T = %d waypoints, %d trajectories per measurement" % (torch.cuda.get_device_name(0), T, args.reps))
    for name, frame in (("cassie_fixed", "LeftFootFront"), ("arm7", "tool")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        for B, visitor, p, label in ((65536, ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(), "stop rule 1e-4, <= 100 iterations"),
                                     (65536, ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=10), "never-stop, 10 iterations"),
                                     (1, ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(), "stop rule 1e-4, <= 100 iterations")):
            q0, confs = track_common.configurations(model, name, B, T, jump=False)
            Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
            TG = torch.stack([ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(q.T)).cuda(), data) for q in confs])
            out = (torch.empty((T, model.nq, B), dtype=torch.float64, device="cuda"), torch.empty((T, B), dtype=torch.uint8, device="cuda"),
                   torch.empty((T, B), dtype=torch.int32, device="cuda"))

            def fused():
                ik_amd.dls_track_batch(problem, Q0, TG, data, visitor, p, out=out)

            def chained():
                q = Q0
                for k in range(T):
                    q, _, _ = ik_amd.dls_batch(problem, q, TG[k], data, visitor, p, out=(out[0][k], out[1][k], out[2][k]))

            def measure(fn):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                for _ in range(args.reps):
                    fn()
                stop.record()
                torch.cuda.synchronize()
                return start.elapsed_time(stop) / args.reps

            chained(), torch.cuda.synchronize()
            ref = [o.clone() for o in out]
            fused(), torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip(ref, out))
            mean_it = float(out[2].double().mean())
            for fn in (fused, chained, fused, chained):   # warm-up
                fn()
            ms = {"fused": [], "chained": []}
            for _ in range(2):
                ms["fused"].append(measure(fused))
                ms["chained"].append(measure(chained))
            print("%-36s B = %-6d %s" % (ik_amd.dls_track_kernel(data, visitor, p), B, label))
            print("    mean iterations per waypoint %.2f; outputs bit-identical: %s" % (mean_it, same))
            for k in ("fused", "chained"):
                what = "dls_track_batch, one call " if k == "fused" else "%d chained dls_batch calls" % T
                print("    %-28s %8.4f / %8.4f ms per trajectory   %7.2f / %7.2f us per waypoint" % (what, ms[k][0], ms[k][1], 1e3 * ms[k][0] / T, 1e3 * ms[k][1] / T))
            print("    chained / fused: %.2f / %.2f" % (ms["chained"][0] / ms["fused"][0], ms["chained"][1] / ms["fused"][1]))


if __name__ == "__main__":
    main()
