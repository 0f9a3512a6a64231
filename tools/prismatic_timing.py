"""What the chain kernels buy a robot with a prismatic joint: the builds a chain with sliding joints runs on now -- hot-rtc, and general
(IKGPU_CHAIN_HOT=0) -- against the route such a problem took before, the generic lane program compiled for it at run time
(IKGPU_DLS_KERNEL=generic: dls_generic<...,static>), in one process, on one stream.

    python tools/prismatic_timing.py [--reps 20] [--cells small] > profiles/prismatic_timing.txt

Models (tests/prismatic_common.py, made by string edit): a UR5 on a linear rail along x (NJ = 7, Full) and arm8 with {j3, j6} prismatic,
task frame l7 (NJ = 7, Full, oblique axes).  B = 65536 and B = 1.  Inputs: q0 uniform in the limits, targets the frame at
clip(q0 + U(-0.15, 0.15) s) with s = 1/3 on prismatic entries (the tests' recipe at the tool's batch size).  Measured:
  * 50 fixed iterations (never-stop) of dls_batch on the three routes;
  * dls_track_batch, T = 64 waypoints from q0 towards the target, and dls_path_batch, (P, T) = (3, 16), max_joint_step = 0.25, under
    the default stop rule, on the three routes -- one launch on the chain builds, T (P T) launches of the generic program's loop.
Device events around `reps` calls that end in a synchronise, after a warm-up; the routes alternate over five rounds and the MEDIAN of
the five is reported with the smallest and the largest.  Nothing is gated: the figures are what they are."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

ROUNDS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", default="all", help="all | small (B = 1 only)")
    args = ap.parse_args()
    import torch
    import ik_amd
    import chain_shapes_common as CS
    import prismatic_common as PC
    from test_gpu_refill import env

    print("# device: %s; %d calls per measurement, median (min .. max) of %d alternating rounds, ms per call" % (torch.cuda.get_device_name(0), args.reps, ROUNDS))
    for robot, frame in (("ur5_rail", "tool0"), ("arm8_j3_j6", "l7")):
        model = ik_amd.Model.from_urdf_xml(PC.robot_xml(robot))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        routes = {}
        for label, e in (("hot-rtc", {}), ("general", {"IKGPU_CHAIN_HOT": "0"}), ("generic (the route before)", {"IKGPU_DLS_KERNEL": "generic"})):
            with env(**e):
                routes[label] = ik_amd.dls_data(problem, device=0)
        lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
        flat = model.flat()
        scale = np.ones(model.nq)
        for j in range(1, len(flat["jtype"])):
            if int(flat["jtype"][j]) == 2:
                scale[int(flat["idx_q"][j])] = PC.PRIS_SCALE
        for B in (65536, 1):
            if args.cells == "small" and B > 1:
                continue
            rng = np.random.default_rng(1)
            q0 = rng.uniform(lo, hi, (B, model.nq))
            qs = np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape) * scale, lo, hi)
            dev = lambda q: torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
            Q0 = dev(q0)
            first = routes["general"]
            fk = lambda q: ik_amd.task_frames_fk_batch(problem, dev(q), first)                       # [1, 12, B]
            TG = fk(qs)
            T = 64
            TW = torch.stack([fk(q0 + (k + 1) / T * (qs - q0)) for k in range(T)])                  # [T, 1, 12, B]
            P, PT = 3, 16
            V = torch.stack([fk(np.clip(q0 + (s + 1) / P * 3.0 * (qs - q0), lo, hi)) for s in range(P)])   # [P, 1, 12, B]: three times as far
            never, p50 = ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=50)
            stop, p100 = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(max_iterations=100)
            jobs = (("dls_batch, never-stop, 50 iterations", lambda d: ik_amd.dls_batch(problem, Q0, TG, d, never, p50), lambda d: d.kernel),
                    ("dls_track_batch, T = 64, default rule", lambda d: ik_amd.dls_track_batch(problem, Q0, TW, d, stop, p100), lambda d: ik_amd.dls_track_kernel(d, stop, p100)),
                    ("dls_path_batch, (P, T) = (3, 16), max_joint_step 0.25, default rule",
                     lambda d: ik_amd.dls_path_batch(problem, Q0, V, d, PT, 0.25, stop, p100), lambda d: ik_amd.dls_path_kernel(d, stop, p100)))

            def measure(fn):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                for _ in range(args.reps):
                    fn()
                end.record()
                torch.cuda.synchronize()
                return start.elapsed_time(end) / args.reps

            for what, call, name in jobs:
                print("%s / %s, B = %d: %s" % (robot, frame, B, what))
                ms = {label: [] for label in routes}
                for label, d in routes.items():      # warm-up
                    call(d), call(d)
                for _ in range(ROUNDS):
                    for label, d in routes.items():
                        ms[label].append(measure(lambda: call(d)))
                base = float(np.median(ms["generic (the route before)"]))
                for label, d in routes.items():
                    m = float(np.median(ms[label]))
                    print("    %-28s %-46s %9.4f (%9.4f .. %9.4f)   generic / this = %.2f" % (label, name(d), m, min(ms[label]), max(ms[label]), base / m))
    return 0


if __name__ == "__main__":
    sys.exit(main())
