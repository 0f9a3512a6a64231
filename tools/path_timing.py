"""What the path job buys: ikgpu_dls_path_batch (ik_amd.dls_path_batch, one launch that reads P via poses per problem, applies the
joint-step rule on the lane and leaves a path at its first waypoint that was not met) against what a caller does without it, on the same
stream, in one process.

    python tools/path_timing.py [--reps 3] > profiles/path_timing.txt

Baselines, both ending in the same torch code (`rule` below) that applies the met rule -- stop-rule flag and joint step -- and counts
the leading met waypoints:
  (a) P chained ik_amd.dls_line_batch calls, segment s started from the last configuration of segment s - 1 (so from the pose at that
      result, not from the via itself), their outputs written into one [P T] trajectory;
  (b) ik_amd.path_targets + ik_amd.dls_track_batch: the definition.
Configurations: Cassie leg and UR5, B in {1, 4096, 65536}, (P, T) = (3, 16), max_joint_step 0 and the robot's threshold of
tests/path_common.py, the default stop rule (100 iterations, 1e-4); once with every path feasible (resampled from the paths of the
recipe that the job follows to the end under the threshold) and once with the recipe of tests/path_common.py as drawn (a pool of 4096
paths, resampled to B).  Device events around `reps` calls that end in a synchronise, after a warm-up; the three sides alternate over
five rounds and the median is printed with the smallest and largest round.  All sides write into preallocated outputs; the waypoints of
(b) are a fresh tensor per call, as a caller's would be.  Also printed: whether `reached` and the written slabs of the launch equal (b)'s."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

P, T, POOL, ROUNDS = 3, 16, 4096, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--B", type=int, nargs="*", default=[1, 4096, 65536])
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import workload
    import line_common
    import path_common

    N = P * T
    visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
    print("# device: %s; P = %d via poses, T = %d waypoints per segment, %d calls per measurement, median (min .. max) of %d alternating rounds, ms per call"
          % (torch.cuda.get_device_name(0), P, T, args.reps, ROUNDS))

    def measure(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.reps

    for name, frame in (("cassie_fixed", "LeftFootFront"), ("ur5", "tool0")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        threshold = path_common.JOINT_STEP[name]
        sup = torch.from_numpy(np.flatnonzero(data.support)).cuda()
        dev = lambda q0, vias: (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.from_numpy(np.ascontiguousarray(vias.transpose(0, 2, 3, 1))).cuda())
        pq0, pvias = path_common.inputs_exact(model, frame, POOL, P, 0)
        done = ik_amd.dls_path_batch(problem, *dev(pq0, pvias), data, T, threshold, visitor, p)[3].cpu().numpy()
        good = np.flatnonzero(done == N)
        print("# %s: %s; %d of the %d drawn paths are followed to the end under %.2f rad" % (name, ik_amd.dls_path_kernel(data, visitor, p), len(good), POOL, threshold))
        rng = np.random.default_rng(0)

        def rule(Q, ok, Q0, step):
            """reached [B] from the tracking outputs Q [N, nq, B], ok [N, B]: the leading waypoints that met the stop rule without a jump."""
            met = ok.bool()
            if step > 0:
                prev = torch.cat([Q0[None], Q[:-1]])
                met = met & ~((Q - prev).abs().index_select(1, sup) > step).any(dim=1)
            return met.to(torch.int32).cumprod(dim=0).sum(dim=0).to(torch.int32)

        for B in args.B:
            for mix in ("every path feasible", "the recipe as drawn"):
                pick = good[rng.integers(0, len(good), B)] if mix.startswith("every") else rng.integers(0, POOL, B)
                Q0, V = dev(pq0[pick], np.ascontiguousarray(pvias[:, pick]))
                for step in (0.0, threshold):
                    outs = {k: (torch.zeros((N, model.nq, B), dtype=torch.float64, device="cuda"), torch.zeros((N, B), dtype=torch.uint8, device="cuda"),
                                torch.zeros((N, B), dtype=torch.int32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda")) for k in "pab"}
                    got = {}

                    def path():
                        ik_amd.dls_path_batch(problem, Q0, V, data, T, step, visitor, p, out=outs["p"])
                        got["p"] = outs["p"][3]

                    def lines():
                        Q, ok, it, _ = outs["a"]
                        q = Q0
                        for s in range(P):
                            seg = slice(s * T, (s + 1) * T)
                            ik_amd.dls_line_batch(problem, q, V[s], data, T, visitor, p, out=(Q[seg], ok[seg], it[seg], outs["a"][3]))
                            q = Q[(s + 1) * T - 1]
                        got["a"] = rule(Q, ok, Q0, step)

                    def track():
                        Q, ok, it, _ = outs["b"]
                        ik_amd.dls_track_batch(problem, Q0, ik_amd.path_targets(problem, Q0, V, data, T), data, visitor, p, out=(Q, ok, it))
                        got["b"] = rule(Q, ok, Q0, step)

                    sides = (("p", path, "dls_path_batch, one launch"), ("a", lines, "(a) %d x dls_line_batch + rule" % P), ("b", track, "(b) path_targets + dls_track_batch + rule"))
                    for _, fn, _ in sides:   # warm-up, and the results that are compared
                        fn()
                    torch.cuda.synchronize()
                    r = got["p"].cpu().numpy()
                    mask = torch.from_numpy(line_common.written(r, N)).cuda()
                    sel = lambda a: (a.permute(0, 2, 1) if a.dim() == 3 else a)[mask]
                    same = bool(torch.equal(got["p"], got["b"])) and all(torch.equal(sel(x), sel(y)) for x, y in zip(outs["p"][:3], outs["b"][:3]))
                    ms = {k: [] for k, _, _ in sides}
                    for _ in range(ROUNDS):
                        for k, fn, _ in sides:
                            ms[k].append(measure(fn))
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    print("%s  B = %d  %s  max_joint_step = %.2f" % (name, B, mix, step))
                    print("    complete paths %d of %d (baseline (a): %d); reached and written slabs equal to (b): %s"
                          % (int((r == N).sum()), B, int((got["a"].cpu().numpy() == N).sum()), same))
                    for k, _, what in sides:
                        print("    %-44s %9.4f (%9.4f .. %9.4f)" % (what, med[k], min(ms[k]), max(ms[k])))
                    print("    (a) / path: %.2f    (b) / path: %.2f" % (med["a"] / med["p"], med["b"] / med["p"]))


if __name__ == "__main__":
    main()
