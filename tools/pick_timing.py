"""What choosing the winner in the launch buys: ikgpu_dls_pick_batch (ik_amd.dls_pick_batch) against the composition it replaces -- K x
ik_amd.dls_batch from ikgpu_multistart_starts' starts, K x ik_amd.evaluate_batch where the rule needs the Jacobian, the cost and the
arg-min in torch, the gather -- and against ik_amd.dls_multistart_batch at the same K, on one stream, in one process.

    python tools/pick_timing.py [--reps 5] [--cells small] > profiles/pick_timing.txt

ur5 (dls_chain<NJ=6,full,hot>) and arm7 (dls_chain<NJ=7,full,hot-rtc>); targets and starts uniform between the joint limits
(tests/multistart_common.py); B in {1, 4096, 65536} x K in {4, 8}, the default stop rule (100 iterations, 1e-4); the rules DISTANCE (from a
uniform q_ref, weights 0.25 .. 2: no Jacobian) and MANIPULABILITY (the Jacobian).  All versions take the SAME K - 1 caller's starts and
write into preallocated outputs.  Device events around `reps` calls that end in a synchronise, after a warm-up; the three versions
alternate over five rounds and the median is printed.  Checked per cell, over the problems in which some start converged (the
composition has no error fall-back): winner / Q / success / iterations equal; a problem whose winner differs is counted and its two
costs printed (torch.linalg.det rounds differently from the lane's L D L^T: a near-tie may go the other way).  No speed is promised:
the ratio is printed, and a cell where the fused call is slower than the composition says so.  Exit status 1 when a cell's outputs
differ beyond such near-ties (relative cost difference above 1e-9)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", default="all", help="all | small (B <= 4096)")
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import workload
    import multistart_common as MC

    bad = 0
    print("# device: %s; %d calls per measurement, median of 5 alternating rounds" % (torch.cuda.get_device_name(0), args.reps))
    for name, frame in (("ur5", "tool0"), ("arm7", "tool")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        nq = model.nq
        visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
        lam2 = float(p.damping) ** 2
        lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
        for B in (1, 4096, 65536):
            if args.cells == "small" and B > 4096:
                continue
            q0, qt = MC.uniform_configurations(model, B, 0)
            Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
            TG = ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), data)
            dev = Q0.device
            rng = np.random.default_rng(11)
            QR = torch.from_numpy(np.ascontiguousarray(rng.uniform(lo, hi, (B, nq)).T)).cuda()
            w = rng.uniform(0.25, 2.0, nq)
            sup = torch.from_numpy(np.flatnonzero(np.asarray(data.support))).to(dev)
            W = torch.from_numpy(w).to(dev)[sup][:, None]
            for K in (4, 8):
                starts = ik_amd.multistart_starts(data, Q0, K, 0)
                Qs = torch.empty((K, nq, B), dtype=torch.float64, device=dev)
                oks = torch.empty((K, B), dtype=torch.uint8, device=dev)
                its = torch.empty((K, B), dtype=torch.int32, device=dev)
                cols = torch.arange(B, device=dev)
                for rule in (ik_amd.PickRule.DISTANCE, ik_amd.PickRule.MANIPULABILITY):
                    out = ik_amd.dls_pick_batch(problem, Q0, TG, data, visitor, p, num_starts=K, rule=rule, q_ref=QR, weights=w, starts=starts)
                    ms_out = ik_amd.dls_multistart_batch(problem, Q0, TG, data, visitor, p, num_starts=K, starts=starts)
                    ref = {}

                    def fused():
                        ik_amd.dls_pick_batch(problem, Q0, TG, data, visitor, p, num_starts=K, rule=rule, q_ref=QR, weights=w, starts=starts, out=out)

                    def multistart():
                        ik_amd.dls_multistart_batch(problem, Q0, TG, data, visitor, p, num_starts=K, starts=starts, out=ms_out)

                    def composed():
                        costs = []
                        for k in range(K):
                            ik_amd.dls_batch(problem, Q0 if k == 0 else starts[k - 1], TG, data, visitor, p, out=(Qs[k], oks[k], its[k]))
                            if rule == ik_amd.PickRule.MANIPULABILITY:
                                J = ik_amd.evaluate_batch(problem, Qs[k], TG, data)[1].permute(2, 0, 1)            # [B, M, nv]
                                G = J @ J.transpose(1, 2) + lam2 * torch.eye(J.shape[1], dtype=torch.float64, device=dev)
                                costs.append(torch.linalg.det(G).rsqrt())
                            else:
                                costs.append((W * (Qs[k][sup] - QR[sup]) ** 2).sum(dim=0))
                        cost = torch.stack(costs)                                                                   # [K, B]
                        key = torch.where(oks.bool(), cost, torch.full_like(cost, float("inf")))
                        win = key.argmin(dim=0)                                                                      # (the first minimum: the lowest index)
                        ref["win"], ref["cost"], ref["all"] = win, cost[win, cols], cost
                        ref["Q"], ref["ok"], ref["it"] = Qs[win, :, cols].t(), oks[win, cols], its[win, cols]

                    def measure(fn):
                        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        start.record()
                        for _ in range(args.reps):
                            fn()
                        stop.record()
                        torch.cuda.synchronize()
                        return start.elapsed_time(stop) / args.reps

                    composed(), fused(), multistart(), torch.cuda.synchronize()
                    some = ref["ok"].bool()
                    differ = some & (out[3].long() != ref["win"])
                    near = True
                    for b in torch.nonzero(differ).flatten().tolist():
                        a, c = float(ref["all"][int(out[3][b]), b]), float(ref["cost"][b])
                        near = near and abs(a - c) <= 1e-9 * max(abs(a), abs(c))
                        print("    problem %d: the call picks start %d (cost %.17g in torch), torch picks %d (%.17g)" % (b, int(out[3][b]), a, int(ref["win"][b]), c))
                    agree = some & ~differ
                    same = bool(torch.equal(out[0][:, agree], ref["Q"][:, agree]) and torch.equal(out[1][agree], ref["ok"][agree]) and
                                torch.equal(out[2][agree], ref["it"][agree]) and torch.equal(out[1].bool(), some)) and near
                    bad += not same
                    ms = {"fused": [], "composed": [], "multistart": []}
                    for fn in (fused, composed, multistart):   # warm-up
                        fn()
                    for _ in range(5):
                        ms["fused"].append(measure(fused))
                        ms["composed"].append(measure(composed))
                        ms["multistart"].append(measure(multistart))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    print("%-36s B = %-6d K = %d rule %-14s" % (ik_amd.dls_pick_kernel(data, visitor, p, K, rule), B, K, rule.name))
                    print("    some start converged in %d of %d problems; the winner is not the lowest-index converged start in %d; winners that differ from torch's: %d"
                          % (int(some.sum()), B, int((some & (out[3] != ms_out[3])).sum()), int(differ.sum())))
                    print("    winner / Q / success / iterations equal where some start converged: %s" % same)
                    print("    %-52s %9.4f ms per call" % ("dls_pick_batch, one call", med["fused"]))
                    what = "%d x dls_batch%s + cost, arg-min, gather in torch" % (K, " + %d x evaluate_batch" % K if rule == ik_amd.PickRule.MANIPULABILITY else "")
                    print("    %-52s %9.4f ms per call" % (what, med["composed"]))
                    print("    %-52s %9.4f ms per call" % ("dls_multistart_batch, one call", med["multistart"]))
                    print("    composed / fused: %.2f   fused / multistart: %.2f%s" % (med["composed"] / med["fused"], med["fused"] / med["multistart"],
                                                                                      "   THE FUSED CALL IS SLOWER THAN THE COMPOSITION" if med["fused"] > med["composed"] else ""))
    print("# cells whose outputs differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
