"""What returning the solution set from one launch buys: ikgpu_dls_solutions_batch (ik_amd.dls_solutions_batch) against the composition it
replaces -- K x ik_amd.dls_batch from ikgpu_multistart_starts' starts and the greedy rule in torch -- on the same stream, in one process.

    python tools/solutions_timing.py [--reps 5] [--cells small] > profiles/solutions_timing.txt

Cassie leg (dls_chain<NJ=7,full,hot>, separation 0.5 rad) and ur5 (dls_chain<NJ=6,full,hot>, 0.1 rad); targets and starts uniform between
the joint limits (tests/multistart_common.py); B in {1, 4096, 65536} x K in {8, 16}, N = K, the default stop rule (100 iterations, 1e-4).
Both versions take the SAME K - 1 caller's starts and write into preallocated, prefilled outputs (slots past count[b] are not written by
either).  The torch rule runs without a host synchronisation: K (K - 1) / 2 masked comparisons and K N masked copies.  Device events
around `reps` calls that end in a synchronise, after a warm-up; the two versions alternate and every cell is measured twice (the two
figures show the run-to-run spread).  Checked per cell: Q / count / which / iterations bit-identical.  No speed is promised: the ratio
is printed, and a cell where the fused call is slower says so.  Exit status 1 when a cell's outputs differ."""
import argparse
import os
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
    print("# device: %s; %d calls per measurement" % (torch.cuda.get_device_name(0), args.reps))
    for name, frame, sep in (("cassie_fixed", "LeftFootFront", 0.5), ("ur5", "tool0", 0.1)):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        nq = model.nq
        visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
        for B in (1, 4096, 65536):
            if args.cells == "small" and B > 4096:
                continue
            q0, qt = MC.uniform_configurations(model, B, 0)
            Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
            TG = ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), data)
            dev = Q0.device
            sup = torch.from_numpy(np.flatnonzero(np.asarray(data.support))).to(dev)
            for K in (8, 16):
                N = K
                starts = ik_amd.multistart_starts(data, Q0, K, 0)

                def outputs():
                    return (torch.full((N, nq, B), float("nan"), dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev),
                            torch.full((N, B), -7, dtype=torch.int32, device=dev), torch.full((N, B), -7, dtype=torch.int32, device=dev))

                out, ref = outputs(), outputs()
                Qs = torch.empty((K, nq, B), dtype=torch.float64, device=dev)
                oks = torch.empty((K, B), dtype=torch.uint8, device=dev)
                its = torch.empty((K, B), dtype=torch.int32, device=dev)

                def fused():
                    ik_amd.dls_solutions_batch(problem, Q0, TG, data, visitor, p, num_starts=K, max_solutions=N, separation=sep, starts=starts, out=out)

                def composed():
                    for k in range(K):
                        ik_amd.dls_batch(problem, Q0 if k == 0 else starts[k - 1], TG, data, visitor, p, out=(Qs[k], oks[k], its[k]))
                    S = Qs[:, sup, :]                                          # [K, support, B]
                    kept = torch.zeros((K, B), dtype=torch.bool, device=dev)
                    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
                    for k in range(K):
                        ok = oks[k].bool() & (cnt < N)
                        for j in range(k):
                            ok &= ~(kept[j] & ~((S[k] - S[j]).abs() >= sep).any(dim=0))
                        kept[k] = ok
                        for n in range(min(k + 1, N)):
                            m = ok & (cnt == n)
                            ref[0][n] = torch.where(m, Qs[k], ref[0][n])
                            ref[2][n] = torch.where(m, torch.full_like(ref[2][n], k), ref[2][n])
                            ref[3][n] = torch.where(m, its[k], ref[3][n])
                        cnt += ok
                    ref[1].copy_(cnt)

                def measure(fn):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    start.record()
                    for _ in range(args.reps):
                        fn()
                    stop.record()
                    torch.cuda.synchronize()
                    return start.elapsed_time(stop) / args.reps

                composed(), fused(), torch.cuda.synchronize()
                same = all(np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True) for a, b in zip(out, ref))
                for fn in (fused, composed, fused, composed):   # warm-up
                    fn()
                ms = {"fused": [], "composed": []}
                for _ in range(2):
                    ms["fused"].append(measure(fused))
                    ms["composed"].append(measure(composed))
                slower = min(ms["fused"]) > min(ms["composed"])
                bad += not same
                count = out[1].cpu().numpy()
                print("%-40s B = %-6d K = %-2d N = %-2d separation %.1f rad" % (ik_amd.dls_solutions_kernel(data, visitor, p, K), B, K, N, sep))
                print("    converged %d of %d from start 0; problems by number of solutions %s, mean %.2f"
                      % (int(oks[0].sum()), B, np.bincount(count, minlength=K + 1).tolist(), float(count.mean())))
                print("    Q / count / which / iterations bit-identical: %s" % same)
                for k in ("fused", "composed"):
                    what = "dls_solutions_batch, one call" if k == "fused" else "%d x dls_batch + the rule in torch" % K
                    print("    %-36s %9.4f / %9.4f ms per call" % (what, ms[k][0], ms[k][1]))
                print("    composed / fused: %.2f / %.2f%s" % (ms["composed"][0] / ms["fused"][0], ms["composed"][1] / ms["fused"][1],
                                                              "   THE FUSED CALL IS SLOWER" if slower else ""))
    print("# cells whose outputs differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
