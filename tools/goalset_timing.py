"""What fusing G goals per problem into one launch buys: ikgpu_dls_goalset_batch (ik_amd.dls_goalset_batch) against the same answer through
the entry points that existed before it -- q0 and the starts replicated G times, ik_amd.dls_multistart_batch (K >= 2) or ik_amd.dls_batch
plus ikgpu_evaluate_batch (K = 1) on B x G problems, and the reduction to winner, goal and reachable in torch -- on the same stream, in
one process.

    python tools/goalset_timing.py --reps 40 [--rounds 5] [--cells small] > profiles/goalset_timing.txt

arm7 (hot-rtc where hipRTC is available) and ur5 (dls_chain<NJ=6,full,hot>); goals and starts uniform between the joint limits
(tests/goalset_common.py); (G, K) in {(4, 1), (8, 1), (4, 2)} x B in {65536 / (G K), 65536}: the first fills the machine's 65536 lanes
once, the second G K times; the default stop rule (100 iterations, 1e-4).  Both versions take the SAME K - 1 caller's starts and write
into preallocated outputs; the composition's replication of q0, the starts and the goals is part of what it costs a caller and is
timed with it.  Device events around `reps` calls that end in a synchronise, after a warm-up; the two versions alternate for `rounds`
rounds and the median and the range of each are printed (the range is the run-to-run spread on a shared machine).  Checked per cell:
q / success / iterations / goal / start / reachable bit-identical (err_sq: the largest difference is printed -- at K = 1 the
composition takes it from the stage kernel, the fused kernel from its own build's evaluation).  Exit status 1 when a cell's outputs
differ.

What to expect, to be checked against the figures: the solve itself costs the same lane-iterations on both sides, so the fused call
saves the G x replicated inputs (nq + 12 doubles per candidate goal instead of per problem), the G x outputs (nq + 2 values per goal
written and read back) and the reduction's launches."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cells", default="all", help="all | small (B = 65536 / (G K) only)")
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import capi, workload
    import goalset_common as GC

    L = capi.lib()
    bad = 0
    print("# device: %s; %d calls per measurement, %d alternating rounds: median (min .. max) ms per call" % (torch.cuda.get_device_name(0), args.reps, args.rounds))
    for name, frame in (("arm7", "tool"), ("ur5", "tool0")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        nq, M = model.nq, data.rows
        visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
        for G, K in ((4, 1), (8, 1), (4, 2)):
            for B in (65536 // (G * K), 65536):
                if args.cells == "small" and B == 65536:
                    continue
                dev = torch.device("cuda:0")
                q0, qt = GC.goal_configurations(model, B, G, 0)
                Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).to(dev)
                GL = torch.stack([ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(qt[g].T)).to(dev), data) for g in range(G)]).contiguous()
                starts = ik_amd.multistart_starts(data, Q0, K, 0) if K > 1 else None
                i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
                u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
                f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
                out = (torch.empty_like(Q0), u8(B), i32(B), i32(B), i32(B), f64(B), u8(G, B))
                ref = tuple(torch.empty_like(o) for o in out)
                n = G * B
                wide = (f64(nq, n), u8(n), i32(n), i32(n), f64(n))           # the composition's G results per problem, problem g B + b
                E = f64(M, n)
                rank = torch.arange(G, dtype=torch.float64, device=dev)[:, None] - float(G)     # a reached goal g ranks as g - G < 0
                cols = torch.arange(B, device=dev)
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def fused():
                    ik_amd.dls_goalset_batch(problem, Q0, GL, data, visitor, p, num_starts=K, starts=starts, out=out)

                def composed():
                    q0r = Q0.repeat(1, G)                                     # [nq, G B]
                    tgr = GL.permute(1, 2, 0, 3).reshape(1, 12, n)            # (a copy: the goals of problem g B + b)
                    if K > 1:
                        ik_amd.dls_multistart_batch(problem, q0r, tgr, data, visitor, p, num_starts=K, starts=starts.repeat(1, 1, G), out=wide)
                        err = wide[4].view(G, B)
                    else:
                        ik_amd.dls_batch(problem, q0r, tgr, data, visitor, p, out=wide[:3])
                        capi.check(L.ikgpu_evaluate_batch(data._h, n, wide[0].data_ptr(), tgr.data_ptr(), E.data_ptr(), None, capi.SOA, stream))
                        err = (E * E).sum(dim=0).view(G, B)
                        wide[3].zero_()
                    oks = wide[1].view(G, B)
                    win = torch.where(oks.bool(), rank, torch.nan_to_num(err, nan=float("inf"))).argmin(dim=0)
                    ref[0].copy_(wide[0].view(nq, G, B)[:, win, cols])
                    ref[1].copy_(oks[win, cols]), ref[2].copy_(wide[2].view(G, B)[win, cols]), ref[3].copy_(win)
                    ref[4].copy_(wide[3].view(G, B)[win, cols]), ref[5].copy_(err[win, cols]), ref[6].copy_(oks)

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
                same = all(torch.equal(out[i], ref[i]) for i in (0, 1, 2, 3, 4, 6))
                derr = float((out[5].sqrt() - ref[5].sqrt()).abs().max())
                for fn in (fused, composed, fused, composed):   # warm-up
                    fn()
                ms = {"fused": [], "composed": []}
                for _ in range(args.rounds):
                    ms["fused"].append(measure(fused))
                    ms["composed"].append(measure(composed))
                bad += not same
                print("%-40s B = %-6d G = %d K = %d" % (ik_amd.dls_goalset_kernel(data, visitor, p, G, K), B, G, K))
                print("    reached a goal: %d of %d; goal 0 reachable for %d; mean iterations of the winners %.2f"
                      % (int(out[1].sum()), B, int(out[6][0].sum()), float(out[2].double().mean())))
                print("    q / success / iterations / goal / start / reachable bit-identical: %s; max |sqrt(err_sq) difference| %.3g" % (same, derr))
                med = {}
                for k in ("fused", "composed"):
                    what = "dls_goalset_batch, one call" if k == "fused" else ("replicate + dls_multistart_batch + torch" if K > 1 else "replicate + dls_batch + evaluate + torch")
                    med[k] = statistics.median(ms[k])
                    print("    %-42s %9.4f (%9.4f .. %9.4f) ms per call" % (what, med[k], min(ms[k]), max(ms[k])))
                print("    composed / fused (medians): %.2f" % (med["composed"] / med["fused"]))
    print("# cells whose outputs differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
