"""What fusing K starts per problem into one launch buys: ikgpu_dls_multistart_batch (ik_amd.dls_multistart_batch) against the composition
it replaces -- K x ik_amd.dls_batch, K x ikgpu_evaluate_batch and the selection in torch -- on the same stream, in one process.

    python tools/multistart_timing.py [--reps 5] [--cells small] > profiles/multistart_timing.txt

Cassie leg (dls_chain<NJ=7,full,hot>) and arm7 (hot-rtc where hipRTC is available); targets and starts uniform between the joint
limits (tests/multistart_common.py); B in {1, 4096, 65536} x K in {4, 8} x {the default stop rule (100 iterations, 1e-4), never-stop at
50 iterations}.  Both versions take the SAME K - 1 caller's starts and write into preallocated outputs.  Device events around `reps`
calls that end in a synchronise, after a warm-up; the two versions alternate and every cell is measured twice (the two figures show the
run-to-run spread).  Checked per cell: q / success / iterations / winner bit-identical (err_sq: the largest difference is printed -- the
fused kernel takes it from its own build's evaluation, the composition from the stage kernel), and the fused call not slower (the
better of its two figures against the better of the composition's).  Exit status 1 when a cell fails either check."""
import argparse
import ctypes as C
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
    from ik_amd import api, capi, workload
    import multistart_common as MC

    L = capi.lib()
    bad = 0
    print("# device: %s; %d calls per measurement" % (torch.cuda.get_device_name(0), args.reps))
    for name, frame in (("cassie_fixed", "LeftFootFront"), ("arm7", "tool")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        nq, M = model.nq, data.rows
        for B in (1, 4096, 65536):
            if args.cells == "small" and B > 4096:
                continue
            q0, qt = MC.uniform_configurations(model, B, 0)
            Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
            TG = ik_amd.task_frames_fk_batch(problem, torch.from_numpy(np.ascontiguousarray(qt.T)).cuda(), data)
            for K in (4, 8):
                starts = ik_amd.multistart_starts(data, Q0, K, 0)
                for visitor, p, label in ((ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters(), "stop rule 1e-4, <= 100 iterations"),
                                          (ik_amd.never_stop_visitor(), ik_amd.dls_parameters(max_iterations=50), "never-stop, 50 iterations")):
                    dev = Q0.device
                    out = (torch.empty_like(Q0), torch.empty((B,), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                           torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev))
                    ref = tuple(torch.empty_like(o) for o in out)
                    Qs = torch.empty((K, nq, B), dtype=torch.float64, device=dev)
                    oks = torch.empty((K, B), dtype=torch.uint8, device=dev)
                    its = torch.empty((K, B), dtype=torch.int32, device=dev)
                    Es = torch.empty((K, M, B), dtype=torch.float64, device=dev)
                    rank = torch.arange(K, dtype=torch.float64, device=dev)[:, None] - float(K)     # a converged start k ranks as k - K < 0
                    cols = torch.arange(B, device=dev)
                    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                    def fused():
                        ik_amd.dls_multistart_batch(problem, Q0, TG, data, visitor, p, num_starts=K, starts=starts, out=out)

                    def composed():
                        for k in range(K):
                            ik_amd.dls_batch(problem, Q0 if k == 0 else starts[k - 1], TG, data, visitor, p, out=(Qs[k], oks[k], its[k]))
                        for k in range(K):
                            capi.check(L.ikgpu_evaluate_batch(data._h, B, Qs[k].data_ptr(), TG.data_ptr(), Es[k].data_ptr(), None, capi.SOA, stream))
                        err = torch.nan_to_num((Es * Es).sum(dim=1), nan=float("inf"))
                        win = torch.where(oks.bool(), rank, err).argmin(dim=0)
                        ref[0].copy_(Qs[win, :, cols].t())
                        ref[1].copy_(oks[win, cols]), ref[2].copy_(its[win, cols]), ref[3].copy_(win), ref[4].copy_(err[win, cols])

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
                    same = all(torch.equal(a, b) for a, b in zip(out[:4], ref[:4]))
                    derr = float((out[4].sqrt() - ref[4].sqrt()).abs().max())
                    for fn in (fused, composed, fused, composed):   # warm-up
                        fn()
                    ms = {"fused": [], "composed": []}
                    for _ in range(2):
                        ms["fused"].append(measure(fused))
                        ms["composed"].append(measure(composed))
                    not_slower = min(ms["fused"]) <= min(ms["composed"])
                    bad += (not same) + (not not_slower)
                    print("%-42s B = %-6d K = %d  %s" % (ik_amd.dls_multistart_kernel(data, visitor, p, K), B, K, label))
                    print("    converged %d of %d from start 0, %d with the best of %d; mean iterations of the winners %.2f"
                          % (int(oks[0].sum()), B, int(out[1].sum()), K, float(out[2].double().mean())))
                    print("    q / success / iterations / winner bit-identical: %s; max |sqrt(err_sq) difference| %.3g" % (same, derr))
                    for k in ("fused", "composed"):
                        what = "dls_multistart_batch, one call" if k == "fused" else "%d x dls_batch + %d x evaluate + torch" % (K, K)
                        print("    %-36s %9.4f / %9.4f ms per call" % (what, ms[k][0], ms[k][1]))
                    print("    composed / fused: %.2f / %.2f   fused not slower: %s" % (ms["composed"][0] / ms["fused"][0], ms["composed"][1] / ms["fused"][1], not_slower))
    print("# cells failing a check: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
