"""What the line job buys: ikgpu_dls_line_batch (ik_amd.dls_line_batch, one launch that reads one goal per problem and leaves a failed
line at once) against the pair it is defined by, ik_amd.line_targets + ik_amd.dls_track_batch, on the same stream, in one process.

    python tools/line_timing.py [--T 64] [--reps 5] > profiles/line_timing.txt

Cassie leg (dls_chain<NJ=7,full,hot>), B = 65536, the default stop rule (100 iterations, 1e-4), two cells:
  (i)  every line feasible: starts and goals as tests/line_common.py draws them, resampled from the lines the job itself follows to
       the goal;
  (ii) the same batch with ONE line per wave (problem 64 w of wave w) that fails a quarter of the way along: a feasible line
       stretched to four times its length and rotation, kept when the job leaves it at waypoint T/4 (or as near as the draw has).
Device events around `reps` calls that end in a synchronise, after a warm-up; the two sides alternate and every cell is measured
twice (the two figures show the run-to-run spread).  Both sides write into preallocated outputs; the pair's waypoints are a fresh
[T, 1, 12, B] tensor per call, as a caller's would be.  Prints ms per call and what was checked: the written slabs of the two sides
are bit-identical."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import workload
    import line_common
    import twin

    T, B = args.T, args.B
    name, frame = "cassie_fixed", "LeftFootFront"
    model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
    problem = ik_amd.InverseKinematicsProblem(model)
    problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
    data = ik_amd.dls_data(problem, device=0)
    visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
    print("# device: %s; %s, B = %d, T = %d waypoints, %d calls per measurement" % (torch.cuda.get_device_name(0), ik_amd.dls_line_kernel(data, visitor, p), B, T, args.reps))

    dev = lambda q0, goals: (torch.from_numpy(np.ascontiguousarray(q0.T)).cuda(), torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda())
    rng = np.random.default_rng(0)
    q0, goals = line_common.inputs_exact(model, frame, B, 0)
    reached = ik_amd.dls_line_batch(problem, *dev(q0, goals), data, T, visitor, p)[3].cpu().numpy()
    good = np.flatnonzero(reached == T)
    pick = good[rng.integers(0, len(good), B)]
    fq0, fgoals = q0[pick], goals[pick]                                   # (i): B feasible lines
    # (ii) candidates: feasible lines stretched four times (waypoints 0 .. T/4 - 1 of the stretched line lie on the feasible one)
    sq0, sgoals = q0[good], goals[good].copy()
    om_start = ik_amd.task_frames_fk_batch(problem, dev(sq0, sgoals)[0], data).permute(2, 0, 1).cpu().numpy()   # [n, 1, 12]
    for b in range(len(good)):
        R0, p0 = om_start[b, 0, :9].reshape(3, 3), om_start[b, 0, 9:]
        R1, p1 = sgoals[b, 0, :9].reshape(3, 3), sgoals[b, 0, 9:]
        w, _ = twin.log3(R0.T @ R1)
        if 4.0 * np.linalg.norm(w) > line_common.MAX_ROTATION:
            w = w * 0.0
        sgoals[b, 0, :9] = (R0 @ twin.exp3(4.0 * w)).reshape(9)
        sgoals[b, 0, 9:] = p0 + 4.0 * (p1 - p0)
    sreached = ik_amd.dls_line_batch(problem, *dev(sq0, sgoals), data, T, visitor, p)[3].cpu().numpy()
    at = min(np.unique(sreached), key=lambda r: abs(int(r) - T // 4))
    bad = np.flatnonzero(sreached == at)
    print("# %d of %d drawn lines are followed to the goal; %d stretched lines fail at waypoint %d (wanted %d)" % (len(good), B, len(bad), at, T // 4))
    iq0, igoals = fq0.copy(), fgoals.copy()
    first = np.arange(0, B, 64)
    take = bad[rng.integers(0, len(bad), len(first))]
    iq0[first], igoals[first] = sq0[take], sgoals[take]

    for label, (cq0, cgoals) in (("(i) every line feasible", (fq0, fgoals)), ("(ii) one line per wave fails at waypoint %d" % at, (iq0, igoals))):
        Q0, G = dev(cq0, cgoals)
        out_l = (torch.empty((T, model.nq, B), dtype=torch.float64, device="cuda"), torch.empty((T, B), dtype=torch.uint8, device="cuda"),
                 torch.empty((T, B), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))
        out_p = tuple(torch.empty_like(o) for o in out_l[:3])

        def line():
            ik_amd.dls_line_batch(problem, Q0, G, data, T, visitor, p, out=out_l)

        def pair():
            ik_amd.dls_track_batch(problem, Q0, ik_amd.line_targets(problem, Q0, G, data, T), data, visitor, p, out=out_p)

        def measure(fn):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.reps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop) / args.reps

        for o in out_l[:3]:
            o.zero_()
        line(), pair(), torch.cuda.synchronize()
        r = out_l[3].cpu().numpy()
        mask = torch.from_numpy(line_common.written(r, T)).cuda()
        sel = lambda a: (a.permute(0, 2, 1) if a.dim() == 3 else a)[mask]
        same = all(torch.equal(sel(a), sel(b)) for a, b in zip(out_l[:3], out_p))
        for fn in (line, pair, line, pair):   # warm-up
            fn()
        ms = {"line": [], "pair": []}
        for _ in range(2):
            ms["line"].append(measure(line))
            ms["pair"].append(measure(pair))
        print("%s" % label)
        print("    reached == T for %d of %d lines; mean iterations per written waypoint %.2f; written slabs bit-identical: %s"
              % (int((r == T).sum()), B, float(out_l[2][mask].double().mean()), same))
        for k, what in (("line", "dls_line_batch, one launch"), ("pair", "line_targets + dls_track_batch")):
            print("    %-32s %9.4f / %9.4f ms per call" % (what, ms[k][0], ms[k][1]))
        print("    pair / line: %.2f / %.2f" % (ms["pair"][0] / ms["line"][0], ms["pair"][1] / ms["line"][1]))


if __name__ == "__main__":
    main()
