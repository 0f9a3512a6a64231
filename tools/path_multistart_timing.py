"""What the path multi-start call buys: ikgpu_dls_path_multistart_batch (ik_amd.dls_path_multistart_batch: a scout launch over B x K lanes
that stores no trajectory, then one path launch from the winner's entry) against what a caller composes without it, on the same stream,
in one process.

    python tools/path_multistart_timing.py [--reps 3]          (writes profiles/path_multistart_timing.txt)

The composition, in torch: K x ik_amd.dls_batch against via 0 (+ ik_amd.evaluate_batch for the errors), K x ik_amd.dls_path_batch from
each result into K full trajectory buffers, the key (entered, N - reached | error, k) reduced over the K starts, and the gather of the
winner's entry, counts and trajectory.  Workload: tests/path_multistart_common.py (a pool of 4096 problems of recipe seed 1, resampled to
B; starts generated from seed 7), ur5 and arm7, K in {4, 8}, B in {1, 4096, 65536 / K}, three vias and T = 16 (N = 32 waypoints), the
robot's max_joint_step, the default stop rule (100 iterations, 1e-4); the call is timed scout-only (trajectory=False) and with the
trajectory, the composition always gathers the trajectory.  Device events around `reps` calls that end in a synchronise, after a
warm-up; the sides alternate over five rounds and the median is printed with the smallest and largest round.  Every side writes into
preallocated outputs.  In every cell the outputs are asserted equal: q_entry, the entry flags and counts, winner, reached, reached_all
and the written slabs of the trajectory.  err_sq is the scout's own evaluation and is compared to 1e-10 in the norm; where NO start
entered, starts that end in the same local minimum differ in their error by rounding and the two evaluations may rank them differently:
such problems are counted and printed, and their entry is compared through the error alone."""
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
    ap.add_argument("--K", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_multistart_timing.txt"))
    args = ap.parse_args()
    import torch
    import ik_amd
    from ik_amd import workload
    import line_common
    import path_common
    import path_multistart_common as PM

    N = (P - 1) * T
    visitor, p = ik_amd.inverse_kinematics_visitor(), ik_amd.dls_parameters()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# device: %s; %d vias, T = %d (N = %d waypoints behind via 0), %d calls per measurement, median (min .. max) of %d alternating rounds, ms per call"
        % (torch.cuda.get_device_name(0), P, T, N, args.reps, ROUNDS))

    def measure(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.reps

    for name, frame in (("ur5", "tool0"), ("arm7", "tool")):
        model = ik_amd.Model.from_urdf_file(os.path.join(workload.MODELS_DIR, name + ".kin.urdf"))
        problem = ik_amd.InverseKinematicsProblem(model)
        problem.add_frame_task("t", ik_amd.FrameTask.create(model, frame, ik_amd.KinematicType.Full))
        data = ik_amd.dls_data(problem, device=0)
        step = path_common.JOINT_STEP[name]
        pq0, pvias = PM.inputs(model, frame, POOL, 1)
        rng = np.random.default_rng(0)
        nq = model.nq
        for K in args.K:
            say("# %s, K = %d: %s, then %s" % (name, K, ik_amd.dls_path_multistart_kernel(data, visitor, p, K), ik_amd.dls_path_kernel(data, visitor, p)))
            for B in (1, 4096, 65536 // K):
                pick = rng.integers(0, POOL, B)
                Q0 = torch.from_numpy(np.ascontiguousarray(pq0[pick].T)).cuda()
                V = torch.from_numpy(np.ascontiguousarray(pvias[:, pick].transpose(0, 2, 1)[:, None])).cuda()      # [P, 1, 12, B]
                V1 = V[1:].contiguous()
                gen = ik_amd.multistart_starts(data, Q0, K, PM.START_SEED)
                f = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
                result = lambda traj: ik_amd.api.PathMultistartResult(
                    f((nq, B), torch.float64), f((B,), torch.uint8), f((B,), torch.int32), f((B,), torch.int32), f((B,), torch.float64), f((B,), torch.int32),
                    f((K, B), torch.int32), f((N, nq, B), torch.float64) if traj else None, f((N, B), torch.uint8) if traj else None,
                    f((N, B), torch.int32) if traj else None)
                outs = {"s": result(False), "t": result(True)}
                singles = [(f((nq, B), torch.float64), f((B,), torch.uint8), f((B,), torch.int32)) for _ in range(K)]
                paths = [(f((N, nq, B), torch.float64), f((N, B), torch.uint8), f((N, B), torch.int32), f((B,), torch.int32)) for _ in range(K)]
                got = {}
                ks = torch.arange(K, device="cuda")[:, None]
                cols = torch.arange(B, device="cuda")

                def scout():
                    ik_amd.dls_path_multistart_batch(problem, Q0, V, data, T, step, visitor, p, num_starts=K, seed=PM.START_SEED, trajectory=False, out=outs["s"])

                def full():
                    ik_amd.dls_path_multistart_batch(problem, Q0, V, data, T, step, visitor, p, num_starts=K, seed=PM.START_SEED, trajectory=True, out=outs["t"])

                def composed():
                    errs = []
                    for k in range(K):
                        ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], V[0], data, visitor, p, out=singles[k])
                        e = ik_amd.evaluate_batch(problem, singles[k][0], V[0], data, jacobian=False)
                        e = e[0] if isinstance(e, tuple) else e
                        errs.append((e * e).sum(dim=0))
                        ik_amd.dls_path_batch(problem, singles[k][0], V1, data, T, step, visitor, p, out=paths[k])
                    entered = torch.stack([s[1] for s in singles]).bool()                                     # [K, B]
                    reached_k = torch.stack([q[3] for q in paths])
                    err = torch.stack(errs)
                    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
                    val = torch.where(entered, (N - reached_k).double(), torch.full_like(err, float("inf")))
                    some = entered.any(dim=0)
                    val = torch.where(some[None, :], val, err)
                    winner = torch.where(val == val.amin(dim=0)[None, :], ks, K).amin(dim=0)                  # the lowest index among the smallest
                    reached_all = torch.where(entered, reached_k, torch.full_like(reached_k, -1))
                    got["c"] = (torch.stack([s[0] for s in singles])[winner, :, cols].t(), torch.stack([s[1] for s in singles])[winner, cols],
                                torch.stack([s[2] for s in singles])[winner, cols], winner.to(torch.int32), err[winner, cols],
                                reached_all[winner, cols].clamp(min=0), reached_all,
                                torch.stack([q[0] for q in paths])[winner, :, :, cols].permute(1, 2, 0),
                                torch.stack([q[1] for q in paths])[winner, :, cols].t(), torch.stack([q[2] for q in paths])[winner, :, cols].t())

                sides = (("s", scout, "dls_path_multistart_batch, scout only"), ("t", full, "dls_path_multistart_batch with the trajectory"),
                         ("c", composed, "%d x dls_batch + %d x dls_path_batch + reduce + gather" % (K, K)))
                for _, fn, _ in sides:   # warm-up, and the results that are compared
                    fn()
                torch.cuda.synchronize()
                c, t, s = got["c"], outs["t"], outs["s"]
                # where no start entered the key is the error, and starts that end in the same local minimum differ in it by rounding: the
                # scout's own evaluation and evaluate_batch may then rank them differently -- such a problem must have the same error to 1e-10
                same = t.winner == c[3]
                some = t.entry_success.bool()
                assert bool((same | ~some).all()), (name, K, B)
                assert float((t.err_sq.sqrt() - c[4].sqrt()).abs().max()) <= 1e-10 and torch.equal(s.err_sq, t.err_sq), (name, K, B)
                for i in (0, 1, 2, 3, 5, 6):
                    assert torch.equal(t[i][..., same], c[i].to(t[i].dtype)[..., same]) and torch.equal(s[i], t[i]), (name, K, B, i)
                assert torch.equal(t.reached_all, c[6]), (name, K, B)
                mask = torch.from_numpy(line_common.written(t.reached.cpu().numpy(), N)).cuda() & t.entry_success.bool()[None, :]
                sel = lambda a: (a.permute(0, 2, 1) if a.dim() == 3 else a)[mask]
                assert all(torch.equal(sel(x), sel(y)) for x, y in zip(t[7:], c[7:])), (name, K, B)
                ms = {k: [] for k, _, _ in sides}
                for _ in range(ROUNDS):
                    for k, fn, _ in sides:
                        ms[k].append(measure(fn))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                r = t.reached.cpu().numpy()
                say("%s  K = %d  B = %d  max_joint_step = %.2f" % (name, K, B, step))
                say("    entered %d of %d, winner complete %d; outputs equal to the composition: True (%d problems without an entered start ranked by rounding); trajectory buffers %.3f MB against %.3f MB"
                    % (int(t.entry_success.sum()), B, int(((r == N) & (t.entry_success.cpu().numpy() == 1)).sum()), int((~same).sum()), 8e-6 * N * nq * B, 8e-6 * N * nq * B * K))
                for k, _, what in sides:
                    say("    %-58s %9.4f (%9.4f .. %9.4f)" % (what, med[k], min(ms[k]), max(ms[k])))
                say("    composition / scout: %.2f    composition / with trajectory: %.2f" % (med["c"] / med["s"], med["c"] / med["t"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
