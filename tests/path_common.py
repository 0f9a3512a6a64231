"""The inputs the path tests share (tests/test_path_emulation.py on the CPU, tests/test_gpu_path.py on the device), the twin's waypoints
(oracle/twin.py) and the met rule of ikgpu_dls_path_batch in numpy.

tests/line_common.py's recipe extended to P segments.  Per problem: q_0 = mid + U(-0.6, 0.6) x half-range of the limits; via s =
FK(q_s) with q_s = q_{s-1} + d, d = U(-0.3, 0.3) and, for every third problem (offset by s), U(-1.2, 1.2) unclipped -- so some segments
end outside the workspace or the limits, and some are reached only by swinging to another branch.  Segment 0 draws what
line_common.inputs draws for the same seed.  Problems whose relative rotation exceeds 2.5 rad in some segment are dropped."""
import numpy as np

import line_common
import oracle as O
import twin

# max_joint_step of the tests, rad: the issue's thresholds (a UR5 or arm7 waypoint step of the recipe has median 0.05-0.06 and p90
# 0.34-0.41 rad; a Cassie leg step p90 0.07-0.10, p99 0.25-0.26 rad).
JOINT_STEP = {"ur5": 0.5, "arm7": 0.5, "cassie_fixed": 0.25}


def inputs(model, frame, B, P, seed):
    """(q0 [n, nq], vias [P, n, 1, 12]) with n <= B: the problems whose every segment turns by at most line_common.MAX_ROTATION."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q0 = mid + rng.uniform(-0.6, 0.6, (B, model.nq)) * half
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    prev = O.fk_batch(om, q0, [fid])                                           # [B, 1, 12]
    q, vias, keep = q0, [], np.ones(B, bool)
    for s in range(P):
        d = rng.uniform(-0.3, 0.3, (B, model.nq))
        far = rng.uniform(-1.2, 1.2, (B, model.nq))
        d[s % 3::3] = far[s % 3::3]
        q = q + d
        via = O.fk_batch(om, q, [fid])
        keep &= line_common.rotation_angle(prev[:, 0, :9].reshape(B, 3, 3), via[:, 0, :9].reshape(B, 3, 3)) <= line_common.MAX_ROTATION
        vias.append(via)
        prev = via
    return np.ascontiguousarray(q0[keep]), np.ascontiguousarray(np.stack(vias)[:, keep])


def inputs_exact(model, frame, B, P, seed):
    """The first B kept problems of a larger draw: exactly B paths."""
    q0, vias = inputs(model, frame, B + B // 4 + 32, P, seed)
    assert q0.shape[0] >= B
    return np.ascontiguousarray(q0[:B]), np.ascontiguousarray(vias[:, :B])


def twin_waypoints(tm, frame, q0, vias, T):
    """ikgpu_path_targets restated on the twin: [P T, n, 12] for one FrameTask on `frame` in the universe (q0 [n, nq], vias [P, n, 12])."""
    P, n = vias.shape[:2]
    out = np.empty((P * T, n, 12))
    out[:T] = line_common.twin_waypoints(tm, frame, q0, vias[0], T)
    for s in range(1, P):
        for b in range(n):
            M0, M1 = line_common.from12(vias[s - 1, b]), line_common.from12(vias[s, b])
            R0, p0 = M0[:3, :3], M0[:3, 3]
            w, _ = twin.log3(R0.T @ M1[:3, :3])
            for k in range(T):
                f = (k + 1) / T
                out[s * T + k, b] = line_common.to12(twin.se3(R0 @ twin.exp3(f * w), p0 + f * (M1[:3, 3] - p0))) if k < T - 1 else vias[s, b]
    return out


def met_rule(ok, q, q0, support, max_joint_step):
    """The definition's rule on what the tracking call returned: ok [N, n], q [N, n, nq], q0 [n, nq], support [nq] (ikgpu_problem_support).
    Returns (reached [n] int32, jumped [N, n]): waypoint m is met when ok and, with max_joint_step > 0, no support entry has
    fabs(q_m - q_{m-1}) > max_joint_step (q_{-1} = q0); reached counts the met waypoints before the first that was not."""
    prev = np.concatenate([q0[None], q[:-1]])
    step = np.abs(q - prev)[:, :, np.asarray(support, bool)]
    jumped = (step > max_joint_step).any(axis=2) if max_joint_step != 0.0 else np.zeros(ok.shape, bool)
    met = (ok == 1) & ~jumped
    return np.cumprod(met.astype(np.int64), axis=0).sum(axis=0).astype(np.int32), jumped


def endings(ok, reached, N):
    """How each path ends: (by a jump with success = 1, by the stop rule, complete), three masks [n]."""
    n = reached.shape[0]
    complete = reached == N
    last_ok = ok[np.minimum(reached, N - 1), np.arange(n)] == 1
    return ~complete & last_ok, ~complete & ~last_ok, complete


def check_conditions(ok, reached, P, T, values=True):
    """The conditions of the issue on a reference, asserted before anything is compared: at least 5 lanes end by a jump with success = 1,
    at least 5 by the stop rule, at least 1 is complete; and (values) reached takes 0, T - 1, T and P T."""
    jump, stop, complete = endings(ok, reached, P * T)
    counts = (int(jump.sum()), int(stop.sum()), int(complete.sum()))
    assert counts[0] >= 5 and counts[1] >= 5 and counts[2] >= 1, counts
    if values:
        have = set(reached.tolist())
        assert {0, T - 1, T, P * T} <= have, sorted(have)
    return counts
