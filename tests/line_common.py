"""The inputs the line tests share (tests/test_line_emulation.py on the CPU, tests/test_gpu_line.py on the device) and the twin's
waypoints (oracle/twin.py: log3, exp3 and FK in numpy) they are held to.

Per problem: q0 = mid + U(-0.6, 0.6) x half-range of the limits, goal = FK(q0 + d) with d = U(-0.3, 0.3) and, for every third problem,
U(-1.2, 1.2) unclipped -- so some lines end outside the workspace or the limits and fail on the way.  Problems whose relative rotation
exceeds 2.5 rad are dropped (a rotation near pi has an ill-conditioned axis: callers split such moves)."""
import numpy as np

import oracle as O
import twin

MAX_ROTATION = 2.5
ROBOTS = [("cassie_fixed", "LeftFootFront"), ("ur5", "tool0"), ("arm7", "tool")]

# Bar of the waypoint comparison against the twin: ten times the emulator's measured maximum entry error on rotations up to 2.5 rad
# (2.62e-13 over the three robots, seeds 0-3 and the regimes of regime_goals), and never above 1e-10 (the
# project's bar for e and J in tests/test_gpu_chain_shapes.py: needing more would mean the arithmetic is wrong).  The maximum is the
# jump of log3's own convention at its Taylor threshold -- theta / sin(theta) against 1, theta^3 / 6 = 3.0e-13 at theta = 2^-13 --
# which the rounding of acos puts on either side of the threshold; away from that one angle the maximum is 4.1e-15.
WAYPOINT_MEASURED = 2.62e-13
WAYPOINT_BAR = 10 * WAYPOINT_MEASURED
assert WAYPOINT_BAR <= 1e-10


def rotation_angle(R0, R1):
    """Angle of R0^T R1, [B]."""
    tr = np.einsum("bki,bki->b", R0, R1)
    return np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))


def inputs(model, frame, B, seed):
    """(q0 [n, nq], goals [n, 1, 12]) with n <= B: the problems whose relative rotation is at most MAX_ROTATION."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q0 = mid + rng.uniform(-0.6, 0.6, (B, model.nq)) * half
    d = rng.uniform(-0.3, 0.3, (B, model.nq))
    far = rng.uniform(-1.2, 1.2, (B, model.nq))
    d[::3] = far[::3]
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    start, goal = O.fk_batch(om, q0, [fid]), O.fk_batch(om, q0 + d, [fid])     # [B, 1, 12]
    keep = rotation_angle(start[:, 0, :9].reshape(B, 3, 3), goal[:, 0, :9].reshape(B, 3, 3)) <= MAX_ROTATION
    return np.ascontiguousarray(q0[keep]), np.ascontiguousarray(goal[keep])


def inputs_exact(model, frame, B, seed):
    """The first B kept problems of a larger draw: exactly B lines."""
    q0, goals = inputs(model, frame, B + B // 8 + 16, seed)
    assert q0.shape[0] >= B
    return np.ascontiguousarray(q0[:B]), np.ascontiguousarray(goals[:B])


def to12(M):
    return np.concatenate([M[:3, :3].reshape(9), M[:3, 3]])


def from12(v):
    return twin.se3(np.asarray(v[:9]).reshape(3, 3), np.asarray(v[9:12]))


def twin_waypoints(tm, frame, q0, goals, T, reference="universe"):
    """ikgpu_line_targets restated on the twin: [T, n, 12] for one FrameTask on `frame` (q0 [n, nq], goals [n, 12])."""
    fid, rid = twin.frame_id(tm, frame), twin.frame_id(tm, reference)
    out = np.empty((T, q0.shape[0], 12))
    for b in range(q0.shape[0]):
        _, oMf = twin.fk(tm, q0[b])
        M0 = twin.se3_inv(oMf[rid]) @ oMf[fid]
        R0, p0 = M0[:3, :3], M0[:3, 3]
        M1 = from12(goals[b])
        w, _ = twin.log3(R0.T @ M1[:3, :3])
        for k in range(T):
            s = (k + 1) / T
            out[k, b] = to12(twin.se3(R0 @ twin.exp3(s * w), p0 + s * (M1[:3, 3] - p0))) if k < T - 1 else goals[b]
    return out


def regime_goals(tm, frame, q0, T):
    """Goals that put the waypoint arithmetic into each of its regimes, one per row of q0 (cycled), with what each is:
    the start's own rotation bit for bit (theta = 0), theta = 1e-9, theta at the Taylor threshold of exp3 for the first waypoint and for
    the whole rotation, theta = 2.5 rad, and zero translation."""
    fid = twin.frame_id(tm, frame)
    thetas = [("theta=0", 0.0), ("theta=1e-9", 1e-9), ("s*theta at the exp3 threshold", twin.TAYLOR_PREC3 * T), ("theta at the threshold", twin.TAYLOR_PREC3),
              ("theta=2.5", 2.5), ("zero translation", 0.7)]
    rng = np.random.default_rng(5)
    goals, names = [], []
    for b in range(q0.shape[0]):
        name, th = thetas[b % len(thetas)]
        _, oMf = twin.fk(tm, q0[b])
        M0 = oMf[fid]
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        R1 = M0[:3, :3] if th == 0.0 else M0[:3, :3] @ twin.exp3(th * axis)
        p1 = M0[:3, 3] if name == "zero translation" else M0[:3, 3] + rng.uniform(-0.1, 0.1, 3)
        goals.append(to12(twin.se3(R1, p1)))
        names.append(name)
    return np.array(goals), names


def reached_from_flags(ok):
    """The count the definition gives: leading ones of success [T, n] per problem."""
    T = ok.shape[0]
    alive = np.cumprod(ok.astype(np.int64), axis=0)
    return alive.sum(axis=0).astype(np.int32), T


def written(reached, T):
    """mask [T, n]: slab k of problem b is written when k <= min(reached[b], T - 1)."""
    return np.arange(T)[:, None] <= np.minimum(reached, T - 1)[None, :]
