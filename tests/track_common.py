"""The trajectory the tracking tests share (tests/test_track_emulation.py on the CPU, tests/test_gpu_track.py on the device): built to
put lanes INTO each branch of the tracking lane programs, not to hope a draw reaches it.

Per problem, from workload.chain_workload(..., "uniform")'s (q0, qs), the waypoints are the task frame's placement at
  waypoint 0        q0: every lane stops at iteration 0, so slab 0 holds the entries outside the chain UNCLIPPED
  waypoints 1..T-2  q0 + k / (T - 2) * 0.5 * (qs - q0): a smooth motion, about one iteration per waypoint
  waypoint T/2      its predecessor's again: an iteration-0 stop in mid-trajectory
  waypoint T-1      a fresh uniform draw (seed 1): a jump that runs some lanes out of iterations (jump=False: smooth to the end)
On cassie_fixed the last entry of the start (outside the left leg's chain) is set 9 rad beyond its limit, so the clip of the
pass-through entries switches on between slab 0 and slab 1.  A UR5 start stays inside its limits (its last entry is IN the chain and
the whole trajectory would turn chaotic)."""
import numpy as np


def configurations(model, name, B, T, jump=True):
    """Returns (start [B, nq], [T configurations [B, nq] whose forward kinematics are the waypoints])."""
    from ik_amd import workload
    lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
    nominal = workload.UR5_NOMINAL if name.startswith("ur") else workload.cassie_nominal(model.names) if name.startswith("cassie") else np.zeros(model.nq)
    narrow = 2.0 if name.startswith("ur") else None
    q0, qs = workload.chain_workload(lo, hi, nominal, np.arange(B), 0, "uniform", narrow)
    _, qfar = workload.chain_workload(lo, hi, nominal, np.arange(B), 1, "uniform", narrow)
    way = []
    for k in range(T):
        if k == 0:
            qk = q0
        elif k == T - 1 and jump:
            qk = qfar
        else:
            kk = k - 1 if k == T // 2 else k
            qk = q0 + (kk / (T - 2)) * 0.5 * (qs - q0)
        way.append(np.clip(qk, lo, hi))
    start = q0.copy()
    if name.startswith("cassie"):
        start[:, -1] += 9.0
    return start, way
