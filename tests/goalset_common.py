"""What the goal-set tests share (tests/test_goalset_emulation.py on the CPU, tests/test_gpu_goalset.py on the device): the workload and
the assertions that follow from the definition in include/ikgpu.h (ikgpu_dls_goalset_batch).

Workload: the G goals of a problem are the task frame's placement at G configurations drawn uniformly between the joint limits, one draw
of multistart_common.uniform_configurations per goal (seed + 1000 g); the starts come from the draw of goal 0's seed -- the regime in
which a single start of ik::dls reaches a given goal for 36-41 % of the problems on an arm, so that with a few goals every class of the
rule (goal 0 wins, a later goal wins, none reached) is populated."""
import numpy as np

import multistart_common as MC


def goal_configurations(model, B, G, seed):
    """(start [B, nq], configurations whose forward kinematics are the goals [G, B, nq])."""
    q0 = MC.uniform_configurations(model, B, seed)[0]
    qt = np.stack([MC.uniform_configurations(model, B, seed + 1000 * g)[1] for g in range(G)])
    return q0, qt


def check_goalset(got, singles, errs, err_at_result, K, label=""):
    """got = (q [B, nq], success [B], iters [B], goal [B], start [B], err_sq [B], reachable [G, B]) of the goal-set call; singles[j] =
    (q, success, iters) of the single solve of candidate j = g K + k (start k against goal g); errs[j] [B] = ||e||^2 of the reference
    evaluation at singles[j]'s q against goal g (read only for the problems no candidate solved); err_at_result [B] = ||e|| of the
    reference evaluation at got's q against goal got[3].  The four assertions of the definition."""
    q, ok, it, goal, start, err_sq, reachable = got
    B, J = q.shape[0], len(singles)
    G = J // K
    assert G * K == J and reachable.shape == (G, B), label
    assert goal.min() >= 0 and goal.max() < G and start.min() >= 0 and start.max() < K, label
    win = goal.astype(np.int64) * K + start
    rows = np.arange(B)
    # 1. the outputs are the single solve's of candidate goal K + start, bit for bit
    for x, ref, what in zip((q, ok, it), zip(*singles), ("q", "success", "iterations")):
        assert np.array_equal(x, np.stack(ref)[win, rows]), (label, what)
    # 2. the winner has the minimal key: exact in the success class and in the index among successes ...
    S = np.stack([s[1] for s in singles]).astype(bool)      # [J, B]
    any_ok = S.any(axis=0)
    first_ok = S.argmax(axis=0)
    assert np.array_equal(ok.astype(bool), any_ok), label
    assert np.array_equal(win[any_ok], first_ok[any_ok]), label
    # ... and among failures the smallest error, to 1e-10 in the norm
    E = np.sqrt(np.stack(errs))                             # [J, B]
    fail = ~any_ok
    assert (E[win, rows][fail][None, :] <= E[:, fail] + 1e-10).all(), label
    # 3. err_sq is the winner's error
    assert np.isfinite(err_sq).all() and (err_sq >= 0).all(), label
    worst = float(np.abs(np.sqrt(err_sq) - err_at_result).max())
    assert worst <= 5e-11, (label, worst)
    # 4. a goal is reachable exactly when one of its starts met the stop rule
    assert np.array_equal(reachable, S.reshape(G, K, B).any(axis=1).astype(np.uint8)), label
    return worst
