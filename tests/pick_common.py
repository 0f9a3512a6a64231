"""What the pick tests share (tests/test_pick_emulation.py on the CPU, tests/test_gpu_pick.py on the device): the four costs of
include/ikgpu.h (ikgpu_dls_pick_batch) restated in numpy on the oracle's evaluation, and the three assertions that follow from the
definition.  No tests here.

Bars.  DISTANCE, MAX_DISTANCE and LIMIT_MARGIN are a handful of IEEE operations on the winner's own q: 1e-12 relative (the issue's
figure; the n-term sums and the one division round to a few 1e-16).  MANIPULABILITY is compared with numpy.linalg.det(G)^-1/2,
G = J J^T + damping^2 I with J from the oracle at the winner's q: 8 kappa(G) 2^-53 relative, the bar tests/test_ldlt_solve_host.py sets
for the unpivoted L D L^T against a pivoted reference -- an elimination without pivoting loses up to kappa(G) ulp in a pivot, and the
lane program's Jacobian differs from the oracle's by rounding that the determinant amplifies likewise."""
import numpy as np

DISTANCE, MAX_DISTANCE, LIMIT_MARGIN, MANIPULABILITY = range(4)
RULES = (DISTANCE, MAX_DISTANCE, LIMIT_MARGIN, MANIPULABILITY)
RULE_NAMES = ("distance", "max_distance", "limit_margin", "manipulability")
REL = 1e-12
TIE = 1e-12          # two best reference keys closer than this (relative) but not equal: the problem is left out of the minimal-key check
MAX_LEFT_OUT = 0.02


# The draw, chosen on the CPU oracle alone so that at most 2 % of the problems have their two best reference keys within TIE for every
# rule, K in {2, 8, 64}, B = 130 (counted with O.dls_batch from the generated starts of the seeds 1 .. 12).  Ties per rule (DISTANCE,
# MAX_DISTANCE, LIMIT_MARGIN, MANIPULABILITY), K = 2 / 8 / 64:
#   ur5, seed 9:             0 0 0 0 / 0 0 0 0 / 1 1 1 0     (with 64 starts a solution and its copy a full turn away are both found: the
#                                                             same Jacobian, MANIPULABILITY equal to rounding -- up to 3 with other seeds)
#   rail UR5, seed 2:        0 0 0 0 / 0 0 0 0 / 0 1 0 0
#   ur5 Position, seed 7:    0 0 1 0 / 0 0 0 0 / 0 0 0 0     (its solutions wander to the limits: 1 .. 4 under LIMIT_MARGIN with every seed)
# The Cassie leg and arm7 have one redundant degree of freedom, and narrow limits: from uniform starts up to a fifth of the problems have
# two converged starts with a joint ON a limit, i.e. LIMIT_MARGIN = 0.5 exactly for both, whatever the seed (Cassie 23 .. 32 of 130 at
# K = 2, arm7 10 .. 13 at K = 8) -- so their starts are the caller's (workload below): no tie at K = 2 or 8, and nearly every start
# converges.  The seed of those two is not read by the main call (it names the generated starts of the equality checks).
NEAR = ("cassie_fixed", "arm7")
DRAW_SEED = {("ur5", 2): 9, ("ur5_rail", 2): 2, ("arm7", 2): 5, ("ur5", 0): 7, ("cassie_fixed", 2): 5}


def workload(model, name, B, K):
    """(start [B, nq], configuration whose forward kinematics is the target [B, nq], caller's starts [K-1, B, nq] or None: generated).
    Every model not in NEAR: tests/multistart_common.py's uniform draws.  The Cassie leg and arm7: targets in the middle half of every
    joint's range and all K starts within 0.3 of the half-range of the target's configuration."""
    import multistart_common as MC
    if name not in NEAR:
        q0, qt = MC.uniform_configurations(model, B, 0)
        return q0, qt, None
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(0)
    qt = mid + 0.5 * half * rng.uniform(-1, 1, (B, model.nq))
    starts = np.stack([qt + 0.3 * half * rng.uniform(-1, 1, (B, model.nq)) for _ in range(8)])
    more = np.stack([qt + 0.3 * half * rng.uniform(-1, 1, (B, model.nq)) for _ in range(max(K - 8, 0))]) if K > 8 else starts[:0]
    starts = np.concatenate([starts, more])[:K]
    return starts[0], qt, starts[1:]


def reference_costs(rule, q, support, lo, hi, q_ref, w, J=None, damping=None):
    """cost [n] of configurations q [n, nq] under `rule`.  MANIPULABILITY: from J [n, M, nv], the weighted task Jacobian of the reference
    evaluation at q, and it also returns kappa(G) [n], G = J J^T + damping^2 I."""
    s = np.flatnonzero(support)
    if rule == DISTANCE:
        return (w[s] * (q[:, s] - q_ref[:, s]) ** 2).sum(axis=1), None
    if rule == MAX_DISTANCE:
        return (w[s] * np.abs(q[:, s] - q_ref[:, s])).max(axis=1), None
    if rule == LIMIT_MARGIN:
        with np.errstate(over="ignore"):                    # (a free-flyer's entries carry -+DBL_MAX: finite, but no finite range)
            s = np.array([i for i in s if np.isfinite(lo[i]) and np.isfinite(hi[i]) and lo[i] < hi[i] and np.isfinite(hi[i] - lo[i])], dtype=int)
        if s.size == 0:
            return np.zeros(q.shape[0]), None
        return 0.5 - (np.minimum(q[:, s] - lo[s], hi[s] - q[:, s]) / (hi[s] - lo[s])).min(axis=1), None
    G = J @ J.transpose(0, 2, 1) + damping * damping * np.eye(J.shape[1])
    with np.errstate(all="ignore"):
        return 1.0 / np.sqrt(np.linalg.det(G)), np.linalg.cond(G)


def oracle_evaluation(O, om, tasks, tg):
    """evaluate(q [n, nq]) -> (e [n, M], J [n, M, nv]) on the CPU oracle; tg [n, ntasks, 12]."""
    def evaluate(q):
        eJ = [O.evaluate(om, tasks, tg[b], q[b]) for b in range(q.shape[0])]
        return np.stack([x[0] for x in eJ]), np.stack([x[1] for x in eJ])
    return evaluate


def all_reference_costs(evaluate, singles, support, lo, hi, q_ref, w, damping):
    """{rule: (cost [K, B], kappa [K, B] or None)} over the K single solves' results, and err [K, B] = ||e||^2 of the reference
    evaluation there.  evaluate(q [B, nq]) -> (e [B, M], J [B, M, nv])."""
    eJ = [evaluate(s[0]) for s in singles]
    out = {}
    for rule in RULES:
        cs, ks = zip(*[reference_costs(rule, s[0], support, lo, hi, q_ref, w, x[1], damping) for s, x in zip(singles, eJ)])
        out[rule] = (np.stack(cs), np.stack(ks) if ks[0] is not None else None)
    return out, np.stack([(x[0] ** 2).sum(axis=1) for x in eJ])


def check_pick(got, singles, rule, cost_ref, kappa, err_ref, label=""):
    """got = (q [B, nq], success, iters, winner, cost, err_sq) of the pick call; singles[k] = (q, success, iters) of the single solve from
    start k; cost_ref / kappa / err_ref [K, B] from all_reference_costs.  The three assertions of the definition; returns
    (problems with two or more converged starts, problems whose winner is not the lowest-index converged start, problems left out)."""
    q, ok, it, win, cost, err_sq = got
    B, K = q.shape[0], len(singles)
    rows = np.arange(B)
    assert win.min() >= 0 and win.max() < K, label
    # 1. the outputs are the single solve's from start winner[b], bit for bit
    for x, ref, what in zip((q, ok, it), zip(*singles), ("q", "success", "iterations")):
        assert np.array_equal(x, np.stack(ref)[win, rows]), (label, what)
    # 2. the winner attains the minimal key: a converged start whenever there is one, among them the smallest cost ...
    S = np.stack([s[1] for s in singles]).astype(bool)      # [K, B]
    any_ok = S.any(axis=0)
    assert np.array_equal(ok.astype(bool), any_ok), label
    keyed = np.where(S, cost_ref, np.inf)
    order = np.sort(keyed, axis=0)
    close = np.zeros(B, bool)
    if K > 1:
        # (an EXACT tie of the reference costs stays in: it comes from identical operands -- the same joint on the same limit, the same q
        # -- which tie in the lane's arithmetic too, and the definition sends it to the lower index, which argmin returns)
        two = any_ok & np.isfinite(order[1]) & (order[1] != order[0])
        close[two] = (order[1][two] - order[0][two]) <= TIE * np.maximum(np.abs(order[1][two]), np.abs(order[0][two]))
    checked = any_ok & ~close
    assert np.array_equal(win[checked], keyed.argmin(axis=0)[checked]), (label, np.flatnonzero(checked & (win != keyed.argmin(axis=0))))
    assert close.sum() <= MAX_LEFT_OUT * B, (label, int(close.sum()))
    # ... and when none converged the smallest error, to 1e-10 in the norm (tests/multistart_common.py)
    E = np.sqrt(err_ref)
    fail = ~any_ok
    assert (E[win, rows][fail][None, :] <= E[:, fail] + 1e-10).all(), label
    # 3. cost is the winner's cost, recomputed
    want = cost_ref[win, rows]
    assert np.isfinite(cost).all() and (cost >= 0).all(), label
    if rule == MANIPULABILITY:
        rel = np.abs(cost - want) / want
        worst = rel / (8 * kappa[win, rows] * 2.0 ** -53)
        print("%s: manipulability cost against numpy: worst relative difference %.3g, %.3g of its bar (kappa there %.3g, median kappa %.3g)"
              % (label, rel.max(), worst.max(), kappa[win, rows][worst.argmax()], np.median(kappa[win, rows])))
        assert worst.max() <= 1.0, (label, "cost off by %.3g of its bar" % worst.max())
    else:
        rel = np.abs(cost - want) / np.maximum(np.abs(want), np.finfo(float).tiny)
        rel[(cost == 0) & (want == 0)] = 0.0
        assert rel.max() <= REL, (label, rel.max())
    assert np.abs(np.sqrt(err_sq) - E[win, rows]).max() <= 5e-11, label      # (err_sq as the multi-start call reports it)
    first_ok = S.argmax(axis=0)
    return int((S.sum(axis=0) >= 2).sum()), int((any_ok & (win != first_ok)).sum()), int(close.sum())
