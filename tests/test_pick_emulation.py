"""The pieces of the pick kernels (device/pick.hpp: the four costs and the key; dls_chain_pick_lane and pick_store in
ik_amd/csrc/device/chain_kernel_body.hpp, hot_pick_lane in device/chain_hot.hpp), compiled for the host by this test
(tests/lane_emu/pick_emu.cpp) and run lane after lane.

ikgpu_dls_pick_batch is DEFINED through K single solves (include/ikgpu.h), so "right" is (tests/pick_common.py check_pick):
q / success / iterations equal, by np.array_equal, what the single-solve body of the SAME lane program returns from start winner[b];
the winner attains the minimal key over the K single solves, with the cost recomputed in numpy on the oracle's evaluation (a problem
whose two best reference keys differ by less than 1e-12 relative without being equal is left out, at most 2 % of them; an exact tie
must go to the lower index); and cost[b] is that recomputation
within 1e-12 relative (MANIPULABILITY: against numpy.linalg.det within 8 kappa(G) 2^-53 relative, see pick_common).

The workload is tests/pick_common.py's (workload, DRAW_SEED: chosen on the oracle alone so that ties are rare), with a q_ref drawn
uniformly (seed 11) and weights 0.25 .. 2.  Counted with the oracle's solves and costs alone, K = 8 on ur5 (seed 9), B = 130: 103
problems have two or more converged starts; the winner is not the lowest-index converged start in 68 (DISTANCE), 70 (MAX_DISTANCE),
66 (LIMIT_MARGIN) and 69 (MANIPULABILITY) problems; no problem is left out for a tie.  (The lane programs round differently from the
oracle and from each other, so a start on the edge of the stop rule may fall the other way: they count 107 .. 111 problems with two or
more converged starts, 66 .. 75 winners that are not the first converged start, and leave out at most one problem.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, urdf_path

import oracle as O
import multistart_common as MC
import pick_common as PK

B = 130
_p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
PROGRAMS = {"runtime": 0, "device_general": 1, "hot": 2}


@pytest.fixture(scope="module")
def emu(native_built):
    src = os.path.join(ROOT, "tests", "lane_emu", "pick_emu.cpp")
    out = os.path.join(ROOT, "tests", "lane_emu", "libpick_emu.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp",
                                                    "device/multistart.hpp", "device/pick.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.pick_emu_last_error.restype = C.c_char_p
    for f in (L.pick_emu_distance, L.pick_emu_max_distance, L.pick_emu_limit_margin, L.pick_emu_manipulability):
        f.restype = C.c_double
    L.pick_emu_key.restype = C.c_uint64
    L.pick_emu_key.argtypes = [C.c_int, C.c_double, C.c_double]
    return L


# ---- the costs ---------------------------------------------------------------------------------------------------------------------
def test_distance_and_limit_margin_costs_follow_their_formulas(emu):
    rng = np.random.default_rng(0)
    for n in (1, 6, 7, 8):
        for _ in range(50):
            q, ref, w = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0, 2, n)
            w[rng.integers(n)] = 0.0
            d = emu.pick_emu_distance(n, _p(w), _p(q), _p(ref))
            m = emu.pick_emu_max_distance(n, _p(w), _p(q), _p(ref))
            assert abs(d - (w * (q - ref) ** 2).sum()) <= PK.REL * d and abs(m - (w * np.abs(q - ref)).max()) <= PK.REL * m
            lo, hi = rng.uniform(-4, -3, n), rng.uniform(3, 4, n)
            q[0] = lo[0] if n > 1 else q[0]                      # a joint on its limit: margin 0, cost 0.5
            want = 0.5 - (np.minimum(q - lo, hi - q) / (hi - lo)).min()
            got = emu.pick_emu_limit_margin(n, _p(q), _p(lo), _p(hi))
            assert abs(got - want) <= PK.REL * want and 0 <= got <= 0.5
            assert n == 1 or got == 0.5
    q = np.array([0.5, -0.25, 1.0])
    assert emu.pick_emu_distance(3, _p(np.ones(3)), _p(q), _p(q)) == 0.0 and emu.pick_emu_max_distance(3, _p(np.ones(3)), _p(q), _p(q)) == 0.0
    # entries without finite limits, or with lower >= upper, take no part; a support with none of the other kind costs 0
    lo, hi = np.array([-np.inf, -1.0, 2.0]), np.array([1.0, np.inf, 2.0])
    assert emu.pick_emu_limit_margin(3, _p(q), _p(lo), _p(hi)) == 0.0
    lo, hi = np.array([-np.inf, -1.0, 0.0]), np.array([1.0, 1.0, 4.0])
    assert emu.pick_emu_limit_margin(3, _p(q), _p(lo), _p(hi)) == 0.5 - min(0.75 / 2.0, 1.0 / 4.0)
    big = np.finfo(float).max                                                  # a free-flyer's entries: finite limits without a finite range
    assert emu.pick_emu_limit_margin(3, _p(q), _p(np.array([-big, -1.0, 0.0])), _p(np.array([big, 1.0, 4.0]))) == 0.5 - min(0.75 / 2.0, 1.0 / 4.0)
    assert emu.pick_emu_limit_margin(2, _p(q), _p(np.array([-big, -big])), _p(np.array([big, big]))) == 0.0
    mid = np.array([0.0, 0.0, 2.0])
    assert emu.pick_emu_limit_margin(3, _p(mid), _p(lo), _p(hi)) == 0.0      # every bounded joint in the middle of its range


def test_manipulability_cost_is_the_determinant_of_the_damped_gram_matrix(emu):
    rng = np.random.default_rng(1)
    worst = 0.0
    for M in (6, 3):
        for trial in range(200):
            J = rng.normal(size=(M, 7)) * 10.0 ** rng.uniform(-3, 1, (M, 1))      # rows of very different size: kappa up to ~1e8
            if trial % 4 == 0:
                J[M - 1] = J[0] + 1e-5 * rng.normal(size=7)                       # two nearly dependent rows: the damping carries the pivot
            lam = 10.0 ** rng.uniform(-3, -1)
            G = J @ J.T + lam * lam * np.eye(M)
            got = emu.pick_emu_manipulability(M, _p(np.ascontiguousarray(G)))
            det_ref, kappa = np.linalg.det(G), np.linalg.cond(G)
            want = 1.0 / np.sqrt(det_ref)
            off = abs(got - want) / (8 * kappa * 2.0 ** -53 * want)
            worst = max(worst, off)
            assert off <= 1.0, (M, trial, kappa, off)
    print("manipulability: worst |cost - det_numpy^-1/2| = %.3g of the bar 8 kappa 2^-53" % worst)


def test_the_key_orders_convergence_then_cost_then_index(emu):
    key = lambda ok, cost, err: emu.pick_emu_key(int(ok), float(cost), float(err))
    inf, nan = float("inf"), float("nan")
    # a converged start beats any failed one, whatever the two values
    assert key(True, 1e300, 0.0) < key(False, 0.0, 0.0) and key(True, inf, 0.0) < key(False, 0.0, 1e-300)
    # among converged starts the cost orders (the error is not looked at), among failed ones the error (the cost is not)
    assert key(True, 0.1, 5.0) < key(True, 0.2, 1.0) and key(True, 0.1, 5.0) == key(True, 0.1, 0.0)
    assert key(False, 5.0, 0.1) < key(False, 1.0, 0.2) and key(False, 5.0, 0.1) == key(False, 0.0, 0.1)
    assert key(True, 0.0, 1.0) == 0 and key(True, 5e-324, 0.0) == 1
    # NaN / infinity rank last within their class
    for bad in (inf, nan, -nan, -inf):
        assert key(True, bad, 0.0) == key(True, inf, 0.0) > key(True, 1.7e308, 0.0)
        assert key(False, 0.0, bad) == key(False, 0.0, inf) > key(False, 0.0, 1.7e308)

    def select(items):
        keys = np.array([key(*x) for x in items], dtype=np.uint64)
        log2K = int(np.log2(len(items)))
        return emu.pick_emu_select(log2K, _p(keys))

    assert select([(False, 0, 1e-9), (True, 7.0, 0), (True, 3.0, 0), (False, 0, 0.0)]) == 2
    assert select([(False, 0, 3.0), (True, 2.0, 0), (True, 2.0, 0), (True, 2.5, 0)]) == 1          # a cost tie goes to the lower index
    assert select([(True, 2.0, 0)] * 8) == 0
    assert select([(True, nan, 0), (True, inf, 0), (True, 9e307, 0), (False, 0, 0.0)]) == 2        # NaN / inf cost last among the converged
    assert select([(True, nan, 0), (False, 0, 0.0)]) == 0                                           # ... but still ahead of a failed start
    assert select([(False, 1e-3, 4.0), (False, 1e-9, 2.0), (False, 5.0, 2.0), (False, 0.0, nan)]) == 1   # none converged: the error, lowest index
    rng = np.random.default_rng(2)
    for log2K in (1, 3, 6):
        K = 1 << log2K
        for _ in range(40):
            items = [(rng.random() < 0.4, float(rng.integers(0, 4)), float(rng.integers(0, 4))) for _ in range(K)]
            want = min(range(K), key=lambda k: (0 if items[k][0] else 1, items[k][1] if items[k][0] else items[k][2], k))
            assert select(items) == want


# ---- the lane programs -------------------------------------------------------------------------------------------------------------
def setup(name, K=8):
    import ik_amd
    from ik_amd import capi
    import prismatic_common as PC
    robot, frame, ktype = {"ur5": ("ur5", "tool0", 2), "arm7": ("arm7", "tool", 2), "cassie_fixed": ("cassie_fixed", "LeftFootFront", 2), "ur5_rail": ("ur5_rail", "tool0", 2),
                           "ur5_position": ("ur5", "tool0", 0)}[name]
    urdf = PC.robot_xml(robot).encode() if robot == "ur5_rail" else open(urdf_path(robot), "rb").read()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    q0, qt, near = PK.workload(model, robot, B, K)
    tg = O.fk_batch(om, qt, [fid])                                   # [B, 1, 12]
    task = capi.Task(fid, 0, ktype, 0, (C.c_double * 6)(*[1.0] * 6))
    ot = O.make_tasks([(fid, 0, ktype, 0, None)])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(11)
    q_ref = rng.uniform(lo, hi, (B, model.nq))
    w = rng.uniform(0.25, 2.0, model.nq)
    return urdf, model, om, task, ot, q0, tg, lo, hi, q_ref, w, near, PK.DRAW_SEED[(robot, ktype)]


def emu_support(emu, urdf, task, nq):
    sup = np.zeros(nq, np.uint8)
    assert emu.pick_emu_support(urdf, C.c_size_t(len(urdf)), C.byref(task), _p(sup)) == 0, emu.pick_emu_last_error()
    return sup.astype(bool)


def emu_starts(emu, urdf, task, q0, K, seed):
    out = np.full((K - 1,) + q0.shape, np.nan)
    rc = emu.pick_emu_starts(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(q0.shape[0]), K, _p(np.ascontiguousarray(q0)), C.c_uint64(seed), _p(out), 1)
    assert rc == 0, emu.pick_emu_last_error()
    return out


def single_solves(emu, urdf, task, program, starts_all, tg, prm):
    res = []
    for qs in starts_all:
        qi = np.ascontiguousarray(qs)
        qo, ok, it = np.full(qi.shape, np.nan), np.full(B, 7, np.uint8), np.full(B, -7, np.int32)
        rc = emu.pick_emu_single(urdf, C.c_size_t(len(urdf)), C.byref(task), program, C.c_int64(B), _p(qi), _p(np.ascontiguousarray(tg.reshape(B, 12))),
                                 C.byref(prm), _p(qo), _p(ok), _p(it), 1)
        assert rc == 0, emu.pick_emu_last_error()
        res.append((qo, ok, it))
    return res


def pick(emu, urdf, task, program, q0, starts, seed, tg, prm, K, rule, q_ref, w, layout, optional=True):
    """One call of the pick lane programs.  q0, q_ref [B, nq], starts None or [K-1, B, nq], tg [B, 1, 12]; AoS views back."""
    cv = lambda a: None if a is None else np.ascontiguousarray(a if layout == 1 else a.T)
    qi, ri = cv(q0), cv(q_ref)
    si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
    ti = cv(tg.reshape(B, 12))
    qo = np.full(qi.shape, np.nan)
    ok, it, win, cost, err = ((np.full(B, 7, np.uint8), np.full(B, -7, np.int32), np.full(B, -7, np.int32), np.full(B, np.nan), np.full(B, np.nan))
                              if optional else (None,) * 5)
    rc = emu.pick_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), program, C.c_int64(B), K, _p(qi), _p(si), C.c_uint64(seed), _p(ti), C.byref(prm),
                          rule, _p(ri), _p(w), _p(qo), _p(ok), _p(it), _p(win), _p(cost), _p(err), layout)
    assert rc == 0, emu.pick_emu_last_error()
    return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, win, cost, err


CASES = [(n, p) for n in ("ur5", "cassie_fixed", "ur5_rail") for p in sorted(PROGRAMS)] + [("ur5_position", "runtime"), ("ur5_position", "device_general")]


@pytest.mark.parametrize("name,program", CASES)
@pytest.mark.parametrize("K", [2, 8])
def test_pick_program_returns_the_cheapest_converged_single_solve(emu, name, program, K):
    from ik_amd import capi
    urdf, model, om, task, ot, q0, tg, lo, hi, q_ref, w, near, SEED = setup(name, K)
    prog = PROGRAMS[program]
    support = emu_support(emu, urdf, task, model.nq)
    damping = 1e-2
    prm = capi.DlsParams(100, damping, 1.0, 1e-4)
    gen = emu_starts(emu, urdf, task, q0, K, SEED)                   # [K-1, B, nq]
    explicit = gen if near is None else near                        # the starts of the main call (near: the caller's, None: generated), spelt out
    singles = single_solves(emu, urdf, task, prog, np.concatenate([q0[None], explicit]), tg, prm)
    refs, err_ref = PK.all_reference_costs(PK.oracle_evaluation(O, om, ot, tg), singles, support, lo, hi, q_ref, w, damping)
    n_ok = [int(s[1].sum()) for s in singles]
    # (a Position task far from the target's orientation: the oracle's Jacobian and the lane program's agree to 1e-12 only, log3 near pi, and
    # MANIPULABILITY is defined on the latter -- tests/test_gpu_pick.py checks it against ikgpu_evaluate_batch)
    for rule in (PK.RULES if name != "ur5_position" else PK.RULES[:3]):
        label = (name, program, K, PK.RULE_NAMES[rule])
        got = pick(emu, urdf, task, prog, q0, near, SEED, tg, prm, K, rule, q_ref, w, 1)
        several, moved, left_out = PK.check_pick(got, singles, rule, refs[rule][0], refs[rule][1], err_ref, label)
        print("%s %s K=%d %-14s: converged %s of %d per start; %d problems with >= 2 converged starts, winner not the first converged one in %d, left out %d"
              % (name, program, K, PK.RULE_NAMES[rule], n_ok, B, several, moved, left_out))
        if K == 8 and name == "ur5":                                # not vacuous: the rule has something to choose from, and chooses
            assert several >= B / 2 and moved >= B / 5, label
        assert (~got[1].astype(bool)).any() or name != "ur5"        # (some problems fail from every start: the error fallback is exercised)
        # the caller's starts instead of generated ones, the other layout, and without the optional arrays: the same bits
        for starts, layout in ((explicit, 1), (near, 0), (explicit, 0)):
            again = pick(emu, urdf, task, prog, q0, starts, SEED, tg, prm, K, rule, q_ref, w, layout)
            for x, y in zip(again, got):
                assert np.array_equal(x, y), (label, layout, starts is None)
        q_only = pick(emu, urdf, task, prog, q0, near, SEED, tg, prm, K, rule, q_ref, w, 0, optional=False)
        assert all(x is None for x in q_only[1:]) and np.array_equal(q_only[0], got[0]), label
    # q_ref = NULL is q0, w = NULL is ones: the same bits as passing them
    for rule in (PK.DISTANCE, PK.MAX_DISTANCE):
        a = pick(emu, urdf, task, prog, q0, None, SEED, tg, prm, K, rule, None, None, 1)
        b = pick(emu, urdf, task, prog, q0, gen, SEED, tg, prm, K, rule, q0, np.ones(model.nq), 1)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (name, program, K, rule, "defaults")
    # every start equal to q0 with DISTANCE from q0: every key ties, the lowest index wins
    same = np.broadcast_to(q0, (K - 1,) + q0.shape).copy()
    tie = pick(emu, urdf, task, prog, q0, same, SEED, tg, prm, K, PK.DISTANCE, None, None, 1)
    assert (tie[3] == 0).all() and np.array_equal(tie[0], singles[0][0]) and np.array_equal(tie[1], singles[0][1])
