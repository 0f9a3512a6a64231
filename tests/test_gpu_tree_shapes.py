"""Every build of the free-flyer tree kernel on the device, on robots other than Cassie as well: the matrix of
tests/tree_shapes_common.py -- (NJ, chains) in {(7,2), (7,1), (6,2), (6,1)} x {hot, hot-never, mask, general x {folded, unfolded} x
{none, posture, constraint, posture+constraint, pik}} -- through the C ABI at B = 197 against the CPU oracle.  Per case:

  (a) the kernel name and the build string (include/ikgpu.h ikgpu_dls_tree_build_plan: what the launcher dispatches on);
  (b) task_frames_fk_batch within 1e-13 and evaluate_batch (e and dense J) within 1e-10 of the oracle, in both layouts (the stage
      kernels of a problem with extras run on the generic program: capi.cpp routes them);
  (c) step-synchronised (rule S1 of tests/test_gpu_full_size.py): from the oracle's k-th iterate, k = 0, 1, 2, the device's next
      iterate is within STEP_BAR = 1e-9 rad on every lane; the on-limit problems keep their joint on the limit;
  (d) the stop-rule run: flags and iteration counts equal to the oracle's, q within TOL = 1e-6 rad, a stop at iteration 0 returns q0
      untouched (also its entries beyond their limits), AoS equals SoA to the bit, two runs give the same bits;
  (e) constraint cells against O.dls_batch_constrained, and the constraint holds to first order (tests/test_gpu_constraints.py);
  (f) pik cells against O.pik_batch;
  (g) against the generic kernel on the same problem: flags equal, q within 1e-8 rad (as tests/test_gpu_tree_fixed_base.py).
Then (h) the folded and the unfolded general builds on the SAME geometry -- dual_ur5 with the second arm's mount turned by a full
turn, whose rotation matrix differs from the identity by rounding only, so that chain B loses the mask bit and nothing else changes --
agree within STEP_BAR after 1, 2 and 3 steps; (i) the refill twins (NJ = 7) forced at small ragged sizes return the lock-step bits;
and the posture rows outside the chains up to the cap of 32 (one chain: more than 64 KB of LDS per workgroup from 28 rows on; the
other limb pinned: either side of the park buffer's 63 entries).

Alignment-row cases are not run past 3 iterations under full steps (their stop rule takes damping 1e-1 and a half step).  A device
lane that needs the oracle-instability exclusion goes through assert_within_bar_or_oracle_unstable, unchanged."""
import numpy as np
import pytest

import tree_shapes_common as TS
from test_gpu_full_size import STEP_BAR
from test_gpu_generic import assert_within_bar_or_oracle_unstable
from test_gpu_refill import env

pytestmark = pytest.mark.gpu
FK_BAR, EVAL_BAR, GENERIC_BAR = 1e-13, 1e-10, 1e-8


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _soa(torch, q, tg):
    return torch.from_numpy(np.ascontiguousarray(q.T)).cuda(), torch.from_numpy(np.ascontiguousarray(tg.transpose(1, 2, 0))).cuda()


class Device:
    """The case's problem on the device: ik::dls, or ik::pik with two levels for a pik cell."""

    def __init__(self, torch, x):
        import ik_amd
        self.ik, self.torch, self.x, self.pik = ik_amd, torch, x, x.case.pik
        self.data = ik_amd.pik_data(x.problem, device=0) if self.pik else ik_amd.dls_data(x.problem, device=0)

    def kernel(self, rule):
        if self.pik:
            self.data.lambda_ = [rule[1], rule[4]]
        return self.data.kernel

    def solve(self, q0, tg, rule, layout="soa"):
        """(q [B, nq], success, iterations) as numpy arrays; q0 [B, nq], tg [B, ntasks, 12]."""
        ik, torch = self.ik, self.torch
        if layout == "soa":
            Q0, T = _soa(torch, q0, tg)
        else:
            Q0, T = torch.from_numpy(np.ascontiguousarray(q0)).cuda(), torch.from_numpy(np.ascontiguousarray(tg)).cuda()
        v = ik.inverse_kinematics_visitor(rule[3])
        if self.pik:
            self.data.lambda_ = [rule[1], rule[4]]
            Q, ok, it = ik.pik_batch(self.x.problem, Q0, T, self.data, v, ik.pik_parameters(max_iterations=rule[0], step_length=rule[2]), layout=layout)
        else:
            Q, ok, it = ik.dls_batch(self.x.problem, Q0, T, self.data, v, ik.dls_parameters(max_iterations=rule[0], damping=rule[1], step_length=rule[2]),
                                     layout=layout)
        Q = Q.cpu().numpy()
        return (Q.T if layout == "soa" else Q), ok.cpu().numpy(), it.cpu().numpy()


def _one_step(rule):
    return (1,) + tuple(rule[1:3]) + (-1.0,) + tuple(rule[4:])


def _check_stages(torch, dev, x):
    """(b): the stage kernels in both layouts."""
    import oracle as O
    ik = dev.ik
    frames = [i for i, s in enumerate(x.ospec) if s[2] < 3]
    want_fk = O.fk_batch(x.om, x.q0, [x.ospec[i][0] for i in frames])
    want = [O.evaluate(x.om, x.tasks, x.tg[b], x.q0[b]) for b in range(TS.B)]
    want_e, want_J = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    Q0, T = _soa(torch, x.q0, x.tg)
    Qa, Ta = torch.from_numpy(np.ascontiguousarray(x.q0)).cuda(), torch.from_numpy(np.ascontiguousarray(x.tg)).cuda()
    worst = [0.0, 0.0, 0.0]
    for layout in ("soa", "aos"):
        F = ik.task_frames_fk_batch(x.problem, Q0 if layout == "soa" else Qa, dev.data, layout=layout).cpu().numpy()
        e, J = ik.evaluate_batch(x.problem, Q0 if layout == "soa" else Qa, T if layout == "soa" else Ta, dev.data, layout=layout)
        e, J = e.cpu().numpy(), J.cpu().numpy()
        if layout == "soa":
            F, e, J = F.transpose(2, 0, 1), e.T, J.transpose(2, 0, 1)
        worst = [max(worst[0], np.abs(F[:, frames] - want_fk).max()), max(worst[1], np.abs(e - want_e).max()), max(worst[2], np.abs(J - want_J).max())]
    assert worst[0] <= FK_BAR and worst[1] <= EVAL_BAR and worst[2] <= EVAL_BAR, (x.case.id, worst)
    return worst


def _first_order_constraint(dev, x):
    """(e): after ONE small step the constrained coordinates of the pinned frame have moved by O(step^2) only."""
    import oracle as O
    rule = (1, 1e-2, 0.01, -1.0)
    q1, _, _ = dev.solve(x.q0, x.tg, rule)
    f, t, r = x.case.cons[0]
    fid = x.model.getFrameId(f)
    checked = 0
    for b in range(0, TS.B, 7):
        moved = np.abs(q1[b] - x.q0[b]).max()
        inside = np.all((q1[b] > x.lo + 1e-9) & (q1[b] < x.hi - 1e-9)) and np.all((x.q0[b] >= x.lo) & (x.q0[b] <= x.hi))
        if not inside or moved <= 1e-5:
            continue
        p0, p1 = O.fk(x.om, x.q0[b])[1][fid][9:], O.fk(x.om, q1[b])[1][fid][9:]
        assert np.abs(p1 - p0).max() < 20 * moved * moved + 1e-12, (x.case.id, b, np.abs(p1 - p0).max(), moved)
        checked += 1
    assert checked >= 5, (x.case.id, checked)


def _check_case(torch, case, monkeypatch):
    import oracle as O
    for name in ("IKGPU_DLS_KERNEL", "IKGPU_PIK_KERNEL", "IKGPU_REFILL", "IKGPU_TREE_NEVER_OFF"):
        monkeypatch.delenv(name, raising=False)
    x = TS.inputs(case)
    dev = Device(torch, x)
    rules = TS.rules(case)
    # (a)
    for rule in rules:
        kernel, build = TS.plan_names(case, rule)
        assert build == (case.build_never if rule[3] < 0 else case.build), (case.id, rule, build)
        if case.pik:
            assert kernel == case.kernel and dev.kernel(rule) == case.kernel[:-1] + ",pik_levels=2>", (case.id, dev.kernel(rule))
        else:
            assert kernel == case.kernel and dev.kernel(rule) == case.kernel, (case.id, dev.kernel(rule))
    # (b)
    stage = _check_stages(torch, dev, x)
    # (c)
    q_k, steps = np.array(x.q0), []
    for k in range(3):
        one = _one_step(rules[k])
        want, _, _ = TS.oracle_solve(O, x, x.tg, q_k, one)
        got, _, it = dev.solve(q_k, x.tg, one)
        assert (it == 1).all()
        d = np.abs(got - want).max(axis=1)
        steps.append(d.max())
        assert d.max() <= STEP_BAR, (case.id, k, d.max(), int(d.argmax()))
        if k == 0:
            for b, j in x.on_limit:
                assert got[b, j] == x.q0[b, j], (case.id, b, j)
        q_k = want
    # (d), and (e) / (f) through the case's own oracle solve
    rule = rules[-1]
    tg = np.array(x.tg)
    zero = np.arange(10, 20)
    tg[zero] = TS.targets_at(O, x.om_free, x.ospec, x.q0[zero])     # the stop test holds at q0: no step, no clipping
    q, ok, it = dev.solve(x.q0, tg, rule)
    q_ref, ok_ref, it_ref = TS.oracle_solve(O, x, tg, x.q0, rule)
    assert (it_ref[zero] == 0).all() and ok_ref[zero].all(), (case.id, it_ref[zero])
    assert np.array_equal(ok, ok_ref) and np.array_equal(it, it_ref), (case.id, rule, np.flatnonzero(it != it_ref))
    assert np.array_equal(q[zero], x.q0[zero]), case.id
    assert_within_bar_or_oracle_unstable(lambda t_, q_: TS.oracle_solve(O, x, t_, q_, rule), q, q_ref, tg, x.q0, (case.id, rule))
    qa, oka, ita = dev.solve(x.q0, tg, rule, layout="aos")
    q2, ok2, it2 = dev.solve(x.q0, tg, rule)
    for a, b_, c_ in ((q, qa, q2), (ok, oka, ok2), (it, ita, it2)):
        assert np.array_equal(a, b_) and np.array_equal(a, c_), case.id
    if case.cons:
        _first_order_constraint(dev, x)
    # (g)
    monkeypatch.setenv("IKGPU_PIK_KERNEL" if case.pik else "IKGPU_DLS_KERNEL", "generic")
    monkeypatch.setenv("IKGPU_GENERIC_STATIC", "0")     # the interpreter forms: nothing is compiled at run time for the comparison
    gen = Device(torch, x)
    assert gen.kernel(rule).startswith("pik_generic<" if case.pik else "dls_generic<"), gen.kernel(rule)
    qg, okg, itg = gen.solve(x.q0, tg, rule)
    monkeypatch.delenv("IKGPU_PIK_KERNEL" if case.pik else "IKGPU_DLS_KERNEL")
    assert np.array_equal(ok, okg) and np.array_equal(it, itg), case.id
    dg = np.abs(q - qg).max()
    assert dg <= GENERIC_BAR, (case.id, dg)
    print("%s [%s | %s]: FK %.1e, e %.1e, J %.1e; step maxima %s rad; stop rule: iterations %d..%d, success %.3f, max |dq| %.2e rad; "
          "against the generic kernel %.2e" % (case.id, case.kernel, case.build, stage[0], stage[1], stage[2], " ".join("%.2e" % s for s in steps),
                                               it.min(), it.max(), ok.mean(), np.abs(q - q_ref).max(), dg))


def _shape_cases(nj, folded):
    return [c for c in TS.CASES if c.nj == nj and ("-folded-" in c.id) == folded]


@pytest.mark.parametrize("case", _shape_cases(7, False), ids=lambda c: c.id)
def test_tree_builds_nj7_unfolded(torch_cuda, monkeypatch, case):
    _check_case(torch_cuda, case, monkeypatch)


@pytest.mark.parametrize("case", _shape_cases(7, True), ids=lambda c: c.id)
def test_tree_builds_nj7_folded(torch_cuda, monkeypatch, case):
    _check_case(torch_cuda, case, monkeypatch)


@pytest.mark.parametrize("case", _shape_cases(6, True), ids=lambda c: c.id)
def test_tree_builds_nj6_folded(torch_cuda, monkeypatch, case):
    _check_case(torch_cuda, case, monkeypatch)


@pytest.mark.parametrize("case", _shape_cases(6, False), ids=lambda c: c.id)
def test_tree_builds_nj6_unfolded(torch_cuda, monkeypatch, case):
    _check_case(torch_cuda, case, monkeypatch)


@pytest.mark.parametrize("case", TS.EDGE_CASES, ids=lambda c: c.id)
def test_posture_rows_outside_the_chains_up_to_the_cap(torch_cuda, monkeypatch, case):
    _check_case(torch_cuda, case, monkeypatch)


def test_the_gpu_matrix_reaches_every_build(torch_cuda):
    ran = [c for nj in (6, 7) for f in (True, False) for c in _shape_cases(nj, f)]
    assert len(ran) == len(TS.CASES) and {c.build for c in ran} | {c.build_never for c in ran} == TS.every_build_string()


@pytest.mark.parametrize("extras", ["none", "posture", "pik", "constraint", "posture+constraint"])
def test_folded_and_unfolded_general_builds_agree_on_the_same_geometry(torch_cuda, monkeypatch, extras):
    """(h) dual_ur5 with the second arm mounted straight (both chains carry HotMask<6>: folded) and turned by a full turn about z
    (rpy "0 0 6.283185307179586": the rotation's sine is -2.4e-16, not zero, so chain B loses bit 0 and the unfolded build runs on a
    robot that is the same to rounding).  Same starts, targets re-derived per robot; 1, 2 and 3 steps."""
    torch = torch_cuda
    for name in ("IKGPU_DLS_KERNEL", "IKGPU_PIK_KERNEL", "IKGPU_REFILL", "IKGPU_TREE_NEVER_OFF"):
        monkeypatch.delenv(name, raising=False)
    a = TS.CASE_BY_ID["nj6-ch2-folded-dual_ur5-general-" + extras]
    b = a._replace(id=a.id.replace("dual_ur5", "dual_ur5_turn"), robot="dual_ur5_turn", build=a.build.replace(",folded,", ",unfolded,"),
                   build_never=a.build_never.replace(",folded,", ",unfolded,"))
    xa, xb = TS.inputs(a), TS.inputs(b)
    assert np.array_equal(xa.q0, xb.q0) and np.abs(xa.tg - xb.tg).max() < 1e-14
    da, db = Device(torch, xa), Device(torch, xb)
    for k, rule in enumerate(TS.rules(a)[:3]):
        assert TS.plan_names(a, rule)[1] == a.build_never and TS.plan_names(b, rule)[1] == b.build_never, (TS.plan_names(a, rule), TS.plan_names(b, rule))
        qa, oka, ita = da.solve(xa.q0, xa.tg, rule)
        qb, okb, itb = db.solve(xb.q0, xb.tg, rule)
        assert np.array_equal(ita, itb) and np.array_equal(oka, okb)
        d = np.abs(qa - qb).max()
        print("general,%s after %d steps: folded against unfolded %.2e rad" % (extras, k + 1, d))
        assert d <= STEP_BAR, (extras, k + 1, d)


@pytest.mark.parametrize("case_id,twin", TS.REFILL_CASES)
def test_refill_twins_return_the_lock_step_bits(torch_cuda, monkeypatch, case_id, twin):
    """(i) every refill twin on one chain and on two, IKGPU_REFILL=1 forced at small ragged sizes against IKGPU_REFILL=0."""
    torch = torch_cuda
    for name in ("IKGPU_DLS_KERNEL", "IKGPU_TREE_NEVER_OFF"):
        monkeypatch.delenv(name, raising=False)
    case = TS.CASE_BY_ID[case_id]
    x = TS.inputs(case)
    dev = Device(torch, x)
    base = TS.rules(case)[-1]
    assert TS.plan_names(case, base)[1].endswith(",refill=" + twin)
    for n in (1, 63, 65, TS.B):
        for max_it in (1, 2, 5, 100):
            rule = (max_it,) + tuple(base[1:])
            for layout in ("soa", "aos"):
                with env(IKGPU_REFILL="0"):
                    want = dev.solve(x.q0[:n], x.tg[:n], rule, layout=layout)
                for mode in ("1", "2"):
                    with env(IKGPU_REFILL=mode):
                        got = dev.solve(x.q0[:n], x.tg[:n], rule, layout=layout)
                    for w, g in zip(want, got):
                        assert np.array_equal(w, g), (case_id, n, max_it, layout, mode)
            assert (want[2] <= max_it).all() and (want[2][want[1] == 0] == max_it).all()
