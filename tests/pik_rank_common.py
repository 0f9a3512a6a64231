"""The rank rule of ik::pik (reference ik/ik/pik.cpp:58-61: the complete orthogonal decomposition behind pinv counts a pivot only
above eps * min(rows, cols) * the largest pivot) on inputs where keeping or dropping a direction changes the answer: weights that
put one row a factor 1e3 above / 1e4 below the threshold, an exact zero row, structurally rank-deficient levels, an empty middle
level, an all-zero level.  Shared by the emulator tests (tests/test_pik_rank_emulation.py), the host-compiled lane program
(tests/test_static_host.py) and the device tests (tests/test_gpu_pik_rank.py): the same inputs, the same references, one rule.

The acceptance rule is decided by the reference alone.  Per case and parameter set, q_d = the double oracle's ik::pik and q_q = the
same statements in _Float128 (oracle/ik_oracle_ext.c).  A lane is DETERMINED when max|q_d - q_q| <= 1e-9: the reference's own
rounding does not decide its answer.  Every determined lane of a form must be within 1e-8 rad of q_q, with the double oracle's
success flag and iteration count.  At most 2 of the 130 lanes may be undetermined (none after one iteration).

Inputs: test_gpu_generic.build (near targets, reachable), B = 130 = two full waves + a tail of two, not a multiple of the
cooperative form's four problems per workgroup."""
import ctypes as C
import os

import numpy as np

import oracle as O
from test_gpu_generic import build

B = 130
DETERMINED = 1e-9     # max|q_d - q_q| of a lane the reference itself determines
BAR = 1e-8            # rad, every determined lane of every form against q_q
MAX_UNDETERMINED = 2  # of B lanes, per case and parameter set (0 for the one-iteration sets)

_POS, _ORI, _FULL = 0, 1, 2
_FOOT_W = lambda w: [1.0, 1.0, 1.0, 1.0, w, 1.0]
_TREE = lambda w: ("cassie", True, [("frame", "LeftFootFront", "universe", _FULL, 0, _FOOT_W(w)), ("frame", "pelvis", "universe", _FULL, 0, None),
                                    ("align", "LeftFootFront", "universe", 1, 1, None)])
_TREE_POS = lambda w: ("cassie", True, [("frame", "LeftFootFront", "universe", _POS, 0, [1.0, 1.0, w]), ("frame", "pelvis", "universe", _FULL, 0, None),
                                        ("align", "LeftFootFront", "universe", 1, 1, None)])
_POS_W = lambda w: ("ur5", False, [("frame", "tool0", "universe", _POS, 0, [1.0, 1.0, w]), ("frame", "tool0", "universe", _ORI, 1, None)])

# case -> (model, free-flyer, specs as test_gpu_generic.build takes them: (kind, frame, reference, type-or-axis, priority, weights))
CASES = {
    "pos_w1e-12_then_ori": _POS_W(1e-12),     # row kept: a factor 1e3 above the threshold
    "pos_w1e-19_then_ori": _POS_W(1e-19),     # row dropped: a factor 1e4 below
    "pos_w0_then_ori": _POS_W(0.0),           # exact zero row (Eigen: "the rest is zero"); the answer of the 1e-19 case
    "forearm_full_then_tool_pos": ("ur5", False, [("frame", "forearm_link", "universe", _FULL, 0, None),      # 6 rows on 3 joints: rank 3
                                                  ("frame", "tool0", "universe", _POS, 1, None)]),
    "pos_then_full": ("ur5", False, [("frame", "tool0", "universe", _POS, 0, None), ("frame", "tool0", "universe", _FULL, 1, None)]),   # projected rank 3 of 6
    "leg_full_then_other_foot": ("cassie_fixed", False, [("frame", "LeftFootFront", "universe", _FULL, 0, None),   # rank 5 of 6
                                                         ("frame", "RightFootFront", "universe", _FULL, 1, None)]),
    "align_w1e-12_between": ("ur5", False, [("frame", "tool0", "universe", _POS, 0, None), ("align", "tool0", "universe", 1, 1, [1e-12]),
                                            ("frame", "tool0", "universe", _ORI, 2, None)]),
    "empty_middle_level": ("ur5", False, [("frame", "tool0", "universe", _POS, 0, None), ("frame", "tool0", "universe", _ORI, 2, None)]),
    "all_zero_level": ("ur5", False, [("frame", "tool0", "universe", _POS, 0, [0.0, 0.0, 0.0]), ("frame", "tool0", "universe", _ORI, 1, None)]),
    "tree_foot_w1e-12": _TREE(1e-12),
    "tree_foot_w1e-19": _TREE(1e-19),
    # The two above decide nothing observable: the foot's Full task already fixes the foot's orientation, so the alignment row
    # projects to rounding noise (|a P| = 2e-15 of |a| = 1.7, at any weighting) and level 1 is a no-op -- the _Float128 answers of the
    # two are the same bits.  With the foot's POSITION at level 0 the alignment keeps four directions, and dropping the third row
    # moves the _Float128 answer by 1e-3 rad at least and 0.5 rad in the median (against the same row kept at 1e-12).  Only the
    # dropped side can be held to the bar: the double reference itself is off by 5e-17 / w there (median 4.5e-5 rad at w = 1e-12,
    # 5.6e-11 at 1e-6), so every weight below ~1e-6 that is kept leaves the case undetermined.
    "tree_pos_w1e-19": _TREE_POS(1e-19),    # row dropped by `n2 > thr2`
    "tree_pos_w0": _TREE_POS(0.0),          # row skipped by `w6[r] == 0`; the answer of the case above
    "full_rank_control": ("ur5", False, [("frame", "tool0", "universe", _POS, 0, None), ("frame", "tool0", "universe", _ORI, 1, None)]),
}
TREE_CASES = ("tree_foot_w1e-12", "tree_foot_w1e-19", "tree_pos_w1e-19", "tree_pos_w0")
# Cases whose LAST projector the reference itself does not determine, so that they run without the secondary step `P da` (the one
# reader of that projector) on every form -- the tree build takes no da anyway.  Measured on the two oracles, seed 3 (4 and 5 alike):
#   * tree_foot_*: the alignment row of a frame whose whole pose is a level-0 task projects to rounding noise, and a one-row level always
#     counts rank 1 (its only pivot is the largest): with da all 130 lanes differ between double and _Float128, median 4e-3 rad,
#     at ANY weighting of the foot rows, unit included.  Without da the two agree to 1.2e-13 on every lane.
#   * align_w1e-12_between: the last level puts three orientation rows on the two directions left; its third pivot is noise of a
#     few eps against a threshold of 3 eps: with da 41 / 80 / 96 lanes (1 / 6 / 30 iterations) differ by up to 0.26 rad, at an
#     alignment weight of 1e-12, 1e-3 or 1 alike, 21 to 43 lanes at seeds 3, 4, 5.  Without da: 5.6e-13 on every lane.
WITHOUT_DA = ("tree_foot_w1e-12", "tree_foot_w1e-19", "align_w1e-12_between")
SEEDS = {}            # case -> seed where the committed one (3) leaves a lane out; none needed
DEFAULT_SEED = 3


class Inputs:
    def __init__(self, case):
        name, ff, specs = CASES[case]
        self.case, self.free_flyer = case, ff
        (self.ik_amd, _, self.model, self.problem, _, self.om, self.ot, self.q0, self.tg) = build(
            name, ff, specs, B, seed=SEEDS.get(case, DEFAULT_SEED), device=False)
        self.levels = self.problem.max_priority_level() + 1
        self.nv = self.model.nv
        self.da = 0.01 * np.cos(np.arange(self.nv))
        self._refs = {}

    # ---- what the emulator's entry points take -------------------------------------------------------------------------------------
    def urdf(self):
        from conftest import urdf_path
        return open(urdf_path(CASES[self.case][0]), "rb").read()

    def capi_tasks(self):
        from ik_amd import capi
        tasks = (capi.Task * len(self.ot))()
        for i, t in enumerate(self.ot):
            tasks[i] = capi.Task(t.frame, t.reference, t.type, t.priority, (C.c_double * 6)(*t.weight))
        return tasks

    # ---- parameter sets: (iters, step, tol, lambda per level, da) --------------------------------------------------------------------
    def param_sets(self, tree=False):
        """tree: what the tree build takes -- no secondary step (da != 0 moves the call to pik_generic)."""
        n = self.levels
        sets = [(1, 1.0, -1.0, [0.1] * n, self.da), (6, 1.0, -1.0, [0.1] * n, self.da), (6, 1.0, -1.0, [0.1] * n, None),
                (30, 0.5, 1e-8, [0.05, 0.1, 0.2][:n], self.da)]
        if tree or self.case in WITHOUT_DA:   # the da = None set, and the other two with da dropped
            sets = [(it, st, tol, lam, None) for it, st, tol, lam, da in sets if not (it == 6 and da is not None)]
        return sets

    def lambda0_sets(self):
        """lambda = 0 on a level: the per-lane one-sided-Jacobi interpreter's own regime.  One iteration (over six undamped ones the
        reference is chaotic: its two precisions end 13 rad apart)."""
        assert self.levels == 2
        return [(1, 1.0, -1.0, lam, da) for lam in ([0.0, 0.0], [0.0, 0.1]) for da in (self.da, None)]

    # ---- the reference --------------------------------------------------------------------------------------------------------------
    def reference(self, prm_set):
        iters, step, tol, lam, da = prm_set
        key = (iters, step, tol, tuple(lam), da is not None)
        if key not in self._refs:
            threads = min(16, os.cpu_count() or 1)
            mk = lambda: O.pik_params(iters, step, tol, list(lam), None if da is None else list(da))
            q_d, ok_d, it_d = O.pik_batch(self.om, self.ot, self.tg, self.q0, mk(), threads)
            q_q, _, _ = O.pik_batch(self.om, self.ot, self.tg, self.q0, mk(), threads, ext="q")
            determined = np.abs(q_d - q_q).max(axis=1) <= DETERMINED
            left_out = int(B - determined.sum())
            assert left_out <= (0 if iters == 1 else MAX_UNDETERMINED), (self.case, key, left_out)
            for a in (q_d, ok_d, it_d, q_q, determined):
                a.setflags(write=False)
            self._refs[key] = (q_d, ok_d, it_d, q_q, determined)
        return self._refs[key]

    def check(self, form, prm_set, q, ok, it):
        """Holds one form's result to the acceptance rule; returns (max|q - q_q| over determined lanes, lanes left out)."""
        q_d, ok_d, it_d, q_q, det = self.reference(prm_set)
        q, ok, it = np.asarray(q), np.asarray(ok), np.asarray(it)
        assert q.shape == q_q.shape
        err = np.abs(q - q_q).max(axis=1)
        worst = float(err[det].max())
        tag = (form, self.case, prm_set[0], prm_set[3], prm_set[4] is not None)
        print("pik_rank %-22s %-28s iters=%-2d lambda=%s da=%d  max|q-q_q|=%.3e  oracle_d=%.3e  left_out=%d"
              % (form, self.case, prm_set[0], prm_set[3], prm_set[4] is not None, worst, float(np.abs(q_d - q_q).max(axis=1)[det].max()),
                 int(B - det.sum())))
        assert np.isfinite(q[det]).all(), tag
        assert worst <= BAR, tag + (worst, int((err[det] > BAR).sum()))
        assert np.array_equal(ok[det].astype(bool), ok_d[det].astype(bool)) and np.array_equal(it[det], it_d[det]), tag
        return worst, int(B - det.sum())


_INPUTS = {}


def inputs(case):
    if case not in _INPUTS:
        _INPUTS[case] = Inputs(case)
    return _INPUTS[case]


def same_answer(form, prm_set, case_a, qa, case_b, qb):
    """pos_w0_then_ori and pos_w1e-19_then_ori: an exact zero row and a row below the threshold leave the same answer, to the bar,
    on the lanes both references determine."""
    det = inputs(case_a).reference(prm_set)[4] & inputs(case_b).reference(prm_set)[4]
    d = float(np.abs(np.asarray(qa) - np.asarray(qb)).max(axis=1)[det].max())
    assert d <= BAR, (form, case_a, case_b, prm_set[0], d)
    return d
