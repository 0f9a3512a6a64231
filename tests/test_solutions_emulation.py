"""The pieces of the solution-set kernels (device/solutions.hpp: solutions_offer, solutions_take; dls_chain_solutions_lane and
solutions_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_solutions_lane in device/chain_hot.hpp), compiled for the host by this
test (tests/lane_emu/solutions_emu.cpp) and run with the K lanes of a group step by step.

ikgpu_dls_solutions_batch is DEFINED through K single solves (include/ikgpu.h), so "right" is: count and which equal the greedy rule
restated in numpy (tests/solutions_common.py) over what the single-solve lane program (tests/lane_emu/lane_emu.cpp) returns from the K
starts; every written slab is np.array_equal to the single solve from which[n][b] over all nq entries; unwritten slots keep their
prefill.  The workload must put the rule to work: the conditions of test_the_workload_exercises_the_rule are asserted, not assumed."""
import ctypes as C

import numpy as np
import pytest

import solutions_common as SC
from test_multistart_emulation import B, PROGRAMS, _compile, _p, emu_mask, emu_starts, setup, single_solves

MODELS = [("ur5", "tool0", 0.1), ("cassie_fixed", "LeftFootFront", 0.5)]
SEED = 3


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/multistart.hpp",
             "device/solutions.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    single = _compile("lane_emu.cpp", "liblane_emu.so", chain + ("device/tree_solver.hpp", "device/tree_kernel_body.hpp", "device/generic_solver.hpp",
                                                                 "device/pik_solver.hpp", "device/coop_solver.hpp", "device/pik_coop.hpp", "generic_tables.hpp"))
    multi = _compile("multistart_emu.cpp", "libmultistart_emu.so", chain)
    sol = _compile("solutions_emu.cpp", "libsolutions_emu.so", chain)
    single.lane_emu_last_error.restype = C.c_char_p
    multi.multistart_emu_last_error.restype = C.c_char_p
    sol.solutions_emu_last_error.restype = C.c_char_p
    return single, multi, sol


def solutions(sol, urdf, task, q0, starts, tg, prm, K, N, sep, layout, optional=True):
    """One call of the solution-set lane programs.  q0 [B, nq], starts None or [K-1, B, nq], tg [B, 1, 12]; AoS views back."""
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
    ti = np.ascontiguousarray(tg.reshape(B, 12) if layout == 1 else tg.reshape(B, 12).T)
    qo = np.full((N,) + qi.shape, SC.NAN_FILL)
    count = np.full(B, SC.INT_FILL, np.int32)
    which, it = (np.full((N, B), SC.INT_FILL, np.int32), np.full((N, B), SC.INT_FILL, np.int32)) if optional else (None, None)
    rc = sol.solutions_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(B), K, N, _p(qi), _p(si), C.c_uint64(SEED), _p(ti), C.byref(prm),
                               C.c_double(sep), _p(qo), _p(count), _p(which), _p(it), layout)
    assert rc == 0, sol.solutions_emu_last_error()
    return (qo if layout == 1 else np.ascontiguousarray(qo.transpose(0, 2, 1))), count, which, it


def _singles(emus, name, frame, K):
    from ik_amd import capi
    single, multi, sol = emus
    urdf, model, om, task, ot, q0, tg = setup(name, frame)
    gen = emu_starts(multi, urdf, task, q0, K, SEED)                 # [K-1, B, nq]
    prm = capi.DlsParams(100, 1e-2, 1.0, 1e-4)
    _, support = emu_mask(multi, urdf, C.byref(task), 1, model.nq)
    return urdf, model, task, q0, tg, gen, prm, support


def test_the_workload_exercises_the_rule(emus, monkeypatch):
    """On the general program: the conditions without which the tests below could pass vacuously."""
    for k in ("LANE_EMU_TRIG", "LANE_EMU_HOT"):
        monkeypatch.delenv(k, raising=False)
    single = emus[0]
    K = 8
    urdf, model, task, q0, tg, gen, prm, support = _singles(emus, "ur5", "tool0", K)
    singles = single_solves(single, urdf, task, np.concatenate([q0[None], gen]), tg, prm)
    count, which, dropped = SC.greedy(singles, support, 0.1, K)
    print("ur5 K=8 sep=0.1: problems by count %s, mean %.2f, most %d, near-duplicates dropped %d"
          % (np.bincount(count, minlength=K + 1).tolist(), count.mean(), count.max(), int(dropped.sum())))
    assert (count == 1).any() and (count >= 3).any()
    count3, _, _ = SC.greedy(singles, support, 0.1, 3)
    assert ((count > 3) & (count3 == 3)).any()                       # N = 3 truncates some problem's set
    urdf, model, task, q0, tg, gen, prm, support = _singles(emus, "cassie_fixed", "LeftFootFront", K)
    assert not support.all()                                         # the leg's chain leaves entries of q outside the support
    singles = single_solves(single, urdf, task, np.concatenate([q0[None], gen]), tg, prm)
    count, which, dropped = SC.greedy(singles, support, 0.5, K)
    print("cassie_fixed K=8 sep=0.5: problems by count %s, %d problems with a near-duplicate dropped" % (np.bincount(count, minlength=K + 1).tolist(), int((dropped > 0).sum())))
    assert (dropped > 0).sum() >= B / 4


@pytest.mark.parametrize("name,frame,sep", MODELS)
@pytest.mark.parametrize("program", sorted(PROGRAMS))
@pytest.mark.parametrize("K", [2, 8])
def test_solutions_program_returns_the_greedy_set_of_single_solves(emus, monkeypatch, name, frame, sep, program, K):
    single, multi, sol = emus
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    urdf, model, task, q0, tg, gen, prm, support = _singles(emus, name, frame, K)
    singles = single_solves(single, urdf, task, np.concatenate([q0[None], gen]), tg, prm)
    n_ok = np.stack([s[1] for s in singles]).astype(bool).sum(axis=0)        # converged starts per problem
    for N in sorted({1, min(3, K), K}):
        got = solutions(sol, urdf, task, q0, None, tg, prm, K, N, sep, 1)
        count, which = SC.check_set(got, singles, support, sep, N, (name, program, K, N))
        assert count.max() == N or N == K
        # the caller's starts instead of generated ones, the other layout: the same bits (NaN prefill included)
        for starts, layout in ((gen, 1), (None, 0), (gen, 0)):
            again = solutions(sol, urdf, task, q0, starts, tg, prm, K, N, sep, layout)
            for x, y in zip(again, got):
                assert np.array_equal(x, y, equal_nan=True), (name, program, K, N, layout, starts is None)
        # without which / iters
        bare = solutions(sol, urdf, task, q0, None, tg, prm, K, N, sep, 0, optional=False)
        assert bare[2] is None and bare[3] is None
        assert np.array_equal(bare[0], got[0], equal_nan=True) and np.array_equal(bare[1], got[1])
        # sep = 0 keeps every converged start, up to N
        all_of = solutions(sol, urdf, task, q0, None, tg, prm, K, N, 0.0, 1)
        SC.check_set(all_of, singles, support, 0.0, N, (name, program, K, N, "sep = 0"))
        assert np.array_equal(all_of[1], np.minimum(n_ok, N))
    # caller's starts whose entries OUTSIDE the support differ from q0's: a kept start's own column is what a single solve clips
    if name == "cassie_fixed":
        hi = np.asarray(model.upperPositionLimit)
        mine = gen.copy()
        mine[:, :, -1] = hi[-1] + 1.0 + np.arange(K - 1)[:, None]    # (the last entry lies outside the left leg's chain)
        assert not support[-1]
        own = single_solves(single, urdf, task, np.concatenate([q0[None], mine]), tg, prm)
        got = solutions(sol, urdf, task, q0, mine, tg, prm, K, K, sep, 1)
        count, which = SC.check_set(got, own, support, sep, K, (name, program, K, "own columns"))
        later = which > 0                                             # [N, B]: slots filled from one of the caller's starts
        assert later.any() and (got[0][..., -1][later] == hi[-1]).all()
