"""hot_evaluate and one DLS step of the hot chain program with its sin / cos from the table (ik_amd/csrc/device/lane_math.hpp
dsincos_lut; device/chain_hot.hpp hot_evaluate, which a plain HotTable sends to the header's array), on the host against the oracle.

The lane program is tests/hot_eval/hot_fold_shim.cpp as it stands, compiled here into a shared object of this file's own.  Chains: the
ones of tests/hot_fold_common.py, which include the Cassie leg and UR5.  Bars, the ones tests/test_hot_fold_host.py holds the same
quantities to: 1e-11 on every entry of e and J and 1e-9 rad on the step, with that file's allowance towards a rotation by pi
(hot_fold_common.conditioned, by the oracle's own angle), 1e-6 inside the theta -> pi band.

Configurations: uniform in the limits (64), every run's members on their limits in the four patterns of hot_fold_common.run_rows (the
largest sums of a folded run), and the same uniform draws with every chain joint moved by a whole number of turns -- 1, -1, 8 and -8
times 2 pi as the nearest doubles -- which walks the table index through its wrap at negative multiples while e and J stay what they
were up to the rounding of the shifted angle: the oracle is evaluated at the shifted q itself, and the bar grows by the reduction
term only, NJ joints x 4e-17 |x| x (1 rad/rad + REACH m/rad).  The step is compared from the unshifted rows alone (a start outside
the limits is clipped back in one step, which would hide the evaluation).

The invariant of hot_gram / hot_step: every member of a run of parallel joints carries the same bits in col[j][3..5]."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hot_fold_common as HF
import oracle as O

BAR, BAR_NEAR_PI = 1e-11, 1e-6
STEP_BAR, STEP_BAR_NEAR_PI = 1e-9, 1e-6
REDUCTION, REACH = 4e-17, 2.0
TURNS = (1, -1, 8, -8)


@pytest.fixture(scope="module")
def shim(native_built):
    src = os.path.join(ROOT, "tests", "hot_eval", "hot_fold_shim.cpp")
    out = os.path.join(ROOT, "tests", "hot_eval", "libhot_lut_evaluate_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp",
                                                    "device/sincos_lut_table.hpp", "device/chain_solver.hpp", "device/chain_kernel_body.hpp",
                                                    "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.hot_fold_last_error.restype = C.c_char_p
    return L


@pytest.fixture(scope="module", params=HF.CHAINS, ids=[c.name for c in HF.CHAINS])
def evaluated(request, shim):
    """Every configuration of one chain through the shim in ONE call, and the oracle's e, J and first iterate for them, computed once."""
    import ik_amd
    from ik_amd import capi
    c = request.param
    urdf = HF.chain_xml(c).encode()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(c.frame)
    flat = model.flat()
    qidx, j = [], int(flat["frame_parent"][fid])
    while j > 0:
        qidx.insert(0, int(flat["idx_q"][j]))
        j = int(flat["parent"][j])
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(1024)
    base = rng.uniform(lo, hi, (64, lo.size))
    tg_base = O.fk_batch(om, rng.uniform(lo, hi, (64, lo.size)), [fid])
    groups = [("uniform", base, tg_base, np.zeros(64))]
    rows = HF.run_rows(c, lo, hi, qidx, base)
    if len(rows):
        groups.append(("run_sums", rows, tg_base[:len(rows)], np.zeros(len(rows))))
    shifted = base.copy()
    shift = np.empty(64)
    for b in range(64):
        shift[b] = TURNS[b % 4] * 2.0 * np.pi
        shifted[b, qidx] += shift[b]
    groups.append(("whole_turns", shifted, tg_base, shift))
    q = np.ascontiguousarray(np.concatenate([g[1] for g in groups]))
    tg = np.ascontiguousarray(np.concatenate([g[2] for g in groups]))
    moved = np.concatenate([g[3] for g in groups])
    n, nv = q.shape[0], model.nv
    e, J, q1 = np.empty((n, 6)), np.empty((n, 6, nv)), np.empty_like(q)
    leader, folded, nj = (C.c_int * 8)(), (C.c_int * 8)(), C.c_int(0)
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    p = lambda a: C.c_void_p(a.ctypes.data)
    colbuf = np.empty(n * 7 * 6)
    rc = shim.hot_fold_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), p(q), p(tg), C.c_int(1), C.c_double(1e-4), p(e), p(J), p(colbuf),
                           p(q1), leader, folded, C.byref(nj))
    assert rc == 0, shim.hot_fold_last_error()
    col = colbuf[:n * nj.value * 6].reshape(n, nj.value, 6)
    ot = O.make_tasks([(fid, 0, 2, 0, None)])
    eo, Jo = np.empty_like(e), np.empty_like(J)
    for b in range(n):
        eo[b], Jo[b] = O.evaluate(om, ot, tg[b], q[b])
    q1o, _, _ = O.dls_batch(om, ot, tg, q, O.params(1, 1e-2, 1.0, -1.0))
    span, at = {}, 0
    for g in groups:
        span[g[0]] = slice(at, at + g[1].shape[0])
        at += g[1].shape[0]
    # what the one-word reduction may add to an entry of e or J: per joint 4e-17 (|shift| + the angle itself), rotation and translation
    extra = nj.value * REDUCTION * (np.abs(moved) + 2.0 * np.pi) * (1.0 + REACH) * (moved != 0.0)
    return dict(chain=c, e=e, J=J, col=col, eo=eo, Jo=Jo, q1=q1, q1o=q1o, span=span, qidx=qidx, extra=extra,
                leader=list(leader)[:nj.value], theta=np.linalg.norm(eo[:, 3:], axis=1))


@pytest.mark.parametrize("group", ["uniform", "run_sums", "whole_turns"])
def test_error_and_jacobian_match_the_oracle(evaluated, group):
    if group not in evaluated["span"]:
        assert not HF.runs(evaluated["chain"])
        return
    s = evaluated["span"][group]
    de, dJ = np.abs(evaluated["e"][s] - evaluated["eo"][s]).max(axis=1), np.abs(evaluated["J"][s] - evaluated["Jo"][s]).max(axis=(1, 2))
    bars = HF.conditioned(evaluated["theta"][s], BAR + evaluated["extra"][s], BAR_NEAR_PI)
    print("%s %s: max |de| %.2e, max |dJ| %.2e over %d configurations, worst share of the bar %.3f (bars up to %.1e)"
          % (evaluated["chain"].name, group, de.max(), dJ.max(), s.stop - s.start, (np.maximum(de, dJ) / bars).max(), bars.max()))
    assert np.isfinite(evaluated["e"][s]).all() and np.isfinite(evaluated["J"][s]).all()
    assert (de < bars).all() and (dJ < bars).all(), (int(np.argmax(np.maximum(de, dJ) / bars)), de.max(), dJ.max())


def test_parallel_joints_share_their_angular_rows_bitwise(evaluated):
    leader, col = evaluated["leader"], evaluated["col"]
    assert leader == evaluated["chain"].leader
    for j, L in enumerate(leader):
        if L != j:
            assert np.array_equal(col[:, j, 3:].view(np.uint64), col[:, L, 3:].view(np.uint64)), (j, L)


def test_one_step_of_the_lane_program_matches_the_oracle(evaluated):
    qidx = evaluated["qidx"]
    for group in ("uniform", "run_sums"):
        if group not in evaluated["span"]:
            continue
        s = evaluated["span"][group]
        d = np.abs(evaluated["q1"][s] - evaluated["q1o"][s])[:, qidx].max(axis=1)
        bars = HF.conditioned(evaluated["theta"][s], STEP_BAR, STEP_BAR_NEAR_PI)
        print("%s %s one step: max |dq| vs oracle %.2e, worst share of the bar %.3e" % (evaluated["chain"].name, group, d.max(), (d / bars).max()))
        assert np.isfinite(evaluated["q1"][s]).all()
        assert (d <= bars).all(), (group, int(np.argmax(d / bars)), d.max())
