"""The pieces of the multi-start kernels (device/multistart.hpp: the draw, the key, the selection; dls_chain_multistart_lane and
multistart_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_multistart_lane in device/chain_hot.hpp), compiled for the host by
this test (tests/lane_emu/multistart_emu.cpp) and run lane after lane.

ikgpu_dls_multistart_batch is DEFINED through K single solves (include/ikgpu.h), so "right" is: q / success / iterations equal, by
np.array_equal, what the single-solve lane program (tests/lane_emu/lane_emu.cpp) returns from start winner[b]; the winner has the
minimal key over the K single solves (exact in the success class and in the index among successes; among failures to 1e-10 in the error
norm, errors from the oracle); and |sqrt(err_sq) - ||e_oracle||| <= 5e-11 -- sqrt(6) x twice the 1e-11 by which the stage tests bound a
lane program's error against the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, urdf_path

import oracle as O
import multistart_common as MC

B = 130


def _compile(src_name, out_name, deps):
    src = os.path.join(ROOT, "tests", "lane_emu", src_name)
    out = os.path.join(ROOT, "tests", "lane_emu", out_name)
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in deps]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def emus(native_built):
    chain = ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp", "device/multistart.hpp",
             "device/chain_kernel_body.hpp", "device/chain_hot.hpp")
    single = _compile("lane_emu.cpp", "liblane_emu.so", chain + ("device/tree_solver.hpp", "device/tree_kernel_body.hpp", "device/generic_solver.hpp",
                                                                 "device/pik_solver.hpp", "device/coop_solver.hpp", "device/pik_coop.hpp", "generic_tables.hpp"))
    multi = _compile("multistart_emu.cpp", "libmultistart_emu.so", chain)
    single.lane_emu_last_error.restype = C.c_char_p
    multi.multistart_emu_last_error.restype = C.c_char_p
    multi.multistart_emu_uniform.restype = C.c_double
    multi.multistart_emu_uniform.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int]
    return single, multi


_p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None


def setup(name, frame, seed=0):
    import ik_amd
    from ik_amd import capi
    urdf = open(urdf_path(name), "rb").read()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    q0, qt = MC.uniform_configurations(model, B, seed)
    tg = O.fk_batch(om, qt, [fid])                                   # [B, 1, 12]
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    ot = O.make_tasks([(fid, 0, 2, 0, None)])
    return urdf, model, om, task, ot, q0, tg


def emu_starts(multi, urdf, task, q0, K, seed, layout=1, free_flyer=0, ntasks=1):
    """ikgpu_multistart_starts on the emulator's copy of the draw.  q0 [B, nq]; returns [K-1, B, nq] whatever the layout it ran in."""
    n, nq = q0.shape
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    out = np.full((K - 1,) + qi.shape, np.nan)
    rc = multi.multistart_emu_starts(urdf, C.c_size_t(len(urdf)), free_flyer, C.byref(task) if ntasks == 1 else task, ntasks, C.c_int64(n), K, _p(qi),
                                     C.c_uint64(seed), _p(out), layout)
    assert rc == 0, multi.multistart_emu_last_error()
    return out if layout == 1 else np.ascontiguousarray(out.transpose(0, 2, 1))


def emu_mask(multi, urdf, tasks, ntasks, nq, free_flyer=0):
    draw, sup = np.zeros(nq, np.uint8), np.zeros(nq, np.uint8)
    rc = multi.multistart_emu_mask(urdf, C.c_size_t(len(urdf)), free_flyer, tasks, ntasks, _p(draw), _p(sup))
    assert rc == 0, multi.multistart_emu_last_error()
    return draw.astype(bool), sup.astype(bool)


@pytest.mark.parametrize("name,frame", [("cassie_fixed", "LeftFootFront"), ("ur5", "tool0"), ("arm7", "tool")])
def test_generated_starts_follow_the_formula(emus, name, frame):
    single, multi = emus
    urdf, model, om, task, ot, q0, tg = setup(name, frame)
    lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
    nq = model.nq
    draw, sup = emu_mask(multi, urdf, C.byref(task), 1, nq)
    assert draw.any() and not (draw & ~sup).any()           # only entries of the support are drawn
    assert np.array_equal(draw, sup & np.isfinite(lo) & np.isfinite(hi) & (lo < hi))   # (every joint of these models is revolute)
    seed, K = 12345, 8
    st = emu_starts(multi, urdf, task, q0[:5], K, seed)                                  # [K-1, 5, nq]
    # the formula, restated in Python
    for k in range(1, K):
        for b in range(5):
            for i in range(nq):
                if draw[i]:
                    want = MC.draw(seed, b, k, i, float(lo[i]), float(hi[i]))
                    assert abs(st[k - 1, b, i] - want) <= 2 * np.spacing(max(abs(want), abs(st[k - 1, b, i]))), (k, b, i)
                    assert multi.multistart_emu_uniform(seed, b, k, i) == MC.uniform(seed, b, k, i)
    assert (st[:, :, draw] >= lo[draw]).all() and (st[:, :, draw] <= hi[draw]).all()
    # entries that are not drawn are q0's, bit for bit
    assert np.array_equal(st[:, :, ~draw].view(np.uint64), np.broadcast_to(q0[:5][:, ~draw], (K - 1, 5, int((~draw).sum()))).copy().view(np.uint64))
    # a function of (seed, b, k, i) only: not of B, K or the layout
    big = np.tile(q0, (4097 // B + 1, 1))[:4097]
    big[:5] = q0[:5]
    assert np.array_equal(emu_starts(multi, urdf, task, big, K, seed)[:, :5][:, :, draw], st[:, :, draw])
    assert np.array_equal(emu_starts(multi, urdf, task, q0[:5], 2, seed)[0], st[0])
    assert np.array_equal(emu_starts(multi, urdf, task, q0[:5], K, seed, layout=0), st)
    other = emu_starts(multi, urdf, task, q0[:5], K, seed + 1)
    assert not (other[:, :, draw] == st[:, :, draw]).any()
    # sanity of the generator: the mean of u over 4096 problems x the chain's joints (more than 10 sigma wide)
    idx = np.flatnonzero(draw)
    u = np.array([[multi.multistart_emu_uniform(seed, b, 1, int(i)) for i in idx] for b in range(4096)])
    assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.02, u.mean()


def test_a_free_flyer_and_the_joints_outside_the_support_are_never_drawn(emus):
    import ik_amd
    from ik_amd import capi
    single, multi = emus
    urdf = open(urdf_path("cassie"), "rb").read()
    tasks = (capi.Task * 2)()
    flat_fixed = ik_amd.Model.from_urdf_xml(open(urdf_path("cassie_fixed"), "rb").read())
    nq = flat_fixed.nq + 7
    # frame ids of the free-flyer model: looked up through the C ABI
    L = capi.lib()
    h = C.c_void_p()
    capi.check(L.ikgpu_model_from_urdf(urdf, C.c_size_t(len(urdf)), 1, C.byref(h)))
    try:
        for t, frame in zip(tasks, (b"LeftFootFront", b"pelvis")):
            t.frame, t.reference, t.type, t.priority = L.ikgpu_model_frame_id(h, frame), 0, 2, 0
            for k in range(6):
                t.weight[k] = 1.0
    finally:
        L.ikgpu_model_destroy(h)
    draw, sup = emu_mask(multi, urdf, tasks, 2, nq, free_flyer=1)
    assert sup[:7].all() and not draw[:7].any()             # the free-flyer's seven entries: in the support, never drawn
    assert draw[7:].any() and not (draw & ~sup).any() and not draw[7:][~sup[7:]].any()
    q0 = np.zeros((3, nq))
    q0[:, 6] = 1.0
    q0[:, 7:] = 0.123
    st = emu_starts(multi, urdf, tasks, q0, 4, 7, free_flyer=1, ntasks=2)
    assert np.array_equal(st[:, :, ~draw], np.broadcast_to(q0[:, ~draw], (3, 3, int((~draw).sum())))) and (st[:, :, draw] != 0.123).all()


def single_solves(single, urdf, task, starts_all, tg, prm):
    """The single-solve lane program from each of the K starts.  starts_all [K, B, nq] -> K tuples (q [B, nq], success, iters)."""
    res = []
    for qs in starts_all:
        qi = np.ascontiguousarray(qs)
        qo, ok, it = np.empty_like(qi), np.zeros(B, np.uint8), np.zeros(B, np.int32)
        rc = single.lane_emu_run(urdf, C.c_size_t(len(urdf)), 0, C.byref(task), 1, 0, C.c_int64(B), _p(qi), _p(np.ascontiguousarray(tg)), C.byref(prm),
                                 _p(qo), _p(ok), _p(it), None, None, None, 1)
        assert rc == 0, single.lane_emu_last_error()
        res.append((qo, ok, it))
    return res


def multistart(multi, urdf, task, q0, starts, seed, tg, prm, K, layout, optional=True):
    """One call of the multi-start lane programs.  q0 [B, nq], starts None or [K-1, B, nq], tg [B, 1, 12]; AoS views back."""
    nq = q0.shape[1]
    qi = np.ascontiguousarray(q0 if layout == 1 else q0.T)
    si = None if starts is None else np.ascontiguousarray(starts if layout == 1 else starts.transpose(0, 2, 1))
    ti = np.ascontiguousarray(tg.reshape(B, 12) if layout == 1 else tg.reshape(B, 12).T)
    qo = np.full(qi.shape, np.nan)
    ok, it, win, err = (np.full(B, 7, np.uint8), np.full(B, -7, np.int32), np.full(B, -7, np.int32), np.full(B, np.nan)) if optional else (None,) * 4
    rc = multi.multistart_emu_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(B), K, _p(qi), _p(si), C.c_uint64(seed), _p(ti), C.byref(prm),
                                  _p(qo), _p(ok), _p(it), _p(win), _p(err), layout)
    assert rc == 0, multi.multistart_emu_last_error()
    return (qo if layout == 1 else np.ascontiguousarray(qo.T)), ok, it, win, err


PROGRAMS = {"general": {}, "device_general": {"LANE_EMU_TRIG": "0"}, "hot": {"LANE_EMU_HOT": "1"}}
_oracle_cache = {}


@pytest.mark.parametrize("name,frame", [("cassie_fixed", "LeftFootFront"), ("ur5", "tool0")])
@pytest.mark.parametrize("program", sorted(PROGRAMS))
@pytest.mark.parametrize("K", [2, 8])
def test_multistart_program_returns_the_best_single_solve(emus, monkeypatch, name, frame, program, K):
    from ik_amd import capi
    single, multi = emus
    urdf, model, om, task, ot, q0, tg = setup(name, frame)
    for k, v in PROGRAMS[program].items():
        monkeypatch.setenv(k, v)
    seed = 3
    gen = emu_starts(multi, urdf, task, q0, K, seed)                 # [K-1, B, nq]
    starts_all = np.concatenate([q0[None], gen])
    norm = lambda q: np.array([np.linalg.norm(O.evaluate(om, ot, tg[b], q[b])[0]) for b in range(B)])
    for max_it, tol in ((100, 1e-4), (5, -1.0)):
        prm = capi.DlsParams(max_it, 1e-2, 1.0, tol)
        singles = single_solves(single, urdf, task, starts_all, tg, prm)
        errs = [norm(s[0]) ** 2 for s in singles]
        got = multistart(multi, urdf, task, q0, None, seed, tg, prm, K, 1)
        worst = MC.check_selection(got, singles, errs, norm(got[0]), (name, program, K, max_it))
        n_ok = [int(s[1].sum()) for s in singles]
        print("%s %s K=%d %s: converged %s of %d per start, %d with the best of %d; max |sqrt(err_sq) - ||e_oracle||| = %.3g"
              % (name, program, K, (max_it, tol), n_ok, B, int(got[1].sum()), K, worst))
        if tol > 0:
            assert 0 < n_ok[0] < B and got[1].sum() >= n_ok[0]        # both classes are present, and more starts never lose one
            assert (got[3] > 0).any() and (got[3] == 0).any()
        else:
            assert not got[1].any() and len(np.unique(got[3])) == K   # never-stop: the arg-min of the error, every start wins somewhere
        # the caller's starts instead of generated ones, the other layout, and without the optional arrays: the same bits
        for starts, layout in ((gen, 1), (None, 0), (gen, 0)):
            again = multistart(multi, urdf, task, q0, starts, seed, tg, prm, K, layout)
            for x, y in zip(again, got):
                assert np.array_equal(x, y), (name, program, K, max_it, layout, starts is None)
        q_only = multistart(multi, urdf, task, q0, None, seed, tg, prm, K, 0, optional=False)
        assert all(x is None for x in q_only[1:]) and np.array_equal(q_only[0], got[0])
    # caller's starts whose entries OUTSIDE the support differ from q0's: the winner's own column is what a single solve clips
    if name == "cassie_fixed":
        lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
        mine = gen.copy()
        mine[:, :, -1] = hi[-1] + 1.0 + np.arange(K - 1)[:, None]    # (the last entry lies outside the left leg's chain)
        prm = capi.DlsParams(100, 1e-2, 1.0, 1e-4)
        singles = single_solves(single, urdf, task, np.concatenate([q0[None], mine]), tg, prm)
        got = multistart(multi, urdf, task, q0, mine, seed, tg, prm, K, 1)
        MC.check_selection(got, singles, [norm(s[0]) ** 2 for s in singles], norm(got[0]), (name, program, K, "own columns"))
        assert (got[0][got[3] > 0, -1] == hi[-1]).all() and (got[3] > 0).any()
