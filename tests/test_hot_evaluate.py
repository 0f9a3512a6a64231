"""hot_evaluate of the structure-specialised chain program (ik_amd/csrc/device/chain_hot.hpp), stage-wise on the host: the error
vector e = log6(fMt) and the task Jacobian J = -Jlog6(tMf) J_local it builds tip to base in the task frame, against the oracle's
(reference ik/ik/frame.hpp:37-62,152-182), for the two structure codes kernels_hot.hip instantiates (Cassie leg, UR5).  The shim
tests/hot_eval/hot_eval_shim.cpp is compiled here the way tests/test_lane_emulation.py compiles its emulator.

Bars: 1e-11 on every entry of e and J, the one tests/test_lane_emulation.py holds the chain program's e and J to against the oracle;
1e-6 for the targets a rotation by almost pi away, the bar tests/test_gpu_rotation_by_pi.py holds that regime to (sin(theta) comes from
1 + cos(theta) there: the oracle's own double arithmetic is 1e-8 from its _Float128 build)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, urdf_path

import oracle as O

MODELS = [("cassie_fixed", "LeftFootFront"), ("ur5", "tool0")]
BAR, BAR_NEAR_PI = 1e-11, 1e-6
PI_GAPS = (1e-9, 1e-6, 1e-2)
# no component near zero: sin(theta) a_i = delta a_i stays far above rounding, so the signs of the axis are unambiguous down to
# delta = 1e-9 (AT pi log3 has two values and the oracle itself is discontinuous, see tests/test_gpu_rotation_by_pi.py)
PI_AXES = np.array([[1.0, 2.0, 3.0], [-2.0, 1.0, -1.5], [1.0, -1.0, 2.0]])


@pytest.fixture(scope="module")
def shim(native_built):
    src = os.path.join(ROOT, "tests", "hot_eval", "hot_eval_shim.cpp")
    out = os.path.join(ROOT, "tests", "hot_eval", "libhot_eval_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp",
                                                    "device/chain_solver.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.hot_eval_last_error.restype = C.c_char_p
    return L


def _rot(axis, theta):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def _cases(model, om, fid):
    """(label, q [n, nq], targets [n, 1, 12]) for the five groups."""
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(0)
    q = rng.uniform(lo, hi, (256, lo.size))
    tg = O.fk_batch(om, rng.uniform(lo, hi, (256, lo.size)), [fid])
    out = [("uniform", q, tg)]
    # every joint on its lower and on its upper limit: one at a time over a uniform configuration, and all together
    ql = []
    for j in range(lo.size):
        for lim in (lo, hi):
            ql.append(q[len(ql)].copy())
            ql[-1][j] = lim[j]
    ql += [lo.copy(), hi.copy()]
    ql = np.array(ql)
    out.append(("on_limits", ql, tg[:len(ql)]))
    out.append(("at_target", q[:64], O.fk_batch(om, q[:64], [fid])))
    qp, tp = [], []
    here = O.fk_batch(om, q[:8], [fid])
    for b in range(8):
        for gap in PI_GAPS:
            for axis in PI_AXES:
                t = here[b, 0].copy()
                t[:9] = (t[:9].reshape(3, 3) @ _rot(axis, np.pi - gap)).ravel()
                qp.append(q[b])
                tp.append(t[None])
    out.append(("near_pi", np.array(qp), np.array(tp)))
    out.append(("zero", np.zeros((16, lo.size)), tg[:16]))
    return out


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] for m in MODELS])
def evaluated(request, shim):
    """Every case of one model through the shim in ONE call, and the oracle's e and J for them, computed once."""
    import ik_amd
    from ik_amd import capi
    name, frame = request.param
    urdf = open(urdf_path(name), "rb").read()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(frame)
    cases = _cases(model, om, fid)
    q = np.ascontiguousarray(np.concatenate([c[1] for c in cases]))
    tg = np.ascontiguousarray(np.concatenate([c[2] for c in cases]))
    n, nv = q.shape[0], model.nv
    e, J = np.empty((n, 6)), np.empty((n, 6, nv))
    leader, nj = (C.c_int * 8)(), C.c_int(0)
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    p = lambda a: C.c_void_p(a.ctypes.data)
    colbuf = np.empty(n * 7 * 6)
    rc = shim.hot_eval_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), p(q), p(tg), p(e), p(J), p(colbuf), leader, C.byref(nj))
    assert rc == 0, shim.hot_eval_last_error()
    col = colbuf[:n * nj.value * 6].reshape(n, nj.value, 6)
    ot = O.make_tasks([(fid, 0, 2, 0, None)])
    eo, Jo = np.empty_like(e), np.empty_like(J)
    for b in range(n):
        eo[b], Jo[b] = O.evaluate(om, ot, tg[b], q[b])
    span, at = {}, 0
    for label, qc, _ in cases:
        span[label] = slice(at, at + qc.shape[0])
        at += qc.shape[0]
    return dict(name=name, e=e, J=J, col=col, eo=eo, Jo=Jo, span=span, leader=list(leader)[:nj.value])


@pytest.mark.parametrize("group", ["uniform", "on_limits", "at_target", "zero"])
def test_error_and_jacobian_match_the_oracle(evaluated, group):
    s = evaluated["span"][group]
    de, dJ = np.abs(evaluated["e"][s] - evaluated["eo"][s]).max(), np.abs(evaluated["J"][s] - evaluated["Jo"][s]).max()
    print("%s %s: max |de| %.2e, max |dJ| %.2e over %d configurations" % (evaluated["name"], group, de, dJ, s.stop - s.start))
    assert np.isfinite(evaluated["e"][s]).all() and np.isfinite(evaluated["J"][s]).all()
    assert de < BAR and dJ < BAR
    if group == "at_target":   # theta = 0, e = 0 (to the rounding of the two forward kinematics)
        assert np.abs(evaluated["e"][s]).max() < BAR


def test_error_and_jacobian_a_rotation_by_almost_pi_from_the_target(evaluated):
    s = evaluated["span"]["near_pi"]
    e, eo = evaluated["e"][s], evaluated["eo"][s]
    de, dJ = np.abs(e - eo).max(axis=1), np.abs(evaluated["J"][s] - evaluated["Jo"][s]).max(axis=(1, 2))
    gaps = np.tile(np.repeat(PI_GAPS, len(PI_AXES)), 8)
    for g in PI_GAPS:
        print("%s pi - %.0e: max |de| %.2e, max |dJ| %.2e" % (evaluated["name"], g, de[gaps == g].max(), dJ[gaps == g].max()))
    assert np.isfinite(e).all() and np.isfinite(evaluated["J"][s]).all()
    assert np.abs(np.linalg.norm(eo[:, 3:], axis=1) - (np.pi - gaps)).max() < 1e-6     # the cases are where they claim to be
    assert de.max() < BAR_NEAR_PI and dJ.max() < BAR_NEAR_PI


def test_parallel_joints_share_their_angular_rows_bitwise(evaluated):
    """hot_gram and hot_step read col[leader][3..5] for every member of a run of parallel joints: the members' own must be the same bits."""
    leader, col = evaluated["leader"], evaluated["col"]
    if evaluated["name"] == "cassie_fixed":
        assert leader == [0, 1, 2, 2, 2, 2, 2]     # hip roll, hip yaw, then five parallel pitch axes
    for j, L in enumerate(leader):
        if L != j:
            assert np.array_equal(col[:, j, 3:].view(np.uint64), col[:, L, 3:].view(np.uint64)), (j, L)
