"""The front end of log6_and_jlog6_hot (ik_amd/csrc/device/lane_math.hpp: 1 / h from one reciprocal square root, h = z zc / h,
1 / theta from a reciprocal of its own, two floors that keep the discarded arms of the selects finite) on the host, through
tests/lane_math/lane_math_shim.cpp, in the regimes where those scalars change hands: theta exactly 0, the switch between the Taylor
and the closed forms at 2^-13 (one ulp either side of it), 1e-3, 1, pi - 1e-2 (where the theta -> pi formula of log3 begins),
pi - 1e-9, and a trace clamped to -1.

e = log6(fMt), and A, C of Jlog6(tMf) = [A  C A; 0  A], are finite everywhere and agree with the oracle's log6 / Jlog6 (reference
ik/ik/frame.hpp:50-61,162-166) within the bars of tests/test_hot_evaluate.py: 1e-11, and 1e-6 from pi - 1e-2 on (sin(theta) comes
from 1 + cos(theta) there: the oracle's own double arithmetic is 1e-8 from its _Float128 build).

The clamped case is a rotation by pi - 1e-9 with one diagonal entry lowered until the trace is <= -1: the antisymmetric part of R
still carries the signs of the axis (AT pi log3 has two values, see tests/test_gpu_rotation_by_pi.py), and both sides then see
theta = pi, 1e-9 from where the rotation is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import oracle as O

BAR, BAR_NEAR_PI = 1e-11, 1e-6      # tests/test_hot_evaluate.py
T13 = 2.0 ** -13
REGIMES = [("zero", 0.0, BAR), ("switch_minus_ulp", np.nextafter(T13, 0.0), BAR), ("switch", T13, BAR),
           ("switch_plus_ulp", np.nextafter(T13, 1.0), BAR), ("1e-3", 1e-3, BAR), ("one", 1.0, BAR),
           ("pi_minus_1e-2", np.pi - 1e-2, BAR_NEAR_PI), ("pi_minus_1e-9", np.pi - 1e-9, BAR_NEAR_PI), ("clamped", np.pi - 1e-9, BAR_NEAR_PI)]
# no component near zero: the signs of the axis stay unambiguous down to pi - 1e-9 (tests/test_hot_evaluate.py PI_AXES)
AXES = np.array([[1.0, 2.0, 3.0], [-2.0, 1.0, -1.5], [1.0, -1.0, 2.0]])
PE = np.array([[0.3, -0.2, 0.4], [-0.05, 0.45, 0.1], [0.0, 0.0, 0.0]])


@pytest.fixture(scope="module")
def shim(native_built):
    src = os.path.join(ROOT, "tests", "lane_math", "lane_math_shim.cpp")
    out = os.path.join(ROOT, "tests", "lane_math", "liblane_math_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src, os.path.join(csrc, "device", "lane_math.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src])
    return C.CDLL(out)


def _exp3(w):
    """exp of the rotation vector w, in longdouble and rounded once: R is the rotation by |w| to the last bit of its entries."""
    w = np.asarray(w, np.longdouble)
    t = np.sqrt(w @ w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], np.longdouble)
    if t == 0.0:
        return np.eye(3)
    return (np.eye(3, dtype=np.longdouble) + (np.sin(t) / t) * K + ((1.0 - np.cos(t)) / (t * t)) * (K @ K)).astype(np.float64)


@pytest.fixture(scope="module")
def evaluated(shim):
    """Every regime x axis x translation through the shim in one call, and the oracle's log6 / Jlog6 for them, computed once."""
    Re, pe, label = [], [], []
    for name, theta, _ in REGIMES:
        for axis in AXES:
            for p in PE:
                R = _exp3(np.asarray(axis, np.longdouble) / np.sqrt(np.asarray(axis, np.longdouble) @ np.asarray(axis, np.longdouble)) * np.longdouble(theta))
                if name == "clamped":
                    R[0, 0] -= 4.5e-16
                    assert np.trace(R) <= -1.0
                Re.append(R.ravel())
                pe.append(p)
                label.append(name)
    Re, pe = np.ascontiguousarray(Re), np.ascontiguousarray(pe)
    n = Re.shape[0]
    e, A, Cm, Bm = np.empty((n, 6)), np.empty((n, 9)), np.empty((n, 9)), np.empty((n, 9))
    p = lambda a: C.c_void_p(a.ctypes.data)
    shim.lane_math_log6(C.c_int64(n), p(Re), p(pe), p(e), p(A), p(Cm), p(Bm))
    eo, Jo = np.empty((n, 6)), np.empty((n, 6, 6))
    for s in range(n):
        R = Re[s].reshape(3, 3)
        eo[s] = O.log6(np.concatenate([Re[s], pe[s]]))
        Jo[s] = O.Jlog6(np.concatenate([R.T.ravel(), -R.T @ pe[s]]))     # tMf = fMt^-1
    return dict(label=np.array(label), e=e, A=A.reshape(n, 3, 3), C=Cm.reshape(n, 3, 3), Bm=Bm.reshape(n, 3, 3), eo=eo, Jo=Jo)


@pytest.mark.parametrize("name,theta,bar", REGIMES, ids=[r[0] for r in REGIMES])
def test_log6_and_jlog6_in_every_regime_of_the_scalars(evaluated, name, theta, bar):
    s = evaluated["label"] == name
    e, A, Cm, Bm, eo, Jo = (evaluated[k][s] for k in ("e", "A", "C", "Bm", "eo", "Jo"))
    assert np.isfinite(e).all() and np.isfinite(A).all() and np.isfinite(Cm).all() and np.isfinite(Bm).all()
    de = np.abs(e - eo).max()
    dA = max(np.abs(A - Jo[:, :3, :3]).max(), np.abs(A - Jo[:, 3:, 3:]).max())
    dCA = max(np.abs(Cm @ A - Jo[:, :3, 3:]).max(), np.abs(Bm - Jo[:, :3, 3:]).max())
    print("%s: max |de| %.2e, |dA| %.2e, |d(C A)| %.2e over %d placements" % (name, de, dA, dCA, int(s.sum())))
    assert np.abs(Jo[:, 3:, :3]).max() == 0.0
    assert np.abs(np.linalg.norm(eo[:, 3:], axis=1) - (np.pi if name == "clamped" else theta)).max() < 1e-6   # the cases are where they claim to be
    assert de < bar and dA < bar and dCA < bar
    if name == "zero":
        assert np.array_equal(e[:, 3:], np.zeros_like(e[:, 3:])) and np.abs(A - np.eye(3)[None]).max() == 0.0
