"""The 6 x 6 solve of the DLS step (ik_amd/csrc/device/lane_math.hpp ldlt_solve<6>: an unpivoted L D L^T, right-looking) on the host,
through tests/lane_math/lane_math_shim.cpp, compiled here the way tests/test_hot_evaluate.py compiles its shim.  M = 6 is the
size of the headline loop (a Full task); the tree program keeps its own chol_solve, which this change leaves as it was.

G = J J^T + lambda^2 I for a random 6 x 7 J and lambda^2 in {1e-4, 1e-12, 100}, and a rank-deficient J (two equal columns, one zero
row) at lambda^2 = 1e-4: G x = b against a solve of the same double-precision G and b in numpy's longdouble (Gaussian elimination
with partial pivoting and one step of refinement, written out below: numpy.linalg has no extended-precision solve).

Bar: ||x - x_ref|| / ||x_ref|| <= 8 kappa_2(G) 2^-53.  An unpivoted factorisation of an SPD matrix is backward stable -- the
computed x solves (G + dG) x = b with ||dG|| <= c n u ||G||, c a small constant (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Theorem 10.4 for L L^T; the L D L^T of an SPD matrix has the same bound) -- so the forward error is at most
kappa c n u; 8 stands for c n at n = 6.  The bar is not fitted to what the code gives.  Where long double is no wider than double the
reference is no better than the code and the test cannot tell anything: it then fails rather than skips.

Worst observed ratio err / (kappa 2^-53), 64 systems per case: 2.11 at lambda^2 = 100 (kappa ~ 1: two roundings), 0.45 at 1e-4, 0.33 at
1e-12, 1.7e-4 for the rank-deficient J (kappa ~ 1e5, most of it never realised by these right-hand sides)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

U = 2.0 ** -53
FACTOR = 8.0
LAM2 = (1e-4, 1e-12, 100.0)
N = 64   # systems per case


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(ROOT, "tests", "lane_math", "lane_math_shim.cpp")
    out = os.path.join(ROOT, "tests", "lane_math", "liblane_math_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src, os.path.join(csrc, "device", "lane_math.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src])
    return C.CDLL(out)


def _solve_longdouble(G, b):
    """x with G x = b in longdouble: partial pivoting, then one refinement step with the residual in longdouble."""
    def ge(A, r):
        A, r = A.copy(), r.copy()
        n = r.size
        for k in range(n):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            if p != k:
                A[[k, p]] = A[[p, k]]
                r[[k, p]] = r[[p, k]]
            for i in range(k + 1, n):
                m = A[i, k] / A[k, k]
                A[i, k:] -= m * A[k, k:]
                r[i] -= m * r[k]
        x = np.zeros(n, np.longdouble)
        for k in range(n - 1, -1, -1):
            x[k] = (r[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
        return x
    Gl, bl = G.astype(np.longdouble), b.astype(np.longdouble)
    x = ge(Gl, bl)
    return x + ge(Gl, bl - Gl @ x)


def _systems(case):
    rng = np.random.default_rng(11)
    J = rng.normal(size=(N, 6, 7))
    if case == "rank_deficient":
        J[:, :, 4] = J[:, :, 1]      # two equal columns
        J[:, 3, :] = 0.0             # one zero row: G_33 = lambda^2 alone
        lam2 = 1e-4
    else:
        lam2 = case
    G = J @ J.transpose(0, 2, 1) + lam2 * np.eye(6)[None]
    G = 0.5 * (G + G.transpose(0, 2, 1))
    b = rng.normal(size=(N, 6))
    return np.ascontiguousarray(G), np.ascontiguousarray(b)


@pytest.mark.parametrize("case", list(LAM2) + ["rank_deficient"], ids=lambda c: str(c))
def test_solve_against_extended_precision(shim, case):
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "long double is no wider than double here: no reference"
    G, b = _systems(case)
    x = np.empty_like(b)
    p = lambda a: C.c_void_p(a.ctypes.data)
    shim.lane_math_solve6(C.c_int64(N), p(G), p(b), p(x))
    assert np.isfinite(x).all()
    worst = 0.0
    for s in range(N):
        ref = _solve_longdouble(G[s], b[s])
        sv = np.linalg.svd(G[s], compute_uv=False)
        kappa = sv[0] / sv[-1]
        err = float(np.linalg.norm((x[s].astype(np.longdouble) - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))
        worst = max(worst, err / (kappa * U))
        assert err <= FACTOR * kappa * U, (case, s, err, kappa)
    print("%s: worst err / (kappa 2^-53) = %.3g over %d systems" % (case, worst, N))
