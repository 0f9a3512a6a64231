"""dsincos_lut (ik_amd/csrc/device/lane_math.hpp), the sin / cos of the hot chain loops, on the host: the routine compiled with g++
through a shim of its own (tests/sincos_lut/sincos_lut_shim.cpp) on the literals of device/sincos_lut_table.hpp.

Bar: |s - sin x| and |c - cos x| <= 5e-16 + 4e-17 |x|.  The routine's own budget is 3.4e-16 -- the table entry's rounding (1.11e-16) and
the two nested multiply-adds of the combination (1.11e-16 each), the polynomials' errors entering multiplied by |r| <= 3.1e-3 -- plus the
one-word reduction's 3.9e-17 |x|; the rest is margin for the second-order terms.  The reference is sin / cos in 80-bit long double
(64-bit mantissa, error below 1e-19; asserted to be that format), so none of the bar is spent on the reference.

Points: 400 001-point grids over +-(2 pi + 0.05), +-50 and +-3000; 0, -0, 1e-300; every multiple k h of the table's step for |k| <= 8192
(+-50.3 rad) and for the 2049 k around +-3000 / h, with the doubles one ulp on either side of each; every half-step tie (k + 1/2) h of
the same k with its two neighbours (where the rounding of k flips and |r| is largest); the negative ones among them wrap the index
(k mod 1024 of a negative k), which is asserted on the multiples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

N = 1024
LD = np.longdouble


def _bar(x):
    return 5e-16 + 4e-17 * np.abs(x)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(ROOT, "tests", "sincos_lut", "sincos_lut_shim.cpp")
    out = os.path.join(ROOT, "tests", "sincos_lut", "libsincos_lut_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src, os.path.join(csrc, "device", "lane_math.hpp"), os.path.join(csrc, "device", "sincos_lut_table.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-o", out, src])
    L = C.CDLL(out)
    L.sincos_lut_step.restype = C.c_double
    return L


def _run(shim, x):
    x = np.ascontiguousarray(x, float)
    s, c, r = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    idx = np.empty(x.size, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    shim.sincos_lut_run(C.c_int64(x.size), p(x), p(s), p(c), p(idx), p(r))
    return s, c, idx, r


def _check(shim, x, label):
    assert np.finfo(LD).nmant >= 63      # the reference is wider than double
    s, c, idx, r = _run(shim, x)
    xl = x.astype(LD)
    ds = np.abs(s.astype(LD) - np.sin(xl)).astype(float)
    dc = np.abs(c.astype(LD) - np.cos(xl)).astype(float)
    unit = np.abs(s * s + c * c - 1.0).max()
    print("%s: %d points, max |ds| %.3e, max |dc| %.3e, worst share of the bar %.3f, max |s^2 + c^2 - 1| %.2e, max |r| %.6e"
          % (label, x.size, ds.max(), dc.max(), (np.maximum(ds, dc) / _bar(x)).max(), unit, np.abs(r).max()))
    assert (idx >= 0).all() and (idx < N).all()
    assert (ds <= _bar(x)).all() and (dc <= _bar(x)).all(), (x[np.argmax(np.maximum(ds, dc) / _bar(x))])
    assert unit <= 1e-15
    return idx, r


def _ks():
    far = int(round(3000.0 / (2 * np.pi / N)))
    return np.concatenate([np.arange(-8192, 8193), np.arange(far - 1024, far + 1025), np.arange(-far - 1024, -far + 1025)])


def _with_neighbours(x):
    return np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])


@pytest.mark.parametrize("lim", [2 * np.pi + 0.05, 50.0, 3000.0])
def test_grids(shim, lim):
    _check(shim, np.linspace(-lim, lim, 400001), "grid +-%g" % lim)


def test_zero_and_tiny(shim):
    x = np.array([0.0, -0.0, 1e-300])
    s, c, idx, _ = _run(shim, x)
    _check(shim, x, "0, -0, 1e-300")
    assert (idx == 0).all() and (c == 1.0).all() and s[0] == 0.0 and s[1] == 0.0 and s[2] == 1e-300


def test_multiples_of_the_step_and_their_neighbours(shim):
    k = _ks()
    h = LD(2) * LD(np.pi) + LD(1.2246467991473532e-16) * 2     # 2 pi to long double precision (pi's double and its remainder)
    x0 = (k.astype(LD) * h / N).astype(float)
    idx, r = _check(shim, _with_neighbours(x0), "multiples of the step, +-1 ulp")
    # at a multiple itself the index is k mod 1024, also for negative k, and the residual is the reduction's error alone
    assert np.array_equal(idx[:k.size], np.mod(k, N))
    assert (np.abs(r[:k.size]) <= 4e-17 * np.abs(x0) + 2.0 ** -52 * np.abs(x0)).all()
    assert (k < 0).any() and (np.mod(k[k < 0], N) != 0).any()


def test_half_step_ties_and_their_neighbours(shim):
    k = _ks()
    h = LD(2) * LD(np.pi) + LD(1.2246467991473532e-16) * 2
    x0 = ((k.astype(LD) + LD(0.5)) * h / N).astype(float)
    idx, r = _check(shim, _with_neighbours(x0), "half-step ties, +-1 ulp")
    # either neighbour of the tie is a correct choice; the residual never exceeds half a step by more than the reduction's slack
    assert ((idx[:k.size] == np.mod(k, N)) | (idx[:k.size] == np.mod(k + 1, N))).all()
    assert (np.abs(r) <= np.pi / N + 1e-15 * (1.0 + np.abs(np.tile(x0, 3)))).all()
    assert len(np.unique(idx)) == N


def test_non_finite_arguments_index_inside_the_table(shim):
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, 2.0 ** 60])
    with np.errstate(all="ignore"):
        _, _, idx, _ = _run(shim, x)
    assert (idx >= 0).all() and (idx < N).all()


def test_the_shim_reads_the_headers_literals(shim):
    import re
    tab = np.empty(2 * N)
    shim.sincos_lut_table(C.c_void_p(tab.ctypes.data))
    text = open(os.path.join(ROOT, "ik_amd", "csrc", "device", "sincos_lut_table.hpp")).read()
    lits = re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", text[text.index("#define IKD_SINCOS_LUT_VALUES"):])
    assert shim.sincos_lut_size() == N and np.array_equal(tab, np.array([float.fromhex(v) for v in lits]))
    assert shim.sincos_lut_step() == 6.28318530717958623200 / N
