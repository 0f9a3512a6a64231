"""Inputs, references, bars and checks of the lane-primitive probe (tests/lane_math/lane_probe_ops.hpp): what
tests/test_lane_probe_host.py runs through the host shim and tests/test_gpu_lane_probe.py through the device program, under each of
the product's three translation-unit recipes.  No tests here.

Every operation gets ONE input set [n_in, n] (structure-of-arrays, finite values only), built so that lanes sit on each switch of the
primitive, a reference wider than double -- numpy.longdouble (asserted to carry at least 63 mantissa bits) on the grids and sweeps,
mpmath at 50 digits on the edge points and the small sets --, and a bar taken from the project or derived, never from what the code
under test returns:

  drcp / drsqrt / dsqrt   relative error <= 2^-52: each ends in one FMA whose exact argument is within e^3 ~ 1e-22 of the true value,
                          half an ulp plus second-order terms; one ulp is the bar.  dsqrt(0) is +0 to the bit.
  dfma3                   the bits of __builtin_fma, and of the correctly rounded a b + c (mpmath).
  dacos                   2 ulp of the true value: fdlibm's rational form is below 1 ulp with an exact division and square root, the two
                          replaced operations are within 1 ulp each and enter through terms of at most a quarter of the result.
  sin / cos               the bars of tests/test_lane_emulation.py and tests/test_sincos_lut_host.py.
  log6 / Jlog6            1e-11, and 1e-6 from pi - 1e-2 on (tests/test_hot_evaluate.py); front ends within 1e-12 of each other.
  solves                  ||x - x_ref|| / ||x_ref|| <= 8 kappa_2(G) 2^-53 (tests/test_ldlt_solve_host.py).
  log3 / exp3 / waypoints line_common.WAYPOINT_BAR; 1e-6 from pi - 1e-2 on.
  quat_to_R / integrate   1e-13 per entry, the project's stage bar for a frame placement.

The closed forms are restated from SURVEY.md App. A.2, A.3, A.5 twice -- scalar in mpmath, vectorised in longdouble --;
tests/test_lane_probe_host.py holds both to the double oracle and to oracle/twin.py, so a wrong restatement cannot pass for a wide
reference."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

import line_common

try:
    import mpmath
    from mpmath import mp, mpf
    mp.dps = 50
    MPMATH_ERROR = None
except Exception as exc:   # the tests fail with this message, they do not skip
    mpmath = None
    MPMATH_ERROR = "mpmath cannot be imported: %r" % (exc,)

LD = np.longdouble
LM = os.path.join(ROOT, "tests", "lane_math")
CSRC = os.path.join(ROOT, "ik_amd", "csrc")
VARIANTS = ("general", "hot", "static")
T13 = 2.0 ** -13
U52 = 2.0 ** -52
NEAR_PI = np.pi - 1e-2
BAR_LOG6, BAR_NEAR_PI, BAR_FRONT_ENDS = 1e-11, 1e-6, 1e-12
BAR_FRAME = 1e-13
SOLVE_FACTOR = 8.0
# operations written in explicit dfma so that every recipe computes the same bits (device/line.hpp, the dsincos_lut pieces)
BIT_IDENTICAL_ACROSS_RECIPES = ("log3", "exp3", "line_t1", "line_t3", "line_t8", "dsincos_lut1", "dsincos_lut7")


def require_wide_references():
    assert MPMATH_ERROR is None, MPMATH_ERROR
    assert np.finfo(LD).nmant >= 63, "long double is no wider than double here: no reference"


# ------------------------------------------------------------------------------------------------------------------------------
# building and running
# ------------------------------------------------------------------------------------------------------------------------------
def flag_sets():
    """The three recipes, READ from the product: Makefile HIPFLAGS / HOTFLAGS (+ the -O3 -std=c++17 of its CXXFLAGS) and rtc.cpp kFlags."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, mk, re.M).group(1).split()
    arch = var("ARCH")[0]
    hip = [f.replace("$(ARCH)", arch) for f in var("HIPFLAGS")]
    hot = var("HOTFLAGS")
    cxx = [f for f in var("CXXFLAGS") if f.startswith("-O") or f.startswith("-std=")]
    rtc = open(os.path.join(CSRC, "rtc.cpp")).read()
    kflags = re.findall(r'"([^"]+)"', re.search(r"kFlags\[\]\s*=\s*\{(.*?)\};", rtc, re.S).group(1))
    general = cxx + hip
    return {"general": general, "hot": general + hot, "static": general + hot + ["-DIKD_STATIC_TABLES=1"], "rtc": kflags}


def _deps():
    dev = os.path.join(CSRC, "device")
    return [os.path.join(LM, "lane_probe_ops.hpp")] + [os.path.join(dev, f) for f in sorted(os.listdir(dev)) if f.endswith(".hpp")]


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build_host():
    src, out = os.path.join(LM, "lane_probe_host.cpp"), os.path.join(LM, "liblane_probe_host.so")
    if _stale(out, [src] + _deps()):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out, src])
    L = C.CDLL(out)
    L.list.restype = C.c_char_p
    return L


def build_device(variant):
    src, out = os.path.join(LM, "lane_probe.hip"), os.path.join(LM, "lane_probe_" + variant)
    if _stale(out, [src] + _deps()):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc] + flag_sets()[variant] + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out, src])
    return out


def op_names():
    """The names of the table's rows, read from the header's text (for parametrising the tests without compiling anything at collection;
    sizes and everything else come from `--list`, and tests/test_lane_probe_host.py holds the two to each other)."""
    text = open(os.path.join(LM, "lane_probe_ops.hpp")).read()
    return sorted(re.findall(r"^\s*X\((\w+), *\d+(?:, *\d+)?\)", text, re.M))


def parse_table(text):
    if isinstance(text, bytes):
        text = text.decode()
    return {f[0]: (int(f[1]), int(f[2])) for f in (line.split() for line in text.strip().splitlines())}


def run_host(L, op, x):
    table = parse_table(L.list())
    ni, no = table[op]
    x = np.ascontiguousarray(x, float)
    assert x.shape[0] == ni, (op, x.shape, ni)
    out = np.full((no, x.shape[1]), np.nan)
    with np.errstate(all="ignore"):
        rc = L.run(op.encode(), C.c_int64(x.shape[1]), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data))
    assert rc == 0, op
    return out


def run_device(exe, op, xs, table):
    """One child process, one launch per input set of xs; the outputs, or raises RuntimeError with what the child said."""
    ni, no = table[op]
    with tempfile.TemporaryDirectory() as d:
        args = [exe]
        for k, x in enumerate(xs):
            x = np.ascontiguousarray(x, "<f8")
            assert x.shape[0] == ni and np.isfinite(x).all()
            x.tofile(os.path.join(d, "in%d.f64" % k))
            args += [op, str(x.shape[1]), os.path.join(d, "in%d.f64" % k), os.path.join(d, "out%d.f64" % k)]
        try:
            r = subprocess.run(args, timeout=120, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            raise RuntimeError("%s %s: no result within 120 s" % (os.path.basename(exe), op))
        if r.returncode != 0:
            raise RuntimeError("%s %s: exit status %d: %s" % (os.path.basename(exe), op, r.returncode, r.stderr.strip()[-400:]))
        return [np.fromfile(os.path.join(d, "out%d.f64" % k), "<f8").reshape(no, x.shape[1]) for k, x in enumerate(xs)]


def permutation(n):
    """A fixed permutation that mixes the regimes of an ordered input set within every wave."""
    return np.random.default_rng(1234).permutation(n)


SMALL_N = (1, 63, 64, 65, 130)


# ------------------------------------------------------------------------------------------------------------------------------
# wide restatements of the closed forms
# ------------------------------------------------------------------------------------------------------------------------------
def _m(v):
    return [mpf(float(a)) for a in v]


def mp_cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def mp_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def mp_matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def mp_skew(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def mp_log3(R):
    """(w, theta) of a rotation given as nine mpf, row-major rows."""
    tr = R[0][0] + R[1][1] + R[2][2]
    theta = mpf(0) if tr >= 3 else (mp.pi if tr <= -1 else mp.acos((tr - 1) / 2))
    if theta >= mp.pi - mpf(1e-2):
        c = -(tr - 1) / 2
        beta = theta * theta / (1 + c)
        sg = (1 if R[2][1] > R[1][2] else -1, 1 if R[0][2] > R[2][0] else -1, 1 if R[1][0] > R[0][1] else -1)
        tmp = [(R[k][k] + c) * beta for k in range(3)]
        return [sg[k] * (mp.sqrt(tmp[k]) if tmp[k] > 0 else mpf(0)) for k in range(3)], theta
    t = (theta / mp.sin(theta) if theta > T13 else mpf(1)) / 2
    return [t * (R[2][1] - R[1][2]), t * (R[0][2] - R[2][0]), t * (R[1][0] - R[0][1])], theta


def _mp_scalars(t):
    t2 = t * t
    if t < T13:
        return 1 - t2 / 12 - t2 * t2 / 720, mpf(1) / 12 + t2 / 720, (2 - t2 / 6) / 2, mpf(1) / 360
    st, ct = mp.sin(t), mp.cos(t)
    alpha = t * st / (2 * (1 - ct))
    beta = 1 / t2 - st / (2 * t * (1 - ct))
    bdot = -2 / (t2 * t2) + (1 + st / t) / (2 * t2 * (1 - ct))
    return alpha, beta, alpha, bdot


def mp_log6(R, p):
    w, t = mp_log3(R)
    alpha, beta, _, _ = _mp_scalars(t)
    wxp, wp = mp_cross(w, p), mp_dot(w, p)
    return [alpha * p[i] - wxp[i] / 2 + beta * wp * w[i] for i in range(3)] + w, t


def mp_jlog6_blocks(w, t, p):
    """A = Jlog3(theta, w) and C with Jlog6 = [[A, C A], [0, A]] for the transform whose log3 is w and translation p."""
    _, beta, diag, bdot = _mp_scalars(t)
    sk = mp_skew(w)
    A = [[beta * w[i] * w[j] + (diag if i == j else 0) + sk[i][j] / 2 for j in range(3)] for i in range(3)]
    wp = mp_dot(w, p)
    v3 = [bdot * wp * w[i] - (t * t * bdot + 2 * beta) * p[i] for i in range(3)]
    sp = mp_skew(p)
    Cm = [[v3[i] * w[j] + beta * w[i] * p[j] + (wp * beta if i == j else 0) + sp[i][j] / 2 for j in range(3)] for i in range(3)]
    return A, Cm


def mp_log6_and_jlog6_inv(Re, pe):
    """What the lane functions return for fMt = (Re, pe): e = log6(fMt), and A, C, C A of Jlog6(tMf), tMf = fMt^-1
    (log3(R^T) = -log3(R) with the same theta: SURVEY.md A.3).  Rows of 6, 9, 9, 9 floats, and theta."""
    R = [_m(Re[0:3]), _m(Re[3:6]), _m(Re[6:9])]
    p = _m(pe)
    e, t = mp_log6(R, p)
    u = [-a for a in e[3:]]
    pp = [-sum(R[k][i] * p[k] for k in range(3)) for i in range(3)]
    A, Cm = mp_jlog6_blocks(u, t, pp)
    B = mp_matmul(Cm, A)
    flat = lambda M: [float(M[i][j]) for i in range(3) for j in range(3)]
    return [float(a) for a in e], flat(A), flat(Cm), flat(B), float(t)


def mp_exp3(w):
    t2 = mp_dot(w, w)
    t = mp.sqrt(t2)
    if t < T13:
        a_wxv, a_v, diag = mpf(1) / 2 - t2 / 24, 1 - t2 / 6, 1 - t2 / 2
    else:
        a_wxv, a_v, diag = (1 - mp.cos(t)) / t2, mp.sin(t) / t, mp.cos(t)
    sk = mp_skew(w)
    return [[a_wxv * w[i] * w[j] + a_v * sk[i][j] + (diag if i == j else 0) for j in range(3)] for i in range(3)]


def mp_exp6(nu):
    v, w = nu[:3], nu[3:]
    t2 = mp_dot(w, w)
    t = mp.sqrt(t2)
    if t < T13:
        a_wxv, a_v, a_w = mpf(1) / 2 - t2 / 24, 1 - t2 / 6, mpf(1) / 6 - t2 / 120
    else:
        a_wxv, a_v = (1 - mp.cos(t)) / t2, mp.sin(t) / t
        a_w = (1 - a_v) / t2
    wxv, wv = mp_cross(w, v), mp_dot(w, v)
    return mp_exp3(w), [a_v * v[i] + a_w * wv * w[i] + a_wxv * wxv[i] for i in range(3)]


def mp_quat_to_R(q):
    """Eigen::Quaternion::toRotationMatrix of (x, y, z, w), not normalised."""
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def mp_matrix_to_quat(R):
    t = R[0][0] + R[1][1] + R[2][2]
    q = [mpf(0)] * 4
    if t > 0:
        t = mp.sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 1 if R[1][1] > R[0][0] else 0
        i = 2 if R[2][2] > R[i][i] else i
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3], q[j], q[k] = (R[k][j] - R[j][k]) * t, (R[j][i] + R[i][j]) * t, (R[k][i] + R[i][k]) * t
    return q


def mp_freeflyer_integrate(qb, v):
    """pinocchio::integrate for the free-flyer: the new (p, quaternion) as 7 floats, and the dot product of the
    converted quaternion with the previous one, whose sign decides the hemisphere."""
    qb, v = _m(qb), _m(v)
    R1 = mp_quat_to_R(qb[3:7])
    E, tr = mp_exp6(v)
    p = [qb[i] + sum(R1[i][k] * tr[k] for k in range(3)) for i in range(3)]
    q = mp_matrix_to_quat(mp_matmul(R1, E))
    dp = sum(q[k] * qb[3 + k] for k in range(4))
    if dp < 0:
        q = [-a for a in q]
    n2 = sum(a * a for a in q)
    q = [a * (3 - n2) / 2 for a in q]
    return [float(a) for a in p + q], float(dp)


# ---- the same in longdouble, vectorised over lanes: R [n, 3, 3], vectors [n, 3] --------------------------------------------------
LD_PI = LD(np.pi) + LD(1.2246467991473532e-16)     # pi's double and its remainder


def ld_skew(w):
    K = np.zeros(w.shape[:-1] + (3, 3), LD)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 2], w[..., 1], w[..., 2], -w[..., 0], -w[..., 1], w[..., 0]
    return K


def ld_exp3(w):
    w = np.asarray(w, LD)
    t2 = (w * w).sum(-1)
    t = np.sqrt(t2)
    small = t < T13
    ts, t2s = np.where(small, LD(1), t), np.where(small, LD(1), t2)
    a_wxv = np.where(small, LD(0.5) - t2 / 24, (1 - np.cos(ts)) / t2s)
    a_v = np.where(small, 1 - t2 / 6, np.sin(ts) / ts)
    diag = np.where(small, 1 - t2 / 2, np.cos(ts))
    return a_wxv[..., None, None] * w[..., :, None] * w[..., None, :] + a_v[..., None, None] * ld_skew(w) + diag[..., None, None] * np.eye(3, dtype=LD)


def ld_log3(R):
    R = np.asarray(R, LD)
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    x = np.clip((tr - 1) / 2, LD(-1), LD(1))
    theta = np.where(tr >= 3, LD(0), np.where(tr <= -1, LD_PI, np.arccos(x)))
    d = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    st = np.sin(theta)
    fac = np.where(theta > T13, theta / np.where(st == 0, LD(1), st), LD(1)) / 2
    w = fac[..., None] * d
    near = theta >= LD_PI - LD(1e-2)
    c = -(tr - 1) / 2
    beta = theta * theta / np.where(near, 1 + c, LD(1))
    tmp = (np.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]], -1) + c[..., None]) * beta[..., None]
    wn = np.where(d > 0, LD(1), LD(-1)) * np.sqrt(np.maximum(tmp, 0))
    return np.where(near[..., None], wn, w), theta


def _ld_scalars(t):
    t2 = t * t
    small = t < T13
    ts = np.where(small, LD(1), t)
    st, ct = np.sin(ts), np.cos(ts)
    alpha = np.where(small, 1 - t2 / 12 - t2 * t2 / 720, ts * st / (2 * (1 - ct)))
    beta = np.where(small, LD(1) / 12 + t2 / 720, 1 / (ts * ts) - st / (2 * ts * (1 - ct)))
    diag = np.where(small, (2 - t2 / 6) / 2, alpha)
    bdot = np.where(small, LD(1) / 360, -2 / (ts ** 4) + (1 + st / ts) / (2 * ts * ts * (1 - ct)))
    return alpha, beta, diag, bdot


def ld_log6_and_jlog6_inv(Re, pe):
    """Vectorised mp_log6_and_jlog6_inv: Re [n, 9], pe [n, 3] -> e [n, 6], A, C, C A [n, 9], theta [n] (longdouble)."""
    R = np.asarray(Re, LD).reshape(-1, 3, 3)
    p = np.asarray(pe, LD)
    w, t = ld_log3(R)
    alpha, beta, diag, bdot = _ld_scalars(t)
    wp = (w * p).sum(-1)
    v = alpha[:, None] * p - np.cross(w, p) / 2 + (beta * wp)[:, None] * w
    u = -w
    pp = -np.einsum("nki,nk->ni", R, p)
    I = np.eye(3, dtype=LD)
    A = beta[:, None, None] * u[:, :, None] * u[:, None, :] + diag[:, None, None] * I + ld_skew(u) / 2
    up = (u * pp).sum(-1)
    v3 = (bdot * up)[:, None] * u - (t * t * bdot + 2 * beta)[:, None] * pp
    Cm = v3[:, :, None] * u[:, None, :] + beta[:, None, None] * u[:, :, None] * pp[:, None, :] + (up * beta)[:, None, None] * I + ld_skew(pp) / 2
    n = R.shape[0]
    return np.concatenate([v, w], 1), A.reshape(n, 9), Cm.reshape(n, 9), (Cm @ A).reshape(n, 9), t


def rotation(axis, theta):
    """exp3(theta axis / |axis|) in longdouble, rounded once: the rotation to the last bit of its entries, [3, 3] float."""
    a = np.asarray(axis, LD)
    return ld_exp3(a / np.sqrt(a @ a) * LD(theta)).astype(float)


def ulps(out, ref):
    """|out - ref| in units of the spacing of double at ref (ref longdouble)."""
    return (np.abs(out.astype(LD) - ref) / np.spacing(np.abs(ref.astype(float))).astype(LD)).astype(float)


def neighbours(x, k=1):
    x = np.atleast_1d(np.asarray(x, float))
    lo, hi, out = x, x, [x]
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------------------------------
# drcp, drsqrt, dsqrt
# ------------------------------------------------------------------------------------------------------------------------------
_MANTISSAS = np.concatenate([[1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0)], neighbours(np.sqrt(2.0))])
_DENORMALS = np.concatenate([2.0 ** np.arange(-1074.0, -1022.0), [np.nextafter(2.0 ** -1022, 0.0), 3e-310, 1e-315]])


def _log_uniform(rng, n):
    return rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-1022, 1021, n).astype(float)


@functools.lru_cache(None)
def scalar_inputs(op):
    """x [1, n] and barred [n]: lanes inside the stated domain (the others -- denormal in, denormal out, +-0 -- are run and reported)."""
    rng = np.random.default_rng(7)
    grid = _log_uniform(rng, 200000)
    mant = (_MANTISSAS[None, :] * 2.0 ** np.arange(-1022.0, 1021.0, 7.0)[:, None]).ravel()
    if op == "drcp":
        pow2 = 2.0 ** np.arange(-1022.0, 1023.0)
        th = np.pi - 10.0 ** np.linspace(-9, -2, 29)
        callers = np.concatenate([
            neighbours(1e-300)[[0, 2]], 10.0 ** np.arange(-299.0, 1.0, 13.0),                      # theta h, down to its floor
            neighbours(2.0 ** -200)[[0, 2]], neighbours(T13), [np.pi, NEAR_PI],                        # dmax(theta, 2^-200)
            2.0 * 2.0 ** -np.arange(1.0, 55.0),                                                        # 2 z
            1.0 - np.cos(th), neighbours(2.0)[[0, 1]],                                                 # 1 + cphi at theta >= pi - 1e-2
            neighbours(1e-4), neighbours(1e-12), neighbours(100.0)])                                   # lambda^2
        inside = np.concatenate([pow2, grid, -grid[::4], mant, -mant, callers])
        outside = np.concatenate([_DENORMALS, -_DENORMALS[::8], [0.0, -0.0], neighbours(2.0 ** 1023)[[0, 2]], [np.finfo(float).max], 2.0 ** 1022 * _MANTISSAS[1:]])
    elif op == "drsqrt":
        inside = np.concatenate([2.0 ** np.arange(-1022.0, 1024.0), grid, mant, [np.finfo(float).max], neighbours(1e-300), neighbours(2.0 ** -200), neighbours(1e-4), neighbours(1e-12)])
        outside = np.concatenate([_DENORMALS, [0.0, -0.0]])
    else:
        ax = np.concatenate([1.0 - 2.0 ** -np.arange(1.0, 54.0), [np.nextafter(1.0, 0.0)], np.nextafter(1.0 - 2.0 ** -np.arange(1.0, 53.0), 1.0)])
        k = np.arange(1.0, 4097.0)
        inside = np.concatenate([[0.0], 2.0 ** np.arange(-1022.0, 1024.0), grid, mant, k * k, neighbours(1e-300), neighbours(2.0 ** -1022)[[0, 2]],      # (the floor, before and now)
                                 [np.finfo(float).max], (1.0 - ax) * 0.5])
        outside = np.concatenate([_DENORMALS, [-0.0]])
    x = np.concatenate([inside, outside])
    barred = np.arange(x.size) < inside.size
    return x[None, :], barred


def check_scalar(op, out, report=print):
    """-> (max relative error / 2^-52 on the stated domain, the same as a share of the bar)."""
    require_wide_references()
    (x,), barred = scalar_inputs(op)
    y = out[0]
    xl = x.astype(LD)
    with np.errstate(all="ignore"):
        ref = {"drcp": lambda: 1 / xl, "drsqrt": lambda: 1 / np.sqrt(xl), "dsqrt": lambda: np.sqrt(xl)}[op]()
        rel = (np.abs(y.astype(LD) - ref) / np.abs(ref)).astype(float)
    if op == "dsqrt":
        assert x[0] == 0.0 and y[0] == 0.0 and not np.signbit(y[0]), "dsqrt(0) must be +0 to the bit"
        rel[0] = 0.0
    assert np.isfinite(y[barred]).all(), (op, x[barred][~np.isfinite(y[barred])][:4])
    worst = int(np.argmax(np.where(barred, rel, 0.0)))
    fig = rel[worst] / U52
    out_of_range = {}
    for name, sel in (("denormal in", (np.abs(x) < 2.0 ** -1022) & (x != 0)), ("denormal out", np.abs(x) > 2.0 ** 1022), ("+0", (x == 0) & ~np.signbit(x)), ("-0", (x == 0) & np.signbit(x))):
        sel = sel & ~barred
        if sel.any():
            with np.errstate(all="ignore"):
                r = rel[sel]
            out_of_range[name] = "%d lanes, %d finite, max rel err %s, e.g. f(%r) = %r" % (
                sel.sum(), np.isfinite(y[sel]).sum(), "%.2e" % np.nanmax(np.where(np.isfinite(r), r, np.nan)) if np.isfinite(r).any() else "-", x[sel][0], y[sel][0])
    report("%s: %d lanes in the domain, max rel err %.3f x 2^-52 at x = %r; outside (reported only): %s" % (op, barred.sum(), fig, x[worst], out_of_range))
    assert fig <= 1.0, (op, fig, x[worst], y[worst])
    return fig, fig, out_of_range


# ------------------------------------------------------------------------------------------------------------------------------
# dfma3
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def dfma3_inputs():
    rng = np.random.default_rng(8)
    n = 100000
    a, b = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n), rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)
    c = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)
    c[: n // 2] = -(a * b)[: n // 2]          # the addend cancels the rounded product: the result is the product's rounding error
    c[: n // 8] = np.nextafter(c[: n // 8], 0.0)
    # the acos polynomials' own shape: z * p + constant
    a[-1000:], c[-1000:] = rng.uniform(0, 0.25, 1000), 1.66666666666666657415e-01
    return np.stack([a, b, c])


def check_dfma3(out, report=print):
    require_wide_references()
    x = dfma3_inputs()
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)), "dfma3 and __builtin_fma differ in bits"
    idx = np.concatenate([np.arange(0, 1000), np.arange(x.shape[1] - 1000, x.shape[1])])
    exact = np.array([float(mpf(float(x[0, i])) * mpf(float(x[1, i])) + mpf(float(x[2, i]))) for i in idx])
    assert np.array_equal(out[0][idx], exact), "not the correctly rounded a b + c"
    report("dfma3: %d triples bit-equal to __builtin_fma, %d of them to the correctly rounded value" % (x.shape[1], idx.size))
    return 0.0, 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# dacos
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def dacos_inputs():
    k = np.arange(1.0, 54.0)
    edge = np.concatenate([neighbours([1.0, -1.0])[[0, 1, 2, 5]], neighbours([0.5, -0.5], 2), neighbours(0.0), [-0.0], 1.0 - 2.0 ** -k, -1.0 + 2.0 ** -k,
                           neighbours([0.25, 0.75, -0.75])])
    edge = edge[np.abs(edge) <= 1.0]
    above = np.array([np.nextafter(1.0, 2.0), 1.5, -np.nextafter(1.0, 2.0), -1.5])
    return np.concatenate([edge, above, np.linspace(-1.0, 1.0, 200001)])[None, :], edge.size, above.size


@functools.lru_cache(None)
def _dacos_reference():
    require_wide_references()
    (x,), n_edge, n_above = dacos_inputs()
    with np.errstate(all="ignore"):
        ref = np.arccos(x.astype(LD))
    for i in range(n_edge):      # the edge points in mpmath; kept in two doubles' worth of digits
        v = mp.acos(mpf(float(x[i])))
        hi = float(v)
        ref[i] = LD(hi) + LD(float(v - mpf(hi)))
    return ref


def check_dacos(out, report=print):
    (x,), n_edge, n_above = dacos_inputs()
    y, ref = out[0], _dacos_reference()
    inside = np.abs(x) < 1.0
    u = np.zeros(x.size)
    u[inside] = ulps(y[inside], ref[inside])
    worst = int(np.argmax(u))
    report("dacos: %d points, max error %.3f ulp at x = %r" % (x.size, u[worst], x[worst]))
    assert np.array_equal(y[x >= 1.0], np.zeros((x >= 1.0).sum())), "acos(x >= 1) must be exactly 0"
    assert np.array_equal(y[x <= -1.0], np.full((x <= -1.0).sum(), np.pi)), "acos(x <= -1) must be exactly kPi"
    assert (x[n_edge:n_edge + n_above] != np.clip(x[n_edge:n_edge + n_above], -1, 1)).all()
    assert u[worst] <= 2.0, (u[worst], x[worst], y[worst])
    return u[worst], u[worst] / 2.0


# ------------------------------------------------------------------------------------------------------------------------------
# sin / cos
# ------------------------------------------------------------------------------------------------------------------------------
LUT_N = 1024
_TWO_PI_LD = 2 * LD_PI
_SINCOS_RANGES = {"dsincos": (50.0,), "dsincos_fast": (50.0, 3000.0), "dsincos_bounded2": (np.pi + 0.05,), "dsincos_bounded3": (2 * np.pi + 0.05,),
                  "dsincos_hot": (2 * np.pi + 0.05, 50.0, 3000.0), "dsincos_lut1": (2 * np.pi + 0.05, 50.0, 3000.0)}


def _lut_ks():
    far = int(round(3000.0 / (2 * np.pi / LUT_N)))
    return np.concatenate([np.arange(-8192, 8193), np.arange(far - 1024, far + 1025), np.arange(-far - 1024, -far + 1025)])


@functools.lru_cache(None)
def _lut_points():
    """(multiples k h of the table step, half-step ties (k + 1/2) h, k): tests/test_sincos_lut_host.py's points."""
    k = _lut_ks()
    return (k.astype(LD) * _TWO_PI_LD / LUT_N).astype(float), ((k.astype(LD) + LD(0.5)) * _TWO_PI_LD / LUT_N).astype(float), k


@functools.lru_cache(None)
def sincos_inputs(op):
    """x [1, n] and, for the table routine, the slice of the exact multiples and their k.
    A routine with several ranges (dsincos_fast two, dsincos_hot and the table routine three) runs the 400 001-point grid of EACH range of
    tests/test_lane_emulation.py / tests/test_sincos_lut_host.py in the one case, up to 1.3 M lanes: the grids are those tests' own, and
    the whole GPU file takes 35 s with them (measured)."""
    lims = _SINCOS_RANGES[op]
    lim = max(lims)
    mult, ties, k = _lut_points()
    keep = np.abs(mult) <= lim
    special = np.array([0.0, -0.0, 1e-300, np.pi / 4, -np.pi / 2, min(lim, np.pi), lim, -lim, 50.0 if lim >= 50 else 1.0, -50.0 if lim >= 50 else -1.0])
    tk = ties[np.abs(ties) <= lim - 1e-9]
    x = np.concatenate([mult[keep], neighbours(mult[keep])[keep.sum():], neighbours(tk), special] + [np.linspace(-l, l, 400001) for l in lims])
    return x[None, :], int(keep.sum()), k[keep]


def _sincos_bar(op, x):
    if op.startswith("dsincos_lut"):
        return 5e-16 + 4e-17 * np.abs(x)
    if op == "dsincos_hot":
        return np.where(np.abs(x) <= 2 * np.pi + 0.05, 2e-15, 2e-15 + 4e-17 * np.abs(x))
    return np.full(x.shape, 2e-15)


def _check_sincos_values(op, x, s, c, report, label):
    require_wide_references()
    xl = x.astype(LD)
    d = np.maximum(np.abs(s.astype(LD) - np.sin(xl)), np.abs(c.astype(LD) - np.cos(xl))).astype(float)
    bar = _sincos_bar(op, x)
    worst = int(np.argmax(d / bar))
    unit = np.abs(s * s + c * c - 1.0).max()
    report("%s: %d points, max |error| %.3e, worst share of the bar %.3f at x = %r, max |s^2 + c^2 - 1| %.2e" % (label, x.size, d.max(), d[worst] / bar[worst], x[worst], unit))
    assert (d <= bar).all(), (op, x[worst], d[worst], bar[worst])
    assert unit <= (1e-15 if op.startswith("dsincos_lut") else 5e-15), (op, unit)
    return d.max(), d[worst] / bar[worst]


def check_sincos(op, out, report=print):
    (x,), _, _ = sincos_inputs(op)
    s, c = out
    zero = np.flatnonzero(x == 0.0)
    assert (s[zero] == 0.0).all() and (c[zero] == 1.0).all()
    return _check_sincos_values(op, x, s, c, report, op)


def _check_lut_index(x, r, idx):
    """The index is the k of x = k h + r, modulo 1024 (also for negative k), and |r| is at most half a step (plus the reduction's slack)."""
    assert np.array_equal(idx, np.floor(idx)) and (idx >= 0).all() and (idx < LUT_N).all()
    h = _TWO_PI_LD / LUT_N
    kk = (x.astype(LD) - r.astype(LD)) / h
    k = np.rint(kk)
    assert (np.abs(kk - k).astype(float) <= 1e-12 * (1.0 + np.abs(x))).all(), "x - r is no multiple of the table step"
    assert np.array_equal(np.mod(k.astype(np.int64), LUT_N), idx.astype(np.int64)), "index is not k mod 1024"
    assert (np.abs(r) <= np.pi / LUT_N + 1e-15 * (1.0 + np.abs(x))).all()


def check_lut1(out, report=print):
    (x,), n_mult, k = sincos_inputs("dsincos_lut1")
    s, c, r, idx = out
    fig = _check_sincos_values("dsincos_lut1", x, s, c, report, "dsincos_lut1")
    _check_lut_index(x, r, idx)
    assert np.array_equal(idx[:n_mult].astype(np.int64), np.mod(k, LUT_N))          # at a multiple itself: k mod 1024, negative k included
    assert (k < 0).any() and (np.mod(k[k < 0], LUT_N) != 0).any()
    assert (np.abs(r[:n_mult]) <= 4e-17 * np.abs(x[:n_mult]) + U52 * np.abs(x[:n_mult])).all()
    assert len(np.unique(idx)) == LUT_N
    zero = np.flatnonzero(x == 0.0)
    assert (s[zero] == 0.0).all() and (c[zero] == 1.0).all() and (idx[zero] == 0).all()
    return fig


@functools.lru_cache(None)
def lut7_inputs():
    """Seven angles per lane, each row the same points rolled by another offset: the angles of a lane sit in different regimes."""
    (x,), _, _ = sincos_inputs("dsincos_lut1")
    n_pts = x.size - 3 * 400001
    base = np.concatenate([x[:n_pts], x[n_pts::20]])
    return np.stack([np.roll(base, j * 9973) for j in range(7)])


def check_lut7(out, report=print):
    x = lut7_inputs()
    fig = (0.0, 0.0)
    for j in range(7):
        f = _check_sincos_values("dsincos_lut7", x[j], out[j], out[7 + j], (lambda *_: None) if j else report, "dsincos_lut7 (angle 0 of 7)")
        _check_lut_index(x[j], out[14 + j], out[21 + j])
        fig = max(fig, f, key=lambda t: t[1])
    # the same angle gives the same bits in whichever of the seven slots it stands
    for j in range(1, 7):
        for blk in range(4):
            assert np.array_equal(np.roll(out[7 * blk], j * 9973).view(np.uint64), out[7 * blk + j].view(np.uint64)), (j, blk)
    return fig


# ------------------------------------------------------------------------------------------------------------------------------
# log6 / Jlog6
# ------------------------------------------------------------------------------------------------------------------------------
LOG6_OPS = ("log6_inv", "log6_hot_bm", "log6_hot_c", "log6_hot_lean_c", "log6_hot_lean_bm")
# tests/test_log6_scalars_host.py
LOG6_REGIMES = [("zero", 0.0), ("switch_minus_ulp", np.nextafter(T13, 0.0)), ("switch", T13), ("switch_plus_ulp", np.nextafter(T13, 1.0)), ("1e-3", 1e-3), ("one", 1.0),
                ("pi_minus_1e-2", NEAR_PI), ("pi_minus_1e-9", np.pi - 1e-9), ("clamped", np.pi - 1e-9)]
LOG6_AXES = np.array([[1.0, 2.0, 3.0], [-2.0, 1.0, -1.5], [1.0, -1.0, 2.0]])
LOG6_PE = np.array([[0.3, -0.2, 0.4], [-0.05, 0.45, 0.1], [0.0, 0.0, 0.0]])
ZERO_COMPONENT_AXES = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 2.0], [1.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
N_SWEEP, N_SWEEP_AT_PI = 20000, 3000
N_TAYLOR_SWITCH = 3 * 9 + 8 * 3     # edge lanes built within [1 - 1e-8, 1 + 2e-6] of the Taylor threshold 2^-13: three regimes x 9, eight offsets x 3 axes (check_log6_front_ends)
_LOG6_BUILT_THETA = []    # the angle each edge lane was built with, filled by log6_inputs


@functools.lru_cache(None)
def log6_inputs():
    """x [12, n] in regime order -- the edge lanes (mpmath reference) first, then the 20 000-rotation sweep of
    tests/test_lane_emulation.py (longdouble reference) -- and: n_edge, zero [n], at_pi [n] (theta = pi exactly), axis [n, 3]."""
    Re, pe, axes, zero, thetas = [], [], [], [], []

    def add(theta, axis, p, clamped=False):
        R = rotation(axis, theta)
        if clamped:
            R[0, 0] -= 4.5e-16
            assert np.trace(R) <= -1.0
        Re.append(R.ravel()); pe.append(p); axes.append(np.asarray(axis, float) / np.linalg.norm(axis)); zero.append(theta == 0.0); thetas.append(theta)

    for name, theta in LOG6_REGIMES:
        for axis in LOG6_AXES:
            for p in LOG6_PE:
                add(theta, axis, p, name == "clamped")
    # either side of pi - 1e-2 (where the theta -> pi formula begins), of x = +-1/2 (the `mid` switch of the branch-free acos:
    # theta = pi / 3, 2 pi / 3) and of the Taylor threshold, with neighbours
    for centre in (NEAR_PI, np.pi / 3, 2 * np.pi / 3, T13):
        for d in (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6):
            for axis in LOG6_AXES:
                add(centre * (1.0 + d) if centre == T13 else centre + d, axis, LOG6_PE[0])
    for axis in ZERO_COMPONENT_AXES:
        for theta in (1e-3, 1.0, 2.0, 3.0, NEAR_PI - 1e-6):
            for p in LOG6_PE[:2]:
                add(theta, axis, p)
    n_edge = len(Re)
    rng = np.random.default_rng(5)
    n = N_SWEEP
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    theta = np.concatenate([rng.uniform(0.0, np.pi, n - 6000), np.pi - 10.0 ** rng.uniform(-16, -2, 3000), np.full(N_SWEEP_AT_PI, np.pi)])
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(theta)[:, None, None] * K + (1.0 - np.cos(theta))[:, None, None] * (K @ K)
    R[-1500:, 0, 0] -= 4.5e-16           # the last rotations by pi: the trace pushed to and below -1 (x clamps to -1 exactly)
    assert (np.trace(R[-1500:], axis1=1, axis2=2) <= -1.0).sum() > 500
    p = rng.uniform(-0.5, 0.5, (n, 3))
    x = np.concatenate([np.concatenate([np.array(Re), np.array(pe)], 1), np.concatenate([R.reshape(n, 9), p], 1)]).T
    at_pi = np.zeros(x.shape[1], bool)
    at_pi[-N_SWEEP_AT_PI:] = True
    _LOG6_BUILT_THETA[:] = list(thetas)
    return np.ascontiguousarray(x), n_edge, np.concatenate([zero, np.zeros(n, bool)]), at_pi, np.concatenate([np.array(axes), axis])


@functools.lru_cache(None)
def log6_reference():
    """e [n, 6], A, C, B = C A [n, 9] (float: rounded from the wide values) and theta [n]."""
    require_wide_references()
    x, n_edge, _, _, _ = log6_inputs()
    e, A, Cm, B, t = (a.astype(float) for a in ld_log6_and_jlog6_inv(x[:9].T, x[9:].T))
    for i in range(n_edge):
        e[i], A[i], Cm[i], B[i], t[i] = mp_log6_and_jlog6_inv(x[:9, i], x[9:, i])
    return e, A, Cm, B, t


def check_log6(op, out, report=print):
    x, n_edge, zero, at_pi, axis = log6_inputs()
    e_ref, A_ref, C_ref, B_ref, theta = log6_reference()
    out = out.T
    assert np.isfinite(out).all(), (op, np.argwhere(~np.isfinite(out))[:4])
    assert at_pi.sum() == N_SWEEP_AT_PI
    third = C_ref if op.endswith("_c") else B_ref
    ref = np.concatenate([e_ref, A_ref, third], 1)
    bar = np.where(theta >= NEAR_PI, BAR_NEAR_PI, BAR_LOG6)
    d = np.abs(out - ref).max(axis=1)
    worst = int(np.argmax(d / bar))
    report("%s: %d lanes, max |error| %.2e below pi - 1e-2, %.2e from there on; worst share of the bar %.3g (theta %.17g)" % (
        op, x.shape[1], d[theta < NEAR_PI].max(), d[theta >= NEAR_PI].max(), d[worst] / bar[worst], theta[worst]))
    assert (d <= bar).all(), (op, worst, d[worst], bar[worst], theta[worst])
    # AT pi: |w| = pi, and each component pi |n_k|.  The SIGNS of the components come from comparisons of the input's own entries
    # (R_21 > R_12, ...), noise at a rotation by pi: between two computations of the rotation log3 has several values there (DESIGN.md
    # section 5), but on the SAME nine doubles the wide reference takes the same signs, so these lanes are in the signed comparison
    # above as well (at the 1e-6 bar) and no lane is left out of it.
    w = out[at_pi, 3:6]
    assert np.abs(np.linalg.norm(w, axis=1) - np.pi).max() < 1e-7
    assert np.abs(np.abs(w) - np.pi * np.abs(axis[at_pi])).max() < 1e-6
    assert zero.sum() == 9
    assert np.array_equal(out[zero, 3:6], np.zeros((9, 3))) and np.array_equal(out[zero, 6:15], np.tile(np.eye(3).ravel(), (9, 1)))
    return d[theta < NEAR_PI].max(), (d / bar).max()


def check_log6_front_ends(outs, report=print):
    """outs: {op: out [24, n]}.  e, A and C A of every front end within 1e-12 (absolute) of log6_and_jlog6_inv's, on EVERY lane -- the
    sweep the bar was set on (tests/test_lane_emulation.py) and the edge lanes alike -- with one counted exception: the N_TAYLOR_SWITCH
    lanes built at the Taylor threshold 2^-13 (from 1e-8 below it, where the rounding of acos can still put theta above, to 2e-6 above).
    There the closed form of beta_dot = -2 / theta^4 + (...) cancels two terms of 2^53 down to 1 / 360: ONE half-ulp rounding of the
    leading term leaves (2 / theta^4) 2^-53 = 1 in beta_dot, which enters C through v3 u^T, v3 = beta_dot (u.p) u - theta^2 beta_dot p,
    |u| = theta, with at most 2 theta^3 |p| = 2^-51 |p| / theta per front end.  Those lanes are held to 1e-12 + 2 * 2^-51 |p| / theta
    (two front ends; 4.9e-12 at |p| = 0.54, and the plain 1e-12 where p = 0)."""
    x, n_edge, _, _, _ = log6_inputs()
    built = np.array(_LOG6_BUILT_THETA)
    switch = np.zeros(x.shape[1], bool)
    switch[:n_edge] = (built >= T13 * (1.0 - 1e-8)) & (built <= T13 * (1.0 + 2e-6))
    assert switch.sum() == N_TAYLOR_SWITCH, switch.sum()
    bar = np.full(x.shape[1], BAR_FRONT_ENDS)
    bar[switch] += 2.0 * 2.0 ** -51 * np.linalg.norm(x[9:, switch], axis=0) / T13
    base = outs["log6_inv"].T
    worst = 0.0
    for op in LOG6_OPS[1:]:
        o = outs[op].T
        third = o[:, 15:]
        if op.endswith("_c"):
            third = (o[:, 15:].reshape(-1, 3, 3) @ o[:, 6:15].reshape(-1, 3, 3)).reshape(-1, 9)
        d = np.abs(np.concatenate([o[:, :15], third], 1) - base).max(axis=1)
        report("%s against log6_inv: max |difference| %.2e on the sweep, %.2e on the edge lanes off the Taylor threshold, %.2e on the %d lanes at it" % (
            op, d[n_edge:].max(), d[:n_edge][~switch[:n_edge]].max(), d[switch].max(), switch.sum()))
        assert (d < bar).all(), (op, int(np.argmax(d / bar)), d[np.argmax(d / bar)])
        worst = max(worst, d[~switch].max())
    return worst


# ------------------------------------------------------------------------------------------------------------------------------
# solves
# ------------------------------------------------------------------------------------------------------------------------------
SOLVE_CASES = (1e-4, 1e-12, 100.0, "rank_deficient")
N_SYSTEMS = 64


@functools.lru_cache(None)
def solve_inputs(M):
    """x [M M + M, 4 * 64]: the four cases of tests/test_ldlt_solve_host.py, the same construction at M = 3."""
    cols = []
    for case in SOLVE_CASES:
        rng = np.random.default_rng(11)
        J = rng.normal(size=(N_SYSTEMS, M, 7))
        lam2 = case
        if case == "rank_deficient":
            J[:, :, 4] = J[:, :, 1]
            J[:, M // 2, :] = 0.0
            lam2 = 1e-4
        G = J @ J.transpose(0, 2, 1) + lam2 * np.eye(M)[None]
        G = 0.5 * (G + G.transpose(0, 2, 1))
        b = rng.normal(size=(N_SYSTEMS, M))
        cols.append(np.concatenate([G.reshape(N_SYSTEMS, M * M), b], 1))
    return np.ascontiguousarray(np.concatenate(cols).T)


def _solve_longdouble(G, b):
    """x with G x = b in longdouble: partial pivoting, then one refinement step (tests/test_ldlt_solve_host.py)."""
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
        x = np.zeros(n, LD)
        for k in range(n - 1, -1, -1):
            x[k] = (r[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
        return x
    Gl, bl = G.astype(LD), b.astype(LD)
    x = ge(Gl, bl)
    return x + ge(Gl, bl - Gl @ x)


@functools.lru_cache(None)
def solve_reference(M):
    require_wide_references()
    x = solve_inputs(M).T
    ref = np.array([_solve_longdouble(r[:M * M].reshape(M, M), r[M * M:]) for r in x])
    kappa = np.array([(lambda sv: sv[0] / sv[-1])(np.linalg.svd(r[:M * M].reshape(M, M), compute_uv=False)) for r in x])
    return ref, kappa


def check_solve(op, out, report=print):
    M = int(op[-1])
    ref, kappa = solve_reference(M)
    assert np.isfinite(out).all()
    err = (np.sqrt(((out.T.astype(LD) - ref) ** 2).sum(1)) / np.sqrt((ref ** 2).sum(1))).astype(float)
    ratio = err / (kappa * 2.0 ** -53)
    report("%s: worst err / (kappa 2^-53) per case %s" % (op, {str(c): "%.3g" % ratio[i * N_SYSTEMS:(i + 1) * N_SYSTEMS].max() for i, c in enumerate(SOLVE_CASES)}))
    assert (ratio <= SOLVE_FACTOR).all(), (op, ratio.max(), int(np.argmax(ratio)))
    return ratio.max(), ratio.max() / SOLVE_FACTOR


# ------------------------------------------------------------------------------------------------------------------------------
# log3, exp3, waypoints
# ------------------------------------------------------------------------------------------------------------------------------
LINE_AXES = np.array([[1.0, 2.0, 3.0], [-2.0, 1.0, -1.5], [1.0, -1.0, 2.0], [0.3, -0.7, 0.2], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
LINE_THETAS = [0.0, np.nextafter(T13, 0.0), T13, np.nextafter(T13, 1.0), 1e-9, 1.0, line_common.MAX_ROTATION, np.nextafter(NEAR_PI, 0.0), NEAR_PI, np.nextafter(NEAR_PI, 4.0),
               NEAR_PI - 1e-9, NEAR_PI + 1e-9, np.pi - 1e-9]


def log3_bar(theta):
    """The bar of a log3 entry (and of a waypoint built from it) at rotation angle theta: line_common.WAYPOINT_BAR, plus what the
    formula itself loses as theta approaches pi, and 1e-6 from pi - 1e-2 on.  log3 takes sin(theta) from sqrt((1 - x)(1 + x)) with
    x = (trace - 1) / 2 ROUNDED to double: the two additions of the trace and the subtraction leave |dx| <= 1.5 * 2^-53, which enters
    sin(theta) with the relative error dx / (2 (1 + x)) and w = theta / (2 sin theta) (R - R^T)^vee, |w| <= pi, with
    pi * 0.75 * 2^-53 / (1 + cos theta): 1.3e-15 at 2.5 rad, 5.2e-12 at pi - 1e-2.  The loss is in the double evaluation of the trace, the first step of
    the formula as the oracle has it too: an implementation that keeps the formula cannot be held to less there."""
    return np.where(theta >= NEAR_PI, BAR_NEAR_PI, line_common.WAYPOINT_BAR + np.pi * 0.75 * 2.0 ** -53 / np.maximum(1.0 + np.cos(theta), 1e-5))


@functools.lru_cache(None)
def log3_inputs():
    """x [9, n]: the edge angles x axes (mpmath reference), then 4000 random rotations up to 2.5 rad (longdouble reference); n_edge."""
    Rs = [rotation(a, t).ravel() for t in LINE_THETAS for a in (LINE_AXES if t < NEAR_PI - 1e-3 else LINE_AXES[:4])]
    rng = np.random.default_rng(17)
    axis, theta = rng.normal(size=(4000, 3)), rng.uniform(0.0, line_common.MAX_ROTATION, 4000)
    sweep = ld_exp3((axis / np.linalg.norm(axis, axis=1)[:, None]).astype(LD) * theta.astype(LD)[:, None]).astype(float).reshape(-1, 9)
    return np.ascontiguousarray(np.concatenate([np.array(Rs), sweep]).T), len(Rs)


@functools.lru_cache(None)
def log3_reference():
    require_wide_references()
    x, n_edge = log3_inputs()
    w, t = ld_log3(x.T.reshape(-1, 3, 3))
    w, t = w.astype(float), t.astype(float)
    for i in range(n_edge):
        R = _m(x[:, i])
        wi, ti = mp_log3([R[0:3], R[3:6], R[6:9]])
        w[i], t[i] = [float(a) for a in wi], float(ti)
    return w, t


def check_log3(out, report=print):
    w_ref, theta = log3_reference()
    assert np.isfinite(out).all()
    bar = log3_bar(theta)
    d = np.abs(out.T - w_ref).max(axis=1)
    worst = int(np.argmax(d / bar))
    assert (theta >= NEAR_PI).sum() >= 8 and (theta == 0.0).sum() >= 6
    report("log3: %d rotations, max |error| %.2e below pi - 1e-2 (bar %.2e), %.2e from there on" % (theta.size, d[theta < NEAR_PI].max(), line_common.WAYPOINT_BAR, d[theta >= NEAR_PI].max()))
    assert (d <= bar).all(), (worst, d[worst], theta[worst])
    return d[theta < NEAR_PI].max(), (d / bar).max()


@functools.lru_cache(None)
def exp3_inputs():
    """x [3, n]: theta axis for the edge angles (and the Taylor threshold as s theta reaches it for T = 3, 8), pi, 2 pi - 1e-3;
    then 4000 random vectors up to pi."""
    thetas = LINE_THETAS + [np.pi, 2 * np.pi - 1e-3] + [s * t for s in (1.0 / 3.0, 0.125) for t in (3 * T13, 8 * T13)] + list(neighbours(T13, 3))
    ws = [np.asarray(a) / np.linalg.norm(a) * t for t in thetas for a in LINE_AXES]
    rng = np.random.default_rng(18)
    axis, theta = rng.normal(size=(4000, 3)), rng.uniform(0.0, np.pi, 4000)
    return np.ascontiguousarray(np.concatenate([np.array(ws), axis / np.linalg.norm(axis, axis=1)[:, None] * theta[:, None]]).T), len(ws)


@functools.lru_cache(None)
def exp3_reference():
    require_wide_references()
    x, n_edge = exp3_inputs()
    R = ld_exp3(x.T).astype(float).reshape(-1, 9)
    for i in range(n_edge):
        E = mp_exp3(_m(x[:, i]))
        R[i] = [float(E[r][c]) for r in range(3) for c in range(3)]
    return R


def check_exp3(out, report=print):
    x, _ = exp3_inputs()
    assert np.isfinite(out).all()
    d = np.abs(out.T - exp3_reference()).max(axis=1)
    worst = int(np.argmax(d))
    report("exp3: %d vectors, max |error| %.2e (bar %.2e) at |w| = %.17g" % (d.size, d[worst], line_common.WAYPOINT_BAR, np.linalg.norm(x[:, worst])))
    zero = np.flatnonzero((x == 0).all(axis=0))
    assert zero.size >= 6 and np.array_equal(out[:, zero].T, np.tile(np.eye(3).ravel(), (zero.size, 1)))
    assert d[worst] <= line_common.WAYPOINT_BAR
    return d[worst], d[worst] / line_common.WAYPOINT_BAR


@functools.lru_cache(None)
def line_inputs(T):
    """x [24, n]: (from, goal) pairs.  The regimes of line_common.regime_goals -- theta = 0 (the start's own rotation bit for bit), 1e-9,
    s theta and theta at exp3's Taylor threshold, 2.5 rad, zero translation -- and the edge angles of LINE_THETAS, each from several start
    poses; then 600 random lines up to 2.5 rad."""
    rng = np.random.default_rng(19 + T)
    rows = []

    def add(theta, axis, zero_translation=False):
        a0 = rng.normal(size=3)
        R0 = rotation(a0, rng.uniform(0.1, 3.0))
        p0 = rng.uniform(-0.5, 0.5, 3)
        R1 = R0 if theta == 0.0 else (R0.astype(LD) @ ld_exp3(np.asarray(axis, LD) / np.sqrt(np.asarray(axis, LD) @ np.asarray(axis, LD)) * LD(theta))).astype(float)
        p1 = p0 if zero_translation else p0 + rng.uniform(-0.1, 0.1, 3)
        rows.append(np.concatenate([R0.ravel(), p0, R1.ravel(), p1]))

    for theta in LINE_THETAS + [T13 * T, 0.7]:
        for axis in LINE_AXES:
            add(theta, axis, zero_translation=(theta == 0.7))
    for _ in range(600):
        add(rng.uniform(0.0, line_common.MAX_ROTATION), rng.normal(size=3))
    return np.ascontiguousarray(np.array(rows).T)


@functools.lru_cache(None)
def line_reference(T):
    """[n, 3 + 12 T] and theta [n], in longdouble."""
    require_wide_references()
    x = line_inputs(T).T.astype(LD)
    R0, p0, R1, p1 = x[:, :9].reshape(-1, 3, 3), x[:, 9:12], x[:, 12:21].reshape(-1, 3, 3), x[:, 21:24]
    w, theta = ld_log3(np.einsum("nki,nkj->nij", R0, R1))
    cols = [w]
    for k in range(T):
        if k == T - 1:
            cols.append(x[:, 12:24])
        else:
            s = LD(k + 1) / LD(T)
            cols += [(R0 @ ld_exp3(s * w)).reshape(-1, 9), p0 + s * (p1 - p0)]
    return np.concatenate(cols, 1).astype(float), theta.astype(float)


def check_line(op, out, report=print):
    T = int(op[-1])
    ref, theta = line_reference(T)
    x = line_inputs(T)
    assert np.isfinite(out).all()
    bar = log3_bar(theta)
    d = np.abs(out.T - ref).max(axis=1)
    worst = int(np.argmax(d / bar))
    report("%s: %d lines, max |error| %.2e below pi - 1e-2 (bar %.2e), %.2e from there on" % (op, theta.size, d[theta < NEAR_PI].max(), line_common.WAYPOINT_BAR, d[theta >= NEAR_PI].max()))
    assert (theta >= NEAR_PI).sum() >= 12
    assert (d <= bar).all(), (op, worst, d[worst], theta[worst])
    assert np.array_equal(out[3 + 12 * (T - 1):].view(np.uint64), x[12:24].view(np.uint64)), "the last waypoint is the goal's own twelve values"
    return d[theta < NEAR_PI].max(), (d / bar).max()


# ------------------------------------------------------------------------------------------------------------------------------
# quat_to_R, freeflyer_integrate
# ------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_base_orientation.py: rotations ON the branch boundaries of the matrix -> quaternion conversion
SPECIAL_QUATS = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, -1], [np.sqrt(.5), np.sqrt(.5), 0, 0], [np.sqrt(.5), 0, np.sqrt(.5), 0],
                          [0, np.sqrt(.5), np.sqrt(.5), 0], [.5, .5, .5, .5], [.5, .5, .5, -.5], [np.sqrt(.5), 0, 0, np.sqrt(.5)], [0, np.sqrt(.5), 0, -np.sqrt(.5)]], dtype=float)


@functools.lru_cache(None)
def quat_inputs():
    rng = np.random.default_rng(21)
    q = rng.normal(size=(1500, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    q[500:1000] *= rng.uniform(0.9, 1.1, (500, 1))      # used as is, not normalised
    q = np.concatenate([SPECIAL_QUATS, q])
    return np.ascontiguousarray(np.concatenate([rng.uniform(-1, 1, (q.shape[0], 3)), q], 1).T)


@functools.lru_cache(None)
def quat_reference():
    require_wide_references()
    return np.array([[float(a) for row in mp_quat_to_R(_m(c[3:7])) for a in row] for c in quat_inputs().T])


def check_quat_to_R(out, report=print):
    d = np.abs(out.T - quat_reference()).max()
    report("quat_to_R: %d quaternions, max |error| %.2e (bar %.0e)" % (out.shape[1], d, BAR_FRAME))
    assert np.isfinite(out).all() and d <= BAR_FRAME
    return d, d / BAR_FRAME


def _quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions in longdouble."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], LD)


TWIST_ANGLES = [0.0, np.nextafter(T13, 0.0), T13, np.nextafter(T13, 1.0), 1.0, np.pi - 1e-9, np.pi, 2 * np.pi - 1e-3]
N_SIGN_FREE = 16     # lanes built with the converted quaternion (nearly) orthogonal to the previous one: compared up to sign


@functools.lru_cache(None)
def integrate_inputs():
    """x [13, n] (qb[7], v[6]) and sign_free [n].  Twist angles of TWIST_ANGLES about several axes; base orientations such that the
    RESULT lands on each branch of the conversion and on the boundaries (qb = target * exp(-omega)), plus random ones in both
    hemispheres (the sign flip is taken where the converted quaternion is antipodal to qb)."""
    rng = np.random.default_rng(22)
    rows, free = [], []
    dirs = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 2.0, 3.0], [-2.0, 1.0, -1.5], [1.0, -1.0, 2.0], [0.3, -0.7, 0.2], [1.0, 1.0, 0.0]])
    targets = np.concatenate([SPECIAL_QUATS, (lambda q: q / np.linalg.norm(q, axis=1)[:, None])(rng.normal(size=(8, 4)))])
    for t in TWIST_ANGLES:
        near_half_turn = abs(t - np.pi) < 1e-6
        for di, d in enumerate(dirs):
            om = (d / np.linalg.norm(d)).astype(LD) * LD(t)
            half = LD(t) / 2
            back = np.concatenate([-np.sin(half) * (d / np.linalg.norm(d)).astype(LD), [np.cos(half)]])      # exp(-omega) as a quaternion
            for ti, target in enumerate(targets):
                if near_half_turn and not (ti == 8 and di in (3, 4, 5, 6)) and not (ti == 3 and di in (0, 1, 2, 7)):
                    continue     # a turn by pi (to 1e-9) leaves the hemisphere open: only N_SIGN_FREE such lanes, counted below
                qb = _quat_mul(target.astype(LD), back)
                qb = (qb / np.sqrt(qb @ qb)).astype(float) * (1.0 if (ti + di) % 2 else -1.0)
                rows.append(np.concatenate([rng.uniform(-0.5, 0.5, 3), qb, rng.uniform(-0.1, 0.1, 3), om.astype(float)]))
                free.append(near_half_turn)
    for _ in range(600):
        q = rng.normal(size=4)
        rows.append(np.concatenate([rng.uniform(-0.5, 0.5, 3), q / np.linalg.norm(q), rng.uniform(-0.1, 0.1, 3), rng.uniform(-1.7, 1.7, 3)]))
        free.append(False)
    free = np.array(free)
    assert free.sum() == N_SIGN_FREE
    return np.ascontiguousarray(np.array(rows).T), free


@functools.lru_cache(None)
def integrate_reference():
    require_wide_references()
    x, _ = integrate_inputs()
    res = [mp_freeflyer_integrate(c[:7], c[7:]) for c in x.T]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def check_integrate(out, report=print):
    x, free = integrate_inputs()
    ref, dp = integrate_reference()
    out = out.T
    assert np.isfinite(out).all(), np.argwhere(~np.isfinite(out))[:4]      # also at zero twist, whose discarded arms divide by zero
    assert free.sum() == N_SIGN_FREE and (np.abs(dp[free]) < 1e-9).all() and (np.abs(dp[~free]) > 1e-6).all()
    d = np.abs(out - ref)
    flipped = np.abs(np.concatenate([out[:, :3], -out[:, 3:]], 1) - ref)
    d[free] = np.minimum(d[free].max(axis=1), flipped[free].max(axis=1))[:, None]
    worst = int(np.argmax(d.max(axis=1)))
    norm = np.abs(np.linalg.norm(out[:, 3:], axis=1) - 1.0).max()
    taken = (dp < 0).sum()
    report("freeflyer_integrate: %d lanes, max |error| %.2e (bar %.0e), max | |q| - 1 | %.2e, sign flip taken in %d lanes, %d compared up to sign" % (
        out.shape[0], d.max(), BAR_FRAME, norm, taken, free.sum()))
    assert taken > 100 and ((x[7 + 3:13] == 0).all(axis=0) & (x[7:10] != 0).any(axis=0)).sum() >= 100       # antipodal results; zero twist with v != 0
    assert d.max() <= BAR_FRAME, (worst, d[worst], x[:, worst])
    assert norm <= 1e-15
    return d.max(), d.max() / BAR_FRAME


# ------------------------------------------------------------------------------------------------------------------------------
# one entry per operation
# ------------------------------------------------------------------------------------------------------------------------------
def inputs(op):
    if op in ("drcp", "drsqrt", "dsqrt"):
        return scalar_inputs(op)[0]
    if op == "dfma3":
        return dfma3_inputs()
    if op == "dacos":
        return dacos_inputs()[0]
    if op == "dsincos_lut7":
        return lut7_inputs()
    if op in _SINCOS_RANGES:
        return sincos_inputs(op)[0]
    if op in LOG6_OPS:
        return log6_inputs()[0]
    if op in ("ldlt_solve3", "ldlt_solve6", "chol_solve6"):
        return solve_inputs(int(op[-1]))
    if op == "log3":
        return log3_inputs()[0]
    if op == "exp3":
        return exp3_inputs()[0]
    if op.startswith("line_t"):
        return line_inputs(int(op[-1]))
    if op == "quat_to_R":
        return quat_inputs()
    if op == "freeflyer_integrate":
        return integrate_inputs()[0]
    raise KeyError("no inputs for operation %r: the table has an operation this file does not know" % op)


def check(op, out, report=print):
    """Every bar of the operation on its outputs [n_out, n] for inputs(op).  -> (maximum error in the operation's own unit, share of the bar)."""
    if op in ("drcp", "drsqrt", "dsqrt"):
        return check_scalar(op, out, report)[:2]
    if op == "dfma3":
        return check_dfma3(out, report)
    if op == "dacos":
        return check_dacos(out, report)
    if op == "dsincos_lut1":
        return check_lut1(out, report)
    if op == "dsincos_lut7":
        return check_lut7(out, report)
    if op in _SINCOS_RANGES:
        return check_sincos(op, out, report)
    if op in LOG6_OPS:
        return check_log6(op, out, report)
    if op in ("ldlt_solve3", "ldlt_solve6", "chol_solve6"):
        return check_solve(op, out, report)
    if op == "log3":
        return check_log3(out, report)
    if op == "exp3":
        return check_exp3(out, report)
    if op.startswith("line_t"):
        return check_line(op, out, report)
    if op == "quat_to_R":
        return check_quat_to_R(out, report)
    if op == "freeflyer_integrate":
        return check_integrate(out, report)
    raise KeyError(op)


UNITS = {"drcp": "2^-52 rel", "drsqrt": "2^-52 rel", "dsqrt": "2^-52 rel", "dacos": "ulp", "ldlt_solve3": "kappa 2^-53", "ldlt_solve6": "kappa 2^-53", "chol_solve6": "kappa 2^-53"}


def bit_difference(a, b):
    """(share of values whose bits differ, largest difference in ulp of b) between two outputs [n_out, n] of the same inputs.  NaNs that
    both hold count as equal; an output below 1e-3 of its lane's largest (a matrix entry that is zero but for rounding) is measured in
    ulp of that size, not of its own."""
    both_nan = np.isnan(a) & np.isnan(b)
    differ = (a.view(np.uint64) != b.view(np.uint64)) & ~both_nan & ~((a == 0) & (b == 0))
    with np.errstate(all="ignore"):
        lane = np.nanmax(np.where(np.isfinite(b), np.abs(b), 0.0), axis=0, keepdims=True)
        u = np.abs(a - b) / np.spacing(np.maximum(np.maximum(np.abs(b), 1e-3 * lane), 2.0 ** -1022))
    u = np.where(differ & np.isfinite(u), u, 0.0)
    return differ.mean(), u.max()


def same_bits(a, b, fold_zero_sign=False):
    if fold_zero_sign:
        a, b = a + 0.0, b + 0.0
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))
