"""The pass-through plan on the host (ik_amd/csrc/device/chain_kernel_body.hpp PassPlan, problem.cpp fill_pass_plan): the plan the host
builder makes for the four models of tests/pass_plan_common.py against q_in_chain and the limits, and the bodies that read it --
hot_pass_through_from, chain_pass_through_into, the general dls_chain_body, the hot program's hot_chain_body -- compiled with g++
(tests/pass_plan/pass_plan_shim.cpp) and run with and without the plan on the same inputs: equal bits, and the rows outside the chain
equal to the numpy rule bit for bit.  The shim once more as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import oracle as O
import pass_plan_common as PP

B = 67
CSRC = os.path.join(ROOT, "ik_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "pass_plan", "pass_plan_shim.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp", "device/chain_solver.hpp",
                                                "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def _compile(out, flags):
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out, SRC, os.path.join(CSRC, "model.cpp"),
                           os.path.join(CSRC, "problem.cpp")] + flags)


@pytest.fixture(scope="module")
def shim(native_built):
    out = os.path.join(ROOT, "tests", "pass_plan", "libpass_plan_shim.so")
    if _stale(out):
        _compile(out, ["-O2", "-fPIC", "-shared"])
    L = C.CDLL(out)
    L.pass_plan_last_error.restype = C.c_char_p
    assert L.pass_plan_max() == PP.PLAN_MAX
    return L


@pytest.fixture(scope="module", params=PP.CASES, ids=[c.name for c in PP.CASES])
def case(request):
    import ik_amd
    from ik_amd import capi
    c = request.param
    urdf = c.urdf().encode()
    model = ik_amd.Model.from_urdf_xml(urdf)
    fid = model.getFrameId(c.frame)
    q0, q_near, inside = PP.starts(model, c.frame, B, seed=11)
    tg = np.ascontiguousarray(O.fk_batch(O.OracleModel(model.flat()), q_near, [fid]).reshape(B, 12))
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    return dict(c=c, urdf=urdf, model=model, task=capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6)), q0=q0, tg=tg, inside=inside, lo=lo, hi=hi)


class env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("IKGPU_PASS_PLAN")
        os.environ.pop("IKGPU_PASS_PLAN", None) if self.value is None else os.environ.__setitem__("IKGPU_PASS_PLAN", self.value)

    def __exit__(self, *a):
        os.environ.pop("IKGPU_PASS_PLAN", None) if self.old is None else os.environ.__setitem__("IKGPU_PASS_PLAN", self.old)


def _plan(shim, k):
    state, nq, nj = C.c_int(-1), C.c_int(0), C.c_int(0)
    idx = np.full(PP.PLAN_MAX, -1, np.int32)
    lo, hi = np.full(PP.PLAN_MAX, np.nan), np.full(PP.PLAN_MAX, np.nan)
    in_chain, lower, upper = np.zeros(64, np.uint8), np.zeros(64), np.zeros(64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = shim.pass_plan_build(k["urdf"], C.c_size_t(len(k["urdf"])), C.byref(k["task"]), C.byref(state), p(idx), p(lo), p(hi), p(in_chain), p(lower),
                              p(upper), C.byref(nq), C.byref(nj))
    assert rc == 0, shim.pass_plan_last_error()
    n = nq.value
    return state.value, idx, lo, hi, in_chain[:n].astype(bool), lower[:n], upper[:n], nj.value


def test_the_host_builder_lists_the_entries_outside_the_chain(shim, case):
    c = case["c"]
    with env(None):
        state, idx, lo, hi, in_chain, lower, upper, nj = _plan(shim, case)
    assert nj == c.nj and np.array_equal(in_chain, case["inside"]) and np.array_equal(lower, case["lo"]) and np.array_equal(upper, case["hi"])
    outside = np.flatnonzero(~in_chain)
    assert outside.size == c.outside
    if c.outside > PP.PLAN_MAX:
        assert state == 0          # more entries than the plan holds: no plan
        return
    n = outside.size
    assert state == n + 1          # "a plan without entries" (UR5: 1) is not "no plan" (0)
    assert np.array_equal(idx[:n], outside)
    assert np.array_equal(PP.bits(lo[:n]), PP.bits(lower[outside])) and np.array_equal(PP.bits(hi[:n]), PP.bits(upper[outside]))
    # the spare slots: a copy of the last entry (entry 0 of q for a plan without entries) -- a valid address for a load of any slot
    last = outside[-1] if n else 0
    assert (idx[n:] == last).all() and (0 <= idx).all() and (idx < in_chain.size).all()
    if n:
        assert (lo[n:] == lower[last]).all() and (hi[n:] == upper[last]).all()


def test_the_switch_takes_the_plan_away(shim, case):
    with env("0"):
        assert _plan(shim, case)[0] == 0
    with env("1"):
        assert _plan(shim, case)[0] == (0 if case["c"].outside > PP.PLAN_MAX else case["c"].outside + 1)


def _run(shim, k, body, with_plan, layout, iterations=0, tol=-1.0, stepped=None):
    q0 = k["q0"] if layout == 1 else np.ascontiguousarray(k["q0"].T)
    tg = k["tg"] if layout == 1 else np.ascontiguousarray(k["tg"].T)
    q = np.full_like(q0, -7.0)
    ok, it = np.full(B, 9, np.uint8), np.full(B, -9, np.int32)
    st = np.zeros(B, np.uint8) if stepped is None else np.ascontiguousarray(stepped, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    with env(None):
        rc = shim.pass_plan_run(k["urdf"], C.c_size_t(len(k["urdf"])), C.byref(k["task"]), C.c_int(body), C.c_int(with_plan), C.c_int(layout),
                                C.c_int64(B), p(q0), p(tg), C.c_int(iterations), C.c_double(tol), p(st), p(q), p(ok), p(it))
    assert rc == 0, shim.pass_plan_last_error()
    return (q if layout == 1 else np.ascontiguousarray(q.T)), ok, it


@pytest.mark.parametrize("layout", [0, 1], ids=["soa", "aos"])
@pytest.mark.parametrize("body", [0, 1], ids=["hot_pass_through_from", "chain_pass_through_into"])
def test_the_copy_alone_with_and_without_the_plan(shim, case, body, layout):
    stepped = np.arange(B) % 3 != 0
    want = PP.outside_rule(case["q0"], case["lo"], case["hi"], stepped)
    out = ~case["inside"]
    got = [_run(shim, case, body, plan, layout, stepped=stepped)[0] for plan in (0, 1)]
    assert np.array_equal(PP.bits(got[0]), PP.bits(got[1]))
    assert np.array_equal(PP.bits(got[1][:, out]), PP.bits(want[:, out]))
    assert (got[1][:, ~out] == -7.0).all()                     # the chain's entries are not the copy's to write
    if out.any():                                             # the inputs show both rules: a clamp that moves a value, and no clamp
        beyond = (case["q0"] < case["lo"]) | (case["q0"] > case["hi"])
        assert beyond[stepped][:, out].any() and beyond[~stepped][:, out].any()
        assert np.array_equal(got[1][~stepped][:, out], case["q0"][~stepped][:, out])


# (iteration limit, squared tolerance): never-stop, and a stop rule loose enough that some problems stop at iteration 0
RULES = [(0, -1.0), (3, -1.0), (0, 1e-2), (3, 1e-2)]


@pytest.mark.parametrize("layout", [0, 1], ids=["soa", "aos"])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "%d-%g" % r)
@pytest.mark.parametrize("body", [2, 3], ids=["general", "hot"])
def test_whole_solves_with_and_without_the_plan(shim, case, body, rule, layout):
    if body == 3 and case["c"].name not in ("cassie_leg", "ur5"):
        return          # (the shim instantiates the hot program for the two structure codes the library is built with)
    got = [_run(shim, case, body, plan, layout, rule[0], rule[1]) for plan in (0, 1)]
    for x, y in zip(got[0], got[1]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    q, ok, it = got[1]
    out = ~case["inside"]
    want = PP.outside_rule(case["q0"], case["lo"], case["hi"], it > 0)
    assert np.array_equal(PP.bits(q[:, out]), PP.bits(want[:, out]))
    if rule == (3, 1e-2):
        assert (it == 0).any() and (it > 0).any()             # the stop rule is loose enough, and not too loose
    if rule[1] < 0:
        assert (it == rule[0]).all()


def test_stand_alone_under_the_host_sanitizers(native_built):
    """The shim as a program of its own (its main builds four models with a side branch of 0, 5, 16 and 17 joints, runs the three
    structure-free bodies with and without the plan and compares the bits), under -fsanitize=address,undefined."""
    out = os.path.join(ROOT, "tests", "pass_plan", "pass_plan_sanitized")
    if _stale(out):
        _compile(out, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPASS_PLAN_SHIM_MAIN"])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("equal bits") == 12 and "DIFFERENT" not in r.stdout, r.stdout
