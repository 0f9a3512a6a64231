"""The lane primitives of ik_amd/csrc/device/{lane_math,line,tree_solver,chain_hot}.hpp one at a time, every lane placed on a switch of
the primitive, against references wider than double -- here through the HOST shim (tests/lane_math/lane_probe_host.cpp, g++), which
validates the inputs, the references and the bars of tests/lane_probe_common.py without a GPU.  tests/test_gpu_lane_probe.py then runs
the same checks on the arms only the device executes, under each of the product's three translation-unit recipes.

Also here: the wide restatements of the closed forms against the double oracle and oracle/twin.py (a wrong restatement must not pass for
a wide reference), the three device programs cross-compile for gfx950 with flag sets READ from the product's Makefile and rtc.cpp, and
the op table the host shim lists is the one the device programs list."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, urdf_path

import lane_probe_common as P
import oracle as O
import twin


@pytest.fixture(scope="module")
def shim():
    return P.build_host()


@pytest.fixture(scope="module")
def table(shim):
    return P.parse_table(shim.list())


@pytest.fixture(scope="module")
def outputs(shim, table):
    """Every operation through the host shim once, on demand."""
    cache = {}

    def get(op):
        if op not in cache:
            cache[op] = P.run_host(shim, op, P.inputs(op))
        return cache[op]
    return get


def test_every_operation_of_the_table_has_inputs_and_a_check(table):
    P.require_wide_references()
    assert sorted(table) == P.op_names()
    for op, (ni, no) in table.items():
        x = P.inputs(op)
        assert x.shape[0] == ni and np.isfinite(x).all(), op
    assert set(P.LOG6_OPS) <= set(table) and set(P.BIT_IDENTICAL_ACROSS_RECIPES) <= set(table)


@pytest.mark.parametrize("op", P.op_names())
def test_host_arms_meet_every_bar(outputs, op):
    P.check(op, outputs(op))


def test_log6_front_ends_agree(outputs):
    P.check_log6_front_ends({op: outputs(op) for op in P.LOG6_OPS})


def test_lanes_do_not_depend_on_their_neighbours(shim, outputs, table):
    """The property the device test is about, on the host (where it can only fail through the shim or the harness)."""
    for op in ("dacos", "log6_hot_lean_c", "freeflyer_integrate", "dsincos_lut7"):
        x = P.inputs(op)
        perm = P.permutation(x.shape[1])
        out = P.run_host(shim, op, x[:, perm])
        assert P.same_bits(out, outputs(op)[:, perm]), op


# ---- the wide restatements against the double oracle and the twin ----------------------------------------------------------------
def test_restatements_agree_with_the_oracle_and_the_twin(native_built):
    P.require_wide_references()
    rng = np.random.default_rng(3)
    worst = {}
    for _ in range(150):
        axis, theta = rng.normal(size=3), rng.choice([rng.uniform(0, 3.0), rng.uniform(0, 2e-4), 1e-9])
        R, p = P.rotation(axis, theta), rng.uniform(-0.5, 0.5, 3)
        e, A, Cm, B, t = P.mp_log6_and_jlog6_inv(R.ravel(), p)
        (el, Al, Cl, Bl, tl) = (a[0].astype(float) for a in P.ld_log6_and_jlog6_inv(R.ravel()[None], p[None]))
        Mi = np.concatenate([R.T.ravel(), -R.T @ p])
        Jo = O.Jlog6(Mi)
        Jt = twin.Jlog6(twin.se3(R.T, -R.T @ p))
        for name, a, b in (("log6 oracle", e, O.log6(np.concatenate([R.ravel(), p]))), ("log6 twin", e, twin.log6(twin.se3(R, p))), ("log6 longdouble", e, el),
                           ("A oracle", A, Jo[:3, :3].ravel()), ("A twin", A, Jt[3:, 3:].ravel()), ("A longdouble", A, Al), ("C longdouble", Cm, Cl),
                           ("C A oracle", B, Jo[:3, 3:].ravel()), ("C A twin", B, Jt[:3, 3:].ravel()), ("C A longdouble", B, Bl), ("theta longdouble", [t], [tl])):
            worst[name] = max(worst.get(name, 0.0), float(np.abs(np.asarray(a) - np.asarray(b)).max()))
        w = axis / np.linalg.norm(axis) * theta
        E = np.array([[float(a) for a in row] for row in P.mp_exp3(P._m(w))])
        nu = np.concatenate([p, w])
        E6, tr = P.mp_exp6(P._m(nu))
        M6 = O.exp6(nu)
        for name, a, b in (("exp3 twin", E, twin.exp3(w)), ("exp3 longdouble", E, P.ld_exp3(w).astype(float)),
                           ("exp6 oracle", np.concatenate([np.array([[float(a) for a in row] for row in E6]).ravel(), [float(a) for a in tr]]), M6),
                           ("exp6 twin", np.array([float(a) for a in tr]), twin.exp6(nu)[:3, 3])):
            worst[name] = max(worst.get(name, 0.0), float(np.abs(np.asarray(a) - np.asarray(b)).max()))
    print({k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) < 1e-12, worst


def test_integrate_restatement_agrees_with_the_oracle(native_built):
    import ik_amd
    P.require_wide_references()
    model = ik_amd.Model.from_urdf_file(urdf_path("cassie"), free_flyer=True)
    om = O.OracleModel(model.flat())
    x, free = P.integrate_inputs()
    ref, dp = P.integrate_reference()
    assert free.sum() == P.N_SIGN_FREE and (np.abs(dp[free]) < 1e-9).all() and (np.abs(dp[~free]) > 1e-6).all()
    q = np.zeros(model.nq)
    worst = 0.0
    for i in range(0, x.shape[1], 3):
        if free[i]:
            continue
        q[:7] = x[:7, i]
        v = np.zeros(model.nv)
        v[:6] = x[7:, i]
        worst = max(worst, np.abs(O.integrate(om, q, v)[:7] - ref[i]).max())
        R = twin.quat_to_matrix(*x[3:7, i])
        assert np.abs(np.array([[float(a) for a in row] for row in P.mp_quat_to_R(P._m(x[3:7, i]))]) - R).max() < 1e-15
    print("integrate: restatement against the oracle, max |difference| %.1e" % worst)
    assert worst < 1e-12


# ---- the device programs: recipes and table --------------------------------------------------------------------------------------
def test_flag_sets_are_the_products():
    f = P.flag_sets()
    assert f["general"] == ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=on"], f["general"]
    assert f["hot"] == f["general"] + ["-fno-signed-zeros", "-fno-honor-nans", "-fno-honor-infinities"]
    assert sorted(f["rtc"]) == sorted(f["hot"]), "the run-time compiler's flags are no longer the hot recipe"
    assert f["static"] == f["hot"] + ["-DIKD_STATIC_TABLES=1"]
    rtc = open(os.path.join(ROOT, "ik_amd", "csrc", "rtc.cpp")).read()
    assert "#define IKD_STATIC_TABLES 1" in rtc


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_device_program_cross_compiles_and_lists_the_same_table(shim, variant):
    exe = P.build_device(variant)
    assert os.access(exe, os.X_OK)
    listed = subprocess.run([exe, "--list"], timeout=120, capture_output=True, text=True)
    assert listed.returncode == 0, listed.stderr
    assert listed.stdout == shim.list().decode()
    src = open(os.path.join(P.LM, "lane_probe.hip")).read() + open(os.path.join(P.LM, "lane_probe_ops.hpp")).read()
    assert "IKD_HOT_LUT_FROM_HBM" not in src      # the table is read from LDS as the kernels read it: the staging is under test too
