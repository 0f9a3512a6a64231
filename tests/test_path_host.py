"""Host-side contract of the path entry points (include/ikgpu.h ikgpu_path_targets / ikgpu_dls_path_batch / ikgpu_dls_path_kernel /
ikgpu_dls_path_workspace_bytes): declared, bound, exported; invalid calls are refused with a message before any device is touched;
the Python entries check shapes and the joint-step bound before anything else.  No compute call is made (there is no GPU here and the
product has no CPU path); the name query is held here on null arguments only -- a chain, a tree and a derived-visitor problem need a
handle, which needs a device: tests/test_gpu_path.py asserts their three names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_path_targets", "ikgpu_dls_path_batch", "ikgpu_dls_path_workspace_bytes", "ikgpu_dls_path_kernel")


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_path_symbols(ik, native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name) and getattr(capi.lib(), name).argtypes, name
    # the definition cites what it stands in for: the caller's target sequence, the solve's stop test and failure report
    for name, cites in (("ikgpu_path_targets", ["ik_ros/src/cassie.cpp:92-113"]), ("ikgpu_dls_path_batch", ["ik/ik/dls.cpp:61-64,76-77", "ikgpu_problem_support"])):
        before = header[:header.index(name + "(")]
        comment = before[before.rindex("/*"):]
        for c in cites:
            assert c in comment, (name, c)
    for name in ("path_targets", "dls_path_kernel", "dls_path_batch"):
        assert callable(getattr(ik, name)), name
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_path_device" in mirror and "path_workspace_bytes" in mirror
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # symbols are only added


def test_invalid_path_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    solve = lambda h, B, P, T, prm_, lay, step=0.0: L.ikgpu_dls_path_batch(h, B, P, T, None, None, prm_, step, None, None, None, None, lay, None, 0, None)
    targets = lambda h, B, P, T, lay: L.ikgpu_path_targets(h, B, P, T, None, None, None, lay, None)
    assert solve(None, 4, 2, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    assert targets(None, 4, 2, 3, capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    for call in (lambda B, P, T, lay: solve(fake, B, P, T, C.byref(prm), lay), lambda B, P, T, lay: targets(fake, B, P, T, lay)):
        assert call(4, 2, -1, capi.SOA) == capi.ERR_INVALID and "waypoints" in err()
        assert call(-4, 2, 3, capi.SOA) == capi.ERR_INVALID and "batch" in err()
        assert call(4, 0, 3, capi.SOA) == capi.ERR_INVALID and "via poses" in err()
        assert call(4, -2, 3, capi.SOA) == capi.ERR_INVALID and "via poses" in err()
        assert call(4, 2, 3, 7) == capi.ERR_INVALID and "layout" in err()
        # P x T beyond 31 bits, through either factor
        assert call(4, 1 << 16, 1 << 15, capi.SOA) == capi.ERR_INVALID and "too many waypoints" in err()
        assert call(4, 3, 0x7fffffff, capi.SOA) == capi.ERR_INVALID and "too many waypoints" in err()
        assert call(4, 1 << 40, 1 << 40, capi.SOA) == capi.ERR_INVALID and "too many waypoints" in err()
        # nothing to do is a no-op, its pointers may be null; the largest count passes the size check and stops at the null pointers
        assert call(4, 2, 0, capi.SOA) == capi.OK and call(0, 2, 5, capi.AOS) == capi.OK
        assert call(4, 1, 0x7fffffff, capi.SOA) == capi.ERR_INVALID and "null argument" in err()
        assert call(4, 2, 3, capi.SOA) == capi.ERR_INVALID and "null argument" in err()
    assert solve(fake, 4, 2, 3, None, capi.AOS) == capi.ERR_INVALID and "params" in err()
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert solve(fake, 4, 2, 3, C.byref(bad), capi.SOA) == capi.ERR_INVALID and "damping" in err()
    # the joint-step bound: finite and not negative, whatever the sizes
    for step in (float("nan"), float("inf"), -float("inf"), -0.5):
        assert solve(fake, 4, 2, 3, C.byref(prm), capi.SOA, step) == capi.ERR_INVALID and "max_joint_step" in err(), step
        assert solve(fake, 0, 2, 3, C.byref(prm), capi.SOA, step) == capi.ERR_INVALID and "max_joint_step" in err(), step
    assert solve(fake, 4, 2, 0, C.byref(prm), capi.SOA, 0.5) == capi.OK and solve(fake, 4, 2, 0, C.byref(prm), capi.SOA, 0.0) == capi.OK
    # without a stop rule nothing is ever reached (as the line refuses it), whatever the sizes
    never = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(never))
    never.stop_sq_tol = -1.0
    assert solve(fake, 4, 2, 3, C.byref(never), capi.SOA) == capi.ERR_INVALID and "never-stop" in err()
    assert solve(fake, 0, 2, 3, C.byref(never), capi.SOA) == capi.ERR_INVALID and "never-stop" in err()
    assert L.ikgpu_dls_path_kernel(None, C.byref(prm)) == b"" and L.ikgpu_dls_path_kernel(fake, None) == b""
    wb = L.ikgpu_dls_path_workspace_bytes
    assert wb(None, 4, 2, 3, C.byref(prm)) == 0 and wb(fake, 4, 2, 3, None) == 0
    assert wb(fake, 0, 2, 3, C.byref(prm)) == 0 and wb(fake, 4, 2, 0, C.byref(prm)) == 0 and wb(fake, 4, 0, 3, C.byref(prm)) == 0
    assert wb(fake, 4, 1 << 40, 1 << 40, C.byref(prm)) == 0


def test_python_entries_reject_wrong_arguments_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, P, T = m.nq, 8, 3, 5
    # data=None: a shape error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_v = {"soa": np.zeros((P, 1, 12, B)), "aos": np.zeros((P, B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_v["soa"]), ("soa", ok_q["soa"], np.zeros((P, 1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((P, 2, 12, B))), ("aos", ok_q["soa"], ok_v["aos"]), ("aos", ok_q["aos"], ok_v["soa"]),
             ("aos", np.zeros((B,)), ok_v["aos"]), ("soa", ok_q["soa"], np.zeros((P, 1, 7, B))), ("soa", ok_q["soa"], np.zeros((0, 1, 12, B)))]
    entries = (lambda q, v, layout: ik.dls_path_batch(p, q, v, None, T, 0.5, layout=layout), lambda q, v, layout: ik.path_targets(p, q, v, None, T, layout=layout))
    import torch
    for entry in entries:
        for layout, q, v in wrong:
            with pytest.raises(ValueError):
                entry(q, v, layout)
        with pytest.raises(KeyError):
            entry(ok_q["soa"], ok_v["soa"], "rows")
        # right shapes, but host arrays: these entries take device tensors only (still before any device call)
        for layout in ("soa", "aos"):
            with pytest.raises(TypeError):
                entry(ok_q[layout], ok_v[layout], layout)
            with pytest.raises(TypeError):
                entry(torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_v[layout].shape, dtype=torch.float64), layout)
    with pytest.raises(ValueError):
        ik.dls_path_batch(p, ok_q["soa"], ok_v["soa"], None, -1)
    with pytest.raises(ValueError):
        ik.path_targets(p, ok_q["soa"], ok_v["soa"], None, -1)
    for step in (float("nan"), float("inf"), -0.1, "0.5"):
        with pytest.raises(ValueError):
            ik.dls_path_batch(p, ok_q["soa"], ok_v["soa"], None, T, step)
