"""Host-side contract of the line entry points (include/ikgpu.h ikgpu_line_targets / ikgpu_dls_line_batch / ikgpu_dls_line_kernel /
ikgpu_dls_line_workspace_bytes): declared, bound, exported; invalid calls are refused with a message before any device is touched;
the Python entries check shapes before anything else.  No compute call is made (there is no GPU here and the product has no CPU
path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_line_targets", "ikgpu_dls_line_batch", "ikgpu_dls_line_workspace_bytes", "ikgpu_dls_line_kernel")


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_line_symbols(ik, native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name) and getattr(capi.lib(), name).argtypes, name
    # the definition cites what it stands in for: the caller's target sequence, the solve's stop test and failure report
    for name, cites in (("ikgpu_line_targets", ["ik_ros/src/cassie.cpp:92-113"]), ("ikgpu_dls_line_batch", ["ik_ros/src/cassie.cpp:92-113", "ik/ik/dls.cpp:61-64,76-77"])):
        before = header[:header.index(name + "(")]
        comment = before[before.rindex("/*"):]
        for c in cites:
            assert c in comment, (name, c)
    for name in ("line_targets", "dls_line_kernel", "dls_line_batch"):
        assert callable(getattr(ik, name)), name
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_line_device" in mirror
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # nothing existing changed


def test_invalid_line_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    solve = lambda h, B, T, prm_, lay: L.ikgpu_dls_line_batch(h, B, T, None, None, prm_, None, None, None, None, lay, None, 0, None)
    targets = lambda h, B, T, lay: L.ikgpu_line_targets(h, B, T, None, None, None, lay, None)
    assert solve(None, 4, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    assert targets(None, 4, 3, capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert solve(fake, 4, -1, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "waypoints" in err()
    assert solve(fake, -4, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "batch" in err()
    assert solve(fake, 4, 3, C.byref(prm), 7) == capi.ERR_INVALID and "layout" in err()
    assert solve(fake, 4, 3, None, capi.AOS) == capi.ERR_INVALID and "params" in err()
    assert targets(fake, 4, -1, capi.SOA) == capi.ERR_INVALID and "waypoints" in err()
    assert targets(fake, -4, 3, capi.SOA) == capi.ERR_INVALID and "batch" in err()
    assert targets(fake, 4, 3, 7) == capi.ERR_INVALID and "layout" in err()
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert solve(fake, 4, 3, C.byref(bad), capi.SOA) == capi.ERR_INVALID and "damping" in err()
    # without a stop rule nothing is ever reached (as ikgpu_dls_solutions_batch refuses it), whatever the sizes
    never = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(never))
    never.stop_sq_tol = -1.0
    assert solve(fake, 4, 3, C.byref(never), capi.SOA) == capi.ERR_INVALID and "never-stop" in err()
    assert solve(fake, 0, 3, C.byref(never), capi.SOA) == capi.ERR_INVALID and "never-stop" in err()
    # nothing to solve is a no-op, its pointers may be null
    assert solve(fake, 4, 0, C.byref(prm), capi.SOA) == capi.OK
    assert solve(fake, 0, 5, C.byref(prm), capi.AOS) == capi.OK
    assert targets(fake, 4, 0, capi.SOA) == capi.OK and targets(fake, 0, 5, capi.AOS) == capi.OK
    assert L.ikgpu_dls_line_kernel(None, C.byref(prm)) == b"" and L.ikgpu_dls_line_kernel(fake, None) == b""
    assert L.ikgpu_dls_line_workspace_bytes(None, 4, 3, C.byref(prm)) == 0 and L.ikgpu_dls_line_workspace_bytes(fake, 4, 3, None) == 0
    assert L.ikgpu_dls_line_workspace_bytes(fake, 0, 3, C.byref(prm)) == 0 and L.ikgpu_dls_line_workspace_bytes(fake, 4, 0, C.byref(prm)) == 0


def test_python_entries_reject_wrong_shapes_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, T = m.nq, 8, 5
    # data=None: a shape error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_g = {"soa": np.zeros((1, 12, B)), "aos": np.zeros((B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_g["soa"]), ("soa", ok_q["soa"], np.zeros((1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((T, 1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((2, 12, B))), ("aos", ok_q["soa"], ok_g["aos"]), ("aos", ok_q["aos"], ok_g["soa"]),
             ("aos", np.zeros((B,)), ok_g["aos"]), ("soa", ok_q["soa"], np.zeros((1, 7, B)))]
    entries = (lambda q, g, layout: ik.dls_line_batch(p, q, g, None, T, layout=layout), lambda q, g, layout: ik.line_targets(p, q, g, None, T, layout=layout))
    for entry in entries:
        for layout, q, g in wrong:
            with pytest.raises(ValueError):
                entry(q, g, layout)
        with pytest.raises(KeyError):
            entry(ok_q["soa"], ok_g["soa"], "rows")
        with pytest.raises(ValueError):
            ik.dls_line_batch(p, ok_q["soa"], ok_g["soa"], None, -1)
        # right shapes, but host arrays: these entries take device tensors only (still before any device call)
        import torch
        for layout in ("soa", "aos"):
            with pytest.raises(TypeError):
                entry(ok_q[layout], ok_g[layout], layout)
            with pytest.raises(TypeError):
                entry(torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_g[layout].shape, dtype=torch.float64), layout)
