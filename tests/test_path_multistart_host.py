"""Host-side contract of the path multi-start entry points (include/ikgpu.h ikgpu_dls_path_multistart_batch /
ikgpu_dls_path_multistart_workspace_bytes / ikgpu_dls_path_multistart_kernel): declared, bound, exported; invalid calls are refused
with a message before any device is touched; the Python entry checks shapes, dtypes and host arrays before anything else.  No compute
call is made (there is no GPU here and the product has no CPU path).  The refusals that need a problem handle -- the slot restriction,
a workspace that is too short -- and the kernel names per problem kind are asserted by tests/test_gpu_path_multistart.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_dls_path_multistart_batch", "ikgpu_dls_path_multistart_workspace_bytes", "ikgpu_dls_path_multistart_kernel")
CITES = ["ik/ik/dls.cpp:10, :73", "ik/ik/dls.hpp:27", "ik/ik/dls.cpp:61-64,76-77", "ik_ros/src/cassie.cpp:92-113", "ikgpu_problem_support"]


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_symbols(ik, native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name) and getattr(capi.lib(), name).argtypes, name
    before = header[:header.index("ikgpu_dls_path_multistart_batch(")]
    comment = before[before.rindex("/*"):]
    for c in CITES:
        assert c in comment, c
    for name in ("dls_path_multistart_batch", "dls_path_multistart_kernel"):
        assert callable(getattr(ik, name)), name
    assert ik.api.PathMultistartResult._fields == ("q_entry", "entry_success", "entry_iterations", "winner", "err_sq", "reached", "reached_all",
                                                   "q", "success", "iterations")
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_path_multistart_device" in mirror and "dls_path_multistart_workspace_bytes" in mirror
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # symbols are only added


def test_invalid_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()

    def call(h, B, K, P, T, prm_=C.byref(prm), lay=capi.SOA, step=0.0):
        return L.ikgpu_dls_path_multistart_batch(h, B, K, P, T, None, None, 0, None, prm_, step, None, None, None, None, None, None, None, None, None,
                                                 None, lay, None, 0, None)
    assert call(None, 4, 4, 2, 3) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert call(fake, -4, 4, 2, 3) == capi.ERR_INVALID and "batch" in err()
    for K in (0, -1, 65, 1 << 20):
        assert call(fake, 4, K, 2, 3) == capi.ERR_INVALID and "starts" in err(), K
    for P in (0, -2):
        assert call(fake, 4, 4, P, 3) == capi.ERR_INVALID and "via poses" in err(), P
    assert call(fake, 4, 4, 2, -1) == capi.ERR_INVALID and "waypoints" in err()
    # (P - 1) x T beyond 31 bits, through either factor; the largest count passes and stops at the null pointers
    assert call(fake, 4, 4, (1 << 16) + 1, 1 << 15) == capi.ERR_INVALID and "too many waypoints" in err()
    assert call(fake, 4, 4, 3, 0x7fffffff) == capi.ERR_INVALID and "too many waypoints" in err()
    assert call(fake, 4, 4, 1 << 40, 1 << 40) == capi.ERR_INVALID and "too many waypoints" in err()
    assert call(fake, 4, 4, 2, 0x7fffffff) == capi.ERR_INVALID and "null argument" in err()
    assert call(fake, 4, 4, 1, 1 << 40) == capi.ERR_INVALID and "null argument" in err()      # P = 1: no waypoint, whatever T
    assert call(fake, 4, 4, 2, 3, lay=7) == capi.ERR_INVALID and "layout" in err()
    assert call(fake, 4, 4, 2, 3, prm_=None) == capi.ERR_INVALID and "params" in err()
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert call(fake, 4, 4, 2, 3, prm_=C.byref(bad)) == capi.ERR_INVALID and "damping" in err()
    for step in (float("nan"), float("inf"), -float("inf"), -0.5):
        assert call(fake, 4, 4, 2, 3, step=step) == capi.ERR_INVALID and "max_joint_step" in err(), step
        assert call(fake, 0, 4, 2, 3, step=step) == capi.ERR_INVALID and "max_joint_step" in err(), step
    never = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(never))
    never.stop_sq_tol = -1.0
    assert call(fake, 4, 4, 2, 3, prm_=C.byref(never)) == capi.ERR_INVALID and "never-stop" in err()
    assert call(fake, 0, 4, 1, 3, prm_=C.byref(never)) == capi.ERR_INVALID and "never-stop" in err()
    # an empty batch is a no-op, its pointers may be null; a non-empty one stops at the null pointers
    assert call(fake, 0, 4, 2, 3) == capi.OK and call(fake, 0, 1, 1, 0, lay=capi.AOS) == capi.OK
    assert call(fake, 4, 4, 2, 3) == capi.ERR_INVALID and "null argument" in err()
    assert L.ikgpu_dls_path_multistart_kernel(None, C.byref(prm), 4) == b"" and L.ikgpu_dls_path_multistart_kernel(fake, None, 4) == b""
    wb = L.ikgpu_dls_path_multistart_workspace_bytes
    assert wb(None, 4, 4, 2, 3, C.byref(prm), 1) == 0 and wb(fake, 4, 4, 2, 3, None, 1) == 0
    assert wb(fake, 0, 4, 2, 3, C.byref(prm), 1) == 0 and wb(fake, 4, 0, 2, 3, C.byref(prm), 0) == 0 and wb(fake, 4, 65, 2, 3, C.byref(prm), 0) == 0
    assert wb(fake, 4, 4, 0, 3, C.byref(prm), 1) == 0 and wb(fake, 4, 4, 2, -1, C.byref(prm), 1) == 0
    assert wb(fake, 4, 4, 1 << 40, 1 << 40, C.byref(prm), 1) == 0


def test_python_entry_rejects_wrong_arguments_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, P, T, K = m.nq, 8, 3, 5, 4
    # data=None: a shape error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_v = {"soa": np.zeros((P, 1, 12, B)), "aos": np.zeros((P, B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_v["soa"]), ("soa", ok_q["soa"], np.zeros((P, 1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((P, 2, 12, B))), ("aos", ok_q["soa"], ok_v["aos"]), ("aos", ok_q["aos"], ok_v["soa"]),
             ("aos", np.zeros((B,)), ok_v["aos"]), ("soa", ok_q["soa"], np.zeros((P, 1, 7, B))), ("soa", ok_q["soa"], np.zeros((0, 1, 12, B)))]
    entry = lambda q, v, layout, **kw: ik.dls_path_multistart_batch(p, q, v, None, T, 0.5, num_starts=K, layout=layout, **kw)
    import torch
    for layout, q, v in wrong:
        with pytest.raises(ValueError):
            entry(q, v, layout)
    with pytest.raises(KeyError):
        entry(ok_q["soa"], ok_v["soa"], "rows")
    for layout in ("soa", "aos"):
        # right shapes, but host arrays or host tensors: the entry takes device tensors only (still before any device call)
        with pytest.raises(TypeError):
            entry(ok_q[layout], ok_v[layout], layout)
        with pytest.raises(TypeError):
            entry(torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_v[layout].shape, dtype=torch.float64), layout)
        # a wrong shape of the caller's starts is a shape error, whatever the arrays are
        for shape in ((K,) + ok_q[layout].shape, (K - 1,) + ok_q[layout].shape[::-1], ok_q[layout].shape):
            with pytest.raises(ValueError):
                entry(ok_q[layout], ok_v[layout], layout, starts=np.zeros(shape))
    for bad_k in (0, 65, 2.0, None):
        with pytest.raises(ValueError):
            ik.dls_path_multistart_batch(p, ok_q["soa"], ok_v["soa"], None, T, num_starts=bad_k)
    with pytest.raises(ValueError):
        ik.dls_path_multistart_batch(p, ok_q["soa"], ok_v["soa"], None, -1)
    for step in (float("nan"), float("inf"), -0.1, "0.5"):
        with pytest.raises(ValueError):
            ik.dls_path_multistart_batch(p, ok_q["soa"], ok_v["soa"], None, T, step)
