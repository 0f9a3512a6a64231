"""Host-side contract of the solution-set entry points (include/ikgpu.h ikgpu_dls_solutions_batch, ikgpu_dls_solutions_workspace_bytes,
ikgpu_dls_solutions_kernel): declared, bound, exported; invalid calls are refused with a message before any device is touched; the
Python entry checks its arguments before anything else.  No compute call is made (there is no GPU here and the product has no CPU
path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_dls_solutions_batch", "ikgpu_dls_solutions_workspace_bytes", "ikgpu_dls_solutions_kernel")


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_solutions_symbols(native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
        # each comment block cites where the reference itself plans restarts
        before = header[:header.index(name + "(")]
        block = before[before.rindex("/*"):]
        assert re.search(r"dls\.cpp:10\b", block) and re.search(r":73\b", block) and re.search(r"dls\.hpp:27\b", block), name
    # the header says that a full turn apart is a different configuration
    before = header[:header.index("ikgpu_dls_solutions_batch(")]
    assert "full turn" in before[before.rindex("/*"):]
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # symbols are only added
    import ik_amd
    for name in ("dls_solutions_batch", "dls_solutions_kernel"):
        assert callable(getattr(ik_amd, name)), name
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_solutions_device" in mirror and "solutions_workspace_bytes" in mirror and "bool random_restart = false;" in mirror


def test_invalid_solutions_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)   # stands in for a device pointer: never dereferenced by a refused call

    def call(h, B, K, N, prm_, lay, q0=None, targets=None, q_sols=None, count=None, sep=0.1):
        return L.ikgpu_dls_solutions_batch(h, B, K, N, q0, None, 0, targets, prm_, C.c_double(sep), q_sols, count, None, None, lay, None, 0, None)

    assert call(None, 4, 8, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    ptrs = (buf, buf, buf, buf)
    for K in (0, 65, -1):
        assert call(fake, 4, K, 1, C.byref(prm), capi.SOA, *ptrs) == capi.ERR_INVALID and "starts" in err(), K
    for K, N in ((8, 0), (8, -2), (8, 9), (1, 2), (64, 65)):
        assert call(fake, 4, K, N, C.byref(prm), capi.SOA, *ptrs) == capi.ERR_INVALID and "solutions kept" in err(), (K, N)
    for sep in (-0.1, -0.0 - 1e-300, float("inf"), float("-inf"), float("nan")):
        assert call(fake, 4, 8, 3, C.byref(prm), capi.SOA, *ptrs, sep=sep) == capi.ERR_INVALID and "separation" in err(), sep
    assert call(fake, -4, 8, 3, C.byref(prm), capi.SOA, *ptrs) == capi.ERR_INVALID and "batch" in err()
    assert call(fake, 4, 8, 3, C.byref(prm), 7, *ptrs) == capi.ERR_INVALID and "layout" in err()
    assert call(fake, 4, 8, 3, None, capi.AOS, *ptrs) == capi.ERR_INVALID and "params" in err()
    for args in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):   # the last: a null count
        assert call(fake, 4, 8, 3, C.byref(prm), capi.SOA, *args) == capi.ERR_INVALID and "null argument" in err(), args
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert call(fake, 4, 8, 3, C.byref(bad), capi.SOA, *ptrs) == capi.ERR_INVALID and "damping" in err()
    # the never-stop visitor has no converged start by construction
    never = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(never))
    never.stop_sq_tol = -1.0
    assert call(fake, 4, 8, 3, C.byref(never), capi.SOA, *ptrs) == capi.ERR_INVALID and "never-stop" in err() and "stop rule" in err()
    assert call(fake, 0, 8, 3, C.byref(never), capi.SOA) == capi.ERR_INVALID and "never-stop" in err()
    # an empty batch is a no-op, its pointers may be null; sep == 0 and N == K are valid
    assert call(fake, 0, 8, 3, C.byref(prm), capi.SOA) == capi.OK
    assert call(fake, 0, 1, 1, C.byref(prm), capi.AOS, sep=0.0) == capi.OK
    assert call(fake, 0, 64, 64, C.byref(prm), capi.AOS) == capi.OK
    assert call(fake, 0, 8, 9, C.byref(prm), capi.AOS) == capi.ERR_INVALID   # ... but N is still checked

    assert L.ikgpu_dls_solutions_kernel(None, C.byref(prm), 8) == b"" and L.ikgpu_dls_solutions_kernel(fake, None, 8) == b""
    assert L.ikgpu_dls_solutions_workspace_bytes(None, 4, 8, 3, C.byref(prm)) == 0
    assert L.ikgpu_dls_solutions_workspace_bytes(fake, 0, 8, 3, C.byref(prm)) == 0
    assert L.ikgpu_dls_solutions_workspace_bytes(fake, 4, 0, 1, C.byref(prm)) == 0
    assert L.ikgpu_dls_solutions_workspace_bytes(fake, 4, 8, 9, C.byref(prm)) == 0


def test_python_entry_rejects_wrong_arguments_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, K = m.nq, 8, 4
    # data=None: an argument error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_t = {"soa": np.zeros((1, 12, B)), "aos": np.zeros((B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_t["soa"]), ("soa", ok_q["soa"], np.zeros((1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((12, B))),
             ("soa", ok_q["soa"], np.zeros((2, 12, B))), ("aos", ok_q["soa"], ok_t["aos"]), ("aos", ok_q["aos"], ok_t["soa"]),
             ("aos", np.zeros((B,)), ok_t["aos"]), ("soa", ok_q["soa"], np.zeros((1, 7, B)))]
    for layout, q, t in wrong:
        with pytest.raises(ValueError):
            ik.dls_solutions_batch(p, q, t, None, num_starts=K, layout=layout)
    for bad in (0, 65, -3, 2.0):
        with pytest.raises(ValueError):
            ik.dls_solutions_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=bad)
    for bad in (0, K + 1, -1, 2.0):
        with pytest.raises(ValueError):
            ik.dls_solutions_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, max_solutions=bad)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ik.dls_solutions_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, separation=bad)
    with pytest.raises(ValueError):   # starts of the wrong shape
        ik.dls_solutions_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, starts=np.zeros((K, nq, B)))
    with pytest.raises(KeyError):
        ik.dls_solutions_batch(p, ok_q["soa"], ok_t["soa"], None, layout="rows")
    # right shapes, but host arrays: this entry takes device tensors only (still before any device call)
    import torch
    for layout in ("soa", "aos"):
        with pytest.raises(TypeError):
            ik.dls_solutions_batch(p, ok_q[layout], ok_t[layout], None, layout=layout)
        with pytest.raises(TypeError):
            ik.dls_solutions_batch(p, torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_t[layout].shape, dtype=torch.float64), None,
                                   layout=layout)
