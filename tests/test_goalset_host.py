"""Host-side contract of the goal-set entry points (include/ikgpu.h ikgpu_dls_goalset_batch, ikgpu_dls_goalset_workspace_bytes,
ikgpu_dls_goalset_kernel): declared, bound, exported; invalid calls are refused with a message before any device is touched; the Python
entry checks its arguments before anything else.  No compute call is made (there is no GPU here and the product has no CPU path).  What
needs a real problem handle -- the workspace query of a fused and of a loop case, the refusal of a workspace that is too small -- is in
tests/test_gpu_goalset.py: creating a problem needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_dls_goalset_batch", "ikgpu_dls_goalset_workspace_bytes", "ikgpu_dls_goalset_kernel")


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_goalset_symbols(native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name) and getattr(capi.lib(), name).argtypes, name
    assert len(capi.lib().ikgpu_dls_goalset_batch.argtypes) == 20
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # symbols are only added, no struct changed
    import ik_amd
    for name in ("dls_goalset_batch", "dls_goalset_kernel"):
        assert callable(getattr(ik_amd, name)), name
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_goalset_device" in mirror and "goalset_workspace_bytes" in mirror


def test_invalid_goalset_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)   # stands in for a device pointer: never dereferenced by a refused call

    def call(h, B, G, K, prm_, lay, q0=None, goals=None, q_out=None):
        return L.ikgpu_dls_goalset_batch(h, B, G, K, q0, None, 0, goals, prm_, q_out, None, None, None, None, None, None, lay, None, 0, None)

    assert call(None, 4, 4, 2, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    for G in (0, -1, 65):
        assert call(fake, 4, G, 1, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "goals" in err(), G
    for K in (0, -1, 65):
        assert call(fake, 4, 1, K, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "starts" in err(), K
    for G, K in ((8, 16), (64, 2), (3, 22), (5, 13)):
        assert call(fake, 4, G, K, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "at most 64" in err(), (G, K)
    assert call(fake, -4, 4, 2, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "batch" in err()
    assert call(fake, -4, 0, 2, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "batch" in err()   # the batch before the sizes
    assert call(fake, 4, 4, 2, C.byref(prm), 7, buf, buf, buf) == capi.ERR_INVALID and "layout" in err()
    assert call(fake, 4, 0, 2, C.byref(prm), 7, buf, buf, buf) == capi.ERR_INVALID and "goals" in err()          # the sizes before the layout
    assert call(fake, 4, 4, 2, None, capi.AOS, buf, buf, buf) == capi.ERR_INVALID and "params" in err()
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert call(fake, 4, 4, 2, C.byref(prm), capi.SOA, *args) == capi.ERR_INVALID and "null argument" in err(), args
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert call(fake, 4, 4, 2, C.byref(bad), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "damping" in err()
    bad.damping, bad.max_iterations = 1e-2, -1
    assert call(fake, 4, 4, 2, C.byref(bad), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "max_iterations" in err()
    # an empty batch is a no-op, its pointers may be null
    assert call(fake, 0, 4, 2, C.byref(prm), capi.SOA) == capi.OK
    assert call(fake, 0, 1, 1, C.byref(prm), capi.AOS) == capi.OK
    assert call(fake, 0, 3, 5, C.byref(prm), capi.AOS) == capi.OK
    assert call(fake, 0, 0, 1, C.byref(prm), capi.AOS) == capi.ERR_INVALID   # ... but G and K are still checked
    assert call(fake, 0, 16, 8, C.byref(prm), capi.AOS) == capi.ERR_INVALID

    # the queries answer nothing for refused arguments, and never look at the handle then
    name, ws = L.ikgpu_dls_goalset_kernel, L.ikgpu_dls_goalset_workspace_bytes
    assert name(None, C.byref(prm), 4, 2) == b"" and name(fake, None, 4, 2) == b""
    for args in ((None, 4, 4, 2, C.byref(prm)), (fake, 4, 4, 2, None), (fake, 0, 4, 2, C.byref(prm)), (fake, -4, 4, 2, C.byref(prm)),
                 (fake, 4, 0, 2, C.byref(prm)), (fake, 4, 4, 0, C.byref(prm)), (fake, 4, 65, 1, C.byref(prm)), (fake, 4, 16, 8, C.byref(prm)),
                 (fake, 4, -1, 2, C.byref(prm))):
        assert ws(*args) == 0, args


def test_python_entry_rejects_wrong_arguments_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, G, K = m.nq, 8, 4, 2
    # data=None: an argument error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_g = {"soa": np.zeros((G, 1, 12, B)), "aos": np.zeros((G, B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_g["soa"]), ("soa", ok_q["soa"], np.zeros((G, 1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((G, 2, 12, B))), ("aos", ok_q["soa"], ok_g["aos"]), ("aos", ok_q["aos"], ok_g["soa"]),
             ("aos", np.zeros((B,)), ok_g["aos"]), ("soa", ok_q["soa"], np.zeros((G, 1, 7, B))), ("soa", ok_q["soa"], np.zeros((0, 1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((65, 1, 12, B))), ("soa", ok_q["soa"], np.zeros((G, 12, B)))]
    for layout, q, g in wrong:
        with pytest.raises(ValueError):
            ik.dls_goalset_batch(p, q, g, None, num_starts=K, layout=layout)
    for bad in (0, 65, -3, 2.0, 17):   # (17 x 4 goals > 64 candidates)
        with pytest.raises(ValueError):
            ik.dls_goalset_batch(p, ok_q["soa"], ok_g["soa"], None, num_starts=bad)
    with pytest.raises(ValueError):   # starts of the wrong shape
        ik.dls_goalset_batch(p, ok_q["soa"], ok_g["soa"], None, num_starts=K, starts=np.zeros((K, nq, B)))
    with pytest.raises(KeyError):
        ik.dls_goalset_batch(p, ok_q["soa"], ok_g["soa"], None, layout="rows")
    # right shapes, but host arrays: this entry takes device tensors only (still before any device call)
    import torch
    for layout in ("soa", "aos"):
        with pytest.raises(TypeError):
            ik.dls_goalset_batch(p, ok_q[layout], ok_g[layout], None, layout=layout)
        with pytest.raises(TypeError):
            ik.dls_goalset_batch(p, torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_g[layout].shape, dtype=torch.float64), None,
                                 num_starts=K, layout=layout)
