"""Host-side contract of the tracking entry points (include/ikgpu.h ikgpu_dls_track_batch / ikgpu_dls_track_kernel): declared,
bound, exported; invalid calls are refused with a message before any device is touched; the Python entry checks shapes before
anything else.  No compute call is made (there is no GPU here and the product has no CPU path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_tracking_symbols(native_built):
    from ik_amd import capi
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in ("ikgpu_dls_track_batch", "ikgpu_dls_track_kernel"):
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    # each stands in for the reference caller's own loop
    for name in ("ikgpu_dls_track_batch", "ikgpu_dls_track_kernel"):
        before = header[:header.index(name + "(")]
        assert "ik_ros/src/cassie.cpp:92-113" in before[before.rindex("/*"):], name
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # nothing existing changed


def test_invalid_tracking_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    call = lambda h, B, T, prm_, lay: L.ikgpu_dls_track_batch(h, B, T, None, None, prm_, None, None, None, lay, None)
    assert call(None, 4, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert call(fake, 4, -1, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "waypoints" in err()
    assert call(fake, -4, 3, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "batch" in err()
    assert call(fake, 4, 3, C.byref(prm), 7) == capi.ERR_INVALID and "layout" in err()
    assert call(fake, 4, 3, None, capi.AOS) == capi.ERR_INVALID and "params" in err()
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert call(fake, 4, 3, C.byref(bad), capi.SOA) == capi.ERR_INVALID and "damping" in err()
    # nothing to solve is a no-op, its pointers may be null
    assert call(fake, 4, 0, C.byref(prm), capi.SOA) == capi.OK
    assert call(fake, 0, 5, C.byref(prm), capi.AOS) == capi.OK
    assert L.ikgpu_dls_track_kernel(None, C.byref(prm)) == b"" and L.ikgpu_dls_track_kernel(fake, None) == b""


def test_python_entry_rejects_wrong_shapes_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, T = m.nq, 8, 5
    # data=None: a shape error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_t = {"soa": np.zeros((T, 1, 12, B)), "aos": np.zeros((T, B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_t["soa"]), ("soa", ok_q["soa"], np.zeros((T, 1, 12, B + 1))), ("soa", ok_q["soa"], np.zeros((1, 12, B))),
             ("soa", ok_q["soa"], np.zeros((T, 2, 12, B))), ("aos", ok_q["soa"], ok_t["aos"]), ("aos", ok_q["aos"], ok_t["soa"]),
             ("aos", np.zeros((B,)), ok_t["aos"]), ("soa", ok_q["soa"], np.zeros((T, 1, 7, B)))]
    for layout, q, t in wrong:
        with pytest.raises(ValueError):
            ik.dls_track_batch(p, q, t, None, layout=layout)
    with pytest.raises(KeyError):
        ik.dls_track_batch(p, ok_q["soa"], ok_t["soa"], None, layout="rows")
    # right shapes, but host arrays: this entry takes device tensors only (still before any device call)
    import torch
    for layout in ("soa", "aos"):
        with pytest.raises(TypeError):
            ik.dls_track_batch(p, ok_q[layout], ok_t[layout], None, layout=layout)
        with pytest.raises(TypeError):
            ik.dls_track_batch(p, torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_t[layout].shape, dtype=torch.float64), None, layout=layout)
