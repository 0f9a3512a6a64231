"""Host-side contract of the pick entry points (include/ikgpu.h ikgpu_dls_pick_batch, ikgpu_dls_pick_workspace_bytes,
ikgpu_dls_pick_kernel): declared, bound, exported; the ABI version is still 2; the calls that can be refused without a device are
refused with a message before any device is touched; the Python entry checks its arguments before anything else.  No compute call is
made (there is no GPU here and the product has no CPU path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, urdf_path

SYMBOLS = ("ikgpu_dls_pick_batch", "ikgpu_dls_pick_workspace_bytes", "ikgpu_dls_pick_kernel")


@pytest.fixture(scope="module")
def ik(native_built):
    import ik_amd
    return ik_amd


def test_header_binding_and_library_agree_on_the_pick_symbols(native_built):
    from ik_amd import capi
    import ik_amd
    header = open(os.path.join(ROOT, "include", "ikgpu.h")).read()
    declared = set(re.findall(r"\b(ikgpu_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(native_built)
    for name in SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    m = re.search(r"typedef enum \{([^}]*)\} ikgpu_pick_rule;", header)
    assert m
    rules = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert rules == {"IKGPU_PICK_DISTANCE": 0, "IKGPU_PICK_MAX_DISTANCE": 1, "IKGPU_PICK_LIMIT_MARGIN": 2, "IKGPU_PICK_MANIPULABILITY": 3}
    assert {r.name: int(r) for r in ik_amd.PickRule} == {k[len("IKGPU_PICK_"):]: v for k, v in rules.items()}
    assert re.search(r"#define\s+IKGPU_ABI_VERSION\s+2\b", header)
    assert capi.lib().ikgpu_abi_version() == 2   # no struct changed
    for name in ("dls_pick_batch", "dls_pick_kernel", "PickRule"):
        assert callable(getattr(ik_amd, name)), name
    mirror = open(os.path.join(ROOT, "ik_amd", "csrc", "host", "ik", "ik_gpu.hpp")).read()
    assert "dls_pick_batch" in mirror and "pick_workspace_bytes" in mirror


def test_invalid_pick_calls_are_refused_before_any_device_is_touched(ik):
    from ik_amd import capi
    L = capi.lib()
    prm = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(prm))
    err = lambda: L.ikgpu_last_error().decode()
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)   # stands in for a device pointer: never dereferenced by a refused call

    def call(h, B, K, prm_, lay, q0=None, targets=None, q_out=None, rule=0):
        return L.ikgpu_dls_pick_batch(h, B, K, q0, None, 0, targets, prm_, rule, None, None, q_out, None, None, None, None, None, lay, None, 0, None)

    assert call(None, 4, 8, C.byref(prm), capi.SOA) == capi.ERR_INVALID and "null problem" in err()
    # the argument checks come before the handle is looked at: a placeholder stands in for a problem (creating one needs a device)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    for K in (0, 65, -1):
        assert call(fake, 4, K, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "starts" in err(), K
    for rule in (-1, 4, 99):
        assert call(fake, 4, 8, C.byref(prm), capi.SOA, buf, buf, buf, rule=rule) == capi.ERR_INVALID and "rule" in err(), rule
    assert call(fake, -4, 8, C.byref(prm), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "batch" in err()
    assert call(fake, 4, 8, C.byref(prm), 7, buf, buf, buf) == capi.ERR_INVALID and "layout" in err()
    assert call(fake, 4, 8, None, capi.AOS, buf, buf, buf) == capi.ERR_INVALID and "params" in err()
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert call(fake, 4, 8, C.byref(prm), capi.SOA, *args) == capi.ERR_INVALID and "null argument" in err(), args
    bad = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(bad))
    bad.damping = 0.0
    assert call(fake, 4, 8, C.byref(bad), capi.SOA, buf, buf, buf) == capi.ERR_INVALID and "damping" in err()
    # the never-stop visitor: no start converges, the rule could never act
    never = capi.DlsParams()
    L.ikgpu_dls_params_default(C.byref(never))
    never.stop_sq_tol = -1.0
    for rule in range(4):
        assert call(fake, 4, 8, C.byref(never), capi.SOA, buf, buf, buf, rule=rule) == capi.ERR_INVALID and "stop rule" in err(), rule
    assert call(fake, 0, 8, C.byref(never), capi.SOA) == capi.ERR_INVALID   # ... also for an empty batch
    # an empty batch is a no-op, its pointers may be null
    for rule in range(4):
        assert call(fake, 0, 8, C.byref(prm), capi.SOA, rule=rule) == capi.OK
    assert call(fake, 0, 1, C.byref(prm), capi.AOS) == capi.OK
    assert call(fake, 0, 0, C.byref(prm), capi.AOS) == capi.ERR_INVALID   # ... but K and the rule are still checked
    assert call(fake, 0, 8, C.byref(prm), capi.AOS, rule=4) == capi.ERR_INVALID

    assert L.ikgpu_dls_pick_kernel(None, C.byref(prm), 8, 0) == b"" and L.ikgpu_dls_pick_kernel(fake, None, 8, 0) == b""
    assert L.ikgpu_dls_pick_kernel(fake, C.byref(prm), 8, 4) == b"" and L.ikgpu_dls_pick_kernel(fake, C.byref(prm), 8, -1) == b""
    assert L.ikgpu_dls_pick_workspace_bytes(None, 4, 8, C.byref(prm)) == 0
    assert L.ikgpu_dls_pick_workspace_bytes(fake, 0, 8, C.byref(prm)) == 0
    assert L.ikgpu_dls_pick_workspace_bytes(fake, 4, 0, C.byref(prm)) == 0
    assert L.ikgpu_dls_pick_workspace_bytes(fake, 4, 65, C.byref(prm)) == 0


def test_python_entry_rejects_wrong_arguments_before_any_device_call(ik):
    m = ik.Model.from_urdf_file(urdf_path("cassie_fixed"))
    p = ik.InverseKinematicsProblem(m)
    p.add_frame_task("t", ik.FrameTask.create(m, "LeftFootFront"))
    nq, B, K = m.nq, 8, 4
    # data=None: an argument error must be raised before the workspace (a device handle) is looked at
    ok_q = {"soa": np.zeros((nq, B)), "aos": np.zeros((B, nq))}
    ok_t = {"soa": np.zeros((1, 12, B)), "aos": np.zeros((B, 1, 12))}
    wrong = [("soa", np.zeros((nq + 1, B)), ok_t["soa"]), ("soa", ok_q["soa"], np.zeros((1, 12, B + 1))), ("aos", ok_q["soa"], ok_t["aos"]),
             ("aos", np.zeros((B,)), ok_t["aos"])]
    for layout, q, t in wrong:
        with pytest.raises(ValueError):
            ik.dls_pick_batch(p, q, t, None, num_starts=K, layout=layout)
    for bad in (0, 65, -3, 2.0):
        with pytest.raises(ValueError):
            ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=bad)
    for bad in (4, -1, "closest"):
        with pytest.raises(ValueError):
            ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, rule=bad)
    with pytest.raises(ValueError):   # starts of the wrong shape
        ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, starts=np.zeros((K, nq, B)))
    with pytest.raises(ValueError):   # q_ref of the wrong shape
        ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, q_ref=np.zeros((B, nq)))
    with pytest.raises(ValueError):   # weights of the wrong length
        ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, num_starts=K, weights=[1.0] * (nq - 1))
    with pytest.raises(KeyError):
        ik.dls_pick_batch(p, ok_q["soa"], ok_t["soa"], None, layout="rows")
    # right shapes, but host arrays: this entry takes device tensors only (still before any device call)
    import torch
    for layout in ("soa", "aos"):
        with pytest.raises(TypeError):
            ik.dls_pick_batch(p, ok_q[layout], ok_t[layout], None, layout=layout, rule=ik.PickRule.LIMIT_MARGIN)
        with pytest.raises(TypeError):
            ik.dls_pick_batch(p, torch.zeros(ok_q[layout].shape, dtype=torch.float64), torch.zeros(ok_t[layout].shape, dtype=torch.float64), None,
                              layout=layout)
