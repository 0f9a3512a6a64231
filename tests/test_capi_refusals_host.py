"""The refusal order of the C ABI's batch entry points (include/ikgpu.h, ik_amd/csrc/capi.cpp) is part of their contract: for every
call the return code and the text of ikgpu_last_error() are fixed, including WHICH of two simultaneous mistakes is reported, and
every refusal -- and the empty-batch no-op -- happens before the problem handle is read.  One row per rung of each entry point's
ladder, and for neighbouring rungs one call that breaks both and must report the earlier one.  The tracking, multi-start and
solution-set entries have their own files (test_track_host.py, test_multistart_host.py, test_solutions_host.py); this one covers
the rest.  No device is touched: the handle is 64 bytes of nothing, the "device pointers" are placeholders no refused call reads."""
import ctypes as C

import pytest

NULL_PROBLEM, NEG_BATCH, LAYOUT = "null problem", "negative batch size", "unknown layout"
NULL_PARAMS, NULL_ARG, TOO_LARGE = "params is null", "null argument", "batch too large for one launch"
MAX_ITER = "max_iterations must be >= 0"
DAMPING = "damping must be > 0: the device solves JJ^T + damping^2 I by Cholesky (SPD)"
STARTS = "the number of starts must be 1 .. 64"
MAX_LANES = (1 << 31) * 32   # lanes of the largest launch


@pytest.fixture(scope="module")
def abi(native_built):
    from ik_amd import capi

    class Abi:
        L = capi.lib()
        SOA, AOS, POSE7, OK, INVALID = capi.SOA, capi.AOS, capi.TARGETS_POSE7, capi.OK, capi.ERR_INVALID
        fake = C.cast(C.create_string_buffer(64), C.c_void_p)   # stands in for a problem: no refused call may read it
        buf = C.cast(C.create_string_buffer(64), C.c_void_p)    # stands in for a device pointer: never dereferenced
        dls, bad_dls, neg_dls = capi.DlsParams(), capi.DlsParams(), capi.DlsParams()
        pik, neg_pik = capi.PikParams(), capi.PikParams()

        def refused(self, rc, message):
            assert rc == self.INVALID and self.L.ikgpu_last_error().decode() == message, (rc, self.L.ikgpu_last_error().decode(), message)

    a = Abi()
    for prm in (a.dls, a.bad_dls, a.neg_dls):
        a.L.ikgpu_dls_params_default(C.byref(prm))
    a.bad_dls.damping = 0.0
    a.neg_dls.max_iterations = -1
    for prm in (a.pik, a.neg_pik):
        a.L.ikgpu_pik_params_default(C.byref(prm), 1)
    a.neg_pik.max_iterations = -1
    return a


def test_dls_solve_batch_refuses_in_order(abi):
    L, fake, buf, prm = abi.L, abi.fake, abi.buf, C.byref(abi.dls)

    def call(h, B, prm_, lay, q0=None, targets=None, q_out=None):
        return L.ikgpu_dls_solve_batch(h, B, q0, targets, prm_, q_out, None, None, lay, None)

    abi.refused(call(None, 4, prm, abi.SOA, buf, buf, buf), NULL_PROBLEM)
    abi.refused(call(None, -4, prm, abi.SOA, buf, buf, buf), NULL_PROBLEM)          # problem before batch
    abi.refused(call(fake, -4, prm, abi.SOA, buf, buf, buf), NEG_BATCH)
    abi.refused(call(fake, -4, prm, 7, buf, buf, buf), NEG_BATCH)                   # batch before layout
    abi.refused(call(fake, 4, prm, 7, buf, buf, buf), LAYOUT)
    abi.refused(call(fake, 4, prm, abi.SOA | abi.POSE7, buf, buf, buf), LAYOUT)     # (the pose flag belongs to the host entries)
    abi.refused(call(fake, 4, None, 7, buf, buf, buf), LAYOUT)                      # layout before params
    abi.refused(call(fake, 4, None, abi.AOS, buf, buf, buf), NULL_PARAMS)
    abi.refused(call(fake, 4, C.byref(abi.neg_dls), abi.AOS, buf, buf, buf), MAX_ITER)
    abi.refused(call(fake, 4, C.byref(abi.bad_dls), abi.AOS, buf, buf, buf), DAMPING)
    abi.refused(call(fake, 0, None, abi.SOA), NULL_PARAMS)                          # params before the empty batch
    abi.refused(call(fake, 0, C.byref(abi.bad_dls), abi.SOA), DAMPING)
    abi.refused(call(fake, 0, prm, 7), LAYOUT)
    assert call(fake, 0, prm, abi.SOA) == abi.OK and call(fake, 0, prm, abi.AOS) == abi.OK   # the empty batch before its null pointers
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        abi.refused(call(fake, 4, prm, abi.SOA, *args), NULL_ARG)
    abi.refused(call(fake, MAX_LANES + 1, prm, abi.SOA, None, buf, buf), NULL_ARG)  # null argument before the size
    abi.refused(call(fake, MAX_LANES + 1, prm, abi.SOA, buf, buf, buf), TOO_LARGE)


def test_multistart_starts_refuses_in_order(abi):
    L, fake, buf = abi.L, abi.fake, abi.buf
    call = lambda h, B, K, lay, q0=None, out=None: L.ikgpu_multistart_starts(h, B, K, q0, 0, out, lay, None)

    abi.refused(call(None, -4, 8, abi.SOA, buf, buf), NULL_PROBLEM)                 # problem before batch
    abi.refused(call(fake, -4, 8, abi.SOA, buf, buf), NEG_BATCH)
    abi.refused(call(fake, -4, 0, abi.SOA, buf, buf), NEG_BATCH)                    # batch before starts
    for K in (0, 65, -1):
        abi.refused(call(fake, 4, K, abi.SOA, buf, buf), STARTS)
    abi.refused(call(fake, 4, 0, 7, buf, buf), STARTS)                              # starts before layout
    abi.refused(call(fake, 4, 8, 7, buf, buf), LAYOUT)
    abi.refused(call(fake, 0, 8, 7), LAYOUT)                                        # layout before the no-ops
    abi.refused(call(fake, 4, 1, 7), LAYOUT)
    assert call(fake, 0, 8, abi.SOA) == abi.OK and call(fake, 4, 1, abi.AOS) == abi.OK   # the no-ops before their null pointers
    abi.refused(call(fake, 4, 8, abi.SOA, None, buf), NULL_ARG)
    abi.refused(call(fake, 4, 8, abi.SOA, buf, None), NULL_ARG)
    abi.refused(call(fake, MAX_LANES // 8 + 1, 8, abi.SOA, None, buf), NULL_ARG)    # null argument before the size
    abi.refused(call(fake, MAX_LANES // 8 + 1, 8, abi.SOA, buf, buf), TOO_LARGE)    # lanes = B x K
    abi.refused(call(fake, MAX_LANES // 64 + 1, 64, abi.AOS, buf, buf), TOO_LARGE)


def test_dls_solve_batch_host_refuses_in_order_with_the_layout_last(abi):
    L, fake, buf, prm = abi.L, abi.fake, abi.buf, C.byref(abi.dls)

    def call(h, B, prm_, lay, q0=None, targets=None, q_out=None):
        return L.ikgpu_dls_solve_batch_host(h, B, q0, targets, prm_, q_out, None, None, lay)

    abi.refused(call(None, -4, prm, abi.SOA, buf, buf, buf), NULL_PROBLEM)          # problem before batch
    abi.refused(call(fake, -4, prm, abi.SOA, buf, buf, buf), NEG_BATCH)
    abi.refused(call(fake, -4, None, abi.SOA, buf, buf, buf), NEG_BATCH)            # batch before params
    abi.refused(call(fake, 4, None, abi.SOA, buf, buf, buf), NULL_PARAMS)
    abi.refused(call(fake, 4, C.byref(abi.neg_dls), abi.SOA, buf, buf, buf), MAX_ITER)
    abi.refused(call(fake, 4, C.byref(abi.bad_dls), 7, buf, buf, buf), DAMPING)     # params before layout
    abi.refused(call(fake, 0, None, abi.SOA), NULL_PARAMS)                          # params before the empty batch
    # the empty batch comes before its null pointers AND before the layout: this entry looks at the layout last
    assert call(fake, 0, prm, abi.SOA) == abi.OK and call(fake, 0, prm, abi.AOS | abi.POSE7) == abi.OK
    assert call(fake, 0, prm, 7) == abi.OK
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        abi.refused(call(fake, 4, prm, abi.SOA, *args), NULL_ARG)
    abi.refused(call(fake, 4, prm, 7, None, buf, buf), NULL_ARG)                    # null argument before layout
    abi.refused(call(fake, 4, prm, 7, buf, buf, buf), LAYOUT)
    abi.refused(call(fake, 4, prm, 7 | abi.POSE7, buf, buf, buf), LAYOUT)           # (the pose flag is masked, the rest is not)


def test_pik_entries_refuse_before_the_problem_is_read(abi):
    # past "params is null" and a negative max_iterations the PIK parameter check reads the problem's levels: those rungs need a device
    L, fake, buf, prm = abi.L, abi.fake, abi.buf, C.byref(abi.pik)

    def dev(h, B, prm_, lay, q0=None, targets=None, q_out=None):
        return L.ikgpu_pik_solve_batch(h, B, q0, targets, prm_, q_out, None, None, lay, None)

    def host(h, B, prm_, lay, q0=None, targets=None, q_out=None):
        return L.ikgpu_pik_solve_batch_host(h, B, q0, targets, prm_, q_out, None, None, lay)

    abi.refused(dev(None, -4, prm, abi.SOA, buf, buf, buf), NULL_PROBLEM)           # problem before batch
    abi.refused(dev(None, 4, None, abi.SOA, buf, buf, buf), NULL_PROBLEM)           # ... and before params
    abi.refused(dev(fake, -4, prm, 7, buf, buf, buf), NEG_BATCH)                    # batch before layout
    abi.refused(dev(fake, 4, prm, 7, buf, buf, buf), LAYOUT)
    abi.refused(dev(fake, 4, prm, abi.SOA | abi.POSE7, buf, buf, buf), LAYOUT)
    abi.refused(dev(fake, 4, None, 7, buf, buf, buf), LAYOUT)                       # layout before params
    abi.refused(dev(fake, 0, prm, 7), LAYOUT)                                       # ... and before the empty batch
    abi.refused(dev(fake, 4, None, abi.AOS, buf, buf, buf), NULL_PARAMS)
    abi.refused(dev(fake, 0, None, abi.AOS), NULL_PARAMS)                           # params before the empty batch
    abi.refused(dev(fake, 0, C.byref(abi.neg_pik), abi.AOS), MAX_ITER)

    abi.refused(host(None, -4, prm, abi.SOA, buf, buf, buf), NULL_PROBLEM)          # problem before batch
    abi.refused(host(None, 4, None, abi.SOA, buf, buf, buf), NULL_PROBLEM)
    abi.refused(host(fake, -4, None, abi.SOA, buf, buf, buf), NEG_BATCH)            # batch before params
    abi.refused(host(fake, 4, None, 7, buf, buf, buf), NULL_PARAMS)                 # params before layout
    abi.refused(host(fake, 0, None, abi.SOA), NULL_PARAMS)                          # ... and before the empty batch
    abi.refused(host(fake, 4, C.byref(abi.neg_pik), 7), MAX_ITER)                   # ... and before the null pointers

    assert L.ikgpu_pik_kernel(None, prm) == b"" and L.ikgpu_pik_kernel(fake, None) == b""


def test_evaluate_and_fk_refuse_a_null_before_anything_else(abi):
    L, fake, buf = abi.L, abi.fake, abi.buf
    ev = lambda h, B, lay, q=buf, t=buf, e=buf, J=None: L.ikgpu_evaluate_batch(h, B, q, t, e, J, lay, None)
    fk = lambda h, B, lay, q=buf, o=buf: L.ikgpu_task_frames_fk_batch(h, B, q, o, lay, None)

    for args in ((None, 4, abi.SOA), (fake, 4, abi.SOA, None), (fake, 4, abi.SOA, buf, None), (fake, 4, abi.SOA, buf, buf, None)):
        abi.refused(ev(*args), NULL_ARG)
    abi.refused(ev(None, -4, 7), NULL_ARG)                                          # a null before batch
    abi.refused(ev(fake, 0, abi.SOA, None, None, None), NULL_ARG)                   # ... and before the empty batch: no null is excused
    abi.refused(ev(fake, -4, abi.SOA), NEG_BATCH)
    abi.refused(ev(fake, -4, 7), NEG_BATCH)                                         # batch before layout
    abi.refused(ev(fake, 4, 7), LAYOUT)
    abi.refused(ev(fake, 4, abi.SOA | abi.POSE7), LAYOUT)
    abi.refused(ev(fake, 0, 7), LAYOUT)                                             # layout before the empty batch
    assert ev(fake, 0, abi.SOA) == abi.OK and ev(fake, 0, abi.AOS, J=buf) == abi.OK   # (the Jacobian is optional)

    for args in ((None, 4, abi.SOA), (fake, 4, abi.SOA, None), (fake, 4, abi.SOA, buf, None)):
        abi.refused(fk(*args), NULL_ARG)
    abi.refused(fk(None, -4, 7), NULL_ARG)
    abi.refused(fk(fake, 0, abi.SOA, None, None), NULL_ARG)
    abi.refused(fk(fake, -4, abi.SOA), NEG_BATCH)
    abi.refused(fk(fake, -4, 7), NEG_BATCH)
    abi.refused(fk(fake, 4, 7), LAYOUT)
    abi.refused(fk(fake, 0, 7), LAYOUT)
    assert fk(fake, 0, abi.SOA) == abi.OK and fk(fake, 0, abi.AOS) == abi.OK


def test_targets_from_pose7_refuses_in_order(abi):
    L, buf = abi.L, abi.buf
    call = lambda B, ntasks, lay, pose7=buf, out=buf: L.ikgpu_targets_from_pose7(B, ntasks, pose7, out, lay, None)

    abi.refused(call(4, 2, abi.SOA, None), NULL_ARG)
    abi.refused(call(4, 2, abi.SOA, buf, None), NULL_ARG)
    abi.refused(call(-4, 2, abi.SOA, None), NULL_ARG)                               # a null before the sizes
    abi.refused(call(0, 2, abi.SOA, None, None), NULL_ARG)                          # ... and before the no-op
    abi.refused(call(-4, 2, abi.SOA), "negative size")
    abi.refused(call(4, -2, abi.SOA), "negative size")
    abi.refused(call(-4, 2, 7), "negative size")                                    # sizes before layout
    abi.refused(call(4, 2, 7), LAYOUT)
    abi.refused(call(4, 2, abi.SOA | abi.POSE7), LAYOUT)
    abi.refused(call(0, 2, 7), LAYOUT)                                              # layout before the no-ops
    abi.refused(call(4, 0, 7), LAYOUT)
    assert call(0, 2, abi.SOA) == abi.OK and call(4, 0, abi.AOS) == abi.OK and call(0, 0, abi.SOA) == abi.OK


def test_queries_answer_nothing_for_refused_arguments(abi):
    L, fake, prm = abi.L, abi.fake, C.byref(abi.dls)
    ms, sol = L.ikgpu_dls_multistart_workspace_bytes, L.ikgpu_dls_solutions_workspace_bytes
    for args in ((None, 4, 8, prm), (fake, 4, 8, None), (fake, 0, 8, prm), (fake, -4, 8, prm), (fake, 4, 0, prm), (fake, 4, 65, prm), (fake, 4, -1, prm)):
        assert ms(*args) == 0, args
    for args in ((None, 4, 8, 3, prm), (fake, 4, 8, 3, None), (fake, 0, 8, 3, prm), (fake, -4, 8, 3, prm), (fake, 4, 0, 1, prm), (fake, 4, 65, 3, prm),
                 (fake, 4, 8, 0, prm), (fake, 4, 8, 9, prm), (fake, 4, 8, -1, prm)):
        assert sol(*args) == 0, args
    assert L.ikgpu_problem_kernel(None) == b"" and L.ikgpu_problem_rows(None) == -1
    assert L.ikgpu_dls_track_kernel(None, prm) == b"" and L.ikgpu_dls_track_kernel(fake, None) == b""
    abi.refused(L.ikgpu_problem_support(None, abi.buf), "ikgpu_problem_support: null argument")
    abi.refused(L.ikgpu_problem_support(fake, None), "ikgpu_problem_support: null argument")
