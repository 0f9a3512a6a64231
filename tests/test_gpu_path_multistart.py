"""ikgpu_dls_path_multistart_batch on the device: K starts per problem against the path's first pose, each start that entered followed
along the path behind it, the one that gets furthest returned -- with its trajectory from ONE further path launch.  The call is DEFINED
through existing calls (include/ikgpu.h), so the reference here is K x ik_amd.dls_batch from the columns of ik_amd.multistart_starts
against via 0, ik_amd.evaluate_batch(jacobian=False) for the errors, K x ik_amd.dls_path_batch from each result through the later vias,
and the key in numpy (tests/path_multistart_common.py select).  Asserted by np.array_equal: q_entry / entry_success / entry_iterations
against the single solve from start winner[b]; reached_all against the K path calls (-1 where the entry failed); winner and reached
wherever some start entered (the key is then made of exact integers); the trajectory against dls_path_batch from q_entry on the written
slabs of the problems that entered.  Where NO start entered the key is the error, which the scout evaluates in its own build's form
and evaluate_batch in the stage kernels': there the winner has the smallest reference error to 1e-10 in the norm, and err_sq is the
winner's reference error to 5e-11 in the norm everywhere (tests/multistart_common.py check_selection's two bars).  P = 1 is
dls_multistart_batch bit for bit, err_sq and winner included.  For every build of the chain kernel (dls_chain_path_multistart<...>),
K = 2 / 4 / 64, batch sizes around the wave boundary, three shapes, both layouts, generated and supplied starts, with and without the
trajectory and the optional outputs; a tree problem, a derived visitor and K = 3 run loop(...) in a workspace.

Classes on the device's own reference, recipe seed 1, B = 130, K = 4, (P, T) = (3, 6), the robot's max_joint_step -- no start enters /
winner complete / winner partial / winner != lowest converged / >= 2 entered starts tie on the best reached -- measured on an MI355X:
    ur5 (hot) 29 / 57 / 44 / 18 / 40        arm7 (hot-rtc) 15 / 63 / 52 / 31 / 58, (general) 17 / 62 / 51 / 32 / 59
    Cassie leg (hot and general) 0 / 33 / 97 / 2 / 130
(the CPU emulator: tests/test_path_multistart_emulation.py).  They are printed per case and held to the issue's floors
(tests/path_multistart_common.py check_conditions) before anything is compared."""
import ctypes as C

import numpy as np
import pytest

import line_common
import path_common
import path_multistart_common as PM
from test_gpu_track import CASES, FULL_BODY, DEMO, _problem, env

pytestmark = pytest.mark.gpu

SHAPES = [(1, 6), (2, 1), (3, 6)]
MAX_IT, TOL, SEED = 100, 1e-4, 1
NAMES = ("q_entry", "entry_success", "entry_iterations", "winner", "err_sq", "reached", "reached_all", "q", "success", "iterations")


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _rule(ik_amd, visitor=None):
    return visitor or ik_amd.inverse_kinematics_visitor(TOL), ik_amd.dls_parameters(max_iterations=MAX_IT)


_inputs = {}


def _draw(torch, case, B, P):
    """(Q0 [nq, B], vias [P, 1, 12, B]) on the device, SoA: the first B problems and the first P vias of the B = 130 draw."""
    if case[0] not in _inputs:
        _inputs[case[0]] = PM.inputs(_problem(case)[0], case[1], 130, SEED)
    q0, vias = _inputs[case[0]]
    return (torch.from_numpy(np.ascontiguousarray(q0[:B].T)).cuda(),
            torch.from_numpy(np.ascontiguousarray(vias[:P, :B].transpose(0, 2, 1)[:, None])).cuda())


def _aos(Q0, V, S=None):
    return Q0.t().contiguous(), V.permute(0, 3, 1, 2).contiguous(), None if S is None else S.permute(0, 2, 1).contiguous()


def _sentinels(torch, ik_amd, K, N, nq, B, layout, trajectory=True):
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    q_shape = (nq, B) if layout == "soa" else (B, nq)
    return ik_amd.api.PathMultistartResult(
        f(q_shape, float("nan"), torch.float64), f((B,), 7, torch.uint8), f((B,), -7, torch.int32), f((B,), -7, torch.int32),
        f((B,), float("nan"), torch.float64), f((B,), -7, torch.int32), f((K, B), -7, torch.int32),
        f((N,) + q_shape, float("nan"), torch.float64), f((N, B), 7, torch.uint8), f((N, B), -7, torch.int32))


def _host(r, layout):
    """The result as numpy, q_entry [B, nq] and q [N, B, nq] whatever the layout."""
    a = [None if t is None else t.cpu().numpy() for t in r]
    if layout == "soa":
        a[0] = np.ascontiguousarray(a[0].T)
        a[7] = None if a[7] is None else np.ascontiguousarray(a[7].transpose(0, 2, 1))
    return a


def _reference(torch, ik_amd, problem, data, Q0, gen, V, T, step, visitor=None):
    """The definition (SoA): per start the single solve against via 0, its error, the path call from its result; the key in numpy.
    Returns (singles, err_norm [K, n], winner, reached, reached_all)."""
    v, p = _rule(ik_amd, visitor)
    P = V.shape[0]
    N = (P - 1) * T
    singles, errs, reached_k = [], [], []
    for k in range(gen.shape[0] + 1):
        q, ok, it = ik_amd.dls_batch(problem, Q0 if k == 0 else gen[k - 1], V[0], data, v, p)
        e = ik_amd.evaluate_batch(problem, q, V[0], data, jacobian=False)
        e = e[0] if isinstance(e, tuple) else e
        errs.append(np.linalg.norm(e.cpu().numpy(), axis=0))
        if N > 0:
            reached_k.append(ik_amd.dls_path_batch(problem, q, V[1:].contiguous(), data, T, step, v, p)[3].cpu().numpy())
        else:
            reached_k.append(np.zeros(Q0.shape[1], np.int32))
        singles.append((q.t().cpu().numpy(), ok.cpu().numpy(), it.cpu().numpy()))
    errs = np.stack(errs)
    winner, reached, reached_all = PM.select(np.stack([s[1] for s in singles]), errs ** 2, np.stack(reached_k), N)
    return singles, errs, winner, reached, reached_all


def _check(torch, ik_amd, problem, data, got, ref, Q0, V, T, step, label, visitor=None):
    """got: _host() of a SoA call.  The assertions of the module docstring."""
    singles, errs, winner, reached, reached_all = ref
    q_entry, ok, it, win, err_sq, rch, rall, q, succ, its = got
    n, K = q_entry.shape[0], len(singles)
    N = (V.shape[0] - 1) * T
    rows = np.arange(n)
    assert win.min() >= 0 and win.max() < K, label
    for x, i, what in ((q_entry, 0, "q_entry"), (ok, 1, "entry_success"), (it, 2, "entry_iterations")):
        assert np.array_equal(x, np.stack([s[i] for s in singles])[win, rows]), label + (what,)
    assert np.array_equal(rall, reached_all), label
    some = (reached_all >= 0).any(axis=0)
    assert np.array_equal(win[some], winner[some]) and np.array_equal(ok.astype(bool), some), label
    assert np.array_equal(rch, np.maximum(reached_all[win, rows], 0)), label
    assert (errs[win, rows][~some][None, :] <= errs[:, ~some] + 1e-10).all(), label
    assert np.isfinite(err_sq).all() and (err_sq >= 0).all() and np.abs(np.sqrt(err_sq) - errs[win, rows]).max() <= 5e-11, label
    if q is not None and N > 0:
        v, p = _rule(ik_amd, visitor)
        Qe = torch.from_numpy(np.ascontiguousarray(q_entry.T)).cuda()
        pq, pok, pit, prch = ik_amd.dls_path_batch(problem, Qe, V[1:].contiguous(), data, T, step, v, p)
        pq, pok, pit, prch = pq.permute(0, 2, 1).cpu().numpy(), pok.cpu().numpy(), pit.cpu().numpy(), prch.cpu().numpy()
        entered = ok == 1
        assert np.array_equal(prch[entered], rch[entered]), label
        mask = line_common.written(rch, N) & entered[None, :]
        for x, y, what in ((q, pq, "q"), (succ, pok, "success"), (its, pit, "iterations")):
            assert np.array_equal(x[mask], y[mask]), label + (what,)


def _expected_name(data):
    assert data.kernel.startswith("dls_chain<"), data.kernel
    return "dls_chain_path_multistart" + data.kernel[len("dls_chain"):]


def _run(ik_amd, problem, data, Q0, V, T, step, K, layout="soa", starts=None, trajectory=True, out=None, visitor=None):
    v, p = _rule(ik_amd, visitor)
    return _host(ik_amd.dls_path_multistart_batch(problem, Q0, V, data, T, step, v, p, num_starts=K, seed=PM.START_SEED, starts=starts,
                                                  layout=layout, trajectory=trajectory, out=out), layout)


@pytest.mark.parametrize("K,B", [(2, 33), (2, 130), (4, 1), (4, 64), (4, 65), (4, 130), (64, 1), (64, 3)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_two_launches_equal_the_definition(torch_cuda, case, K, B):
    torch = torch_cuda
    import ik_amd
    model, problem, data, _, _ = _problem(case)
    if case[3] == "default" and case[2] == 2 and case[0] != "arm7":
        assert data.kernel.endswith(",hot>"), data.kernel
    if case[3] == "general" or case[2] != 2:
        assert data.kernel.endswith(",general>"), data.kernel
    v, p = _rule(ik_amd)
    assert ik_amd.dls_path_multistart_kernel(data, v, p, K) == _expected_name(data)
    robot_step = path_common.JOINT_STEP[case[0]]
    for P, T in SHAPES:
        N = (P - 1) * T
        Q0, V = _draw(torch, case, B, P)
        gen = ik_amd.multistart_starts(data, Q0, K, PM.START_SEED)
        for step in ((0.0, robot_step) if (K, B) in ((4, 130), (2, 33), (64, 3)) else (robot_step,)):
            label = (case, K, B, P, T, step)
            ref = _reference(torch, ik_amd, problem, data, Q0, gen, V, T, step)
            if (K, B, P, T) == (4, 130, 3, 6) and step > 0 and case[2] == 2:
                counts = PM.check_conditions(case[0], PM.classes(ref[4], ref[2], N))     # on the reference, before anything is compared
                print("%s: %s = %s" % (data.kernel, " / ".join(PM.CLASSES), " / ".join(map(str, counts))))
            got = _run(ik_amd, problem, data, Q0, V, T, step, K, out=_sentinels(torch, ik_amd, K, N, model.nq, B, "soa"))
            _check(torch, ik_amd, problem, data, got, ref, Q0, V, T, step, label)
            # slabs beyond the first waypoint that was not met keep their sentinel for the problems that entered
            if N > 0:
                untouched = ~line_common.written(got[5], N) & (got[1] == 1)[None, :]
                assert np.isnan(got[7][untouched]).all() and (got[8][untouched] == 7).all() and (got[9][untouched] == -7).all(), label
            # the other layout and the caller's starts: the same bits on every scout output and on the written trajectory
            q0a, va, ga = _aos(Q0, V, gen)
            mask = line_common.written(got[5], N) & (got[1] == 1)[None, :] if N > 0 else None
            for again in (_run(ik_amd, problem, data, q0a, va, T, step, K, "aos"), _run(ik_amd, problem, data, Q0, V, T, step, K, starts=gen),
                          _run(ik_amd, problem, data, q0a, va, T, step, K, "aos", starts=ga)):
                for x, y, what in zip(again[:7], got[:7], NAMES):
                    assert np.array_equal(x, y), label + (what,)
                if N > 0:
                    for x, y, what in zip(again[7:], got[7:], NAMES[7:]):
                        assert np.array_equal(x[mask], y[mask]), label + (what,)
            # trajectory=False: the scout alone, the same seven outputs, and nothing written into a sentinel-filled trajectory
            out = _sentinels(torch, ik_amd, K, N, model.nq, B, "soa")
            bare = _run(ik_amd, problem, data, Q0, V, T, step, K, trajectory=False, out=out)
            for x, y, what in zip(bare[:7], got[:7], NAMES):
                assert np.array_equal(x, y), label + (what,)
            assert torch.isnan(out.q).all() and (out.success == 7).all() and (out.iterations == -7).all(), label
        if P == 1:
            # P = 1 is dls_multistart_batch on via 0, bit for bit, and nothing is reached
            ms = ik_amd.dls_multistart_batch(problem, Q0, V[0], data, v, p, num_starts=K, seed=PM.START_SEED)
            got = _run(ik_amd, problem, data, Q0, V, T, robot_step, K)
            for x, y, what in zip(got[:5], _host(ms + (None,) * 5, "soa")[:5], NAMES):
                assert np.array_equal(x, y), (case, K, B, what)
            assert not got[5].any() and set(got[6].ravel().tolist()) <= {0, -1}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%s" % c)
def test_without_the_optional_outputs(torch_cuda, case):
    """Every output but q_entry NULL, then reached_all alone, then the trajectory without success / iters: straight through the C ABI."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import api, capi
    model, problem, data, _, _ = _problem(case)
    B, K, P, T = 65, 4, 3, 6
    N = (P - 1) * T
    step = path_common.JOINT_STEP[case[0]]
    Q0, V = _draw(torch, case, B, P)
    full = _run(ik_amd, problem, data, Q0, V, T, step, K)
    prm = api._params(*_rule(ik_amd))
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(q_entry, reached_all=None, q=None):
        capi.check(capi.lib().ikgpu_dls_path_multistart_batch(
            data._h, B, K, P, T, Q0.data_ptr(), None, PM.START_SEED, V.data_ptr(), C.byref(prm), step, q_entry.data_ptr(), None, None, None, None, None,
            ptr(reached_all), ptr(q), None, None, capi.SOA, None, 0, C.c_void_p(s)))
        torch.cuda.synchronize()
    qe = torch.full((model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
    call(qe)
    assert np.array_equal(qe.t().cpu().numpy(), full[0]), case
    qe.fill_(float("nan"))
    rall = torch.full((K, B), -7, dtype=torch.int32, device="cuda")
    q = torch.full((N, model.nq, B), float("nan"), dtype=torch.float64, device="cuda")
    call(qe, rall, q)
    mask = line_common.written(full[5], N) & (full[1] == 1)[None, :]
    assert np.array_equal(qe.t().cpu().numpy(), full[0]) and np.array_equal(rall.cpu().numpy(), full[6]), case
    assert np.array_equal(q.permute(0, 2, 1).cpu().numpy()[mask], full[7][mask]), case


def _workspace_call(torch, ik_amd, data, Q0, V, T, step, K, visitor, short, trajectory):
    """The call through the C ABI with a workspace `short` bytes smaller than asked for.  Returns (rc, message)."""
    from ik_amd import api, capi
    prm = api._params(*_rule(ik_amd, visitor))
    L = capi.lib()
    P, B = V.shape[0], Q0.shape[1]
    N = (P - 1) * T
    need = L.ikgpu_dls_path_multistart_workspace_bytes(data._h, B, K, P, T, C.byref(prm), 1 if trajectory else 0)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    qe = torch.empty((Q0.shape[0], B), dtype=torch.float64, device="cuda")
    q = torch.empty((N, Q0.shape[0], B), dtype=torch.float64, device="cuda") if trajectory else None
    rc = L.ikgpu_dls_path_multistart_batch(data._h, B, K, P, T, Q0.data_ptr(), None, PM.START_SEED, V.data_ptr(), C.byref(prm), step, qe.data_ptr(), None, None,
                                           None, None, None, None, None if q is None else q.data_ptr(), None, None, capi.SOA, ws.data_ptr(), need - short,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, L.ikgpu_last_error().decode()


@pytest.mark.parametrize("kind", ["tree", "derived_visitor", "three_starts"])
def test_other_cases_run_the_definition_inside_the_call(torch_cuda, kind):
    """A tree problem, a derived-visitor problem and K = 3 report loop(...), equal the same reference and refuse a workspace one byte short
    with the needed size and the sizing function's name."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import capi
    visitor, K = None, 4
    if kind == "tree":
        from test_gpu_generic import build
        B, P, T, step = 33, 3, 3, 0.25
        with env(IKGPU_TREE_STATIC_ROWS="0"):
            _, _, model, problem, data, _, _, q0, tg = build("cassie", True, FULL_BODY, B, seed=0)
        assert data.kernel == "dls_tree<NJ=7,chains=2,base_task>", data.kernel
        more = [build("cassie", True, FULL_BODY, B, seed=s)[8] for s in (1, 2)]
        Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
        V = torch.from_numpy(np.ascontiguousarray(np.stack([tg] + more).transpose(0, 2, 3, 1))).cuda()     # [P, 3, 12, B]
    else:
        B, P, T = 65, 3, 6
        step = path_common.JOINT_STEP["cassie_fixed"]
        model, problem, data, _, _ = _problem(CASES[0])
        Q0, V = _draw(torch, CASES[0], B, P)
        if kind == "derived_visitor":
            visitor = ik_amd.inverse_kinematics_visitor(TOL, step_tolerance=1e-3)
        else:
            K = 3
    N = (P - 1) * T
    v, p = _rule(ik_amd, visitor)
    assert ik_amd.dls_path_multistart_kernel(data, v, p, K) == "loop(%s)" % data.kernel
    gen = ik_amd.multistart_starts(data, Q0, K, PM.START_SEED)
    for s in (0.0, step):
        ref = _reference(torch, ik_amd, problem, data, Q0, gen, V, T, s, visitor)
        got = _run(ik_amd, problem, data, Q0, V, T, s, K, out=_sentinels(torch, ik_amd, K, N, model.nq, B, "soa"), visitor=visitor)
        _check(torch, ik_amd, problem, data, got, ref, Q0, V, T, s, (kind, s), visitor)
        q0a, va, _ = _aos(Q0, V)
        again = _run(ik_amd, problem, data, q0a, va, T, s, K, "aos", visitor=visitor)
        bare = _run(ik_amd, problem, data, Q0, V, T, s, K, trajectory=False, visitor=visitor)
        for x, y, z, what in zip(again[:7], got[:7], bare[:7], NAMES):
            assert np.array_equal(x, y) and np.array_equal(z, y), (kind, s, what)
    print("%s: reached_all values %s" % (kind, np.unique(got[6]).tolist()))
    for trajectory in (True, False):
        rc, msg = _workspace_call(torch, ik_amd, data, Q0, V, T, step, K, visitor, 0, trajectory)
        assert rc == capi.OK, msg
        rc, msg = _workspace_call(torch, ik_amd, data, Q0, V, T, step, K, visitor, 1, trajectory)
        assert rc == capi.ERR_INVALID and "workspace too small" in msg and "ikgpu_dls_path_multistart_workspace_bytes" in msg, msg


def test_a_pelvis_relative_task_is_refused(torch_cuda):
    """IKGPU_ERR_UNSUPPORTED for the demo task set's pelvis-relative foot task when P >= 2: the slot restriction is the path's.  P = 1
    is the multi-start call, which has no such restriction."""
    torch = torch_cuda
    import ik_amd
    from ik_amd import capi
    from test_gpu_generic import build
    B = 8
    _, _, model, problem, data, _, _, q0, tg = build("cassie", True, DEMO, B, seed=0)
    Q0 = torch.from_numpy(np.ascontiguousarray(q0.T)).cuda()
    V = torch.from_numpy(np.ascontiguousarray(np.stack([tg, tg]).transpose(0, 2, 3, 1))).cuda()
    with pytest.raises(capi.IkgpuError) as e:
        ik_amd.dls_path_multistart_batch(problem, Q0, V, data, 4, 0.5, num_starts=4)
    assert e.value.code == capi.ERR_UNSUPPORTED and "moves with the configuration" in e.value.message, e.value.message
    r = ik_amd.dls_path_multistart_batch(problem, Q0, V[:1].contiguous(), data, 4, 0.5, num_starts=2)
    torch.cuda.synchronize()
    assert not r.reached.any().item() and r.q.shape[0] == 0
