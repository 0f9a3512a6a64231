"""The rank rule of ik::pik on the MI355X, on every form a handle can run: the compiled lane program (device/pik_solver.hpp
static_pik, the default), the cooperative interpreter (device/pik_coop.hpp, IKGPU_PIK_STATIC=0), the per-lane interpreter
(pik_level, plus IKGPU_GENERIC_KERNEL=lane; and whenever a lambda is 0) and the tree build (device/tree_solver.hpp PikRow).  Cases,
inputs (B = 130) and the acceptance rule are those of tests/pik_rank_common.py: every case is built so that keeping or dropping a
direction moves the answer by 1e-2 rad or more, every determined lane must be within 1e-8 rad of the _Float128 oracle.

ikgpu_pik_kernel names the two interpreter forms alike ("pik_generic<...>" without ",static"); which of them runs is the
environment's (kernels.hip pik_runs_cooperative), and the emulator tests run each on the same inputs."""
import numpy as np
import pytest

import pik_rank_common as R

pytestmark = pytest.mark.gpu

# form -> environment; the tree cases (two levels in the tree kernel's shape, no da) leave the tree kernel only when told to
FORMS = {
    "static": ({}, {"IKGPU_PIK_KERNEL": "static"}),
    "coop": ({"IKGPU_PIK_STATIC": "0"}, {"IKGPU_PIK_STATIC": "0", "IKGPU_PIK_KERNEL": "generic"}),
    "per_lane": ({"IKGPU_PIK_STATIC": "0", "IKGPU_GENERIC_KERNEL": "lane"},
                 {"IKGPU_PIK_STATIC": "0", "IKGPU_GENERIC_KERNEL": "lane", "IKGPU_PIK_KERNEL": "generic"}),
    "tree": ({}, {}),
}
_ENV = ("IKGPU_PIK_STATIC", "IKGPU_GENERIC_KERNEL", "IKGPU_PIK_KERNEL", "IKGPU_PIK_PROJECTOR")


@pytest.fixture(scope="module")
def torch_cuda(native_built):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_DATA = {}


def _data(inp):
    if inp.case not in _DATA:
        _DATA[inp.case] = inp.ik_amd.pik_data(inp.problem, device=0)
    return _DATA[inp.case]


def _set_form(monkeypatch, form, case):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form][1 if case in R.TREE_CASES else 0].items():
        monkeypatch.setenv(k, v)


def _assert_kernel(form, kernel):
    if form == "tree":
        assert kernel.startswith("dls_tree<NJ=7,chains=1") and kernel.endswith(",pik_levels=2>"), kernel
    elif form == "static":
        assert kernel.startswith("pik_generic<") and kernel.endswith(",static>"), kernel
    else:
        assert kernel.startswith("pik_generic<") and not kernel.endswith(",static>"), kernel


def _solve(torch, inp, form, prm_set, layout="soa"):
    iters, step, tol, lam, da = prm_set
    ik_amd, data = inp.ik_amd, _data(inp)
    data.lambda_ = list(lam)
    data.da = np.zeros(inp.nv) if da is None else np.asarray(da, float)
    _assert_kernel(form, data.kernel)
    if layout == "soa":
        Q0 = torch.from_numpy(np.ascontiguousarray(inp.q0.T)).cuda()
        T = torch.from_numpy(np.ascontiguousarray(inp.tg.transpose(1, 2, 0))).cuda()
    else:
        Q0, T = torch.from_numpy(np.ascontiguousarray(inp.q0)).cuda(), torch.from_numpy(np.ascontiguousarray(inp.tg)).cuda()
    return ik_amd.pik_batch(inp.problem, Q0, T, data, ik_amd.inverse_kinematics_visitor(tol),
                            ik_amd.pik_parameters(max_iterations=iters, step_length=step), layout=layout)


def _run_case(torch, case, form, sets=None):
    """Every parameter set under the acceptance rule, in the environment the caller has set; two calls and the array-of-structures
    layout give the same bits."""
    inp = R.inputs(case)
    out = []
    for prm_set in (inp.param_sets(tree=form == "tree") if sets is None else sets):
        Q, ok, it = _solve(torch, inp, form, prm_set)
        inp.check(form, prm_set, Q.cpu().numpy().T, ok.cpu().numpy(), it.cpu().numpy())
        Q2, ok2, it2 = _solve(torch, inp, form, prm_set)
        assert torch.equal(Q, Q2) and torch.equal(ok, ok2) and torch.equal(it, it2), (case, form, prm_set[0])
        Qa, oka, ita = _solve(torch, inp, form, prm_set, layout="aos")
        assert torch.equal(Q.T.contiguous(), Qa) and torch.equal(ok, oka) and torch.equal(it, ita), (case, form, prm_set[0])
        out.append(Q.cpu().numpy().T)
    return out


@pytest.mark.parametrize("form", ["static", "coop", "per_lane"])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_pik_forms_under_the_rank_rule(torch_cuda, monkeypatch, case, form):
    _set_form(monkeypatch, form, case)
    _run_case(torch_cuda, case, form)


@pytest.mark.parametrize("case", R.TREE_CASES)
def test_tree_build_under_the_rank_rule(torch_cuda, monkeypatch, case):
    """The PikRow basis (unpivoted Gram-Schmidt over the rows with a non-zero weight) keeps the foot row weighted 1e-12 and drops
    the one weighted 1e-19."""
    _set_form(monkeypatch, "tree", case)
    _run_case(torch_cuda, case, "tree")


def test_tree_build_zero_row_and_row_below_the_threshold_leave_the_same_answer(torch_cuda, monkeypatch):
    _set_form(monkeypatch, "tree", "tree_pos_w0")
    qa, qb = _run_case(torch_cuda, "tree_pos_w0", "tree"), _run_case(torch_cuda, "tree_pos_w1e-19", "tree")
    for k, prm_set in enumerate(R.inputs("tree_pos_w0").param_sets(tree=True)):
        R.same_answer("tree", prm_set, "tree_pos_w0", qa[k], "tree_pos_w1e-19", qb[k])


@pytest.mark.parametrize("form", ["static", "coop", "per_lane"])
def test_zero_row_and_row_below_the_threshold_leave_the_same_answer(torch_cuda, monkeypatch, form):
    a, b = R.inputs("pos_w0_then_ori"), R.inputs("pos_w1e-19_then_ori")
    _set_form(monkeypatch, form, a.case)
    qa, qb = _run_case(torch_cuda, a.case, form), _run_case(torch_cuda, b.case, form)
    for k, prm_set in enumerate(a.param_sets()):
        R.same_answer(form, prm_set, a.case, qa[k], b.case, qb[k])


@pytest.mark.parametrize("static_env", ["default", "IKGPU_PIK_STATIC=0"])
def test_lambda_zero_runs_the_per_lane_interpreter(torch_cuda, monkeypatch, static_env):
    """lambda = 0 on a level: the compiled and the cooperative program factor Jbar Jbar^T + lambda^2 I, so the call goes to the
    one-sided-Jacobi program whatever the environment prefers -- and must be the reference's undamped step, not merely finite."""
    inp = R.inputs("full_rank_control")
    _set_form(monkeypatch, "static" if static_env == "default" else "coop", inp.case)
    _run_case(torch_cuda, inp.case, "per_lane", sets=inp.lambda0_sets())
