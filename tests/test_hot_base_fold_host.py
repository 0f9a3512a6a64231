"""The base placement folded into the target (ik_amd/csrc/device/chain_hot.hpp hot_fold_base, hot_evaluate<.., BASE_FOLDED>), on the
host: the lane program compiled with g++ (tests/hot_eval/hot_base_fold_shim.cpp, built here the way tests/test_hot_evaluate.py builds
its shim).  fMt = (Rz(q_0) P_1 ... P_NJ)^-1 (P_0^-1 oMt): the folded form evaluates on P_0^-1 oMt, formed once per target, and its
walk ends with joint 0's own rotation; hot_dls folds at entry and runs every iteration in that form.

Chains: Cassie's leg, UR5 and arm7 as they are; the chains of tests/hot_fold_common.py (run2_whole and run2_twice: the leader of a
folded run is joint 0; all of them: a general P_0 with all three translation components); and two of this file -- identity_base
(P_0 the identity, no translation: the fold is a copy) and shifted_base (identity rotation, all three translation components: the
fold is three subtractions).

Configurations: tests/test_hot_evaluate.py's five groups (uniform in the limits, every joint on each limit, at the target, a rotation
of pi - 1e-9 / 1e-6 / 1e-2 from the target, zero).

Bars.  Folded against unfolded, e and every entry of the columns: 1e-12 absolute -- the two forms differ by a handful of roundings of
O(1) quantities (the existing host test holds the unfolded form to 6.4e-12 of the oracle); a rotation by almost pi away (the band
pi - 1e-2 in which log3 takes its theta -> pi formula): tests/test_hot_evaluate.py's 1e-6.  Between the two, log3's regular formula
turns a rounding d of fMt into pi d / (2 sin^2 theta) of e (tests/hot_fold_common.py, conditioned): at theta = pi - 0.1 that is 160 d,
for the d = 3e-16 of a handful of roundings 5e-14, well inside 1e-12; from there to the band the bar follows the conditioning,
1e-12 sin^2(0.1) / sin^2 theta -- 1e-10 at pi - 1e-2, never 1e-6.  256 uniform draws on each of ten chains do land there (run2_middle:
one at pi - 0.0109, where the two forms are 4.7e-12 apart under a bar of 8.4e-11).  theta is the ORACLE's.
One full never-stop hot_dls of 0, 1, 7 and 50 iterations against the oracle, the chain's entries of q: tests/test_hot_evaluate.py's
bars, 1e-11 (no case of the solve is near pi).  The solves start uniform in the limits with the target the frame at
clip(q0 + U(-0.15, 0.15)), the project's "near" offset: there the DLS iteration contracts towards the solution and the roundings of
the two implementations are not amplified from step to step; from a far start the iterates of two correct implementations part ways
(tests/test_gpu_full_size.py has no lane-wise answer for those either), which no bar on q could tell from a mistake."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hot_fold_common as HF
import oracle as O
from test_hot_evaluate import BAR, BAR_NEAR_PI, _cases

FOLD_BAR = 1e-12
WELL = 0.1          # rad from pi up to which log3's regular formula is well conditioned (docstring)
ITERS = (0, 1, 7, 50)
NSOLVE = 64

MORE = [
    HF.Chain("arm7", "tool", None, None, None),
    HF.Chain("identity_base", "tool", [("0 0 0", "0 0 0", -2.6, 2.6), HF._j(HF.OBL[1], 2.2), HF._j(HF.OBL[2], 2.8)], HF.TOOL, None),
    HF.Chain("shifted_base", "tool", [("0 0 0", "0.11 -0.07 0.05", -2.6, 2.6), HF._j(HF.OBL[1], 2.2), HF._j(HF.OBL[2], 2.8)], HF.TOOL, None),
]
CHAINS = list(HF.CHAINS) + MORE


def _bars(theta):
    """Per configuration (see the docstring): FOLD_BAR up to pi - WELL, then along the conditioning of log3, BAR_NEAR_PI inside the band."""
    theta = np.asarray(theta, float)
    sin2 = np.where(theta > np.pi - WELL, np.maximum(np.sin(theta) ** 2, 1e-300), 1.0)
    return np.where(theta > np.pi - HF.NEAR_PI, BAR_NEAR_PI, FOLD_BAR * np.maximum(1.0, np.sin(WELL) ** 2 / sin2))


@pytest.fixture(scope="module")
def shim(native_built):
    src = os.path.join(ROOT, "tests", "hot_eval", "hot_base_fold_shim.cpp")
    out = os.path.join(ROOT, "tests", "hot_eval", "libhot_base_fold_shim.so")
    csrc = os.path.join(ROOT, "ik_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("model.cpp", "problem.cpp", "model.hpp", "problem.hpp", "device/lane_math.hpp",
                                                    "device/chain_solver.hpp", "device/chain_kernel_body.hpp", "device/chain_hot.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", out, src,
                               os.path.join(csrc, "model.cpp"), os.path.join(csrc, "problem.cpp")])
    L = C.CDLL(out)
    L.hot_base_fold_last_error.restype = C.c_char_p
    return L


def _run(shim, urdf, fid, q, tg, iterations):
    from ik_amd import capi
    n = q.shape[0]
    e, ef, q1 = np.empty((n, 6)), np.empty((n, 6)), np.empty_like(q)
    colbuf, colbuf_f = np.empty(n * 7 * 6), np.empty(n * 7 * 6)
    nj = C.c_int(0)
    task = capi.Task(fid, 0, 2, 0, (C.c_double * 6)(*[1.0] * 6))
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = shim.hot_base_fold_run(urdf, C.c_size_t(len(urdf)), C.byref(task), C.c_int64(n), p(q), p(tg), C.c_int(iterations), C.c_double(1e-4),
                                p(e), p(colbuf), p(ef), p(colbuf_f), p(q1), C.byref(nj))
    assert rc == 0, shim.hot_base_fold_last_error()
    k = n * nj.value * 6
    return e, colbuf[:k].reshape(n, nj.value, 6), ef, colbuf_f[:k].reshape(n, nj.value, 6), q1


@pytest.fixture(scope="module", params=CHAINS, ids=[c.name for c in CHAINS])
def chain(request, shim):
    """One chain: both forms of hot_evaluate on every configuration in ONE call, and what the solves need."""
    import ik_amd
    c = request.param
    urdf = HF.chain_xml(c).encode()
    model = ik_amd.Model.from_urdf_xml(urdf)
    om = O.OracleModel(model.flat())
    fid = model.getFrameId(c.frame)
    flat = model.flat()
    qidx, j = [], int(flat["frame_parent"][fid])
    while j > 0:
        qidx.insert(0, int(flat["idx_q"][j]))
        j = int(flat["parent"][j])
    cases = _cases(model, om, fid)
    q = np.ascontiguousarray(np.concatenate([k[1] for k in cases]))
    tg = np.ascontiguousarray(np.concatenate([k[2] for k in cases]))
    e, col, ef, colf, _ = _run(shim, urdf, fid, q, tg, 0)
    tasks = O.make_tasks([(fid, 0, 2, 0, None)])
    theta = np.array([np.linalg.norm(O.evaluate(om, tasks, tg[b], q[b])[0][3:]) for b in range(q.shape[0])])
    span, at = {}, 0
    for label, qc, _ in cases:
        span[label] = slice(at, at + qc.shape[0])
        at += qc.shape[0]
    return dict(chain=c, urdf=urdf, model=model, om=om, fid=fid, qidx=qidx, e=e, col=col, ef=ef, colf=colf, span=span, theta=theta)


@pytest.mark.parametrize("group", ["uniform", "on_limits", "at_target", "zero"])
def test_folded_form_matches_the_unfolded_one(chain, group):
    s = chain["span"][group]
    de, dc = np.abs(chain["ef"][s] - chain["e"][s]).max(axis=1), np.abs(chain["colf"][s] - chain["col"][s]).max(axis=(1, 2))
    bars = _bars(chain["theta"][s])
    wide = bars > FOLD_BAR
    print("%s %s: folded vs unfolded max |de| %.2e, max |dJ| %.2e over %d configurations; %d more beyond pi - %g (bar up to %.1e): %.2e, %.2e"
          % (chain["chain"].name, group, de[~wide].max(initial=0.0), dc[~wide].max(initial=0.0), (~wide).sum(), wide.sum(), WELL, bars.max(),
             de[wide].max(initial=0.0), dc[wide].max(initial=0.0)))
    assert np.isfinite(chain["ef"][s]).all() and np.isfinite(chain["colf"][s]).all()
    assert (de <= bars).all() and (dc <= bars).all(), (int(np.argmax(np.maximum(de, dc) / bars)), de.max(), dc.max())


def test_folded_form_a_rotation_by_almost_pi_from_the_target(chain):
    s = chain["span"]["near_pi"]
    de, dc = np.abs(chain["ef"][s] - chain["e"][s]).max(), np.abs(chain["colf"][s] - chain["col"][s]).max()
    print("%s near pi: folded vs unfolded max |de| %.2e, max |dJ| %.2e" % (chain["chain"].name, de, dc))
    assert np.isfinite(chain["ef"][s]).all() and np.isfinite(chain["colf"][s]).all()
    assert np.abs(np.linalg.norm(chain["e"][s][:, 3:], axis=1).max() - (np.pi - 1e-9)) < 1e-6      # the cases reach pi - 1e-9
    assert de <= BAR_NEAR_PI and dc <= BAR_NEAR_PI


def test_an_identity_base_placement_folds_to_a_copy(chain):
    """P_0 = identity: P_0^-1 oMt is oMt and neither form composes anything at joint 0 -- the same bits."""
    if chain["chain"].name != "identity_base":
        return
    assert np.array_equal(chain["ef"].view(np.uint64), chain["e"].view(np.uint64))
    assert np.array_equal(chain["colf"].view(np.uint64), chain["col"].view(np.uint64))


def test_full_solves_match_the_oracle(chain, shim):
    model, om, fid, qidx = chain["model"], chain["om"], chain["fid"], chain["qidx"]
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    rng = np.random.default_rng(50)
    q0 = rng.uniform(lo, hi, (NSOLVE, lo.size))
    tg = O.fk_batch(om, np.clip(q0 + rng.uniform(-0.15, 0.15, q0.shape), lo, hi), [fid])
    tasks = O.make_tasks([(fid, 0, 2, 0, None)])
    theta = np.array([np.linalg.norm(O.evaluate(om, tasks, tg[b], q0[b])[0][3:]) for b in range(NSOLVE)])
    assert theta.max() < 0.5 * np.pi      # no solve starts anywhere near the theta -> pi band
    for iters in ITERS:
        q_ref, _, _ = O.dls_batch(om, tasks, tg, q0, O.params(iters, 1e-2, 1.0, -1.0))
        q1 = _run(shim, chain["urdf"], fid, q0, tg, iters)[4]
        d = np.abs(q1 - q_ref)[:, qidx].max()
        print("%s %d iterations: max |dq| vs oracle %.2e" % (chain["chain"].name, iters, d))
        assert np.isfinite(q1).all()
        if iters == 0:
            assert np.array_equal(q1, q0)
        assert d <= BAR, (chain["chain"].name, iters, d)
