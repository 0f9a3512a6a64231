"""The lane primitives on the device, one per launch, every lane placed on a switch of the primitive (tests/lane_probe_common.py), under
each of the product's three translation-unit recipes: `general` (kernels.hip, kernels_tree_refill.hip), `hot` (kernels_hot.hip and every
run-time compiled program) and `static` (the generated lane programs: IKD_CHOOSE becomes a select).  These are the arms behind
`#if IKD_ON_DEVICE` that no CPU test executes: the v_rcp_f64 / v_rsq_f64 seeds with their correction step, dsqrt's floor, the inline-asm
dfma3, the wave-uniform gates of the theta -> pi formula, IKD_CHOOSE as a branch or a select, the LDS staging of the sin / cos table.

Per operation and recipe ONE child process (tests/lane_math/lane_probe.hip, built by tests/lane_probe_common.py with the flags read
from the product) runs the input set in regime order -- whole waves in one regime --, under a fixed permutation that mixes the regimes
within every wave, and at n = 1, 63, 64, 65, 130 with the columns behind n of a NaN-filled output left untouched (the program checks that
itself: exit status 3).  Then:

  accuracy            every bar of tests/lane_probe_common.py, per recipe;
  lane independence   the permuted run, un-permuted, and the short runs are the bits of the ordered run: what a wave-uniform gate
                      (IKD_ANY(near_pi)), a select turned into a divergent branch or a store under a partial EXEC mask would break;
  recipes             log3, exp3, the waypoints and the dsincos_lut pieces are bit-identical across the three recipes (-0 mapped to +0);
                      for every other operation the largest difference is reported;
  host against device reported, not asserted: the share of outputs whose bits differ from the host shim's and the largest difference in
                      ulp -- the size of the gap the CPU emulators cannot see.

If a child is killed or exits non-zero, no further child is started in the session and every remaining case fails with that reason."""
import numpy as np
import pytest

import lane_probe_common as P

pytestmark = pytest.mark.gpu

OPS = P.op_names()


class _Runs:
    def __init__(self):
        self.host = P.build_host()
        self.table = P.parse_table(self.host.list())
        self.exe = {}
        self.cache = {}
        self.host_cache = {}
        self.dead = None          # why no further child process is started

    def device(self, variant, op):
        """(ordered, permuted (un-permuted again), {n: short run}) of one operation under one recipe, run once."""
        key = (variant, op)
        if key in self.cache:
            return self.cache[key]
        assert self.dead is None, "no probe process is started any more: %s" % self.dead
        if variant not in self.exe:
            self.exe[variant] = P.build_device(variant)
        x = P.inputs(op)
        perm = P.permutation(x.shape[1])
        try:
            outs = P.run_device(self.exe[variant], op, [x, x[:, perm]] + [x[:, :n] for n in P.SMALL_N], self.table)
        except RuntimeError as exc:
            self.dead = str(exc)
            raise AssertionError(self.dead)
        back = np.empty_like(outs[1])
        back[:, perm] = outs[1]
        self.cache[key] = (outs[0], back, dict(zip(P.SMALL_N, outs[2:])))
        return self.cache[key]

    def on_host(self, op):
        if op not in self.host_cache:
            self.host_cache[op] = P.run_host(self.host, op, P.inputs(op))
        return self.host_cache[op]


@pytest.fixture(scope="module")
def runs(native_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    P.require_wide_references()
    return _Runs()


@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("op", OPS)
def test_accuracy_on_the_device(runs, op, variant):
    out, _, _ = runs.device(variant, op)
    fig, share = P.check(op, out, report=lambda text: print("[%s] %s" % (variant, text)))
    differ, max_ulp = P.bit_difference(out, runs.on_host(op))
    print("LANE_PROBE %s %s max_error %.4g %s share_of_bar %.3f host_bits_differ %.4f host_max_ulp %.4g" % (op, variant, fig, P.UNITS.get(op, "abs").replace(" ", "_"), share, differ, max_ulp))


@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("op", OPS)
def test_lanes_do_not_depend_on_their_wave(runs, op, variant):
    out, back, short = runs.device(variant, op)
    assert P.same_bits(out, back), "%s [%s]: %d values change with the lanes that share the wave" % (op, variant, (out.view(np.uint64) != back.view(np.uint64)).sum())
    for n, o in short.items():
        assert o.shape[1] == n and P.same_bits(o, out[:, :n]), (op, variant, n)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_log6_front_ends_agree_on_the_device(runs, variant):
    P.check_log6_front_ends({op: runs.device(variant, op)[0] for op in P.LOG6_OPS}, report=lambda text: print("[%s] %s" % (variant, text)))


@pytest.mark.parametrize("op", OPS)
def test_recipes_against_each_other(runs, op):
    outs = {v: runs.device(v, op)[0] for v in P.VARIANTS}
    for v in P.VARIANTS[1:]:
        differ, max_ulp = P.bit_difference(outs[v], outs["general"])
        with np.errstate(all="ignore"):
            gap = np.nanmax(np.abs(outs[v] - outs["general"]))
        print("LANE_PROBE_RECIPES %s %s_against_general bits_differ %.4f max_ulp %.4g max_abs %.3g" % (op, v, differ, max_ulp, gap))
        if op in P.BIT_IDENTICAL_ACROSS_RECIPES:
            assert P.same_bits(outs[v], outs["general"], fold_zero_sign=True), (op, v, differ, max_ulp)


def test_what_the_square_root_family_returns_outside_its_range(runs):
    """Reported for DESIGN.md section 5, not barred: denormal in, denormal out, +-0."""
    for op in ("drcp", "drsqrt", "dsqrt"):
        for variant in P.VARIANTS:
            _, _, outside = P.check_scalar(op, runs.device(variant, op)[0], report=lambda text: None)
            print("LANE_PROBE_OUTSIDE %s %s %s" % (op, variant, outside))
