"""What the pass-through-plan tests share (tests/test_pass_plan_host.py on the CPU, tests/test_gpu_pass_plan.py on the device): the four
models, the starts whose entries outside the chain lie partly outside the limits, and the rule those entries follow.  No tests here.

The plan (ik_amd/csrc/device/chain_kernel_body.hpp PassPlan) carries the entries of q outside the chain and their limits in the kernel
arguments; it holds PLAN_MAX = 16 of them.

  cassie_leg   cassie_fixed, LeftFootFront: NJ = 7, 9 of 16 entries outside the chain
  tarsus       cassie_fixed, lefttarsus:    NJ = 6, 10 of 16 outside
  ur5          ur5, tool0:                  NJ = 6, none outside (a plan without entries)
  wide         a fixed base, three joints to `tool` and a side branch of 17 joints the chain does not take: NJ = 3, 17 of 20 outside --
               one more than the plan holds, so the bodies walk the tables in HBM (the fallback)

A solve writes q_out[i] = min(hi, max(q0[i], lo)) for an entry outside the chain once it has taken a step (iterations > 0) and q0[i]
where it has taken none (the reference clips the whole q after each step, ik/ik/dls.cpp:71)."""
import collections

import numpy as np

from conftest import urdf_path

PLAN_MAX = 16
Case = collections.namedtuple("Case", "name urdf frame nj outside")


def wide_xml(n_side=17):
    out = ['<?xml version="1.0"?>', '<robot name="wide">', '  <link name="base"/>', '  <link name="tool"/>']
    out += ['  <link name="l%d"/>' % j for j in (1, 2, 3)] + ['  <link name="s%d"/>' % j for j in range(1, n_side + 1)]
    origins = [("0.31 -0.42 0.23", "0.05 -0.02 0.21"), ("-0.41 0.52 0.13", "0.02 0.12 0.08"), ("0.27 0.19 -0.58", "-0.03 0.04 0.26")]
    for j, (rpy, xyz) in enumerate(origins, 1):
        out += ['  <joint name="j%d" type="revolute">' % j, '    <origin rpy="%s" xyz="%s"/>' % (rpy, xyz), '    <axis xyz="0 0 1"/>',
                '    <parent link="%s"/>' % ("base" if j == 1 else "l%d" % (j - 1)), '    <child link="l%d"/>' % j,
                '    <limit lower="-2.4" upper="2.6"/>', '  </joint>']
    for j in range(1, n_side + 1):   # every side joint has limits of its own
        out += ['  <joint name="sj%d" type="revolute">' % j, '    <origin rpy="0 0 0" xyz="0.1 0 0.02"/>', '    <axis xyz="0 0 1"/>',
                '    <parent link="%s"/>' % ("base" if j == 1 else "s%d" % (j - 1)), '    <child link="s%d"/>' % j,
                '    <limit lower="%s" upper="%s"/>' % (-0.1 * j, 0.07 * j + 0.01), '  </joint>']
    out += ['  <joint name="tool_joint" type="fixed">', '    <origin rpy="0.21 -0.12 0.33" xyz="0.03 0.02 0.14"/>', '    <parent link="l3"/>',
            '    <child link="tool"/>', '  </joint>', '</robot>', '']
    return "\n".join(out)


CASES = [
    Case("cassie_leg", lambda: open(urdf_path("cassie_fixed")).read(), "LeftFootFront", 7, 9),
    Case("tarsus", lambda: open(urdf_path("cassie_fixed")).read(), "lefttarsus", 6, 10),
    Case("ur5", lambda: open(urdf_path("ur5")).read(), "tool0", 6, 0),
    Case("wide", wide_xml, "tool", 3, 17),
]
BY_NAME = {c.name: c for c in CASES}


def chain_entries(model, frame):
    """The entries of q the chain from the base to `frame` takes, base to tip."""
    flat = model.flat()
    qidx, j = [], int(flat["frame_parent"][model.getFrameId(frame)])
    while j > 0:
        qidx.insert(0, int(flat["idx_q"][j]))
        j = int(flat["parent"][j])
    return qidx


def starts(model, frame, B, seed):
    """(q0 [B, nq], q_near [B, nq]): the chain's entries of q0 uniform in their limits, the others uniform over the limits widened by
    half their span on either side -- about half of them outside, on both sides -- with every fourth row exactly on a limit; q_near is
    the configuration the target is taken at: q0's chain entries moved by up to 0.15 rad inside the limits, every fifth row not at all."""
    lo, hi = np.asarray(model.lowerPositionLimit, float), np.asarray(model.upperPositionLimit, float)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    rng = np.random.default_rng(seed)
    inside = np.zeros(lo.size, bool)
    inside[chain_entries(model, frame)] = True
    span = hi - lo
    q0 = np.where(inside, rng.uniform(lo, hi, (B, lo.size)), rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (B, lo.size)))
    q0[::4] = np.where(inside, q0[::4], np.where(rng.random((q0[::4].shape)) < 0.5, lo, hi))
    q_near = np.clip(np.where(inside, q0 + rng.uniform(-0.15, 0.15, q0.shape), q0), lo, hi)
    q_near[::5] = q0[::5]      # every fifth problem starts AT its target: any stop rule stops it at iteration 0
    return np.ascontiguousarray(q0), np.ascontiguousarray(q_near), inside


def outside_rule(q0, lo, hi, stepped):
    """q0 [B, nq], stepped [B] -> what a solve writes to every entry were it outside the chain."""
    return np.where(np.asarray(stepped, bool)[:, None], np.minimum(hi, np.maximum(q0, lo)), q0)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)
