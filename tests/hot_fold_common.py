"""What the folded-run tests share (tests/test_hot_fold_host.py on the CPU, tests/test_gpu_hot_fold.py on the device): the chains that
put a folded run of parallel joints (ik_amd/csrc/device/chain_hot.hpp, ChainRuns::folded, kHotFoldMinRun = 2) in every position it can
take, as URDF text, and the configurations drawn for them.  No tests here.

Every joint turns about z.  Inside a run the joint origins have an identity rotation and a translation with all three components
non-zero (the along-axis addition and both in-plane terms of p~ += Rz(-phi) t run); an "oblique" joint has a general rpy.

  run2_whole     NJ = 2  the whole chain is one run: the leader is joint 0 and the run touches the tip
  run2_middle    NJ = 4  oblique, run of two, oblique: the run is materialised before a general placement
  run3_middle    NJ = 5  oblique, run of three, oblique: the middle member is neither tip nor leader, its angle is a sum of a sum
  run2_twice     NJ = 5  run of two, oblique, run of two: two folded runs in one chain
  no_run         NJ = 3  three oblique joints: runs of one, one shorter than the threshold -- the unfolded path alone
  cassie_fixed / ur5     the fixture robots as they are (runs of 1, 1, 5 and of 1, 2, 1, 1, 1)

The members of the runs have limits of +-3.3 rad: a run of two reaches |phi| = 6.6 > 2 pi, the run of three 9.9."""
import collections

import numpy as np

from conftest import urdf_path

Chain = collections.namedtuple("Chain", "name frame joints tool leader")
OBL = [("0.31 -0.42 0.23", "0.05 -0.02 0.21"), ("-0.41 0.52 0.13", "0.02 0.12 0.08"), ("0.27 0.19 -0.58", "-0.03 0.04 0.26"),
       ("1.02 -0.31 0.22", "0.07 -0.05 0.09")]
RUN = [("0 0 0", "0.11 -0.07 0.05"), ("0 0 0", "-0.06 0.13 -0.04"), ("0 0 0", "0.09 0.08 0.07")]
TOOL = ("0.21 -0.12 0.33", "0.03 0.02 0.14")


def _j(origin, lim):
    return (origin[0], origin[1], -lim, lim)


# (rpy, xyz, lower, upper) per joint, base to tip; `leader`: ChainRuns::leader, the first joint of each joint's run
CHAINS = [
    Chain("run2_whole", "tool", [_j(OBL[0], 3.3), _j(RUN[0], 3.3)], TOOL, [0, 0]),
    Chain("run2_middle", "tool", [_j(OBL[0], 2.6), _j(OBL[1], 3.3), _j(RUN[0], 3.3), _j(OBL[2], 2.2)], TOOL, [0, 1, 1, 3]),
    Chain("run3_middle", "tool", [_j(OBL[0], 2.6), _j(OBL[1], 3.3), _j(RUN[0], 3.3), _j(RUN[1], 3.3), _j(OBL[2], 2.2)], TOOL, [0, 1, 1, 1, 4]),
    Chain("run2_twice", "tool", [_j(OBL[0], 3.3), _j(RUN[0], 3.3), _j(OBL[1], 2.4), _j(OBL[2], 3.3), _j(RUN[2], 3.3)], TOOL, [0, 0, 2, 3, 3]),
    Chain("no_run", "tool", [_j(OBL[0], 2.6), _j(OBL[1], 1.9), _j(OBL[2], 2.8)], TOOL, [0, 1, 2]),
    Chain("cassie_fixed", "LeftFootFront", None, None, [0, 1, 2, 2, 2, 2, 2]),
    Chain("ur5", "tool0", None, None, [0, 1, 1, 3, 4, 5]),
]
BY_NAME = {c.name: c for c in CHAINS}
MADE_UP = [c.name for c in CHAINS if c.joints is not None]


def chain_xml(c):
    if c.joints is None:
        return open(urdf_path(c.name)).read()
    n = len(c.joints)
    links = ["base"] + ["l%d" % (j + 1) for j in range(n)]
    out = ['<?xml version="1.0"?>', '<robot name="%s">' % c.name] + ['  <link name="%s"/>' % l for l in links + ["tool"]]
    for j, (rpy, xyz, lo, hi) in enumerate(c.joints):
        out += ['  <joint name="j%d" type="revolute">' % (j + 1), '    <origin rpy="%s" xyz="%s"/>' % (rpy, xyz), '    <axis xyz="0 0 1"/>',
                '    <parent link="%s"/>' % links[j], '    <child link="%s"/>' % links[j + 1], '    <limit lower="%s" upper="%s"/>' % (lo, hi), '  </joint>']
    out += ['  <joint name="tool_joint" type="fixed">', '    <origin rpy="%s" xyz="%s"/>' % c.tool, '    <parent link="%s"/>' % links[n],
            '    <child link="tool"/>', '  </joint>', '</robot>', '']
    return "\n".join(out)


def runs(c):
    """The member lists of the runs of two or more joints."""
    by = collections.defaultdict(list)
    for j, L in enumerate(c.leader):
        by[L].append(j)
    return [m for m in by.values() if len(m) > 1]


def run_rows(c, lo, hi, qidx, base):
    """Configurations that put the runs where the folded walk differs most from the unfolded one: per run, every member on its upper
    limit, every member on its lower limit (the largest |phi|), and the two alternating patterns (the sum nearly cancels while every
    member is on a limit); the other joints keep `base`'s values.  qidx: the chain joints' entries of q."""
    rows = []
    for members in runs(c):
        for pattern in ("hi", "lo", "alt", "tla"):
            q = base[len(rows) % len(base)].copy()
            for k, j in enumerate(members):
                up = pattern == "hi" or (pattern == "alt" and k % 2 == 0) or (pattern == "tla" and k % 2 == 1)
                q[qidx[j]] = hi[qidx[j]] if up else lo[qidx[j]]
            rows.append(q)
    return np.array(rows) if rows else np.empty((0, lo.size))


def run_sums(c, q, qidx):
    """max over the runs and the rows of q of |phi|, the sum of a run's angles."""
    return max((np.abs(q[:, [qidx[j] for j in m]].sum(axis=1)).max() for m in runs(c)), default=0.0)


# log3 near pi.  Within NEAR_PI of pi it takes its theta -> pi formula, the regime tests/test_hot_evaluate.py and
# tests/test_gpu_rotation_by_pi.py hold to 1e-6.  Just outside it the regular formula w = theta / (2 sin theta) (R - R^T)v is badly
# conditioned in the oracle as in the lane program: theta = acos((tr R - 1) / 2) carries the rounding d of the trace as d / (2 sin theta),
# and d(theta / sin theta) / d theta ~ pi / sin^2 theta times |(R - R^T)v| / 2 = sin theta turns that into pi d / (2 sin^2 theta) in w.
# R = fMt is a product of up to nine rotations, each entry off by about 9 eps = 1e-15, so d = 3e-15 over the trace's three entries:
# 5e-15 / sin^2 theta, taken twice for two implementations that each carry it: ERR_SIN2 = 1e-14.  A bar b therefore holds as
# b max(1, ERR_SIN2 / (1e-11 sin^2 theta)): unchanged up to pi - 0.032, ten times wider at pi - 1e-2.  theta is the ORACLE's.
NEAR_PI, ERR_SIN2 = 1e-2, 1e-14


def conditioned(theta, regular_bar, near_pi_bar, e_bar=1e-11):
    """Per configuration: near_pi_bar where theta > pi - NEAR_PI, else regular_bar widened by the conditioning of log3 (see above)."""
    theta = np.asarray(theta, float)
    sin2 = np.where(theta > 0.5 * np.pi, np.maximum(np.sin(theta) ** 2, 1e-300), 1.0)      # (towards pi only: near 0 log3 is well conditioned)
    widen = np.maximum(1.0, ERR_SIN2 / (e_bar * sin2))
    return np.where(theta > np.pi - NEAR_PI, near_pi_bar, regular_bar * widen)
