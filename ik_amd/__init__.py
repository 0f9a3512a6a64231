"""ik_amd -- MI355X-native batched damped-least-squares inverse kinematics.

One hot path of dazzmo/ik -- ik::dls() (reference ik/ik/dls.cpp:5-78), and its sibling ik::pik()
(reference ik/ik/pik.cpp:31-103) -- as hand-written gfx950 kernels behind a C ABI (include/ikgpu.h, ik_amd/libikgpu.so).  This package is the host-side
mirror of the reference API for that path plus the ctypes plumbing; it fails loudly when the
native library is missing and has no CPU fallback.
"""
from .api import (AlignAxisTask, AlignAxisType, CentreOfMassTask, FrameConstraint, FrameTask, InverseKinematicsProblem, KinematicType, Model, PickRule, PostureTask, Problem, SE3,  # noqa: F401
                  dls, dls_batch, dls_data, dls_goalset_batch, dls_goalset_kernel, dls_line_batch, dls_line_kernel, dls_multistart_batch, dls_multistart_kernel, dls_parameters, dls_path_batch, dls_path_kernel, dls_path_multistart_batch, dls_path_multistart_kernel, dls_pick_batch, dls_pick_kernel, dls_solutions_batch, dls_solutions_kernel, dls_track_batch, dls_track_kernel, evaluate_batch, inverse_kinematics_visitor, line_targets, multistart_starts, never_stop_visitor, path_targets,
                  pik, pik_batch, pik_data, pik_parameters, plan, precompile, task_frames_fk_batch, tree_build)
from .capi import IkgpuError  # noqa: F401
