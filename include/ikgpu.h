/*
 * ikgpu.h -- C ABI of the MI355X batched damped-least-squares IK path.
 *
 * This is the drop-in boundary for ONE path of dazzmo/ik: the iterative loop ik::dls()
 * (reference ik/ik/dls.cpp:5-78) together with what it calls per iteration
 * (ik/ik/data.cpp:25-58, ik/ik/frame.hpp:37-62,152-182, ik/ik/common.hpp:53-56,
 * ik/ik/visitor.hpp:15-21).  The reference has no FFI of its own -- its boundary is the C++
 * free function
 *
 *     vector_t dls(InverseKinematicsProblem&, const vector_t& q0, dls_data&,
 *                  const inverse_kinematics_visitor&, const dls_parameters&);   // ik/ik/dls.hpp:111-114
 *
 * so each entry point below names the reference interface it stands in for.  The C++ mirror of
 * the reference classes (ik_amd/csrc/host/ik/ *.hpp) and the Python ctypes binding (ik_amd/capi.py)
 * are thin layers over exactly these symbols.  Plain pointers and sizes only; no C++ or torch
 * types cross this boundary; nothing here ever throws.  There is NO CPU fallback: every solve
 * entry point runs hand-written gfx950 kernels or returns an error.
 *
 * Conventions
 *   - SE(3) values are 12 doubles: rotation row-major (9) then translation (3).
 *   - Configuration vectors follow Pinocchio: revolute/prismatic joints one entry; a free-flyer
 *     root is (x y z qx qy qz qw) in q and (v_lin, omega) body-frame in the tangent space.
 *   - Batch layouts: IKGPU_SOA is component-major  [component][B]  (device-native, coalesced);
 *     IKGPU_AOS is problem-major [B][component] (what a column-major nq x B Eigen matrix is).
 *     targets: SOA [ntasks][12][B], AOS [B][ntasks][12].
 *   - All functions return IKGPU_OK (0) or an ikgpu_status error; ikgpu_last_error() gives the
 *     message of the calling thread's last failure.
 */
#ifndef IKGPU_H
#define IKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IKGPU_ABI_VERSION 2   /* 2: ikgpu_dls_params grew the derived-visitor fields */

typedef enum {
    IKGPU_OK = 0,
    IKGPU_ERR_INVALID = 1,     /* bad argument (null pointer, size mismatch, unknown id) */
    IKGPU_ERR_PARSE = 2,       /* URDF text could not be parsed */
    IKGPU_ERR_UNSUPPORTED = 3, /* model / task set has no device kernel (stated in last_error) */
    IKGPU_ERR_DEVICE = 4       /* HIP runtime failure, or no gfx950 device */
} ikgpu_status;

/* IKGPU_JOINT_REVOLUTE_UNBOUNDED: what Pinocchio builds for a URDF "continuous" joint (JointModelRevoluteUnbounded*): nq = 2 -- the
 * configuration holds (cos, sin) of the angle --, nv = 1; its position limits are -1.01 / +1.01 on both entries, and integration rotates
 * the pair by the step and renormalises it to first order (scale (3 - |.|^2) / 2).  Models with such a joint run on the generic kernel. */
typedef enum { IKGPU_JOINT_UNIVERSE = 0, IKGPU_JOINT_REVOLUTE = 1, IKGPU_JOINT_PRISMATIC = 2, IKGPU_JOINT_FREEFLYER = 3,
               IKGPU_JOINT_REVOLUTE_UNBOUNDED = 4 } ikgpu_joint_type;

/* ik::KinematicType, reference ik/ik/frame.hpp:20 (same order). */
typedef enum {
    IKGPU_POSITION = 0, IKGPU_ORIENTATION = 1, IKGPU_FULL = 2,
    /* ik::AlignAxisTask with AlignAxisType::AxisX / AxisY / AxisZ (reference ik/ik/frame.hpp:202-319): one row,
     * e = 1 - axis . target/|target|.  Its target direction (frame.hpp:307) rides in the translation part
     * (doubles 9..11) of the task's 12-double target slot; the rotation part is ignored. */
    IKGPU_ALIGN_AXIS_X = 3, IKGPU_ALIGN_AXIS_Y = 4, IKGPU_ALIGN_AXIS_Z = 5,
    /* ONE row of ik::PostureTask (reference ik/ik/posture.hpp:17-85; a task over nj joints is nj consecutive rows):
     * e = (q[reference] - target) * mask, J = unit row at tangent column `frame` (the reference does not apply the mask
     * to J), both times the weight.  Here `frame` is the tangent index, `reference` the index in q, weight[0] the
     * Task::weighting() entry, weight[1] the mask entry; the target value rides in double 9 of the row's 12-double slot. */
    IKGPU_POSTURE_ROW = 6,
    /* ik::CentreOfMassTask (reference ik/ik/centre_of_mass.hpp:14-62; data.cpp:31-34): three rows,
     * e = oMr^-1 * com(q) - target, J = R(oMr)^T Jcom (pinocchio::jacobianCenterOfMass).  `frame` is not read, `reference`
     * is the reference frame; the target point rides in doubles 9..11 of the task's 12-double slot.  Needs joint masses. */
    IKGPU_CENTRE_OF_MASS = 7
} ikgpu_kinematic_type;

typedef enum { IKGPU_SOA = 0, IKGPU_AOS = 1 } ikgpu_layout;
/* OR-ed into the `layout` argument of the HOST-pointer solve entry points: the targets array holds 7 doubles per task -- translation
 * (x y z) then quaternion (qx qy qz qw), the order of a free-flyer's configuration -- instead of 12; it is expanded on the device
 * (ikgpu_targets_from_pose7), so a target costs 56 instead of 96 bytes over PCIe. */
#define IKGPU_TARGETS_POSE7 0x100

typedef enum { IKGPU_ROOT_FIXED = 0, IKGPU_ROOT_FREEFLYER = 1 } ikgpu_root_joint;

/* Flat kinematic model (what pinocchio::Model holds that the path reads: ik/ik/common.hpp:16).
 * Joint 0 is "universe".  As an input every pointer is caller-owned; as an output of
 * ikgpu_model_get_flat the pointers alias the model and live as long as it does. */
typedef struct {
    int32_t njoints, nq, nv, nframes;
    const int32_t *joint_type;      /* [njoints] ikgpu_joint_type */
    const int32_t *joint_parent;    /* [njoints] */
    const int32_t *joint_idx_q;     /* [njoints] */
    const int32_t *joint_idx_v;     /* [njoints] */
    const double *joint_placement;  /* [njoints][12] parent joint frame -> joint frame */
    const double *joint_axis;       /* [njoints][3]  unit axis (revolute / prismatic) */
    const double *lower, *upper;    /* [nq] position limits (model.lowerPositionLimit / upper) */
    const int32_t *frame_parent;    /* [nframes] parent joint */
    const double *frame_placement;  /* [nframes][12] */
    const char *const *joint_names; /* [njoints] */
    const char *const *frame_names; /* [nframes] */
    /* what pinocchio::centerOfMass reads of model.inertias[j]: mass and lever (centre of mass in the joint frame) of the
     * bodies attached to each joint.  As an input both may be NULL (no masses: a centre-of-mass task is then refused). */
    const double *joint_mass;       /* [njoints] */
    const double *joint_com;        /* [njoints][3] */
} ikgpu_flat_model;

/* One ik::FrameTask (reference ik/ik/frame.hpp:78-200) as the device sees it: frame and
 * reference-frame ids (model.getFrameId), kinematic type, priority level
 * (InverseKinematicsProblem::add_frame_task's third argument, ik/ik/problem.hpp:55-66) and the
 * Task::weighting() vector (ik/ik/task.hpp:40; first `dimension` entries used, default ones).
 * The task's `target` (frame.hpp:189) is per-problem data and is passed to the solve call. */
typedef struct {
    int32_t frame, reference, type, priority;
    double weight[6];
} ikgpu_task;

/* ik::dls_parameters (reference ik/ik/dls.hpp:24-28, ik/ik/common.hpp:59-66) plus the stop rule
 * of inverse_kinematics_visitor::should_stop (ik/ik/visitor.hpp:15-21) as a number: a problem
 * stops, *before* stepping, when ||e[0]||^2 < stop_sq_tol (1e-4 in the reference).  A negative
 * value means "a visitor that never stops": exactly max_iterations steps are taken.
 * max_time and random_restart are unused by the reference loop and have no counterpart. */
#define IKGPU_MAX_VISITOR_LEVELS 8
typedef struct {
    int32_t max_iterations; /* default 100 */
    double damping;         /* default 1e-2; damping^2 is added to the Gram diagonal (dls.cpp:41) */
    double step_length;     /* default 1.0 */
    double stop_sq_tol;     /* default 1e-4; < 0 never stops */
    /* The rest of what a class derived from inverse_kinematics_visitor can decide on: should_stop(ik, e, dq) is virtual and is
     * handed EVERY level's error and the step (ik/ik/visitor.hpp:15-21, called at ik/ik/dls.cpp:61).  A C++ visitor cannot run
     * inside a kernel; this closed family covers what such a visitor realistically tests.  Set by ikgpu_dls_params_default to the
     * reference's own visitor (both switched off; so does zero-initialising the three members).  A solve with either switched on runs on the problem's generic lane program. */
    double dq_sq_tol;       /* > 0: ALSO stop when ||dq||^2 < dq_sq_tol (the step about to be taken is negligible); <= 0 (default 0): off */
    int32_t num_level_tols; /* 0 (default): the error test is ||e[0]||^2 < stop_sq_tol.  n > 0: it is ||e[l]||^2 < level_sq_tol[l] for
                             * every priority level l < n (stop_sq_tol is then not read) */
    double level_sq_tol[IKGPU_MAX_VISITOR_LEVELS];
} ikgpu_dls_params;

typedef struct ikgpu_model ikgpu_model;     /* immutable host-side kinematic model */
typedef struct ikgpu_problem ikgpu_problem; /* model + task table flattened onto one device */

int ikgpu_abi_version(void);
const char *ikgpu_last_error(void);
void ikgpu_dls_params_default(ikgpu_dls_params *p);

/* ---- model loading: stands in for pinocchio::urdf::buildModelFromXML as called at reference
 * ik_ros/src/cassie.cpp:34-35 and ik_ros/src/rviz_model_loader.cpp:24-27.  Reproduces Pinocchio's
 * conventions (joint order, idx_q/idx_v, fixed joints folded into placements, frame table). */
int ikgpu_model_from_urdf(const char *xml, size_t len, int root_joint /* ikgpu_root_joint */, ikgpu_model **out);
/* From arrays (the hook for a caller that already holds a pinocchio::Model). Deep-copies. */
int ikgpu_model_create(const ikgpu_flat_model *flat, ikgpu_model **out);
void ikgpu_model_destroy(ikgpu_model *m);
int ikgpu_model_get_flat(const ikgpu_model *m, ikgpu_flat_model *out);
/* model.getFrameId(name) (reference ik/ik/common.hpp:50): returns nframes when absent. */
int32_t ikgpu_model_frame_id(const ikgpu_model *m, const char *name);
int32_t ikgpu_model_joint_id(const ikgpu_model *m, const char *name);

/* ---- problem: stands in for InverseKinematicsProblem + dls_data construction
 * (reference ik/ik/problem.hpp:17-22, ik/ik/dls.hpp:36-52, ik/ik/data.cpp:8-23).  Analyses the
 * support of every task, picks the kernel specialisation and uploads the constant tables.
 * device: HIP device ordinal. */
int ikgpu_problem_create(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, int32_t device, ikgpu_problem **out);
void ikgpu_problem_destroy(ikgpu_problem *p);
/* Host-only dry run of the analysis ikgpu_problem_create performs: writes the name of the kernel
 * specialisation that would run (NUL-terminated, truncated to cap) or fails with
 * IKGPU_ERR_UNSUPPORTED / IKGPU_ERR_INVALID and the reason in ikgpu_last_error(). Touches no device. */
int ikgpu_problem_plan(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, char *out, size_t cap);
/* The same with ik::FrameConstraint entries (reference ik/ik/frame.hpp:325-449; problem.hpp:68-77): each is an ikgpu_task
 * record of which frame, reference and type (Position / Orientation / Full) are read.  ik::dls keeps its step in the null
 * space of the stacked constraint Jacobian, dq = -N J^T (JJ^T + damping^2 I)^-1 e with N = I - pinv(Jc) Jc (reference
 * ik/ik/dls.cpp:26-34,43-53); ik::pik does not read constraints (reference ik/ik/pik.cpp).  A problem with constraints
 * runs on the generic kernel. */
int ikgpu_problem_create_constrained(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                                     int32_t nconstraints, int32_t device, ikgpu_problem **out);
int ikgpu_problem_plan_constrained(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                                   int32_t nconstraints, char *out, size_t cap);
/* Host-only, touches no device: WHICH compile-time build of the free-flyer tree kernel a solve of this problem with these parameters
 * launches -- the kernel name (`dls_tree<...>`) does not say, it depends on the chains' placements, the weights and the stop rule.
 * Writes "<build>,<folded|unfolded>,<extras>,refill=<twin>" with build hot | hot-never | mask | general, extras none | posture |
 * constraint | posture+constraint | pik and twin (the refill kernel a stop-rule solve larger than the machine would use) hot | mask |
 * fold | general | none -- or "" when the solve does not run on the tree kernel.  pik_levels: 0 for ikgpu_dls_solve_batch (params:
 * its parameters, of which stop_sq_tol is read), 1 or 2 for ikgpu_pik_solve_batch with that many levels, no secondary step and
 * lambda > 0 (params as the level-0 DLS parameters).  The launcher dispatches on the same selection that this reports. */
int ikgpu_dls_tree_build_plan(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                              int32_t nconstraints, const ikgpu_dls_params *params, int32_t pik_levels, char *out, size_t cap);
/* Host-only, touches no device: compiles ahead of time whatever ikgpu_problem_create would compile at run time for this problem
 * -- today the structure-specialised chain kernel (`dls_chain<..,hot-rtc>`) of a fixed-base chain whose placement structure has no
 * pre-built instantiation, through hipRTC -- and leaves the code object in the on-disk cache ($IKGPU_CACHE_DIR, else
 * $XDG_CACHE_HOME/ikgpu, else ~/.cache/ikgpu), so that the first ikgpu_problem_create on the robot does not pay the few seconds
 * of compilation.  There is no counterpart in the reference (its kernels are the CPU's); it belongs to the cold path that stands
 * in for InverseKinematicsProblem + dls_data construction (reference ik/ik/problem.hpp:17-22, ik/ik/dls.hpp:36-52).
 * Returns IKGPU_OK when there was nothing to compile or the compilation succeeded (the name of the kernel that will run is written
 * to `out` as by ikgpu_problem_plan), IKGPU_ERR_UNSUPPORTED when hipRTC is unavailable or the compilation failed (the problem then
 * runs on the general build; the compiler's log is in ikgpu_last_error()). */
int ikgpu_problem_precompile(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                             int32_t nconstraints, char *out, size_t cap);
/* The run-time compiler never runs inside the caller's process (a compiler can abort(); ikgpu_problem_create must not): a cache
 * miss in ikgpu_problem_create / ikgpu_problem_precompile spawns the program `ikgpu_precompile` that is installed next to
 * libikgpu.so (tools/ikgpu_precompile.cpp; $IKGPU_PRECOMPILE_EXE overrides the path) as a child process with the request file
 * below, waits for it (IKGPU_RTC_TIMEOUT_S, default 600), and loads what it left in the cache.  A worker that fails, crashes or
 * hangs costs the caller nothing but the specialised build: the problem is created on its general kernel.  On a cache hit no
 * compiler and no child process run at all -- deployments run `ikgpu_precompile --urdf ...` once (or ikgpu_problem_precompile from
 * a process of their own) and the control process never meets a compiler.
 * ikgpu_rtc_worker_compile is that child's entry point: it reads one request written by the library (format private to the
 * library), compiles it in the calling process and stores the code object in the cache; 0 on success.  It initialises no
 * device.  Nothing else should call it.  No counterpart in the reference (its kernels are compiled with the library). */
int ikgpu_rtc_worker_compile(const char *request_path);
int32_t ikgpu_problem_rows(const ikgpu_problem *p);        /* M = sum of task dimensions */
const char *ikgpu_problem_kernel(const ikgpu_problem *p);  /* name of the chosen specialisation */
/* Which entries of q a solve can move: support[i] = 1 when q[i] is integrated by the kernel (a joint in the support of some
 * task row, or the floating base), 0 when the loop only ever clips it to its limits (reference ik/ik/dls.cpp:67-71 steps the
 * whole q with dq = 0 there, then ik/ik/common.hpp:53-56 clips it).  A consumer that already holds q0 needs only the
 * support entries of the result -- what the compact multi-GPU gather ships.  support: HOST pointer to nq bytes. */
int ikgpu_problem_support(const ikgpu_problem *p, uint8_t *support);

/* ---- the hot path: B independent calls of ik::dls() (reference ik/ik/dls.cpp:5-78) in lockstep.
 * All array arguments are DEVICE pointers on the problem's device:
 *   q0      [nq x B]            initial configurations
 *   targets [ntasks x 12 x B]   FrameTask::target per task, w.r.t. the task's reference frame
 *   q_out   [nq x B]            returned configuration (dls.cpp:63 / :77)
 *   success [B] (uint8, may be NULL)  data.success (dls.cpp:62 / :76)
 *   iters   [B] (int32, may be NULL)  iteration index at which should_stop fired, else max_iterations
 * stream: a hipStream_t (NULL = default stream).  Asynchronous; re-entrant per stream. */
int ikgpu_dls_solve_batch(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                          const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                          int layout /* ikgpu_layout */, void *stream);

/* ---- tracking: a SEQUENCE of T targets per problem, every waypoint started from the result of the one before.  Stands in for the
 * reference caller's own loop (ik_ros/src/cassie.cpp:92-113: the target moves a little on every tick and q_ = ik::dls(*ik_, q_, ...)
 * takes the previous result as the new start), B of them side by side.  DEFINED as T calls of ikgpu_dls_solve_batch on `stream`
 * with the same params,
 *   call k (k = 0 .. T-1):  q0 = (k == 0 ? q0 : slab k-1 of q_traj), targets = slab k of targets,
 *                           q_out = slab k of q_traj, success = slab k of success, iters = slab k of iters
 * and its outputs are bit-identical to what those calls write.  Waypoints are outermost:
 *   q0      [nq x B]                 the start of waypoint 0
 *   targets [T][ntasks x 12 x B]     q_traj [T][nq x B]     success [T][B] (may be NULL)     iters [T][B] (may be NULL)
 * each slab in the batch layout (IKGPU_SOA / IKGPU_AOS) the single solve takes.  DEVICE pointers; asynchronous on `stream`.
 * T == 0 or B == 0 is a no-op; T < 0 is IKGPU_ERR_INVALID.  A chain problem (`dls_chain<...>`) under the reference's visitor runs the
 * whole sequence in ONE launch that keeps q in registers between waypoints (no queue slot, no allocation: capturable in a graph);
 * every other problem kind and the derived visitors run the T launches from inside the call (when one fails, ikgpu_last_error()
 * names the waypoint). */
int ikgpu_dls_track_batch(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *targets,
                          const ikgpu_dls_params *params, double *q_traj, uint8_t *success, int32_t *iters,
                          int layout /* ikgpu_layout */, void *stream);
/* Name of what ikgpu_dls_track_batch runs with these parameters: `dls_chain_track<NJ=7,full,hot>` (or hot-rtc / general: the build
 * ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the chained launches.  The string
 * belongs to the calling thread and lasts until its next call.  (The reference has one solver and no such choice: this names the
 * stand-in of the caller's loop, ik_ros/src/cassie.cpp:92-113.) */
const char *ikgpu_dls_track_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params);

/* ---- multi-start: the best of K starts per problem.  ik::dls is a local method and the reference says so itself (ik/ik/dls.cpp:10
 * "todo - if limited convergence, try random walk"; dls.cpp:73 "If issues, perform random restart"; dls_parameters::random_restart,
 * ik/ik/dls.hpp:27, is a flag nothing reads -- it stays inert here too).  1 <= K <= 64, else IKGPU_ERR_INVALID.  DEFINED through K calls
 * of ikgpu_dls_solve_batch with the same targets and params:
 *   start 0 of problem b is its column of q0; start k >= 1 is slab k-1 of `starts` ([K-1][nq x B], each slab in the batch layout)
 *   when starts != NULL, else the generated start ikgpu_multistart_starts writes for (seed, b, k);
 *   r_k = (q_k, success_k, iters_k) is what the single solve writes from start k, err_k the sum of squares, in row order, of the M-row
 *   weighted error ikgpu_evaluate_batch defines at q_k;
 *   the winner is the k with the smallest key (success_k ? 0 : 1, success_k ? 0 : err_k, k): among the starts that met the stop rule
 *   the lowest index (the caller's own start wins when it converges: a warm start keeps its branch), otherwise the smallest error; a
 *   non-finite err_k ranks as +infinity.  Under the never-stop visitor: the arg-min of the error.
 * q_out [nq x B], success [B], iters [B] are r_winner bit for bit, over all nq entries; winner [B] is the start's index and err_sq [B] is
 * err_winner.  success, iters, winner and err_sq may each be NULL.  DEVICE pointers; asynchronous on `stream`; B == 0 is a no-op.
 * q_out must not overlap q0 or starts.
 * A chain problem under the reference's visitor with K in {2, 4, 8, 16, 32, 64} runs ONE launch (`dls_chain_multistart<...>`): lane
 * gid solves problem gid / K from start gid % K, the K lanes of a group compare their keys across lanes and the winner alone stores
 * (no LDS, no queue slot, no allocation: capturable in a graph; `workspace` is not read).  Every other case -- tree, generic,
 * static-program and derived-visitor problems, K = 1, K not a power of two -- runs the definition from inside the call, start after
 * start, in `workspace` (DEVICE memory of at least ikgpu_dls_multistart_workspace_bytes bytes, else IKGPU_ERR_INVALID); when a step
 * fails, ikgpu_last_error() names the start. */
int ikgpu_dls_multistart_batch(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, const double *starts, uint64_t seed,
                               const double *targets, const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int32_t *winner, double *err_sq, int layout /* ikgpu_layout */, void *workspace, size_t workspace_bytes,
                               void *stream);
/* Bytes of `workspace` ikgpu_dls_multistart_batch needs for these arguments: 0 for the single launch.  (The restarts the reference
 * only plans -- ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27 -- need no memory there either: this serves the loop that stands in for them.) */
size_t ikgpu_dls_multistart_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, const ikgpu_dls_params *params);
/* The generated starts 1 .. K-1 (the random restart of reference ik/ik/dls.cpp:10, :73 and ik/ik/dls.hpp:27, made reproducible):
 * starts_out [K-1][nq x B].  Entry i of a start is DRAWN only if ikgpu_problem_support says 1 for i, i belongs to a revolute or
 * prismatic joint, and both limits are finite with lower[i] < upper[i]; every other entry (the free-flyer's seven, an unbounded
 * joint's) is q0's, bit for bit.  The draw, in uint64 wrapping arithmetic:
 *   mix(z): z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31
 *   h = mix(seed + 0x9E3779B97F4A7C15); h = mix(h + b); h = mix(h + k); h = mix(h + i)
 *   u = (h >> 11) * 2^-53;   value = clip(fma(u, upper[i] - lower[i], lower[i]), lower[i], upper[i])
 * a function of (seed, b, k, i) only: not of B, K, the layout or the build.  K == 1 writes nothing. */
int ikgpu_multistart_starts(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, uint64_t seed,
                            double *starts_out /* [K-1][nq x B] */, int layout /* ikgpu_layout */, void *stream);
/* Name of what ikgpu_dls_multistart_batch runs with these parameters and K: `dls_chain_multistart<NJ=7,full,hot>` (or hot-rtc /
 * general: the build ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run
 * start after start.  The string belongs to the calling thread and lasts until its next call.  (The reference plans its restarts --
 * ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27 -- and has no such choice.) */
const char *ikgpu_dls_multistart_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K);

/* ---- pick: among K starts per problem, the one that met the stop rule with the smallest COST.  The multi-start call answers "did any
 * start reach the target" with the lowest-index one; a caller who runs several starts usually wants a particular solution -- the
 * configuration closest to where the arm is now, the one furthest from its joint limits, the best-conditioned one (TRAC-IK's Distance,
 * Manip1 and Manip2 solve types; the reference itself only plans its restarts: ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27).  1 <= K <= 64.
 * DEFINED through K calls of ikgpu_dls_solve_batch exactly as ikgpu_dls_multistart_batch is: the starts, the draw,
 * r_k = (q_k, success_k, iters_k) and err_k are word for word those of that call;
 *   the winner is the k with the smallest key (success_k ? 0 : 1, success_k ? cost_k : err_k, k): among the starts that met the stop
 *   rule the smallest cost, a tie going to the lowest index; when none did, the smallest error, as multi-start.  A non-finite cost or
 *   error ranks as +infinity.
 * q_out [nq x B], success [B], iters [B] are r_winner bit for bit, over all nq entries; winner [B] is the start's index, cost [B] is
 * cost_winner (also when no start converged) and err_sq [B] is err_winner.  success, iters, winner, cost and err_sq may each be NULL.
 * The costs, all non-negative, over the entries i with ikgpu_problem_support = 1 ("support"), accumulated in increasing i (a chain
 * kernel: along the chain):
 *   IKGPU_PICK_DISTANCE        sum_i w[i] (q_k[i] - q_ref[i])^2
 *   IKGPU_PICK_MAX_DISTANCE    max_i w[i] |q_k[i] - q_ref[i]|
 *   IKGPU_PICK_LIMIT_MARGIN    0.5 - min_i min(q_k[i] - lower[i], upper[i] - q_k[i]) / (upper[i] - lower[i]), the min over the support
 *                              entries with finite limits, lower < upper and a finite upper - lower (a free-flyer's entries, whose
 *                              limits are -+DBL_MAX, take no part); 0 when the support has none.  q_ref and w are not read.
 *   IKGPU_PICK_MANIPULABILITY  1 / sqrt(det(J J^T + damping^2 I)), J the M-row weighted task Jacobian ikgpu_evaluate_batch defines at
 *                              q_k: the product of the pivots of the L D L^T factor the solver forms.  q_ref and w are not read.
 * Plain entries are compared, as in the solution set: no distance modulo 2 pi, prismatic entries in metres.  q_ref: DEVICE [nq x B] in
 * the batch layout, or NULL: q0.  w: HOST [nq], finite and >= 0, or NULL: ones; it is read during the call.
 * IKGPU_ERR_INVALID: an unknown rule, K outside 1 .. 64, w with a negative or non-finite entry, a workspace that is too small, and the
 * never-stop visitor (stop_sq_tol < 0 and no derived visitor: no start converges and the rule could never act, as in the solution
 * set).  q_out must not overlap q0, starts or q_ref.  DEVICE pointers otherwise; asynchronous on `stream`; B == 0 is a no-op.
 * A chain problem under the reference's visitor with K in {2, 4, 8, 16, 32, 64} runs ONE launch (`dls_chain_pick<...>`) with the
 * multi-start kernel's lane mapping: one trailing evaluation after the loop, the cost, the key, the selection across lanes, the
 * winner's stores (no LDS, no queue slot, no allocation: capturable in a graph; `workspace` is not read; w travels in the kernel
 * arguments).  Every other case -- tree, generic, static-program and derived-visitor problems, K = 1, K not a power of two -- runs the
 * definition from inside the call, start after start, in `workspace` (DEVICE memory of at least ikgpu_dls_pick_workspace_bytes bytes);
 * when a step fails, ikgpu_last_error() names the start. */
typedef enum { IKGPU_PICK_DISTANCE = 0, IKGPU_PICK_MAX_DISTANCE = 1, IKGPU_PICK_LIMIT_MARGIN = 2, IKGPU_PICK_MANIPULABILITY = 3 } ikgpu_pick_rule;
int ikgpu_dls_pick_batch(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, const double *starts, uint64_t seed,
                         const double *targets, const ikgpu_dls_params *params, int32_t rule /* ikgpu_pick_rule */,
                         const double *q_ref /* DEVICE [nq x B], or NULL: q0 */, const double *w /* HOST [nq], or NULL: ones */,
                         double *q_out, uint8_t *success, int32_t *iters, int32_t *winner, double *cost, double *err_sq,
                         int layout /* ikgpu_layout */, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_pick_batch needs for these arguments, whatever the rule: 0 for the single launch. */
size_t ikgpu_dls_pick_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, const ikgpu_dls_params *params);
/* Name of what ikgpu_dls_pick_batch runs with these parameters, K and rule: `dls_chain_pick<NJ=6,full,hot>` (or hot-rtc / general: the
 * build ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run start after
 * start; "" for an unknown rule.  The string belongs to the calling thread and lasts until its next call. */
const char *ikgpu_dls_pick_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K, int32_t rule);

/* ---- solution set: the DISTINCT converged starts among K starts per problem, up to N of them.  An IK target rarely has one solution
 * (a 6-joint arm has up to eight branches, a 7-joint chain a whole family) and ik::dls, a local method, finds the one its start leads
 * to (reference ik/ik/dls.cpp:10 "todo - if limited convergence, try random walk"; dls.cpp:73 "If issues, perform random restart";
 * dls_parameters::random_restart, ik/ik/dls.hpp:27, is a flag nothing reads -- it stays inert here too).  1 <= N <= K <= 64, sep finite
 * and >= 0, else IKGPU_ERR_INVALID.  DEFINED through K calls of ikgpu_dls_solve_batch with the same targets and params:
 *   the starts are exactly those of ikgpu_dls_multistart_batch: start 0 of problem b is its column of q0; start k >= 1 is slab k-1 of
 *   `starts` ([K-1][nq x B]) when starts != NULL, else the generated start ikgpu_multistart_starts writes for (seed, b, k);
 *   r_k = (q_k, success_k, iters_k) is what the single solve writes from start k;
 *   the KEPT set of problem b is built greedily in increasing k: start k is kept if and only if success_k is true, fewer than N starts
 *   are kept so far, and for every kept j < k there is an entry i with ikgpu_problem_support = 1 and |q_k[i] - q_j[i]| >= sep (one
 *   IEEE subtraction, fabs and a compare: reproducible bit for bit from the single solves).
 * The comparison is over plain entries: configurations that differ by a full turn of a joint are DIFFERENT configurations (they are
 * to a joint-limited robot); distance modulo 2 pi is not taken.  An entry of a prismatic joint is compared in metres with the same sep: in a
 * support that mixes both kinds sep is one bound over radians and metres.  sep == 0 keeps every converged start, up to N.
 *   count  [B]             the number kept, at most N
 *   q_sols [N][nq x B]     each slab in the batch layout; for n < count[b], slab n holds q of the n-th kept start, bit-identical over all
 *                          nq entries to the single solve from that start (entries outside the support come from that start's own
 *                          column, clipped once a step was taken)
 *   which  [N][B], iters [N][B]   the n-th kept start's index and its iteration count; either may be NULL
 * Slots n >= count[b] are not written.  count and q_sols may not be NULL.  DEVICE pointers; asynchronous on `stream`; B == 0 is a
 * no-op.  q_sols must not overlap q0 or starts.  Under the never-stop visitor (stop_sq_tol < 0 and no derived visitor) no start
 * converges by construction: IKGPU_ERR_INVALID.
 * A chain problem under the reference's visitor with K in {2, 4, 8, 16, 32, 64} runs ONE launch (`dls_chain_solutions<...>`) with the
 * multi-start kernel's lane mapping: the K lanes of a group build the set across lanes after the loop, and every kept lane stores
 * into its slot (no LDS, no queue slot, no allocation: capturable in a graph; `workspace` is not read).  Every other case -- tree,
 * generic, static-program and derived-visitor problems, K = 1, K not a power of two -- runs the definition from inside the call, start
 * after start, in `workspace` (DEVICE memory of at least ikgpu_dls_solutions_workspace_bytes bytes, else IKGPU_ERR_INVALID); when a
 * step fails, ikgpu_last_error() names the start. */
int ikgpu_dls_solutions_batch(const ikgpu_problem *p, int64_t B, int32_t K, int32_t N, const double *q0, const double *starts,
                              uint64_t seed, const double *targets, const ikgpu_dls_params *params, double sep, double *q_sols,
                              int32_t *count, int32_t *which, int32_t *iters, int layout /* ikgpu_layout */, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_solutions_batch needs for these arguments: 0 for the single launch.  (The restarts the reference only
 * plans -- ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27 -- need no memory there either: this serves the loop that stands in for them.) */
size_t ikgpu_dls_solutions_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, int32_t N, const ikgpu_dls_params *params);
/* Name of what ikgpu_dls_solutions_batch runs with these parameters and K: `dls_chain_solutions<NJ=7,full,hot>` (or hot-rtc / general:
 * the build ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run start
 * after start.  The string belongs to the calling thread and lasts until its next call.  (The reference plans its restarts --
 * ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27 -- and has no such choice.) */
const char *ikgpu_dls_solutions_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K);

/* ---- line: follow a STRAIGHT Cartesian line from where the task frame is at q0 to one goal per problem -- the approach or retreat of a
 * grasp, the swing of a foot, a linear move.  The reference's own caller generates its target sequence from a formula on every tick
 * (ik_ros/src/cassie.cpp:92-113); here the formula is the line, and the T waypoints are a function of q0 and the goal.
 * ikgpu_line_targets writes them, W_out [T][ntasks x 12 x B] (the shape of ikgpu_dls_track_batch's targets), from
 *   goals [ntasks x 12 x B]  the shape and meaning of ikgpu_dls_solve_batch's targets: slot by slot the pose M1 = (R1, p1) of the task
 *                            frame in the task's reference frame;
 *   M0 = (R0, p0) = oMr^-1 oMf(q0), the pose of the task frame at q0 in that reference frame, w = log3(R0^T R1);
 *   waypoint k (k = 0 .. T-1), s = (k + 1) / T:   R = R0 exp3(s w),  p = p0 + s (p1 - p0)   for k < T-1
 *   (a straight line of the frame origin at constant angular velocity), and waypoint T-1 is the goal's own 12 doubles, bit for bit --
 *   so T == 1 is the single solve to the goal.
 * log3 follows the rotation part of the error's log6 (theta = acos of the clamped trace, the theta -> pi formula from pi - 1e-2 on);
 * exp3 is Rodrigues' formula with Taylor forms below theta = 2^-13.  A relative rotation near pi has an ill-conditioned axis: split
 * such a move into two lines.  Accepted when every target slot belongs to a FrameTask (IKGPU_POSITION / _ORIENTATION / _FULL) whose
 * reference frame is fixed in the world; alignment, posture and centre-of-mass slots and a reference frame that moves with q are
 * IKGPU_ERR_UNSUPPORTED.  W_out must not overlap q0 or goals.  DEVICE pointers; asynchronous on `stream`; B == 0 or T == 0 is a
 * no-op; T < 0 is IKGPU_ERR_INVALID. */
int ikgpu_line_targets(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *goals,
                       double *W_out /* [T][ntasks x 12 x B] */, int layout /* ikgpu_layout */, void *stream);
/* ikgpu_dls_line_batch is DEFINED as ikgpu_dls_track_batch on W = ikgpu_line_targets(q0, goals), with problem b taking part in waypoint
 * k only while all its earlier waypoints met the stop rule (a problem that has left its line is not solved any further; "met" and "failed" are
 * the reference's own stop test and failure report, ik/ik/dls.cpp:61-64,76-77; the sequence is the caller's, ik_ros/src/cassie.cpp:92-113):
 *   reached [B] (int32, may be NULL)  the waypoints met before the first failure; T when the goal was reached
 *   q_traj [T][nq x B], success [T][B] (may be NULL), iters [T][B] (may be NULL): slabs k <= min(reached[b], T-1) of problem b are
 *   written -- the failed waypoint's among them, with success = 0 -- and are bit-identical to ikgpu_dls_track_batch on W; later slabs
 *   of that problem are unspecified.
 * The argument rules are ikgpu_dls_track_batch's; under the never-stop visitor (stop_sq_tol < 0 and no derived visitor) nothing is
 * ever reached: IKGPU_ERR_INVALID.  A chain problem under the reference's visitor runs ONE launch (`dls_chain_line<...>`): a lane
 * loads q0 and its goal (12 doubles, not T x 12), forms the waypoints itself and keeps q in registers; a lane whose line has failed
 * is inactive from then on and the wave leaves once none of its lanes is alive, so slabs beyond the failed waypoint are NOT written
 * (no queue slot, no allocation: capturable in a graph; `workspace` is not read).  Every other problem kind and the derived visitors
 * run the definition from inside the call -- ikgpu_line_targets into `workspace` (DEVICE memory of at least
 * ikgpu_dls_line_workspace_bytes bytes, else IKGPU_ERR_INVALID), the T launches, and a count of the leading successes (the flags live
 * in the workspace when success is NULL). */
int ikgpu_dls_line_batch(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *goals,
                         const ikgpu_dls_params *params, double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached,
                         int layout /* ikgpu_layout */, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_line_batch needs for these arguments: 0 for the single launch. */
size_t ikgpu_dls_line_workspace_bytes(const ikgpu_problem *p, int64_t B, int64_t T, const ikgpu_dls_params *params);
/* Name of what ikgpu_dls_line_batch runs with these parameters: `dls_chain_line<NJ=7,full,hot>` (or hot-rtc / general: the build
 * ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run waypoint after
 * waypoint.  The string belongs to the calling thread and lasts until its next call. */
const char *ikgpu_dls_line_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params);

/* ---- path: a Cartesian path through P via poses per problem -- approach, grasp, retreat; a foot's lift, swing and touch-down -- with T
 * waypoints per segment and a bound on the joint step between waypoints.  The sequence is still the caller's formula
 * (ik_ros/src/cassie.cpp:92-113); here it is a polyline.  ikgpu_path_targets writes the P * T waypoints, W_out [P*T][ntasks x 12 x B], from
 *   vias [P][ntasks x 12 x B]  P slabs, each with the shape, the meaning and the batch layout of ikgpu_dls_solve_batch's targets;
 *   segment 0 runs from M0 = oMr^-1 oMf(q0), the pose of each task frame at q0 in its reference frame, to via 0: exactly
 *   ikgpu_line_targets(q0, via 0);
 *   segment s >= 1 runs from via s-1's own twelve values (R0, p0) to via s, w = log3(R0^T R1);
 *   waypoint n = s*T + k is the line's waypoint k of T of segment s (R = R0 exp3((k+1)/T w), p = p0 + (k+1)/T (p1 - p0)), and waypoint
 *   s*T + T-1 is via s's own 12 doubles, bit for bit.
 * The slot restrictions, log3 / exp3 and the advice on rotations near pi are ikgpu_line_targets'.  P >= 1, T >= 0, P * T <= 0x7fffffff,
 * else IKGPU_ERR_INVALID; B == 0 or T == 0 is a no-op.  W_out must not overlap q0 or vias.  DEVICE pointers; asynchronous on `stream`. */
int ikgpu_path_targets(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const double *q0, const double *vias,
                       double *W_out /* [P*T][ntasks x 12 x B] */, int layout /* ikgpu_layout */, void *stream);
/* ikgpu_dls_path_batch is DEFINED as ikgpu_dls_track_batch on W = ikgpu_path_targets(q0, vias), with problem b taking part in waypoint n
 * only while all its earlier waypoints were MET.  Waypoint n is met when its solve met the stop rule (the reference's own stop test and
 * failure report, ik/ik/dls.cpp:61-64,76-77) and either max_joint_step == 0 or no entry i with ikgpu_problem_support = 1 has
 *   fabs(q_n[i] - q_prev[i]) > max_joint_step,
 * q_prev being the configuration the solve started from: q0 for n = 0, slab n-1 of q_traj after that (one IEEE subtraction, fabs and a
 * compare on plain entries, as the solution set compares them: no distance modulo 2 pi; an entry of a prismatic joint is compared in
 * metres, so max_joint_step is one bound over radians and metres).  The stop rule alone says nothing about the
 * joints: with 100 iterations per waypoint a solve may reach waypoint n from waypoint n-1's configuration by swinging to another branch,
 * and a "straight-line motion" would contain a joint-space jump (the joint-jump threshold of every Cartesian-path interface).
 *   reached [B] (int32, may be NULL)  the waypoints met before the first one that was not; P * T: the whole path
 *   q_traj [P*T][nq x B], success [P*T][B] (may be NULL), iters [P*T][B] (may be NULL): slabs n <= min(reached[b], P*T-1) of problem b
 *   are written and are bit-identical to ikgpu_dls_track_batch on W; later slabs of that problem are unspecified.  The failing slab
 *   carries the solve's own success: 1 there means the waypoint was reached, but through a jump.
 * max_joint_step must be finite and >= 0 and, under the never-stop visitor (stop_sq_tol < 0 and no derived visitor), nothing is ever
 * reached: IKGPU_ERR_INVALID.  P = 1 with max_joint_step = 0 is ikgpu_dls_line_batch.  A chain problem under the reference's visitor runs
 * ONE launch (`dls_chain_path<...>`): a lane loads q0 and P x 12 doubles (not P * T x 12), keeps q, the previous configuration's chain
 * entries, the segment's start pose and rotation vector and the current via in registers, and has the next via in flight during the
 * last solve of a segment; a lane whose path has ended is inactive from then on and the wave leaves once none of its lanes is alive (no
 * queue slot, no allocation: capturable in a graph; `workspace` is not read).  Every other problem kind and the derived visitors run
 * the definition from inside the call -- ikgpu_path_targets into `workspace` (DEVICE memory of at least
 * ikgpu_dls_path_workspace_bytes bytes, else IKGPU_ERR_INVALID), the P * T launches, and one kernel that applies the met rule to the
 * flags and the joint steps (the flags live in the workspace when success is NULL). */
int ikgpu_dls_path_batch(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const double *q0, const double *vias,
                         const ikgpu_dls_params *params, double max_joint_step, double *q_traj, uint8_t *success, int32_t *iters,
                         int32_t *reached, int layout /* ikgpu_layout */, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_path_batch needs for these arguments: 0 for the single launch. */
size_t ikgpu_dls_path_workspace_bytes(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const ikgpu_dls_params *params);
/* Name of what ikgpu_dls_path_batch runs with these parameters: `dls_chain_path<NJ=7,full,hot>` (or hot-rtc / general: the build
 * ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run waypoint after
 * waypoint.  The string belongs to the calling thread and lasts until its next call. */
const char *ikgpu_dls_path_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params);

/* ---- path multi-start: the start whose IK branch carries the path.  The robot is not on the path yet: it may move freely in joint space
 * to the path's first pose, and WHICH solution of that pose it takes decides how far the Cartesian path can be followed without a
 * joint jump.  ik::dls is a local method (reference ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27), so the K starts of
 * ikgpu_dls_multistart_batch are tried -- the same starts, the same draw, the same err_k, word for word -- and each one that reaches the
 * first pose is followed along the path (the caller's sequence, ik_ros/src/cassie.cpp:92-113, as ikgpu_dls_path_batch defines it).
 *   vias [P][ntasks x 12 x B]  P >= 1 slabs; via 0 is the path's first pose; N = (P-1)*T waypoints lie behind it.
 * Candidate k: r_k = (q_k, success_k, iters_k) is what ikgpu_dls_solve_batch writes from start k with targets = via 0 (the stop test
 * and failure report of ik/ik/dls.cpp:61-64,76-77).  If success_k, reached_k is what ikgpu_dls_path_batch(q0 = q_k, vias = slabs
 * 1 .. P-1, P-1, T, max_joint_step) writes as `reached`: segment 0 of that path runs from the frame's pose at q_k, so the joint-step
 * rule (over the entries with ikgpu_problem_support = 1) is measured from q_k.  If the entry failed, reached_k counts as -1.  N = 0:
 * reached_k = 0 for every start that entered.
 * The winner is the k with the smallest key (success_k ? 0 : 1, success_k ? N - reached_k : err_k, k): among the starts that entered,
 * the one that gets furthest; a tie goes to the lowest index, so a warm start (start 0 = q0) keeps its branch when it is as good as
 * any; when no start entered, the smallest error, as in multi-start; a non-finite error ranks as +infinity.
 *   q_entry [nq x B], entry_success [B], entry_iters [B]   r_winner, bit for bit over all nq entries
 *   winner [B] the winning start, err_sq [B] err_winner, reached [B] reached_winner (0 when the winner's entry failed)
 *   reached_all [K][B]   reached_k, -1 for a failed entry
 *   q_traj [(P-1)*T][nq x B], success, iters [(P-1)*T][B]   (q_traj NULL: no trajectory; success / iters are then not read) for a problem
 *   with entry_success = 1, slabs n <= min(reached, N-1) are written and bit-identical to ikgpu_dls_path_batch(q0 = q_entry, slabs
 *   1 .., P-1, T, max_joint_step); the failing slab carries the solve's own flag; later slabs, and every slab of a problem with
 *   entry_success = 0, are unspecified.
 * Every output except q_entry may be NULL.  q_entry and q_traj must overlap neither each other nor any input.  IKGPU_ERR_INVALID: K
 * outside 1 .. 64, P < 1, T < 0, (P-1)*T > 0x7fffffff, max_joint_step not finite or negative, a workspace that is too short, the
 * never-stop visitor (no start ever enters).  IKGPU_ERR_UNSUPPORTED: the slot restrictions of ikgpu_path_targets, when P >= 2.  B == 0
 * is a no-op.  P = 1 is ikgpu_dls_multistart_batch on via 0, bit for bit, with reached = 0.
 * A chain problem under the reference's visitor with K in {2, 4, .., 64} takes TWO launches and no workspace.  The scout
 * (`dls_chain_path_multistart<...>`): the multi-start lane mapping (lane gid serves problem gid / K from start gid % K); a lane solves
 * the entry, keeps its result in registers and follows the path WITHOUT storing a trajectory; a lane whose entry failed is dead from
 * the start and the wave leaves once none of its lanes is alive; then every lane stores its reached_all entry, the K lanes select and
 * the winner alone stores.  Then, with q_traj, the ordinary `dls_chain_path<...>` launch from q_entry on the same stream: 1 / K of the
 * scout's lanes, ONE trajectory buffer instead of K.  Every other case -- tree, generic and static-program problems, derived visitors,
 * K = 1, K not a power of two -- runs the definition from inside the call, start after start, in `workspace` (DEVICE memory of at
 * least ikgpu_dls_path_multistart_workspace_bytes bytes: one scratch trajectory reused per start, or q_traj itself when given, and the
 * per-start results); ikgpu_last_error names the failing start or waypoint. */
int ikgpu_dls_path_multistart_batch(const ikgpu_problem *p, int64_t B, int32_t K, int64_t P, int64_t T, const double *q0,
                                    const double *starts /* [K-1][nq x B] or NULL: generated from seed */, uint64_t seed, const double *vias,
                                    const ikgpu_dls_params *params, double max_joint_step, double *q_entry, uint8_t *entry_success,
                                    int32_t *entry_iters, int32_t *winner, double *err_sq, int32_t *reached, int32_t *reached_all /* [K][B] */,
                                    double *q_traj /* [(P-1)*T][nq x B], or NULL: no trajectory */, uint8_t *success, int32_t *iters,
                                    int layout /* ikgpu_layout */, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_path_multistart_batch needs for these arguments (with_trajectory: q_traj != NULL): 0 for the two launches. */
size_t ikgpu_dls_path_multistart_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, int64_t P, int64_t T,
                                                 const ikgpu_dls_params *params, int with_trajectory);
/* Name of what ikgpu_dls_path_multistart_batch runs with these parameters: `dls_chain_path_multistart<NJ=6,full,hot>` (or hot-rtc /
 * general: the build ikgpu_problem_kernel reports) for the scout, `loop(<ikgpu_problem_kernel's name>)` for the definition run start
 * after start.  The string belongs to the calling thread and lasts until its next call. */
const char *ikgpu_dls_path_multistart_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K);

/* ---- goal set: reach ANY of G alternative goal poses per problem -- G grasp candidates on an object, G footholds, G docking poses --
 * from K starts, and learn which goals are reachable at all.  ik::dls is a local method (reference ik/ik/dls.cpp:10 "todo - if limited
 * convergence, try random walk"; dls.cpp:73 "If issues, perform random restart"; dls_parameters::random_restart, ik/ik/dls.hpp:27, is a
 * flag nothing reads -- it stays inert here too), and the reference takes one target per task (ik/ik/frame.hpp:189).  G >= 1, K >= 1,
 * G * K <= 64, else IKGPU_ERR_INVALID.  DEFINED through G * K calls of ikgpu_dls_solve_batch with the same params:
 *   goals is [G][ntasks x 12 x B]: each slab has the shape, the meaning and the batch layout of the single solve's `targets`;
 *   the starts are exactly those of ikgpu_dls_multistart_batch and do not depend on the goal: start 0 of problem b is its column of q0;
 *   start k >= 1 is slab k-1 of `starts` ([K-1][nq x B]) when starts != NULL, else the generated start ikgpu_multistart_starts writes
 *   for (seed, b, k);
 *   for candidate j = g * K + k: r_j = (q_j, success_j, iters_j) is what the single solve writes from start k with slab g of `goals` as
 *   its targets, err_j the sum of squares, in row order, of the M-row weighted error ikgpu_evaluate_batch defines at q_j against slab g;
 *   the winner is the j with the smallest key (success_j ? 0 : 1, success_j ? 0 : err_j, j): among the candidates that met the stop
 *   rule the lowest goal index wins and within that goal the lowest start (the caller lists its goals in order of preference, and its
 *   own start keeps its branch), otherwise the smallest error; a non-finite err_j ranks as +infinity.  Under the never-stop visitor: the
 *   arg-min of the error over all G * K.
 * q_out [nq x B], success [B], iters [B] are r_winner bit for bit, over all nq entries (entries outside the support come from the winning
 * start's own column, clipped once a step was taken, as in multi-start); goal [B] = winner / K, start [B] = winner % K, err_sq [B] =
 * err_winner; reachable [G][B] (uint8) = 1 if and only if some start of goal g met the stop rule -- all zero under the never-stop
 * visitor.  success, iters, goal, start, err_sq and reachable may each be NULL.  DEVICE pointers; asynchronous on `stream`; B == 0 is
 * a no-op.  q_out must not overlap q0, starts or goals.
 * A chain problem under the reference's visitor with G and K both powers of two and G * K >= 2 runs ONE launch
 * (`dls_chain_goalset<...>`): lane gid solves problem gid / (G K) from start gid % K against goal (gid / K) % G, the G K lanes of a
 * group compare their keys across lanes, the winner alone stores, and the first lane of each goal stores its flag (no LDS, no queue
 * slot, no allocation: capturable in a graph; `workspace` is not read).  Every other case -- tree, generic, static-program and
 * derived-visitor problems, G or K not a power of two, G = K = 1 -- runs the definition from inside the call, candidate after candidate,
 * in `workspace` (DEVICE memory of at least ikgpu_dls_goalset_workspace_bytes bytes, else IKGPU_ERR_INVALID); when a step fails,
 * ikgpu_last_error() names the goal and the start. */
int ikgpu_dls_goalset_batch(const ikgpu_problem *p, int64_t B, int32_t G, int32_t K, const double *q0, const double *starts, uint64_t seed,
                            const double *goals, const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                            int32_t *goal, int32_t *start, double *err_sq, uint8_t *reachable, int layout /* ikgpu_layout */,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of `workspace` ikgpu_dls_goalset_batch needs for these arguments: 0 for the single launch. */
size_t ikgpu_dls_goalset_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t G, int32_t K, const ikgpu_dls_params *params);
/* Name of what ikgpu_dls_goalset_batch runs with these parameters, G and K: `dls_chain_goalset<NJ=7,full,hot>` (or hot-rtc / general:
 * the build ikgpu_problem_kernel reports) for the single launch, `loop(<ikgpu_problem_kernel's name>)` for the definition run candidate
 * after candidate.  The string belongs to the calling thread and lasts until its next call. */
const char *ikgpu_dls_goalset_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t G, int32_t K);

/* FrameTask::target (an SE(3), reference ik/ik/frame.hpp:189) given as 7 doubles -- translation (x y z), quaternion (qx qy qz qw;
 * converted as Eigen's toRotationMatrix does, i.e. as the free-flyer's configuration is read) -- expanded into the 12-double slots
 * the solve entry points take.  pose7: [ntasks x 7 x B] (IKGPU_SOA) or [B x ntasks x 7] (IKGPU_AOS); targets12 likewise with 12.
 * DEVICE pointers; asynchronous on `stream`.  Slots of tasks that read a vector only (alignment direction, centre-of-mass point,
 * posture value: doubles 9..11) take it from the translation part. */
int ikgpu_targets_from_pose7(int64_t B, int32_t ntasks, const double *pose7, double *targets12, int layout /* ikgpu_layout */, void *stream);

/* Same with HOST pointers: copies in, solves on the device, copies out, synchronises. This is what
 * the single-problem ik::dls() shim calls with B = 1.  layout may carry IKGPU_TARGETS_POSE7.  Batches above 1 MiB of buffers
 * are pipelined in chunks (H2D of chunk k + 1, solve of chunk k, D2H of chunk k - 1 overlap; pinned caller buffers make every
 * copy asynchronous), through an arena the problem keeps: no allocation and no device-wide synchronisation per call. */
int ikgpu_dls_solve_batch_host(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                               const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int layout);

/* ---- the hot path on several GPUs of one node, from ONE process (the reference's caller is a single C++ process,
 * ik_ros/src/cassie.cpp:95-112; it has no multi-device code of its own).  Problems are independent and the model + task table are
 * replicated, so a batch of `total` problems is split into contiguous shards -- rank r of n owns [lo, hi) as ikgpu_shard_range
 * gives it (sizes differ by at most one) -- each device solves its shard with ikgpu_dls_solve_batch into a packed slot
 *     [ q rows: nq x b float64 | iterations: b int32 | success: b uint8 ]        (ikgpu_shard_slot_layout, b = the shard's size)
 * and ONE RCCL all-gather over xGMI leaves every device with every rank's slot: [n][slot_bytes], slot_bytes = the largest
 * shard's layout rounded up to 16 (ikgpu_shard_slot_bytes); slot r is decoded with rank r's own shard size.  The Python
 * one-process-per-GPU path (ik_amd/distributed.py, torch.distributed) uses the same two layout functions. */
void ikgpu_shard_range(int64_t total, int32_t rank, int32_t nranks, int64_t *lo, int64_t *hi);
size_t ikgpu_shard_slot_layout(int32_t rows, int64_t b, size_t *off_q, size_t *off_iters, size_t *off_success); /* returns bytes used */
size_t ikgpu_shard_slot_bytes(int32_t rows, int64_t total, int32_t nranks);
typedef struct ikgpu_shard_group ikgpu_shard_group; /* one problem handle, one stream and one RCCL communicator per device */
/* devices: ndev distinct HIP device ordinals.  Creates the per-device problem handles (as ikgpu_problem_create_constrained) and
 * the communicators (ncclCommInitAll; librccl is opened at run time -- a group of one device works without it). */
int ikgpu_shard_group_create(const ikgpu_model *m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                             int32_t nconstraints, const int32_t *devices, int32_t ndev, ikgpu_shard_group **out);
void ikgpu_shard_group_destroy(ikgpu_shard_group *g);
int32_t ikgpu_shard_group_size(const ikgpu_shard_group *g);
const ikgpu_problem *ikgpu_shard_group_problem(const ikgpu_shard_group *g, int32_t rank);
int32_t ikgpu_shard_group_uses_rccl(const ikgpu_shard_group *g);
void *ikgpu_shard_group_stream(const ikgpu_shard_group *g, int32_t rank); /* the hipStream_t rank's work is enqueued on */
/* Wall time (microseconds) rank's worker thread spent ENQUEUEING its shard's launch in the last ikgpu_dls_solve_batch_sharded call
 * (the launches of the ranks are issued in parallel, one thread per device; the collective follows in one group call).  < 0: no call
 * yet / bad rank.  A measurement aid for deployments: with kernels of 0.1 ms, serial issue over 8 devices would cost as much as
 * the solve.  No counterpart in the reference (one process, one device-less solver). */
double ikgpu_shard_group_last_issue_us(const ikgpu_shard_group *g, int32_t rank);
/* One step.  (`gathered[r]` is written by work enqueued on rank r's own stream, ikgpu_shard_group_stream(g, r), which does not
 * synchronise with the null stream: anything the caller enqueued elsewhere on these buffers -- a fill, a previous reader -- must have
 * completed, or be ordered against that stream, before the call.)
 * q0[r], targets[r]: DEVICE pointers on device r to rank r's shard, component-major ([nq x b_r], [ntasks x 12 x b_r]);
 * gathered[r]: DEVICE pointer on device r to ndev * ikgpu_shard_slot_bytes(nq, total, ndev) bytes.  Asynchronous: the solve and
 * the collective are enqueued on each rank's own stream (inputs must be complete before the call);
 * ikgpu_shard_group_synchronize waits for all of them. */
int ikgpu_dls_solve_batch_sharded(ikgpu_shard_group *g, int64_t total, const double *const *q0, const double *const *targets,
                                  const ikgpu_dls_params *params, void *const *gathered);
int ikgpu_shard_group_synchronize(ikgpu_shard_group *g);

/* ---- the other solver of the reference: B independent calls of ik::pik(), prioritised IK (reference
 * ik/ik/pik.cpp:31-103, declared ik/ik/pik.hpp:56-59), in lockstep.  Arguments as ikgpu_dls_solve_batch.  Every priority
 * level l of the task table is solved in the null space of the levels before it, with the damped pseudo-inverse of
 * pik.cpp:5-22 (damping factor lambda[l]) and the projector update of pik.cpp:58-61.  Runs on the generic device kernel
 * for every problem shape (`pik_generic<...>`). */
#define IKGPU_MAX_PIK_LEVELS 8
#define IKGPU_MAX_PIK_DA 128
/* ik::pik_parameters (reference ik/ik/pik.hpp:11-16; its `damping` and `max_time` are never read by the loop) + the stop
 * rule as in ikgpu_dls_params + the two members of ik::pik_data a caller sets before the call (ik/ik/pik.hpp:41-44). */
typedef struct {
    int32_t max_iterations;               /* default 100 */
    double step_length;                   /* default 1.0 */
    double stop_sq_tol;                   /* default 1e-4; < 0 never stops */
    int32_t num_levels;                   /* the problem's max_priority_level + 1: at least the tasks' max priority + 1 (a level
                                           * without tasks is a no-op, as in the reference's loop pik.cpp:47), <= IKGPU_MAX_PIK_LEVELS */
    double lambda[IKGPU_MAX_PIK_LEVELS];  /* pik_data::lambda, default 1.0 each (pik.hpp:24) */
    const double *da;                     /* pik_data::da, HOST pointer to nv doubles, or NULL for zero (the default);
                                           * read during the call; nv <= IKGPU_MAX_PIK_DA when not NULL */
} ikgpu_pik_params;
void ikgpu_pik_params_default(ikgpu_pik_params *p, int32_t num_levels);
int ikgpu_pik_solve_batch(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                          const ikgpu_pik_params *params, double *q_out, uint8_t *success, int32_t *iters,
                          int layout /* ikgpu_layout */, void *stream);
int ikgpu_pik_solve_batch_host(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                               const ikgpu_pik_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int layout);
/* Name of the kernel ikgpu_pik_solve_batch runs with these parameters.  With ONE priority level, lambda[0] > 0, da == NULL
 * and no constraints in the problem, ik::pik's step  -damp_pinv(J, lambda) e  (reference ik/ik/pik.cpp:5-21,47-61) IS the DLS
 * step  -J^T (J J^T + lambda^2 I)^-1 e  (ik/ik/dls.cpp:39-53) and the loop around it is the same, so the problem's DLS
 * kernel (ikgpu_problem_kernel) runs it; otherwise the generic PIK kernel does. */
const char *ikgpu_pik_kernel(const ikgpu_problem *p, const ikgpu_pik_params *params);

/* ---- stage kernels (device pointers), for stage-by-stage parity and for building targets:
 * evaluate_problem_data + stacking (reference ik/ik/data.cpp:25-58, ik/ik/dls.cpp:18-24):
 *   e_out [M x B], J_out [M x nv x B] (row-major M x nv per problem; J_out may be NULL). */
int ikgpu_evaluate_batch(const ikgpu_problem *p, int64_t B, const double *q, const double *targets,
                         double *e_out, double *J_out, int layout, void *stream);
/* framesForwardKinematics restricted to the task frames (reference ik/ik/data.cpp:28-29):
 *   oMf_out [ntasks x 12 x B] world placement of each task's frame. */
int ikgpu_task_frames_fk_batch(const ikgpu_problem *p, int64_t B, const double *q, double *oMf_out,
                               int layout, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IKGPU_H */
