// capi.cpp -- implementation of include/ikgpu.h.  No exception crosses the boundary; every
// solve runs the gfx950 kernels (kernels.hip) or fails with a message -- there is no CPU path.
#include <hip/hip_runtime.h>

#include <time.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "ikgpu.h"
#include "kernels.hpp"
#include "model.hpp"
#include "problem.hpp"

namespace {

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Staging area of the host-pointer entry points for small batches (solve_staged below): grows on demand, guarded by a mutex a
// caller only ever try-locks.
struct Staging {
    std::mutex mu;
    void *dev = nullptr, *host = nullptr;
    size_t cap = 0;
    void release() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
        cap = 0;
    }
    ~Staging() { release(); }
};
constexpr size_t kStageLimit = size_t(1) << 20;  // batches whose buffers total at most 1 MiB take the staged path

// Per-phase wall clock of the pipelined host entry (solve_pipelined below), switched on by IKGPU_HOST_TRACE=<file>: one line per call --
// total and the time spent waiting for the pipe's mutex, in set-up, enqueueing copies and launches, and in each of the final waits.
// (Round 3 saw 30-75 ms stalls about once per hundred calls: this is how the phase that carries them is found;
// tools/host_entry_tails.py reads the file.)
struct HostTrace {
    FILE *f = nullptr;
    bool on = false;
    HostTrace() {
        if (const char *path = std::getenv("IKGPU_HOST_TRACE")) { f = std::fopen(path, "a"); on = f != nullptr; }
    }
    ~HostTrace() { if (f) std::fclose(f); }
    static double now() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return 1e3 * static_cast<double>(ts.tv_sec) + 1e-6 * static_cast<double>(ts.tv_nsec);
    }
};

// Larger batches through the host-pointer entry points: a pipeline the problem keeps -- one device arena (grow-only), three
// streams, events -- so that a call allocates nothing and never synchronises the device: chunks of problems flow
// H2D (chunk k + 1)  ||  solve (chunk k)  ||  D2H (chunk k - 1).
struct HostPipe {
    std::mutex mu;
    void *dev = nullptr;
    size_t cap = 0;
    static constexpr int kRunStreams = 8;
    hipStream_t in = nullptr, out = nullptr;
    hipStream_t run[kRunStreams] = {};   // chunk k solves on run[k % 8]
    std::vector<hipEvent_t> ev_in, ev_run;
    void release() {
        if (dev) (void)hipFree(dev);
        dev = nullptr;
        cap = 0;
        for (hipEvent_t ev : ev_in) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : ev_run) (void)hipEventDestroy(ev);
        ev_in.clear();
        ev_run.clear();
        if (in) { (void)hipStreamDestroy(in); (void)hipStreamDestroy(out); }
        in = out = nullptr;
        for (hipStream_t &r : run) { if (r) (void)hipStreamDestroy(r); r = nullptr; }
    }
    ~HostPipe() { release(); }
};

}  // namespace

struct ikgpu_problem {
    mutable Staging stage;
    mutable HostPipe pipe;
    ikgpu::ProblemHost host;
    ikgpu::ProblemHost gen;  // the same problem analysed for the generic lane program (what ik::pik runs on)
    ikgpu::DeviceTables dev;
    int device = 0;
    int nframes = 0;
    // A Tree-kind problem with few rows runs ik::dls on the lane program specialised for it at run time instead (gen.generic_build == 2):
    // the dense M x M system of a small task set is cheaper than the tree kernel's arrow elimination (the reference demo's own task
    // set, M = 10: 0.39 against 0.51 ms per 65536 problems); `host` stays the tree analysis (stage kernels, two-level ik::pik)
    bool dls_on_static_gen = false;
    // A derived visitor (ikgpu_dls_params::dq_sq_tol / level_sq_tol) runs on the generic lane program whatever kernel ik::dls itself
    // uses.  For Chain / Tree problems that program's static build is compiled at the FIRST such solve (most callers never use a
    // derived visitor, and creation should not pay for it); until it exists -- or where it cannot -- the per-lane interpreter runs.
    mutable std::once_flag visitor_static_once;
    mutable uint64_t visitor_static_key = 0;
    mutable bool visitor_static = false;
    // ik::pik beyond one level / the tree kernel's two: a compiled lane program (rtc.cpp rtc_pik_static_available), one per
    // (problem, with / without the secondary step da), compiled at the FIRST ik::pik call that wants it (or by
    // ikgpu_problem_precompile) -- most problems are only ever handed to ik::dls
    mutable std::once_flag pik_static_once[2];
    mutable uint64_t pik_static_key[2] = {0, 0};
    mutable bool pik_static[2] = {false, false};
    std::vector<uint8_t> draw;   // [nq] entries a generated start of a multi-start solve draws (problem.hpp multistart_draw_mask)
    std::string dls_name;    // what ikgpu_problem_kernel reports
    std::string pik_name;    // name of the generic PIK kernel instance
    std::string pik_tree_name;  // ... and of the tree kernel running a two-level ik::pik (when the problem has that shape)
    std::string pik_static_name;  // ... and of the compiled lane program (formed at creation: ikgpu_pik_kernel only reads)
    explicit ikgpu_problem(int device_) : device(device_) {}
    ~ikgpu_problem() {   // everything the problem holds on its device, released on that device
        DeviceGuard g(device);
        void *const tables[] = {dev.lower, dev.upper, dev.q_in_chain, dev.draw, dev.chain_desc, dev.g_ints, dev.g_dbls};
        for (void *t : tables) (void)hipFree(t);
        dev.queues.release();
        pipe.release();    // (here, not in the members' own destructors: those run after the guard has gone)
        stage.release();
    }
};
// (each of them owns device memory: a copy would free it twice)
static_assert(!std::is_copy_constructible<Staging>::value && !std::is_copy_constructible<HostPipe>::value &&
                  !std::is_copy_constructible<ikgpu_problem>::value && !std::is_copy_assignable<ikgpu_problem>::value,
              "owners of device memory must not be copyable");

namespace {

thread_local std::string g_last_error;

bool shape_built(const ikgpu::ProblemHost &ph) {
    if (ph.kind == ikgpu::KernelKind::Generic) return true;
    return ph.kind == ikgpu::KernelKind::Chain ? ikgpu::chain_shape_built(ph.chain.nj, ph.tasks[0].type)
                                               : ikgpu::tree_shape_built(ph.chain.nj, ph.chainB.nj > 0 ? 2 : 1);
}

// Analysis + the "is this specialisation compiled" check; a specialised shape without an instantiation
// falls back to the generic kernel.  Throws std::runtime_error on invalid input.
ikgpu::ProblemHost analyse(const ikgpu::Model &m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *cons, int32_t ncons,
                           bool compile_rtc) {
    // IKGPU_DLS_KERNEL=generic skips the register-resident specialisations (the parity tests compare them with the generic kernel)
    const char *force = std::getenv("IKGPU_DLS_KERNEL");
    ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, tasks, ntasks, force && std::strcmp(force, "generic") == 0, cons, ncons);
    if (!shape_built(ph)) ph = ikgpu::analyse_problem(m, tasks, ntasks, /*force_generic=*/true, cons, ncons);
    if (ph.kind == ikgpu::KernelKind::Chain) {   // which build of the chain kernel: decided here, once, and part of the name
        ph.chain_build = ikgpu::select_chain_build(ph, compile_rtc);
        ph.kernel_name = ikgpu::chain_kernel_name(ph);
    }
    if (ph.kind == ikgpu::KernelKind::Generic && ikgpu::rtc_generic_static_available(ph, compile_rtc, &ph.generic_key)) {
        ph.generic_build = 2;   // the lane program specialised for this problem (the name says so: "...,static>")
        ph.kernel_name = ph.kernel_name.substr(0, ph.kernel_name.size() - 1) + ",static>";
    }
    return ph;
}

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// Tree-kind problems the static generic program is tried for first: few rows in the system it solves (IKGPU_TREE_STATIC_ROWS, default
// 12; 0 = never; PostureTask rows do not count when the program eliminates them) and no constraint -- measured, B = 65536, 50
// iterations: the demo's task set (M = 10) 0.40 ms static against 0.51 ms on the tree kernel, with the posture regulariser on all 16
// joints (M = 26, a 10 x 10 system) 0.53 against 0.65,
// but with the right foot pinned 0.78 against 0.71 (the tree kernel projects on the constrained chain's 13 columns only; the static
// program orthogonalises three dense rows of 22).  IKGPU_TREE_STATIC_CONSTRAINED=1 routes those too (tests).
bool tree_prefers_static(const ikgpu::ProblemHost &ph) {
    if (ph.kind != ikgpu::KernelKind::Tree) return false;
    long rows = 12;
    if (const char *env = std::getenv("IKGPU_TREE_STATIC_ROWS")) rows = std::strtol(env, nullptr, 10);
    if (ph.cons_on && !std::getenv("IKGPU_TREE_STATIC_CONSTRAINED")) return false;
    return ikgpu::rtc_static_solve_rows(ph) <= rows;
}

std::string static_name(const ikgpu::ProblemHost &gen) {
    const std::string &n = gen.kernel_name;
    return n.size() > 8 && n.compare(n.size() - 8, 8, ",static>") == 0 ? n : n.substr(0, n.size() - 1) + ",static>";
}

// Which kernel ik::dls runs a problem on: what ikgpu_problem_create builds (compile = true: the run-time compiled builds are
// compiled, first the one `analyse` picks, then the Tree problem's static program) and what ikgpu_problem_plan names without
// compiling anything (compile = false).  Throws std::runtime_error on invalid input.
struct KernelPlan {
    ikgpu::ProblemHost host, gen;   // the problem's own analysis; the same problem analysed for the generic lane program
    bool dls_on_static_gen = false;
    std::string name;               // what ikgpu_problem_kernel reports
};
KernelPlan plan_kernels(const ikgpu::Model &m, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *cons, int32_t ncons, bool compile) {
    KernelPlan k;
    k.host = analyse(m, tasks, ntasks, cons, ncons, compile);
    // (for a Generic problem `analyse` has compiled the static program: gen is a copy of host, build and key included)
    k.gen = k.host.kind == ikgpu::KernelKind::Generic ? k.host : ikgpu::analyse_problem(m, tasks, ntasks, /*force_generic=*/true, cons, ncons);
    k.name = k.host.kernel_name;
    if (tree_prefers_static(k.host) && ikgpu::rtc_generic_static_available(k.gen, compile, &k.gen.generic_key)) {
        k.gen.generic_build = 2;
        k.dls_on_static_gen = true;
        k.name = static_name(k.gen);
    }
    return k;
}

}  // namespace

// (shard.cpp reports through the same thread-local message)
int ikgpu_set_last_error(int code, const std::string &msg) { return fail(code, msg); }

namespace {

int hip_fail(hipError_t e, const char *what) {
    return fail(IKGPU_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// What a launcher returned, as the entry point's return code.
int launched(hipError_t e, const char *what) { return e == hipSuccess ? static_cast<int>(IKGPU_OK) : hip_fail(e, what); }

template <class F>
int guarded(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(IKGPU_ERR_INVALID, "out of host memory");
    } catch (const std::exception &e) {
        return fail(IKGPU_ERR_INVALID, e.what());
    } catch (...) {
        return fail(IKGPU_ERR_INVALID, "unknown C++ exception");
    }
}

// The scope every entry point launches in: `device` selected (and the caller's restored on the way out), no exception past the
// boundary (the launchers throw for a shape without an instantiation).  body(stream) returns the entry point's return code.
template <class F>
int on_device(int device, void *stream, F &&body) {
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(IKGPU_ERR_DEVICE, "hipSetDevice failed");
        return static_cast<int>(body(static_cast<hipStream_t>(stream)));
    });
}

// The refusals of the entry points, each rule once; an entry point composes them in its own order (which is part of its contract:
// tests/test_capi_refusals_host.py).  Only check_pik_params reads the problem, after its own null tests: any other refusal, and the
// empty-batch no-op, never look at the handle.
int refuse_if(bool bad, const char *msg) { return bad ? fail(IKGPU_ERR_INVALID, msg) : IKGPU_OK; }

int null_argument() { return refuse_if(true, "null argument"); }

int check_batch(int64_t B) { return refuse_if(B < 0, "negative batch size"); }

int check_problem(const ikgpu_problem *p) { return refuse_if(!p, "null problem"); }

int check_problem_batch(const ikgpu_problem *p, int64_t B) {
    if (int rc = check_problem(p)) return rc;
    return check_batch(B);
}

int check_layout(int layout) { return refuse_if(layout != IKGPU_SOA && layout != IKGPU_AOS, "unknown layout"); }

// ... of a host-pointer entry, where targets may arrive as 7 doubles per task (IKGPU_TARGETS_POSE7)
int check_host_layout(int layout) { return check_layout(layout & ~IKGPU_TARGETS_POSE7); }

int check_starts(int32_t K) { return refuse_if(K < 1 || K > 64, "the number of starts must be 1 .. 64"); }

// one launch takes B x K lanes (K starts per problem, 1 <= K)
int check_launch_size(int64_t B, int32_t K = 1) { return refuse_if(B > (int64_t(1) << 31) * 32 / K, "batch too large for one launch"); }

int check_have_params(const void *prm) { return refuse_if(!prm, "params is null"); }

int check_max_iterations(int32_t n) { return refuse_if(n < 0, "max_iterations must be >= 0"); }

int check_params(const ikgpu_dls_params *p) {
    if (int rc = check_have_params(p)) return rc;
    if (int rc = check_max_iterations(p->max_iterations)) return rc;
    if (int rc = refuse_if(!(p->damping > 0.0), "damping must be > 0: the device solves JJ^T + damping^2 I by Cholesky (SPD)")) return rc;
    if (p->num_level_tols < 0 || p->num_level_tols > IKGPU_MAX_VISITOR_LEVELS)
        return fail(IKGPU_ERR_INVALID, "num_level_tols must be in 0.." + std::to_string(IKGPU_MAX_VISITOR_LEVELS));
    return IKGPU_OK;
}

int check_pik_params(const ikgpu_problem *p, const ikgpu_pik_params *prm) {
    if (int rc = check_have_params(prm)) return rc;
    if (int rc = check_problem(p)) return rc;
    if (int rc = check_max_iterations(prm->max_iterations)) return rc;
    const int levels = p->gen.generic.nlevels;
    if (levels > IKGPU_MAX_PIK_LEVELS)
        return fail(IKGPU_ERR_UNSUPPORTED, "the problem has " + std::to_string(levels) + " priority levels, ik::pik on the device takes at most " +
                                               std::to_string(IKGPU_MAX_PIK_LEVELS));
    // a problem may declare more levels than its tasks use (the demo does, reference ik_ros/src/cassie.cpp:43): the
    // reference's loop over 0..max_priority_level (ik/ik/pik.cpp:47) is a no-op on a level without rows
    if (prm->num_levels < levels || prm->num_levels > IKGPU_MAX_PIK_LEVELS)
        return fail(IKGPU_ERR_INVALID, "num_levels is " + std::to_string(prm->num_levels) + " but the problem's tasks use " +
                                           std::to_string(levels) + " priority levels (at most " + std::to_string(IKGPU_MAX_PIK_LEVELS) + ")");
    for (int l = 0; l < levels; ++l)
        if (!(prm->lambda[l] >= 0.0)) return fail(IKGPU_ERR_INVALID, "lambda[" + std::to_string(l) + "] must be >= 0");
    if (prm->da && p->gen.nv > IKGPU_MAX_PIK_DA)
        return fail(IKGPU_ERR_UNSUPPORTED, "da is carried by value for nv <= " + std::to_string(IKGPU_MAX_PIK_DA));
    return IKGPU_OK;
}

// The model and task arrays a problem is analysed from (ikgpu_problem_create_constrained, _plan_constrained, _precompile).
int check_problem_inputs(const ikgpu_model *h, const ikgpu_task *tasks, const ikgpu_task *constraints, int32_t nconstraints) {
    if (!h || !tasks || (nconstraints > 0 && !constraints)) return null_argument();
    return refuse_if(nconstraints < 0, "negative constraint count");
}

void copy_name(const std::string &name, char *out, size_t cap) {
    if (!out || !cap) return;
    std::strncpy(out, name.c_str(), cap - 1);
    out[cap - 1] = '\0';
}

// IKGPU_PIK_KERNEL=generic keeps every ik::pik call on the PIK kernel's interpreter forms (the parity tests compare the routes);
// =static also keeps it off the DLS and tree kernels, on the compiled lane program where there is one.
bool pik_forced(bool or_static) {
    const char *force = std::getenv("IKGPU_PIK_KERNEL");
    return force && (std::strcmp(force, "generic") == 0 || (or_static && std::strcmp(force, "static") == 0));
}

// ik::pik with ONE priority level and no secondary velocity is the DLS iteration: P = I, so the level's step is
// dq = -damp_pinv(J, lambda) e = -J^T (J J^T + lambda^2 I)^-1 e (reference ik/ik/pik.cpp:5-21,47-61 against ik/ik/dls.cpp:39-53),
// and the stop test, integration and clamp are the same statements in the same order (pik.cpp:67-77, dls.cpp:61-71).
// ik::pik does not read the problem's constraints, so a problem that has any stays on the PIK kernel.
bool pik_is_one_dls_level(const ikgpu_problem *p, const ikgpu_pik_params *prm) {
    if (pik_forced(/*or_static=*/true)) return false;
    return p->gen.generic.nlevels == 1 && !prm->da && prm->lambda[0] > 0.0 && p->host.constraints.empty();
}

// ik::pik with TWO levels in the shape the tree kernel takes (kernels.hpp tree_takes_two_level_pik: level 0 = the frame tasks with a
// Full task on the base link, level 1 = the AlignAxisTask row -- the reference demo's task set split over two levels): level 0 is
// the tree kernel's arrow solve with damping lambda[0], level 1 a rank-one correction on the chain's joints (device/tree_solver.hpp
// PikRow).  No secondary velocity, lambda > 0 on both levels.
bool pik_is_two_levels_on_the_tree(const ikgpu_problem *p, const ikgpu_pik_params *prm) {
    if (pik_forced(/*or_static=*/true)) return false;
    return p->gen.generic.nlevels == 2 && prm->num_levels == 2 && !prm->da && prm->lambda[0] > 0.0 && prm->lambda[1] > 0.0 &&
           p->host.constraints.empty() && ikgpu::tree_takes_two_level_pik(p->host);
}

// Whether the call has a secondary step at all: a null or all-zero da takes the program without one.
bool pik_has_da(const ikgpu_problem *p, const ikgpu_pik_params *prm) {
    bool has_da = false;
    if (prm->da)
        for (int k = 0; k < p->gen.nv; ++k) has_da = has_da || prm->da[k] != 0.0;
    return has_da;
}

// ik::pik on its compiled lane program: every level's lambda > 0 (the program factors Jbar Jbar^T + lambda^2 I), the program exists
// (compiled here on first use).  IKGPU_PIK_KERNEL=generic / IKGPU_PIK_STATIC=0 keep the interpreter forms.
bool pik_runs_static(const ikgpu_problem *p, const ikgpu_pik_params *prm) {
    if (pik_forced(/*or_static=*/false)) return false;
    for (int l = 0; l < prm->num_levels; ++l)
        if (!(prm->lambda[l] > 0.0)) return false;
    const bool has_da = pik_has_da(p, prm);
    const int v = has_da ? 1 : 0;
    if (!ikgpu::rtc_pik_static_available(p->gen, has_da, /*compile=*/false, nullptr)) return false;
    std::call_once(p->pik_static_once[v], [&] {
        p->pik_static[v] = ikgpu::rtc_pik_static_available(p->gen, has_da, /*compile=*/true, &p->pik_static_key[v]);
    });
    return p->pik_static[v];
}

// Level 0 of an ik::pik call as the parameters of the DLS iteration it is (the derived-visitor members stay off).
ikgpu_dls_params pik_level0_as_dls(const ikgpu_pik_params *prm) {
    ikgpu_dls_params d{};
    d.max_iterations = prm->max_iterations; d.damping = prm->lambda[0]; d.step_length = prm->step_length; d.stop_sq_tol = prm->stop_sq_tol;
    return d;
}

constexpr int kNotStaged = -1;   // (no return code: solve_staged left the call to the pipelined path)

// Host-pointer form of a batched solve, small batches: copy in, run `launch` on device buffers, copy out -- or kNotStaged when the
// batch is too large for the staging area, another thread holds it, or it could not be grown.
template <class Launch>
int solve_staged(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets, double *q_out, uint8_t *success, int32_t *iters,
                 int layout, bool pose7, Launch &launch) {
    const size_t nb_q = sizeof(double) * p->host.nq * B, nb_t = sizeof(double) * 12 * p->host.ntasks * B;
    const size_t nb_t7 = pose7 ? sizeof(double) * 7 * p->host.ntasks * B : 0;
    // Small batches -- the reference's own call pattern is ONE problem per call, 50 times a second (ik_ros/src/cassie.cpp:112)
    // -- go through a staging area the problem keeps: one pinned host buffer and one device buffer laid out
    // [q0 | targets | q_out | iters | success], so a call is two copies and a launch instead of five allocations, five
    // copies, a device synchronise and five frees.  A second thread calling on the same problem meanwhile takes the pipelined path.
    const size_t off_t = nb_q, off_q = off_t + nb_t, off_i = off_q + nb_q, off_s = off_i + sizeof(int32_t) * B;
    const size_t off_7 = (off_s + B + 7) / 8 * 8;                  // (pose7 targets land behind everything else)
    const size_t total = off_7 + nb_t7;
    if (total > kStageLimit) return kNotStaged;
    std::unique_lock<std::mutex> lock(p->stage.mu, std::try_to_lock);
    if (!lock.owns_lock()) return kNotStaged;
    Staging &st = p->stage;
    if (st.cap < total) {
        st.release();
        const size_t cap = std::max<size_t>(total, 4096);
        if (hipMalloc(&st.dev, cap) == hipSuccess && hipHostMalloc(&st.host, cap, hipHostMallocDefault) == hipSuccess) st.cap = cap;
    }
    if (st.cap < total) return kNotStaged;
    char *h = static_cast<char *>(st.host), *d = static_cast<char *>(st.dev);
    std::memcpy(h, q0, nb_q);
    hipError_t e = hipSuccess;
    if (pose7) {
        std::memcpy(h + off_7, targets, nb_t7);
        e = hipMemcpy(d, h, nb_q, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + off_7, h + off_7, nb_t7, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = ikgpu::launch_targets_from_pose7(B, p->host.ntasks, reinterpret_cast<const double *>(d + off_7),
                                                                  reinterpret_cast<double *>(d + off_t), layout, nullptr);
    } else {
        std::memcpy(h + off_t, targets, nb_t);
        e = hipMemcpy(d, h, off_q, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return hip_fail(e, "host-pointer solve (staged copy in)");
    const int rc = launch(B, reinterpret_cast<double *>(d), reinterpret_cast<double *>(d + off_t), reinterpret_cast<double *>(d + off_q),
                          reinterpret_cast<uint8_t *>(d + off_s), reinterpret_cast<int32_t *>(d + off_i), nullptr);
    if (rc != IKGPU_OK) return rc;
    e = hipMemcpy(h + off_q, d + off_q, total - off_q, hipMemcpyDeviceToHost);   // waits for the launch on the null stream
    if (e != hipSuccess) return hip_fail(e, "host-pointer solve (staged copy out)");
    std::memcpy(q_out, h + off_q, nb_q);
    if (iters) std::memcpy(iters, h + off_i, sizeof(int32_t) * B);
    if (success) std::memcpy(success, h + off_s, B);
    return static_cast<int>(IKGPU_OK);
}

// ... and every other batch: the pipelined path.  Chunk k lives compactly on the device ([rows][b_k], component-major, or [b_k][rows]);
// for the component-major layout one 2-D copy per array gathers / scatters the chunk's columns of the caller's [rows][B] arrays.
// Pinned caller buffers make every copy asynchronous; pageable ones still work (the runtime stages them).
template <class Launch>
int solve_pipelined(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets, double *q_out, uint8_t *success, int32_t *iters,
                    int layout, bool pose7, Launch &launch) {
    static HostTrace trace;
    const double t_enter = trace.on ? HostTrace::now() : 0.0;
    std::lock_guard<std::mutex> plock(p->pipe.mu);
    const double t_locked = trace.on ? HostTrace::now() : 0.0;
    HostPipe &pp = p->pipe;
    // Chunks that fill the device: one problem per lane means a launch lasts as long as ONE wave whatever its size, and kernels of
    // different streams were measured NOT to overlap here (B = 65536 in 8 chunks on 8 streams: 0.93 ms; 2 chunks: 0.55 ms; 1 chunk,
    // i.e. no overlap at all: 0.61 ms; tools/host_entry_timing.py) -- so two halves up to 131072 problems, 65536 per chunk above
    // (B = 262144: 1.49 ms against 2.21 unpipelined).
    int64_t chunk = B <= 131072 ? ((B + 1) / 2 + 63) / 64 * 64 : 65536;
    if (const char *env = std::getenv("IKGPU_HOST_CHUNK")) { const long c = std::strtol(env, nullptr, 10); if (c >= 64) chunk = c; }
    const int64_t nchunks = (B + chunk - 1) / chunk;
    const size_t nq = static_cast<size_t>(p->host.nq), nt = static_cast<size_t>(12 * p->host.ntasks);
    const size_t nt7 = pose7 ? static_cast<size_t>(7 * p->host.ntasks) : 0;
    const size_t per_problem = 8 * nq + 8 * nt + 8 * nq + 4 + 1 + 8 * nt7;
    const size_t need = per_problem * static_cast<size_t>(B) + 64 * static_cast<size_t>(nchunks) * 6;   // (every array 64-byte aligned)
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    if (!pp.in) {
        step(hipStreamCreateWithFlags(&pp.in, hipStreamNonBlocking));
        step(hipStreamCreateWithFlags(&pp.out, hipStreamNonBlocking));
        for (hipStream_t &r : pp.run) step(hipStreamCreateWithFlags(&r, hipStreamNonBlocking));
    }
    if (e == hipSuccess && pp.cap < need) {
        if (pp.dev) { (void)hipFree(pp.dev); pp.dev = nullptr; pp.cap = 0; }   // (every call leaves its streams idle)
        step(hipMalloc(&pp.dev, need));
        if (e == hipSuccess) pp.cap = need;
    }
    while (e == hipSuccess && static_cast<int64_t>(pp.ev_in.size()) < nchunks) {
        hipEvent_t a = nullptr, b = nullptr;
        step(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        step(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        if (e == hipSuccess) { pp.ev_in.push_back(a); pp.ev_run.push_back(b); }
    }
    if (e != hipSuccess) return hip_fail(e, "host-pointer solve (pipeline set-up)");
    char *cur = static_cast<char *>(pp.dev);
    auto take = [&](size_t bytes) { char *r = cur; cur += (bytes + 63) / 64 * 64; return r; };
    const bool soa = layout == IKGPU_SOA;
    // rows x [b0, b0 + bk) of a host array with B columns  <->  a compact rows x bk device array (SoA), or bk x rows contiguous (AoS)
    auto copy = [&](void *dev, const void *host_c, void *host, size_t rows, size_t elem, int64_t b0, int64_t bk, bool to_device, hipStream_t st) {
        if (soa && rows > 1) {
            const size_t w = static_cast<size_t>(bk) * elem, hp = static_cast<size_t>(B) * elem;
            return to_device ? hipMemcpy2DAsync(dev, w, static_cast<const char *>(host_c) + static_cast<size_t>(b0) * elem, hp, w, rows, hipMemcpyHostToDevice, st)
                             : hipMemcpy2DAsync(static_cast<char *>(host) + static_cast<size_t>(b0) * elem, hp, dev, w, w, rows, hipMemcpyDeviceToHost, st);
        }
        const size_t off = static_cast<size_t>(b0) * rows * elem, bytes = static_cast<size_t>(bk) * rows * elem;
        return to_device ? hipMemcpyAsync(dev, static_cast<const char *>(host_c) + off, bytes, hipMemcpyHostToDevice, st)
                         : hipMemcpyAsync(static_cast<char *>(host) + off, dev, bytes, hipMemcpyDeviceToHost, st);
    };
    int rc = IKGPU_OK;
    const double t_setup = trace.on ? HostTrace::now() : 0.0;
    for (int64_t k = 0; k < nchunks && rc == IKGPU_OK && e == hipSuccess; ++k) {
        const int64_t b0 = k * chunk, bk = std::min<int64_t>(chunk, B - b0);
        double *d_q0 = reinterpret_cast<double *>(take(8 * nq * bk)), *d_t = reinterpret_cast<double *>(take(8 * nt * bk));
        double *d_q = reinterpret_cast<double *>(take(8 * nq * bk));
        int32_t *d_i = reinterpret_cast<int32_t *>(take(4 * bk));
        uint8_t *d_s = reinterpret_cast<uint8_t *>(take(bk));
        double *d_t7 = pose7 ? reinterpret_cast<double *>(take(8 * nt7 * bk)) : nullptr;
        step(copy(d_q0, q0, nullptr, nq, 8, b0, bk, true, pp.in));
        if (pose7) step(copy(d_t7, targets, nullptr, nt7, 8, b0, bk, true, pp.in));
        else step(copy(d_t, targets, nullptr, nt, 8, b0, bk, true, pp.in));
        step(hipEventRecord(pp.ev_in[k], pp.in));
        const hipStream_t run = pp.run[k % HostPipe::kRunStreams];
        step(hipStreamWaitEvent(run, pp.ev_in[k], 0));
        if (pose7) step(ikgpu::launch_targets_from_pose7(bk, p->host.ntasks, d_t7, d_t, layout, run));
        if (e != hipSuccess) break;
        rc = launch(bk, d_q0, d_t, d_q, d_s, d_i, run);
        if (rc != IKGPU_OK) break;
        step(hipEventRecord(pp.ev_run[k], run));
        step(hipStreamWaitEvent(pp.out, pp.ev_run[k], 0));
        step(copy(d_q, nullptr, q_out, nq, 8, b0, bk, false, pp.out));
        if (iters) step(copy(d_i, nullptr, iters, 1, 4, b0, bk, false, pp.out));
        if (success) step(copy(d_s, nullptr, success, 1, 1, b0, bk, false, pp.out));
    }
    // The arena is reused by the next call: everything in flight has to land first.  When every chunk was enqueued, the copy-out
    // stream is the LAST link of every chain (in -> run[k] -> out, by events), so one wait on it covers all three; after a failure
    // half way through every stream that was touched is waited for.  (Round 3 waited for all ten streams, used or not.)
    const double t_enqueued = trace.on ? HostTrace::now() : 0.0;
    hipError_t w = hipSuccess;
    if (rc != IKGPU_OK || e != hipSuccess) {
        w = hipStreamSynchronize(pp.in);
        for (int64_t k = 0; k < std::min<int64_t>(nchunks, HostPipe::kRunStreams); ++k) { const hipError_t x = hipStreamSynchronize(pp.run[k]); if (w == hipSuccess) w = x; }
    }
    { const hipError_t x = hipStreamSynchronize(pp.out); if (w == hipSuccess) w = x; }
    if (trace.on) {
        const double t_done = HostTrace::now();
        std::fprintf(trace.f, "B %lld chunks %lld total_ms %.4f lock %.4f setup %.4f enqueue %.4f wait %.4f\n", static_cast<long long>(B),
                     static_cast<long long>(nchunks), t_done - t_enter, t_locked - t_enter, t_setup - t_locked, t_enqueued - t_setup, t_done - t_enqueued);
        std::fflush(trace.f);
    }
    if (rc != IKGPU_OK) return rc;
    step(w);
    if (e != hipSuccess) return hip_fail(e, "host-pointer solve (pipeline)");
    return static_cast<int>(IKGPU_OK);
}

// Host-pointer form of a batched solve, on the problem's device: the staging area when it takes the batch, else the pipeline.
template <class Launch>
int host_solve(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets, double *q_out, uint8_t *success,
               int32_t *iters, int layout_in, Launch &&launch) {
    const bool pose7 = (layout_in & IKGPU_TARGETS_POSE7) != 0;   // targets arrive as 7 doubles per task and are expanded on the device
    const int layout = layout_in & ~IKGPU_TARGETS_POSE7;
    return on_device(p->device, nullptr, [&](hipStream_t) {
        const int rc = solve_staged(p, B, q0, targets, q_out, success, iters, layout, pose7, launch);
        return rc != kNotStaged ? rc : solve_pipelined(p, B, q0, targets, q_out, success, iters, layout, pose7, launch);
    });
}

int dispatch_dls(const ikgpu_problem *p, const ikgpu::BatchIO &io, const ikgpu_dls_params *params, hipStream_t st);

}  // namespace

extern "C" {

int ikgpu_abi_version(void) { return IKGPU_ABI_VERSION; }

const char *ikgpu_last_error(void) { return g_last_error.c_str(); }

void ikgpu_dls_params_default(ikgpu_dls_params *p) {
    if (!p) return;
    p->max_iterations = 100;  // reference ik/ik/common.hpp:61
    p->damping = 1e-2;        // reference ik/ik/dls.hpp:25
    p->step_length = 1.0;     // reference ik/ik/common.hpp:65
    p->stop_sq_tol = 1e-4;    // reference ik/ik/visitor.hpp:19
    p->dq_sq_tol = 0.0;       // the derived-visitor family: off (the reference's own visitor)
    p->num_level_tols = 0;
    for (double &t : p->level_sq_tol) t = 0.0;
}

int ikgpu_model_from_urdf(const char *xml, size_t len, int root_joint, ikgpu_model **out) {
    if (!xml || !out) return null_argument();
    if (root_joint != IKGPU_ROOT_FIXED && root_joint != IKGPU_ROOT_FREEFLYER)
        return fail(IKGPU_ERR_INVALID, "root_joint must be IKGPU_ROOT_FIXED or IKGPU_ROOT_FREEFLYER");
    *out = nullptr;
    try {
        auto *h = new ikgpu_model{ikgpu::Model::from_urdf(xml, len, root_joint == IKGPU_ROOT_FREEFLYER)};
        h->m.finalize();  // name views must point into the final object
        *out = h;
        return IKGPU_OK;
    } catch (const std::exception &e) {
        return fail(IKGPU_ERR_PARSE, e.what());
    } catch (...) {
        return fail(IKGPU_ERR_PARSE, "unknown C++ exception");
    }
}

int ikgpu_model_create(const ikgpu_flat_model *flat, ikgpu_model **out) {
    if (!flat || !out) return null_argument();
    *out = nullptr;
    return guarded([&] {
        auto *h = new ikgpu_model{ikgpu::Model::from_flat(*flat)};
        h->m.finalize();
        *out = h;
        return static_cast<int>(IKGPU_OK);
    });
}

void ikgpu_model_destroy(ikgpu_model *m) { delete m; }

int ikgpu_model_get_flat(const ikgpu_model *h, ikgpu_flat_model *out) {
    if (!h || !out) return null_argument();
    const ikgpu::Model &m = h->m;
    out->njoints = m.njoints();
    out->nq = m.nq;
    out->nv = m.nv;
    out->nframes = m.nframes();
    out->joint_type = m.joint_type.data();
    out->joint_parent = m.joint_parent.data();
    out->joint_idx_q = m.joint_idx_q.data();
    out->joint_idx_v = m.joint_idx_v.data();
    out->joint_placement = m.joint_placement.empty() ? nullptr : m.joint_placement[0].data();
    out->joint_axis = m.joint_axis.empty() ? nullptr : m.joint_axis[0].data();
    out->joint_mass = m.joint_mass.data();
    out->joint_com = m.joint_com.empty() ? nullptr : m.joint_com[0].data();
    out->lower = m.lower.data();
    out->upper = m.upper.data();
    out->frame_parent = m.frame_parent.data();
    out->frame_placement = m.frame_placement.empty() ? nullptr : m.frame_placement[0].data();
    out->joint_names = m.joint_name_ptrs.data();
    out->frame_names = m.frame_name_ptrs.data();
    return IKGPU_OK;
}

int32_t ikgpu_model_frame_id(const ikgpu_model *h, const char *name) {
    if (!h || !name) return -1;
    return h->m.frame_id(name);
}

int32_t ikgpu_model_joint_id(const ikgpu_model *h, const char *name) {
    if (!h || !name) return -1;
    return h->m.joint_id(name);
}

int ikgpu_problem_create(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, int32_t device,
                         ikgpu_problem **out) {
    return ikgpu_problem_create_constrained(h, tasks, ntasks, nullptr, 0, device, out);
}

int ikgpu_problem_create_constrained(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                                     int32_t nconstraints, int32_t device, ikgpu_problem **out) {
    if (!out) return null_argument();
    if (int rc = check_problem_inputs(h, tasks, constraints, nconstraints)) return rc;
    *out = nullptr;
    return guarded([&] {
        KernelPlan plan = plan_kernels(h->m, tasks, ntasks, constraints, nconstraints, /*compile=*/true);

        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) return fail(IKGPU_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
        if (device < 0 || device >= ndev) return fail(IKGPU_ERR_INVALID, "device ordinal out of range");
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(IKGPU_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

        return on_device(device, nullptr, [&](hipStream_t) {
            std::unique_ptr<ikgpu_problem> p(new ikgpu_problem(device));   // (a failure below deletes it, and with it what was uploaded)
            p->host = std::move(plan.host);
            p->gen = std::move(plan.gen);
            p->dls_on_static_gen = plan.dls_on_static_gen;
            p->dls_name = plan.name;
            {
                std::string gname = p->gen.kernel_name;   // ("...,static>": the DLS program's build, not ik::pik's)
                const size_t st = gname.find(",static>");
                if (st != std::string::npos) gname = gname.substr(0, st) + ">";
                p->pik_name = "pik_generic" + gname.substr(std::min(gname.find('<'), gname.size()));
            }
            p->pik_static_name = p->pik_name.substr(0, p->pik_name.size() - 1) + ",static>";
            p->pik_tree_name = p->host.kernel_name.substr(0, p->host.kernel_name.size() - (p->host.kernel_name.empty() ? 0 : 1)) + ",pik_levels=2>";
            p->nframes = h->m.nframes();
            const size_t nq = static_cast<size_t>(p->host.nq);
            hipError_t err = hipSuccess;
            auto up = [&](auto **dst, const void *src, size_t bytes) {
                if (err != hipSuccess) return;
                err = hipMalloc(reinterpret_cast<void **>(dst), bytes ? bytes : 8);
                if (err == hipSuccess && bytes) err = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
            };
            up(&p->dev.lower, p->host.lower.data(), nq * sizeof(double));
            up(&p->dev.upper, p->host.upper.data(), nq * sizeof(double));
            up(&p->dev.q_in_chain, p->host.q_in_chain.data(), nq);
            p->draw = ikgpu::multistart_draw_mask(h->m, p->host);
            up(&p->dev.draw, p->draw.data(), nq);
            up(&p->dev.g_ints, p->gen.generic.ints.data(), p->gen.generic.ints.size() * sizeof(int32_t));
            up(&p->dev.g_dbls, p->gen.generic.dbls.data(), p->gen.generic.dbls.size() * sizeof(double));
            if (err == hipSuccess) err = p->dev.queues.grow();
            if (p->host.kind != ikgpu::KernelKind::Generic) {
                const std::vector<double> desc = p->host.kind == ikgpu::KernelKind::Chain ? ikgpu::chain_desc_table(p->host)
                                                                                         : ikgpu::tree_desc_table(p->host);
                up(&p->dev.chain_desc, desc.data(), desc.size() * sizeof(double));
            }
            if (err != hipSuccess) return hip_fail(err, "uploading problem tables");
            *out = p.release();
            return static_cast<int>(IKGPU_OK);
        });
    });
}

int ikgpu_problem_plan(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, char *out, size_t cap) {
    return ikgpu_problem_plan_constrained(h, tasks, ntasks, nullptr, 0, out, cap);
}

int ikgpu_problem_plan_constrained(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                                   int32_t nconstraints, char *out, size_t cap) {
    if (int rc = check_problem_inputs(h, tasks, constraints, nconstraints)) return rc;
    return guarded([&] {
        copy_name(plan_kernels(h->m, tasks, ntasks, constraints, nconstraints, /*compile=*/false).name, out, cap);
        return static_cast<int>(IKGPU_OK);
    });
}

int ikgpu_dls_tree_build_plan(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                              int32_t nconstraints, const ikgpu_dls_params *params, int32_t pik_levels, char *out, size_t cap) {
    if (int rc = check_problem_inputs(h, tasks, constraints, nconstraints)) return rc;
    if (int rc = check_have_params(params)) return rc;
    if (int rc = refuse_if(pik_levels < 0 || pik_levels > 2, "pik_levels must be 0 (ik::dls), 1 or 2")) return rc;
    return guarded([&] {
        const KernelPlan k = plan_kernels(h->m, tasks, ntasks, constraints, nconstraints, /*compile=*/false);
        std::string name;
        if (k.host.kind == ikgpu::KernelKind::Tree) {
            // ik::pik with two levels goes to the tree kernel by itself (ikgpu_pik_solve_batch); with one level it is the DLS iteration
            // and takes ik::dls's route (dispatch_dls: the static lane program first where the plan prefers it, a derived visitor never here)
            const bool pik_tree = pik_levels == 2 && k.gen.generic.nlevels == 2 && k.host.constraints.empty() && !pik_forced(/*or_static=*/true) &&
                                  ikgpu::tree_takes_two_level_pik(k.host);
            const bool dls_tree = pik_levels != 2 && !(pik_levels == 1 && (k.gen.generic.nlevels != 1 || !k.host.constraints.empty() || pik_forced(true))) &&
                                  !k.dls_on_static_gen && !ikgpu::visitor_extended(*params);
            if (pik_tree || dls_tree) {
                const ikgpu::TreeBuild b = ikgpu::select_tree_build(k.host, *params, pik_tree);
                if (b.launchable) name = ikgpu::tree_build_name(b);
            }
        }
        copy_name(name, out, cap);
        return static_cast<int>(IKGPU_OK);
    });
}

int ikgpu_problem_precompile(const ikgpu_model *h, const ikgpu_task *tasks, int32_t ntasks, const ikgpu_task *constraints,
                             int32_t nconstraints, char *out, size_t cap) {
    if (int rc = check_problem_inputs(h, tasks, constraints, nconstraints)) return rc;
    return guarded([&] {
        const std::string want = plan_kernels(h->m, tasks, ntasks, constraints, nconstraints, /*compile=*/false).name;
        const KernelPlan got = plan_kernels(h->m, tasks, ntasks, constraints, nconstraints, /*compile=*/true);
        // the refill twin of the static lane program ik::dls runs on, a Tree problem's or a Generic problem's own
        if (got.dls_on_static_gen) (void)ikgpu::rtc_generic_static_precompile_refill(got.gen);
        else if (got.host.generic_build == 2) (void)ikgpu::rtc_generic_static_precompile_refill(got.host);
        // a problem with several priority levels may be handed to ik::pik: its compiled lane program (without the secondary step)
        // (one level needs the program only for a secondary step, da != 0: compiled at the first such call)
        if (got.gen.generic.nlevels >= 2 && ikgpu::rtc_pik_static_available(got.gen, false, /*compile=*/false, nullptr))
            (void)ikgpu::rtc_pik_static_available(got.gen, false, /*compile=*/true, nullptr);
        copy_name(got.name, out, cap);
        if (want != got.name)   // planned a run-time compiled build, got the pre-built one
            return fail(IKGPU_ERR_UNSUPPORTED, "run-time compilation failed, the problem runs on " + got.name + ": " + ikgpu::rtc_last_log());
        return static_cast<int>(IKGPU_OK);
    });
}

void ikgpu_problem_destroy(ikgpu_problem *p) { delete p; }

int32_t ikgpu_problem_rows(const ikgpu_problem *p) { return p ? p->host.rows : -1; }

const char *ikgpu_problem_kernel(const ikgpu_problem *p) { return p ? p->dls_name.c_str() : ""; }

int ikgpu_problem_support(const ikgpu_problem *p, uint8_t *support) {
    if (!p || !support) return fail(IKGPU_ERR_INVALID, "ikgpu_problem_support: null argument");
    for (int i = 0; i < p->host.nq; ++i) support[i] = p->host.q_in_chain[static_cast<size_t>(i)] ? 1 : 0;
    return IKGPU_OK;
}

int ikgpu_dls_solve_batch(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                          const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters, int layout,
                          void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null)
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        return dispatch_dls(p, ikgpu::BatchIO{B, q0, targets, q_out, success, iters, layout}, params, st);
    });
}

}  // extern "C"

namespace {

// The kernel dispatch of ikgpu_dls_solve_batch for validated arguments, inside on_device.  ikgpu_dls_track_batch loops over it for
// the problem kinds without a tracking kernel, run_starts for the multi-start and solution-set definitions.
int dispatch_dls(const ikgpu_problem *p, const ikgpu::BatchIO &io, const ikgpu_dls_params *params, hipStream_t st) {
    if (ikgpu::visitor_extended(*params)) {
        // a derived visitor (step tolerance / per-level tolerances): the generic lane program implements the family -- the one
        // specialised for this problem when there is one, else its memory-resident per-lane form
        if (p->gen.generic_build != 2)
            std::call_once(p->visitor_static_once, [&] {
                p->visitor_static = ikgpu::rtc_generic_static_available(p->gen, /*compile=*/true, &p->visitor_static_key);
            });
        const bool on_static = p->gen.generic_build == 2 || p->visitor_static;
        const uint64_t key = p->gen.generic_build == 2 ? p->gen.generic_key : p->visitor_static_key;
        const hipError_t ev = on_static ? ikgpu::rtc_launch_generic_static(p->gen, key, io, *params, st, p->dev.queues)
                                        : ikgpu::launch_dls_generic(p->gen, p->dev, io, *params, st, /*force_lane=*/true);
        return launched(ev, "launching the generic DLS kernel (derived visitor)");
    }
    hipError_t e = p->dls_on_static_gen                      ? ikgpu::rtc_launch_generic_static(p->gen, p->gen.generic_key, io, *params, st, p->dev.queues)
                   : p->host.kind == ikgpu::KernelKind::Chain  ? ikgpu::launch_dls_chain(p->host, p->dev, io, ikgpu::ChainJob{}, *params, st)
                   : p->host.kind == ikgpu::KernelKind::Tree ? ikgpu::launch_dls_tree(p->host, p->dev, io, *params, st)
                   : p->host.generic_build == 2              ? ikgpu::rtc_launch_generic_static(p->host, p->host.generic_key, io, *params, st, p->dev.queues)
                                                             : ikgpu::launch_dls_generic(p->host, p->dev, io, *params, st);
    return launched(e, "launching the DLS kernel");
}

// The kernel dispatch of ikgpu_evaluate_batch for validated arguments, inside on_device.
int dispatch_eval(const ikgpu_problem *p, int64_t B, const double *q, const double *targets, double *e_out, double *J_out, int layout, hipStream_t st) {
    hipError_t e = p->host.kind == ikgpu::KernelKind::Chain  ? ikgpu::launch_eval_chain(p->host, p->dev, B, q, targets, e_out, J_out, layout, st)
                   // (a tree problem with the demo's extras -- base-relative reference, alignment row -- has its stages evaluated
                   // by the generic program: the tree stage kernel does not know them)
                   : p->host.kind == ikgpu::KernelKind::Tree && !p->host.tree_extras()
                       ? ikgpu::launch_eval_tree(p->host, p->dev, B, q, targets, e_out, J_out, nullptr, layout, st)
                       : ikgpu::launch_eval_generic(p->gen, p->dev, B, q, targets, e_out, J_out, nullptr, layout, st);
    return launched(e, "launching the evaluate kernel");
}

// A chain problem under the reference's own visitor has a tracking kernel: one launch for the whole sequence.
bool track_is_fused(const ikgpu_problem *p, const ikgpu_dls_params *params) {
    return p->host.kind == ikgpu::KernelKind::Chain && !p->dls_on_static_gen && !ikgpu::visitor_extended(*params);
}

// ... and a multi-start kernel when the K starts of a problem are a power-of-two group of lanes of one wave: log2 K, else -1.
int multistart_fused_log2(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K) {
    if (!track_is_fused(p, params) || K < 2 || K > 64 || (K & (K - 1)) != 0) return -1;
    int l = 0;
    while ((1 << l) < K) ++l;
    return l;
}

// ... and a goal-set kernel when the G x K candidates of a problem are such a group: G and K powers of two, 2 <= G K <= 64.
bool goalset_fused_log2(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t G, int32_t K, int *log2G, int *log2K) {
    if (!track_is_fused(p, params) || G < 1 || K < 1 || G > 64 || K > 64 || G * K < 2 || G * K > 64 || (G & (G - 1)) != 0 || (K & (K - 1)) != 0)
        return false;
    *log2G = *log2K = 0;
    while ((1 << *log2G) < G) ++*log2G;
    while ((1 << *log2K) < K) ++*log2K;
    return true;
}

// G goals x K starts per problem, at most 64 candidates.  report: false = the answer only (a query), no message.
int check_goalset_size(int32_t G, int32_t K, bool report) {
    const bool bad_g = G < 1 || G > 64, bad_k = K < 1 || K > 64;
    if (!report) return (bad_g || bad_k || G * K > 64) ? IKGPU_ERR_INVALID : IKGPU_OK;
    if (int rc = refuse_if(bad_g, "the number of goals must be 1 .. 64")) return rc;
    if (int rc = check_starts(K)) return rc;
    return refuse_if(G * K > 64, "goals x starts must be at most 64 candidates per problem");
}

// What a tracking or multi-start call runs: the fused kernel, "dls_chain<NJ=7,full,hot>" -> "dls_chain_track<NJ=7,full,hot>" for the
// suffix "_track", or the loop over the single solve.
std::string variant_kernel_name(const ikgpu_problem *p, bool fused, const char *suffix) {
    if (!fused) return "loop(" + p->dls_name + ")";
    const size_t lt = p->dls_name.find('<');
    return p->dls_name.substr(0, lt) + suffix + (lt == std::string::npos ? "" : p->dls_name.substr(lt));
}

// What the multi-start and the solution-set entry points share: K starts of each of B problems, supplied (`starts`, K - 1 slabs) or
// drawn from `seed`, and the workspace of the definition run as a loop.
struct StartsCall {
    int64_t B;
    int32_t K;
    const double *q0, *starts;
    uint64_t seed;
    const double *targets;
    const ikgpu_dls_params *params;
    int layout;
    void *workspace;
    size_t workspace_bytes;
};

// The workspace of a definition run as a loop, carved in this order (each part rounded up to 256 bytes): generated start [nq x B], q of
// the start's solve [nq x B], its iterations [B], its success flag [B], and for the multi-start merge (with_error) its error [M x B] and
// the best key [B].  A solution set lives in the caller's outputs.
struct StartWorkspace {
    size_t start, q, iters, success, e, key, total;
};
StartWorkspace start_workspace(const ikgpu_problem *p, int64_t B, bool with_error) {
    size_t end = 0;
    auto take = [&](size_t n) { const size_t at = end; end += (n + 255) / 256 * 256; return at; };
    const size_t b = static_cast<size_t>(B), nq = static_cast<size_t>(p->host.nq), M = static_cast<size_t>(p->host.rows);
    StartWorkspace w{};
    w.start = take(8 * nq * b);
    w.q = take(8 * nq * b);
    w.iters = take(4 * b);
    w.success = take(b);
    if (with_error) {
        w.e = take(8 * M * b);
        w.key = take(8 * b);
    }
    w.total = end;
    return w;
}

// The definition itself, start after start on the same stream: start k drawn unless supplied, solved, and handed to
// step(k, q, ok, it, e, key) -- the solve's outputs and the merge's two arrays in the workspace -- which folds it into the caller's
// outputs.  `what` / `query` name the definition and its workspace query in the refusal of a workspace that is too small.
template <class Step>
int run_starts(const ikgpu_problem *p, const StartsCall &c, const char *what, const char *query, bool with_error, hipStream_t st, Step &&step) {
    const StartWorkspace w = start_workspace(p, c.B, with_error);
    if (!c.workspace || c.workspace_bytes < w.total)
        return fail(IKGPU_ERR_INVALID, std::string(what) + " workspace too small: " + std::to_string(c.workspace_bytes) + " bytes given, " +
                                           std::to_string(w.total) + " needed (" + query + ")");
    char *ws = static_cast<char *>(c.workspace);
    double *start = reinterpret_cast<double *>(ws + w.start), *q = reinterpret_cast<double *>(ws + w.q), *e = with_error ? reinterpret_cast<double *>(ws + w.e) : nullptr;
    unsigned long long *key = with_error ? reinterpret_cast<unsigned long long *>(ws + w.key) : nullptr;
    int32_t *it = reinterpret_cast<int32_t *>(ws + w.iters);
    uint8_t *ok = reinterpret_cast<uint8_t *>(ws + w.success);
    const int64_t q_slab = static_cast<int64_t>(p->host.nq) * c.B;
    for (int k = 0; k < c.K; ++k) {
        auto named = [&](int rc) {
            g_last_error = "start " + std::to_string(k) + ": " + g_last_error;
            return rc;
        };
        const double *from = k == 0 ? c.q0 : c.starts ? c.starts + (k - 1) * q_slab : start;
        if (k > 0 && !c.starts) {
            const hipError_t ed = ikgpu::launch_multistart_starts(p->dev, p->host.nq, c.B, k, k + 1, c.q0, c.seed, start, c.layout, st);
            if (ed != hipSuccess) return named(hip_fail(ed, "launching the multi-start draw"));
        }
        if (const int rc = dispatch_dls(p, ikgpu::BatchIO{c.B, from, c.targets, q, ok, it, c.layout}, c.params, st)) return named(rc);
        if (const int rc = step(k, q, ok, it, e, key)) return named(rc);
    }
    return static_cast<int>(IKGPU_OK);
}

}  // namespace

extern "C" {

const char *ikgpu_dls_track_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, track_is_fused(p, params), "_track");
    return name.c_str();
}

int ikgpu_dls_track_batch(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *targets,
                          const ikgpu_dls_params *params, double *q_traj, uint8_t *success, int32_t *iters, int layout,
                          void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (T < 0) return fail(IKGPU_ERR_INVALID, "negative number of waypoints");
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (B == 0 || T == 0) return IKGPU_OK;  // nothing to solve (the pointers may be null; the problem is not looked at)
    if (!q0 || !targets || !q_traj) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (T > 0x7fffffff) return fail(IKGPU_ERR_INVALID, "too many waypoints for one call");
    return on_device(p->device, stream, [&](hipStream_t st) {
        if (track_is_fused(p, params)) {
            const ikgpu::BatchIO io{B, q0, targets, q_traj, success, iters, layout};
            const ikgpu::ChainJob job{ikgpu::ChainJob::Track, static_cast<int>(T)};
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the DLS tracking kernel");
        }
        // every other kind: the chained calls themselves, on the same stream
        const int64_t q_slab = static_cast<int64_t>(p->host.nq) * B, t_slab = static_cast<int64_t>(p->host.ntasks) * 12 * B;
        for (int64_t k = 0; k < T; ++k) {
            const ikgpu::BatchIO io{B, k == 0 ? q0 : q_traj + (k - 1) * q_slab, targets + k * t_slab, q_traj + k * q_slab,
                                    success ? success + k * B : nullptr, iters ? iters + k * B : nullptr, layout};
            if (const int rc = dispatch_dls(p, io, params, st)) {
                g_last_error = "waypoint " + std::to_string(k) + ": " + g_last_error;
                return rc;
            }
        }
        return static_cast<int>(IKGPU_OK);
    });
}

}  // extern "C"

namespace {

// ikgpu_line_targets takes a problem whose every target slot is a FrameTask's pose in a reference frame fixed in the world.
int check_line_slots(const ikgpu_problem *p) {
    const ikgpu::ProblemHost &g = p->gen;   // (the generic analysis: every kind has one, slot i is task i)
    for (int i = 0; i < g.ntasks; ++i) {
        const int type = g.tasks[static_cast<size_t>(i)].type;
        if (type != IKGPU_POSITION && type != IKGPU_ORIENTATION && type != IKGPU_FULL)
            return fail(IKGPU_ERR_UNSUPPORTED, "target slot " + std::to_string(i) + " is not a FrameTask's pose (alignment, posture and "
                                                   "centre-of-mass slots have no line)");
        if (g.generic.ints[static_cast<size_t>(g.generic.o_trjoint + i)] != 0)
            return fail(IKGPU_ERR_UNSUPPORTED, "target slot " + std::to_string(i) + ": the reference frame moves with the configuration");
    }
    return IKGPU_OK;
}

// ikgpu_line_targets for validated arguments, inside on_device.
int dispatch_line_targets(const ikgpu_problem *p, int64_t B, int T, const double *q0, const double *goals, double *W, int layout, hipStream_t st) {
    if (p->host.kind == ikgpu::KernelKind::Chain)
        return launched(ikgpu::launch_line_targets_chain(p->host, p->dev, B, T, q0, goals, W, layout, st), "launching the line waypoint kernel");
    // every other kind: oMf(q0) of every slot into slab 0 (what ikgpu_task_frames_fk_batch launches), then the waypoints over it
    const hipError_t e = p->host.kind == ikgpu::KernelKind::Tree && !p->host.tree_extras()
                             ? ikgpu::launch_eval_tree(p->host, p->dev, B, q0, q0, nullptr, nullptr, W, layout, st)
                             : ikgpu::launch_eval_generic(p->gen, p->dev, B, q0, q0, nullptr, nullptr, W, layout, st);
    if (e != hipSuccess) return hip_fail(e, "launching the FK kernel");
    return launched(ikgpu::launch_line_targets_from_fk(B, p->gen.ntasks, T, p->dev.g_dbls + p->gen.generic.o_trpl, goals, W, layout, st),
                    "launching the line waypoint kernel");
}

// The workspace of the line definition run as a loop, carved as start_workspace: the waypoints [T][ntasks x 12 x B], then the success
// flags [T][B] (used when the caller passed none).
struct LineWorkspace {
    size_t targets, success, total;
};
LineWorkspace line_workspace(const ikgpu_problem *p, int64_t B, int64_t T) {
    size_t end = 0;
    auto take = [&](size_t n) { const size_t at = end; end += (n + 255) / 256 * 256; return at; };
    const size_t b = static_cast<size_t>(B), t = static_cast<size_t>(T);
    LineWorkspace w{};
    w.targets = take(8 * 12 * static_cast<size_t>(p->gen.ntasks) * b * t);
    w.success = take(b * t);
    w.total = end;
    return w;
}

int check_line_call(const ikgpu_problem *p, int64_t B, int64_t T, int layout) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = refuse_if(T < 0, "negative number of waypoints")) return rc;
    return check_layout(layout);
}

}  // namespace

extern "C" {

int ikgpu_line_targets(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *goals, double *W_out, int layout,
                       void *stream) {
    if (int rc = check_line_call(p, B, T, layout)) return rc;
    if (B == 0 || T == 0) return IKGPU_OK;  // nothing to write (the pointers may be null; the problem is not looked at)
    if (!q0 || !goals || !W_out) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (int rc = refuse_if(T > 0x7fffffff, "too many waypoints for one call")) return rc;
    if (int rc = check_line_slots(p)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) { return dispatch_line_targets(p, B, static_cast<int>(T), q0, goals, W_out, layout, st); });
}

const char *ikgpu_dls_line_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, track_is_fused(p, params), "_line");
    return name.c_str();
}

size_t ikgpu_dls_line_workspace_bytes(const ikgpu_problem *p, int64_t B, int64_t T, const ikgpu_dls_params *params) {
    if (!p || !params || B <= 0 || T <= 0 || track_is_fused(p, params)) return 0;
    return line_workspace(p, B, T).total;
}

int ikgpu_dls_line_batch(const ikgpu_problem *p, int64_t B, int64_t T, const double *q0, const double *goals, const ikgpu_dls_params *params,
                         double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached, int layout, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (int rc = check_line_call(p, B, T, layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (params->stop_sq_tol < 0.0 && !ikgpu::visitor_extended(*params))
        return fail(IKGPU_ERR_INVALID, "the never-stop visitor reaches no waypoint: a line needs a stop rule (stop_sq_tol >= 0)");
    if (B == 0 || T == 0) return IKGPU_OK;  // nothing to solve (the pointers may be null; the problem is not looked at)
    if (!q0 || !goals || !q_traj) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (int rc = refuse_if(T > 0x7fffffff, "too many waypoints for one call")) return rc;
    if (int rc = check_line_slots(p)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        if (track_is_fused(p, params)) {
            const ikgpu::BatchIO io{B, q0, goals, q_traj, success, iters, layout};
            ikgpu::ChainJob job{};
            job.kind = ikgpu::ChainJob::Line;
            job.line = ikdev::LineArgs{reached, static_cast<int>(T)};
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the DLS line kernel");
        }
        // every other kind: the definition itself -- the waypoints, the chained calls, the count of leading successes
        const LineWorkspace w = line_workspace(p, B, T);
        if (!workspace || workspace_bytes < w.total)
            return fail(IKGPU_ERR_INVALID, "line workspace too small: " + std::to_string(workspace_bytes) + " bytes given, " +
                                               std::to_string(w.total) + " needed (ikgpu_dls_line_workspace_bytes)");
        char *ws = static_cast<char *>(workspace);
        double *W = reinterpret_cast<double *>(ws + w.targets);
        uint8_t *ok = success ? success : reinterpret_cast<uint8_t *>(ws + w.success);
        if (const int rc = dispatch_line_targets(p, B, static_cast<int>(T), q0, goals, W, layout, st)) return rc;
        const int64_t q_slab = static_cast<int64_t>(p->host.nq) * B, t_slab = static_cast<int64_t>(p->host.ntasks) * 12 * B;
        for (int64_t k = 0; k < T; ++k) {
            const ikgpu::BatchIO io{B, k == 0 ? q0 : q_traj + (k - 1) * q_slab, W + k * t_slab, q_traj + k * q_slab, ok + k * B,
                                    iters ? iters + k * B : nullptr, layout};
            if (const int rc = dispatch_dls(p, io, params, st)) {
                g_last_error = "waypoint " + std::to_string(k) + ": " + g_last_error;
                return rc;
            }
        }
        if (!reached) return static_cast<int>(IKGPU_OK);
        return launched(ikgpu::launch_line_reached(B, static_cast<int>(T), ok, reached, st), "launching the line count");
    });
}

}  // extern "C"

namespace {

// What the path entry points share with the line's, and P segments: P >= 1, T >= 0, P T waypoints in a 32-bit count.
int check_path_call(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, int layout) {
    if (int rc = check_line_call(p, B, T, layout)) return rc;
    if (int rc = refuse_if(P < 1, "the number of via poses must be at least 1")) return rc;
    return refuse_if(T > 0 && P > 0x7fffffff / T, "too many waypoints for one call (P x T must fit 31 bits)");
}

// ikgpu_path_targets for validated arguments, inside on_device.
int dispatch_path_targets(const ikgpu_problem *p, int64_t B, int P, int T, const double *q0, const double *vias, double *W, int layout, hipStream_t st) {
    if (p->host.kind == ikgpu::KernelKind::Chain)
        return launched(ikgpu::launch_path_targets_chain(p->host, p->dev, B, P, T, q0, vias, W, layout, st), "launching the path waypoint kernel");
    // every other kind: oMf(q0) of every slot into slab 0, then the waypoints over it (dispatch_line_targets)
    const hipError_t e = p->host.kind == ikgpu::KernelKind::Tree && !p->host.tree_extras()
                             ? ikgpu::launch_eval_tree(p->host, p->dev, B, q0, q0, nullptr, nullptr, W, layout, st)
                             : ikgpu::launch_eval_generic(p->gen, p->dev, B, q0, q0, nullptr, nullptr, W, layout, st);
    if (e != hipSuccess) return hip_fail(e, "launching the FK kernel");
    return launched(ikgpu::launch_path_targets_from_fk(B, p->gen.ntasks, P, T, p->dev.g_dbls + p->gen.generic.o_trpl, vias, W, layout, st),
                    "launching the path waypoint kernel");
}

// ikgpu_dls_path_batch for validated arguments, inside on_device (T >= 1): the fused launch, or the definition run as a loop in `workspace`.
// ikgpu_dls_path_multistart_batch runs it from every start's entry result, and once more for the winner's trajectory.
int dispatch_path(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const double *q0, const double *vias, const ikgpu_dls_params *params,
                  double max_joint_step, double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached, int layout, void *workspace,
                  size_t workspace_bytes, hipStream_t st) {
    const int64_t N = P * T;
    if (track_is_fused(p, params)) {
        const ikgpu::BatchIO io{B, q0, vias, q_traj, success, iters, layout};
        ikgpu::ChainJob job{};
        job.kind = ikgpu::ChainJob::Path;
        job.path = ikdev::PathArgs{reached, static_cast<int>(T), static_cast<int>(P), max_joint_step};
        return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the DLS path kernel");
    }
    // every other kind: the definition itself -- the waypoints, the chained calls, the met rule over flags and joint steps
    const LineWorkspace w = line_workspace(p, B, N);
    if (!workspace || workspace_bytes < w.total)
        return fail(IKGPU_ERR_INVALID, "path workspace too small: " + std::to_string(workspace_bytes) + " bytes given, " +
                                           std::to_string(w.total) + " needed (ikgpu_dls_path_workspace_bytes)");
    char *ws = static_cast<char *>(workspace);
    double *W = reinterpret_cast<double *>(ws + w.targets);
    uint8_t *ok = success ? success : reinterpret_cast<uint8_t *>(ws + w.success);
    if (const int rc = dispatch_path_targets(p, B, static_cast<int>(P), static_cast<int>(T), q0, vias, W, layout, st)) return rc;
    const int64_t q_slab = static_cast<int64_t>(p->host.nq) * B, t_slab = static_cast<int64_t>(p->host.ntasks) * 12 * B;
    for (int64_t n = 0; n < N; ++n) {
        const ikgpu::BatchIO io{B, n == 0 ? q0 : q_traj + (n - 1) * q_slab, W + n * t_slab, q_traj + n * q_slab, ok + n * B,
                                iters ? iters + n * B : nullptr, layout};
        if (const int rc = dispatch_dls(p, io, params, st)) {
            g_last_error = "waypoint " + std::to_string(n) + ": " + g_last_error;
            return rc;
        }
    }
    if (!reached) return static_cast<int>(IKGPU_OK);
    const ikgpu::PathReached r{B, p->host.nq, static_cast<int>(N), layout, max_joint_step, p->dev.q_in_chain, ok, q0, q_traj, reached};
    return launched(ikgpu::launch_path_reached(r, st), "launching the path count");
}

}  // namespace

extern "C" {

int ikgpu_path_targets(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const double *q0, const double *vias, double *W_out, int layout,
                       void *stream) {
    if (int rc = check_path_call(p, B, P, T, layout)) return rc;
    if (B == 0 || T == 0) return IKGPU_OK;  // nothing to write (the pointers may be null; the problem is not looked at)
    if (!q0 || !vias || !W_out) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (int rc = check_line_slots(p)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        return dispatch_path_targets(p, B, static_cast<int>(P), static_cast<int>(T), q0, vias, W_out, layout, st);
    });
}

const char *ikgpu_dls_path_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, track_is_fused(p, params), "_path");
    return name.c_str();
}

size_t ikgpu_dls_path_workspace_bytes(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const ikgpu_dls_params *params) {
    if (!p || !params || B <= 0 || T <= 0 || P < 1 || P > 0x7fffffff / T || track_is_fused(p, params)) return 0;
    return line_workspace(p, B, P * T).total;   // the line loop's carving over P T waypoints: the waypoints, then the flags
}

int ikgpu_dls_path_batch(const ikgpu_problem *p, int64_t B, int64_t P, int64_t T, const double *q0, const double *vias,
                         const ikgpu_dls_params *params, double max_joint_step, double *q_traj, uint8_t *success, int32_t *iters,
                         int32_t *reached, int layout, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_path_call(p, B, P, T, layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (!(max_joint_step >= 0.0) || !std::isfinite(max_joint_step))
        return fail(IKGPU_ERR_INVALID, "max_joint_step must be finite and not negative (0: no joint-step rule)");
    if (params->stop_sq_tol < 0.0 && !ikgpu::visitor_extended(*params))
        return fail(IKGPU_ERR_INVALID, "the never-stop visitor reaches no waypoint: a path needs a stop rule (stop_sq_tol >= 0)");
    if (B == 0 || T == 0) return IKGPU_OK;  // nothing to solve (the pointers may be null; the problem is not looked at)
    if (!q0 || !vias || !q_traj) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (int rc = check_line_slots(p)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        return dispatch_path(p, B, P, T, q0, vias, params, max_joint_step, q_traj, success, iters, reached, layout, workspace, workspace_bytes, st);
    });
}

const char *ikgpu_dls_multistart_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, multistart_fused_log2(p, params, K) >= 0, "_multistart");
    return name.c_str();
}

size_t ikgpu_dls_multistart_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, const ikgpu_dls_params *params) {
    if (!p || !params || B <= 0 || K < 1 || K > 64 || multistart_fused_log2(p, params, K) >= 0) return 0;
    return start_workspace(p, B, /*with_error=*/true).total;
}

int ikgpu_multistart_starts(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, uint64_t seed, double *starts_out, int layout,
                            void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_starts(K)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (B == 0 || K == 1) return IKGPU_OK;   // start 0 is q0 itself: nothing to write
    if (!q0 || !starts_out) return null_argument();
    if (int rc = check_launch_size(B, K)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        return launched(ikgpu::launch_multistart_starts(p->dev, p->host.nq, B, 1, K, q0, seed, starts_out, layout, st), "launching the multi-start draw");
    });
}

int ikgpu_dls_multistart_batch(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, const double *starts, uint64_t seed,
                               const double *targets, const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int32_t *winner, double *err_sq, int layout, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_starts(K)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null; the problem is not looked at)
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_launch_size(B, K)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        const int log2K = multistart_fused_log2(p, params, K);
        if (log2K >= 0) {
            const ikgpu::BatchIO io{B, q0, targets, q_out, success, iters, layout};
            const ikgpu::ChainJob job{ikgpu::ChainJob::Multistart, 0, ikdev::MultistartArgs{starts, p->dev.draw, seed, winner, err_sq, log2K}};
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the multi-start DLS kernel");
        }
        // every other case: the definition itself, each start merged into the caller's outputs
        const StartsCall c{B, K, q0, starts, seed, targets, params, layout, workspace, workspace_bytes};
        return run_starts(p, c, "multi-start", "ikgpu_dls_multistart_workspace_bytes", /*with_error=*/true, st,
                          [&](int k, double *q, uint8_t *ok, int32_t *it, double *e, unsigned long long *key) {
                              if (const int rc = dispatch_eval(p, B, q, targets, e, nullptr, layout, st)) return rc;
                              const ikgpu::MultistartMerge m{B, p->host.nq, p->host.rows, layout, k, q, e, ok, it, key, q_out, success, iters, winner, err_sq};
                              return launched(ikgpu::launch_multistart_merge(m, st), "launching the multi-start merge");
                          });
    });
}

}  // extern "C"

namespace {

static_assert(ikdev::kPickMaxChain >= ikgpu::kMaxChain, "PickArgs::w holds a weight per chain joint");

bool pick_rule_known(int32_t rule) { return rule >= IKGPU_PICK_DISTANCE && rule <= IKGPU_PICK_MANIPULABILITY; }

// The workspace of the pick definition run as a loop: the multi-start loop's (start_workspace with the error), then the start's cost
// [B], its dense Jacobian [M x nv x B] and Gram matrix [M x M x B] (the MANIPULABILITY rule) and the weights [nq].
struct PickWorkspace {
    size_t cost, J, G, w, total;
};
PickWorkspace pick_workspace(const ikgpu_problem *p, int64_t B) {
    size_t end = start_workspace(p, B, /*with_error=*/true).total;
    auto take = [&](size_t n) { const size_t at = end; end += (n + 255) / 256 * 256; return at; };
    const size_t b = static_cast<size_t>(B), M = static_cast<size_t>(p->host.rows);
    PickWorkspace w{};
    w.cost = take(8 * b);
    w.J = take(8 * M * static_cast<size_t>(p->host.nv) * b);
    w.G = take(8 * M * M * b);
    w.w = take(8 * static_cast<size_t>(p->host.nq));
    w.total = end;
    return w;
}

}  // namespace

extern "C" {

const char *ikgpu_dls_pick_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K, int32_t rule) {
    if (!p || !params || !pick_rule_known(rule)) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, multistart_fused_log2(p, params, K) >= 0, "_pick");
    return name.c_str();
}

size_t ikgpu_dls_pick_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, const ikgpu_dls_params *params) {
    if (!p || !params || B <= 0 || K < 1 || K > 64 || multistart_fused_log2(p, params, K) >= 0) return 0;
    return pick_workspace(p, B).total;
}

int ikgpu_dls_pick_batch(const ikgpu_problem *p, int64_t B, int32_t K, const double *q0, const double *starts, uint64_t seed,
                         const double *targets, const ikgpu_dls_params *params, int32_t rule, const double *q_ref, const double *w,
                         double *q_out, uint8_t *success, int32_t *iters, int32_t *winner, double *cost, double *err_sq, int layout,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_starts(K)) return rc;
    if (int rc = refuse_if(!pick_rule_known(rule), "unknown pick rule (ikgpu_pick_rule)")) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (params->stop_sq_tol < 0.0 && !ikgpu::visitor_extended(*params))
        return fail(IKGPU_ERR_INVALID, "the never-stop visitor has no converged start: a pick needs a stop rule (stop_sq_tol >= 0)");
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null; the problem is not looked at)
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_launch_size(B, K)) return rc;
    if (w)
        for (int i = 0; i < p->host.nq; ++i)
            if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(IKGPU_ERR_INVALID, "w[" + std::to_string(i) + "] must be finite and not negative");
    const int log2K = multistart_fused_log2(p, params, K);
    // (the loop's workspace is refused here, before the device is selected; run_starts checks its own part again)
    if (log2K < 0 && (!workspace || workspace_bytes < pick_workspace(p, B).total))
        return fail(IKGPU_ERR_INVALID, "pick workspace too small: " + std::to_string(workspace ? workspace_bytes : 0) + " bytes given, " +
                                           std::to_string(pick_workspace(p, B).total) + " needed (ikgpu_dls_pick_workspace_bytes)");
    return on_device(p->device, stream, [&](hipStream_t st) {
        if (log2K >= 0) {
            const ikgpu::BatchIO io{B, q0, targets, q_out, success, iters, layout};
            ikgpu::ChainJob job{};
            job.kind = ikgpu::ChainJob::Pick;
            job.pick.ms = ikdev::MultistartArgs{starts, p->dev.draw, seed, winner, err_sq, log2K};
            job.pick.q_ref = q_ref;
            job.pick.cost = cost;
            job.pick.rule = rule;
            for (int j = 0; j < ikdev::kPickMaxChain; ++j)   // (the support of a chain problem is its chain: w by chain joint)
                job.pick.w[j] = (w && j < p->host.chain.nj) ? w[p->host.chain.qidx[j]] : 1.0;
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the pick DLS kernel");
        }
        // every other case: the definition itself, each start's cost computed and the start merged into the caller's outputs
        const PickWorkspace pw = pick_workspace(p, B);
        char *ws = static_cast<char *>(workspace);
        double *c_k = reinterpret_cast<double *>(ws + pw.cost), *J = reinterpret_cast<double *>(ws + pw.J), *G = reinterpret_cast<double *>(ws + pw.G);
        double *w_dev = nullptr;
        const bool weighted = w && (rule == IKGPU_PICK_DISTANCE || rule == IKGPU_PICK_MAX_DISTANCE);
        if (weighted) {   // (w is pageable host memory: the copy has left it when the call returns)
            w_dev = reinterpret_cast<double *>(ws + pw.w);
            if (const int rc = launched(hipMemcpyAsync(w_dev, w, sizeof(double) * static_cast<size_t>(p->host.nq), hipMemcpyHostToDevice, st), "copying the pick weights"))
                return rc;
        }
        const bool manip = rule == IKGPU_PICK_MANIPULABILITY;
        const StartsCall c{B, K, q0, starts, seed, targets, params, layout, workspace, start_workspace(p, B, true).total};
        return run_starts(p, c, "pick", "ikgpu_dls_pick_workspace_bytes", /*with_error=*/true, st,
                          [&](int k, double *q, uint8_t *ok, int32_t *it, double *e, unsigned long long *key) {
                              if (const int rc = dispatch_eval(p, B, q, targets, e, manip ? J : nullptr, layout, st)) return rc;
                              const ikgpu::PickCost pc{B, p->host.nq, p->host.nv, p->host.rows, layout, rule, params->damping * params->damping,
                                                       p->dev.q_in_chain, p->dev.lower, p->dev.upper, q, q_ref ? q_ref : q0, w_dev, J, G, c_k};
                              if (const int rc = launched(ikgpu::launch_pick_cost(pc, st), "launching the pick cost")) return rc;
                              const ikgpu::PickMerge m{ikgpu::MultistartMerge{B, p->host.nq, p->host.rows, layout, k, q, e, ok, it, key, q_out, success, iters, winner, err_sq},
                                                       c_k, cost};
                              return launched(ikgpu::launch_pick_merge(m, st), "launching the pick merge");
                          });
    });
}

}  // extern "C"

namespace {

// The workspace of the path multi-start definition run as a loop: the multi-start loop's (start_workspace with the error), then start k's
// count [B], ONE scratch trajectory reused by every start ([N][nq x B]; the caller's own q_traj stands in when a trajectory is asked
// for: the winner's run goes over it last) with its flags [N][B] and iteration counts [N][B], and the path call's own workspace.
struct PathMultistartWorkspace {
    size_t reached, traj, success, iters, path, path_bytes, total;
};
PathMultistartWorkspace path_multistart_workspace(const ikgpu_problem *p, int64_t B, int64_t segments, int64_t T, const ikgpu_dls_params *params,
                                                  bool with_trajectory) {
    size_t end = start_workspace(p, B, /*with_error=*/true).total;
    auto take = [&](size_t n) { const size_t at = end; end += (n + 255) / 256 * 256; return at; };
    const size_t b = static_cast<size_t>(B), n = static_cast<size_t>(segments * T);
    PathMultistartWorkspace w{};
    w.reached = take(4 * b);
    if (n > 0) {
        if (!with_trajectory) w.traj = take(8 * static_cast<size_t>(p->host.nq) * b * n);
        w.success = take(b * n);
        w.iters = take(4 * b * n);
        w.path_bytes = track_is_fused(p, params) ? 0 : line_workspace(p, B, segments * T).total;
        w.path = take(w.path_bytes);
    }
    w.total = end;
    return w;
}

// K starts, P >= 1 vias (via 0 and P - 1 segments behind it), T >= 0 waypoints per segment, (P - 1) T in a 32-bit count.
bool path_multistart_sizes_ok(int32_t K, int64_t P, int64_t T) { return K >= 1 && K <= 64 && P >= 1 && T >= 0 && !(T > 0 && P - 1 > 0x7fffffff / T); }

}  // namespace

extern "C" {

const char *ikgpu_dls_path_multistart_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, multistart_fused_log2(p, params, K) >= 0, "_path_multistart");
    return name.c_str();
}

size_t ikgpu_dls_path_multistart_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, int64_t P, int64_t T, const ikgpu_dls_params *params,
                                                 int with_trajectory) {
    if (!p || !params || B <= 0 || !path_multistart_sizes_ok(K, P, T) || multistart_fused_log2(p, params, K) >= 0) return 0;
    return path_multistart_workspace(p, B, P - 1, T, params, with_trajectory != 0).total;
}

int ikgpu_dls_path_multistart_batch(const ikgpu_problem *p, int64_t B, int32_t K, int64_t P, int64_t T, const double *q0, const double *starts,
                                    uint64_t seed, const double *vias, const ikgpu_dls_params *params, double max_joint_step, double *q_entry,
                                    uint8_t *entry_success, int32_t *entry_iters, int32_t *winner, double *err_sq, int32_t *reached,
                                    int32_t *reached_all, double *q_traj, uint8_t *success, int32_t *iters, int layout, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_starts(K)) return rc;
    if (int rc = refuse_if(P < 1, "the number of via poses must be at least 1 (via 0 is the path's first pose)")) return rc;
    if (int rc = refuse_if(T < 0, "negative number of waypoints")) return rc;
    if (int rc = refuse_if(!path_multistart_sizes_ok(K, P, T), "too many waypoints for one call ((P - 1) x T must fit 31 bits)")) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (!(max_joint_step >= 0.0) || !std::isfinite(max_joint_step))
        return fail(IKGPU_ERR_INVALID, "max_joint_step must be finite and not negative (0: no joint-step rule)");
    if (params->stop_sq_tol < 0.0 && !ikgpu::visitor_extended(*params))
        return fail(IKGPU_ERR_INVALID, "the never-stop visitor lets no start enter the path: a path multi-start needs a stop rule (stop_sq_tol >= 0)");
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null; the problem is not looked at)
    if (!q0 || !vias || !q_entry) return null_argument();
    if (int rc = check_launch_size(B, K)) return rc;
    if (P >= 2)
        if (int rc = check_line_slots(p)) return rc;
    const int64_t segments = P - 1, N = segments * T;
    if (!q_traj) success = nullptr, iters = nullptr;   // (not read without a trajectory)
    const int log2K = multistart_fused_log2(p, params, K);
    const PathMultistartWorkspace pw = log2K < 0 ? path_multistart_workspace(p, B, segments, T, params, q_traj != nullptr) : PathMultistartWorkspace{};
    // (the loop's workspace is refused here, before the device is selected; run_starts checks its own part again)
    if (log2K < 0 && (!workspace || workspace_bytes < pw.total))
        return fail(IKGPU_ERR_INVALID, "path multi-start workspace too small: " + std::to_string(workspace ? workspace_bytes : 0) + " bytes given, " +
                                           std::to_string(pw.total) + " needed (ikgpu_dls_path_multistart_workspace_bytes)");
    const double *behind = vias + static_cast<int64_t>(p->host.ntasks) * 12 * B;   // slab 1: via 0 of the path call (read when N > 0 only)
    return on_device(p->device, stream, [&](hipStream_t st) {
        if (log2K >= 0) {
            // the scout: K lanes per problem, no trajectory store; then the winner's trajectory, an ordinary path launch from q_entry
            const ikgpu::BatchIO io{B, q0, vias, q_entry, entry_success, entry_iters, layout};
            ikgpu::ChainJob job{};
            job.kind = ikgpu::ChainJob::PathMultistart;
            job.pms.ms = ikdev::MultistartArgs{starts, p->dev.draw, seed, winner, err_sq, log2K};
            job.pms.reached = reached;
            job.pms.reached_all = reached_all;
            job.pms.T = N > 0 ? static_cast<int>(T) : 0;
            job.pms.P = N > 0 ? static_cast<int>(segments) : 0;
            job.pms.max_joint_step = max_joint_step;
            if (const int rc = launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the path multi-start DLS kernel")) return rc;
            if (!q_traj || N == 0) return static_cast<int>(IKGPU_OK);
            return dispatch_path(p, B, segments, T, q_entry, behind, params, max_joint_step, q_traj, success, iters, nullptr, layout, nullptr, 0, st);
        }
        // every other case: the definition itself -- each start's entry solve, its error, the path call from its result into the scratch
        // trajectory, and the merge into the caller's outputs; then the path call from q_entry for the trajectory
        char *ws = static_cast<char *>(workspace);
        int32_t *r_k = reinterpret_cast<int32_t *>(ws + pw.reached), *it_s = reinterpret_cast<int32_t *>(ws + pw.iters);
        double *traj = q_traj ? q_traj : reinterpret_cast<double *>(ws + pw.traj);
        uint8_t *ok_s = reinterpret_cast<uint8_t *>(ws + pw.success);
        const StartsCall c{B, K, q0, starts, seed, vias, params, layout, workspace, start_workspace(p, B, true).total};
        const int rc = run_starts(p, c, "path multi-start", "ikgpu_dls_path_multistart_workspace_bytes", /*with_error=*/true, st,
                                  [&](int k, double *q, uint8_t *ok, int32_t *it, double *e, unsigned long long *key) {
                                      if (const int rc = dispatch_eval(p, B, q, vias, e, nullptr, layout, st)) return rc;
                                      if (N > 0)
                                          if (const int rc = dispatch_path(p, B, segments, T, q, behind, params, max_joint_step, traj, ok_s, it_s, r_k, layout,
                                                                           ws + pw.path, pw.path_bytes, st))
                                              return rc;
                                      const ikgpu::PathMultistartMerge m{
                                          ikgpu::MultistartMerge{B, p->host.nq, p->host.rows, layout, k, q, e, ok, it, key, q_entry, entry_success, entry_iters, winner, err_sq},
                                          N, N > 0 ? r_k : nullptr, reached, reached_all};
                                      return launched(ikgpu::launch_path_multistart_merge(m, st), "launching the path multi-start merge");
                                  });
        if (rc != IKGPU_OK || !q_traj || N == 0) return rc;
        return dispatch_path(p, B, segments, T, q_entry, behind, params, max_joint_step, q_traj, success, iters, nullptr, layout, ws + pw.path, pw.path_bytes, st);
    });
}

const char *ikgpu_dls_solutions_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t K) {
    if (!p || !params) return "";
    thread_local std::string name;
    name = variant_kernel_name(p, multistart_fused_log2(p, params, K) >= 0, "_solutions");
    return name.c_str();
}

size_t ikgpu_dls_solutions_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t K, int32_t N, const ikgpu_dls_params *params) {
    if (!p || !params || B <= 0 || K < 1 || K > 64 || N < 1 || N > K || multistart_fused_log2(p, params, K) >= 0) return 0;
    return start_workspace(p, B, /*with_error=*/false).total;
}

int ikgpu_dls_solutions_batch(const ikgpu_problem *p, int64_t B, int32_t K, int32_t N, const double *q0, const double *starts, uint64_t seed,
                              const double *targets, const ikgpu_dls_params *params, double sep, double *q_sols, int32_t *count,
                              int32_t *which, int32_t *iters, int layout, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_starts(K)) return rc;
    if (N < 1 || N > K) return fail(IKGPU_ERR_INVALID, "the number of solutions kept must be 1 .. the number of starts");
    if (!(sep >= 0.0) || !std::isfinite(sep)) return fail(IKGPU_ERR_INVALID, "the separation must be finite and not negative");
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (params->stop_sq_tol < 0.0 && !ikgpu::visitor_extended(*params))
        return fail(IKGPU_ERR_INVALID, "the never-stop visitor has no converged start: a solution set needs a stop rule (stop_sq_tol >= 0)");
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null; the problem is not looked at)
    if (!q0 || !targets || !q_sols || !count) return null_argument();
    if (int rc = check_launch_size(B, K)) return rc;
    return on_device(p->device, stream, [&](hipStream_t st) {
        const int log2K = multistart_fused_log2(p, params, K);
        if (log2K >= 0) {
            const ikgpu::BatchIO io{B, q0, targets, q_sols, nullptr, iters, layout};
            ikgpu::ChainJob job{};
            job.kind = ikgpu::ChainJob::Solutions;
            job.sol = ikdev::SolutionsArgs{ikdev::MultistartArgs{starts, p->dev.draw, seed, nullptr, nullptr, log2K}, count, which, sep, N};
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the solution-set DLS kernel");
        }
        // every other case: the definition itself, each start inserted into the caller's outputs
        const StartsCall c{B, K, q0, starts, seed, targets, params, layout, workspace, workspace_bytes};
        return run_starts(p, c, "solution-set", "ikgpu_dls_solutions_workspace_bytes", /*with_error=*/false, st,
                          [&](int k, double *q, uint8_t *ok, int32_t *it, double *, unsigned long long *) {
                              const ikgpu::SolutionsInsert m{B, p->host.nq, layout, k, N, sep, p->dev.q_in_chain, q, ok, it, q_sols, count, which, iters};
                              return launched(ikgpu::launch_solutions_insert(m, st), "launching the solution-set insert");
                          });
    });
}

const char *ikgpu_dls_goalset_kernel(const ikgpu_problem *p, const ikgpu_dls_params *params, int32_t G, int32_t K) {
    if (!p || !params) return "";
    thread_local std::string name;
    int log2G, log2K;
    name = variant_kernel_name(p, goalset_fused_log2(p, params, G, K, &log2G, &log2K), "_goalset");
    return name.c_str();
}

size_t ikgpu_dls_goalset_workspace_bytes(const ikgpu_problem *p, int64_t B, int32_t G, int32_t K, const ikgpu_dls_params *params) {
    int log2G, log2K;
    if (!p || !params || B <= 0 || check_goalset_size(G, K, /*report=*/false) || goalset_fused_log2(p, params, G, K, &log2G, &log2K)) return 0;
    return start_workspace(p, B, /*with_error=*/true).total;
}

int ikgpu_dls_goalset_batch(const ikgpu_problem *p, int64_t B, int32_t G, int32_t K, const double *q0, const double *starts, uint64_t seed,
                            const double *goals, const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                            int32_t *goal, int32_t *start, double *err_sq, uint8_t *reachable, int layout, void *workspace,
                            size_t workspace_bytes, void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_goalset_size(G, K, /*report=*/true)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_params(params)) return rc;
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null; the problem is not looked at)
    if (!q0 || !goals || !q_out) return null_argument();
    if (int rc = check_launch_size(B, G * K)) return rc;
    int log2G = 0, log2K = 0;
    const bool fused = goalset_fused_log2(p, params, G, K, &log2G, &log2K);
    // (the loop's workspace is refused here, before the device is selected; run_starts checks it again goal by goal)
    if (!fused && (!workspace || workspace_bytes < start_workspace(p, B, /*with_error=*/true).total))
        return fail(IKGPU_ERR_INVALID, "goal-set workspace too small: " + std::to_string(workspace ? workspace_bytes : 0) + " bytes given, " +
                                           std::to_string(start_workspace(p, B, true).total) + " needed (ikgpu_dls_goalset_workspace_bytes)");
    return on_device(p->device, stream, [&](hipStream_t st) {
        if (fused) {
            const ikgpu::BatchIO io{B, q0, goals, q_out, success, iters, layout};
            ikgpu::ChainJob job{};
            job.kind = ikgpu::ChainJob::Goalset;
            job.goal = ikdev::GoalsetArgs{ikdev::MultistartArgs{starts, p->dev.draw, seed, nullptr, err_sq, log2K}, goal, start, reachable, log2G};
            return launched(ikgpu::launch_dls_chain(p->host, p->dev, io, job, *params, st), "launching the goal-set DLS kernel");
        }
        // every other case: the definition itself, goal after goal and start after start, candidate j = g K + k merged into the caller's
        // outputs under the multi-start merge's rule with j in place of k (winner = j lands in `goal` when asked for and is split below)
        const int64_t t_slab = static_cast<int64_t>(p->host.ntasks) * 12 * B;
        int32_t *winner = goal ? goal : start;
        for (int g = 0; g < G; ++g) {
            const double *targets = goals + g * t_slab;
            const StartsCall c{B, K, q0, starts, seed, targets, params, layout, workspace, workspace_bytes};
            const int rc = run_starts(p, c, "goal-set", "ikgpu_dls_goalset_workspace_bytes", /*with_error=*/true, st,
                                      [&](int k, double *q, uint8_t *ok, int32_t *it, double *e, unsigned long long *key) {
                                          if (const int rc = dispatch_eval(p, B, q, targets, e, nullptr, layout, st)) return rc;
                                          const ikgpu::MultistartMerge m{B, p->host.nq, p->host.rows, layout, g * K + k, q, e, ok, it, key, q_out, success, iters, winner, err_sq};
                                          if (const int rc = launched(ikgpu::launch_multistart_merge(m, st), "launching the goal-set merge")) return rc;
                                          if (!reachable) return static_cast<int>(IKGPU_OK);
                                          return launched(ikgpu::launch_goalset_reachable(B, k == 0, ok, reachable + static_cast<int64_t>(g) * B, st),
                                                          "launching the goal-set reachability step");
                                      });
            if (rc) {
                g_last_error = "goal " + std::to_string(g) + ", " + g_last_error;
                return rc;
            }
        }
        if (!winner) return static_cast<int>(IKGPU_OK);
        return launched(ikgpu::launch_goalset_split(B, K, winner, goal, start, st), "launching the goal-set index split");
    });
}

int ikgpu_dls_solve_batch_host(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                               const ikgpu_dls_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int layout) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_params(params)) return rc;
    if (B == 0) return IKGPU_OK;  // an empty batch is a no-op (its pointers may be null)
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_host_layout(layout)) return rc;
    return host_solve(p, B, q0, targets, q_out, success, iters, layout, [&](int64_t Bk, const double *d_q0, const double *d_t, double *d_q, uint8_t *d_s, int32_t *d_i, hipStream_t st) {
        return ikgpu_dls_solve_batch(p, Bk, d_q0, d_t, params, d_q, d_s, d_i, layout & ~IKGPU_TARGETS_POSE7, st);
    });
}

void ikgpu_pik_params_default(ikgpu_pik_params *p, int32_t num_levels) {
    if (!p) return;
    p->max_iterations = 100;  // reference ik/ik/pik.hpp:12
    p->step_length = 1.0;     // reference ik/ik/pik.hpp:14
    p->stop_sq_tol = 1e-4;    // reference ik/ik/visitor.hpp:19
    p->num_levels = num_levels;
    for (double &l : p->lambda) l = 1.0;  // reference ik/ik/pik.hpp:24
    p->da = nullptr;                      // reference ik/ik/pik.hpp:26
}

const char *ikgpu_pik_kernel(const ikgpu_problem *p, const ikgpu_pik_params *params) {
    if (!p || !params) return "";
    if (pik_is_one_dls_level(p, params)) return p->dls_name.c_str();
    if (pik_is_two_levels_on_the_tree(p, params)) return p->pik_tree_name.c_str();
    return pik_runs_static(p, params) ? p->pik_static_name.c_str() : p->pik_name.c_str();
}

int ikgpu_pik_solve_batch(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                          const ikgpu_pik_params *params, double *q_out, uint8_t *success, int32_t *iters, int layout,
                          void *stream) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (int rc = check_pik_params(p, params)) return rc;
    if (B == 0) return IKGPU_OK;
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_launch_size(B)) return rc;
    if (pik_is_one_dls_level(p, params)) {
        const ikgpu_dls_params d = pik_level0_as_dls(params);
        return ikgpu_dls_solve_batch(p, B, q0, targets, &d, q_out, success, iters, layout, stream);
    }
    const ikgpu::BatchIO io{B, q0, targets, q_out, success, iters, layout};
    if (pik_is_two_levels_on_the_tree(p, params))
        return on_device(p->device, stream, [&](hipStream_t st) {
            return launched(ikgpu::launch_dls_tree(p->host, p->dev, io, pik_level0_as_dls(params), st, &params->lambda[1]),
                            "launching the tree kernel (two-level ik::pik)");
        });
    const bool on_static = pik_runs_static(p, params);
    return on_device(p->device, stream, [&](hipStream_t st) {
        return launched(on_static ? ikgpu::rtc_launch_pik_static(p->gen, p->pik_static_key[pik_has_da(p, params) ? 1 : 0], io, *params, st)
                                  : ikgpu::launch_pik_generic(p->gen, p->dev, io, *params, st),
                        "launching the PIK kernel");
    });
}

int ikgpu_pik_solve_batch_host(const ikgpu_problem *p, int64_t B, const double *q0, const double *targets,
                               const ikgpu_pik_params *params, double *q_out, uint8_t *success, int32_t *iters,
                               int layout) {
    if (int rc = check_problem_batch(p, B)) return rc;
    if (int rc = check_pik_params(p, params)) return rc;
    if (B == 0) return IKGPU_OK;
    if (!q0 || !targets || !q_out) return null_argument();
    if (int rc = check_host_layout(layout)) return rc;
    return host_solve(p, B, q0, targets, q_out, success, iters, layout, [&](int64_t Bk, const double *d_q0, const double *d_t, double *d_q, uint8_t *d_s, int32_t *d_i, hipStream_t st) {
        return ikgpu_pik_solve_batch(p, Bk, d_q0, d_t, params, d_q, d_s, d_i, layout & ~IKGPU_TARGETS_POSE7, st);
    });
}

// (no problem, so no device to select: the launch runs on the caller's current device)
int ikgpu_targets_from_pose7(int64_t B, int32_t ntasks, const double *pose7, double *targets12, int layout, void *stream) {
    if (!pose7 || !targets12) return null_argument();
    if (B < 0 || ntasks < 0) return fail(IKGPU_ERR_INVALID, "negative size");
    if (int rc = check_layout(layout)) return rc;
    if (B == 0 || ntasks == 0) return IKGPU_OK;
    return guarded([&] {
        return launched(ikgpu::launch_targets_from_pose7(B, ntasks, pose7, targets12, layout, static_cast<hipStream_t>(stream)),
                        "launching the target expansion kernel");
    });
}

int ikgpu_evaluate_batch(const ikgpu_problem *p, int64_t B, const double *q, const double *targets, double *e_out,
                         double *J_out, int layout, void *stream) {
    if (!p || !q || !targets || !e_out) return null_argument();
    if (int rc = check_batch(B)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (B == 0) return IKGPU_OK;
    return on_device(p->device, stream, [&](hipStream_t st) { return dispatch_eval(p, B, q, targets, e_out, J_out, layout, st); });
}

int ikgpu_task_frames_fk_batch(const ikgpu_problem *p, int64_t B, const double *q, double *oMf_out, int layout,
                               void *stream) {
    if (!p || !q || !oMf_out) return null_argument();
    if (int rc = check_batch(B)) return rc;
    if (int rc = check_layout(layout)) return rc;
    if (B == 0) return IKGPU_OK;
    return on_device(p->device, stream, [&](hipStream_t st) {
        hipError_t e = p->host.kind == ikgpu::KernelKind::Chain  ? ikgpu::launch_fk_chain(p->host, p->dev, B, q, oMf_out, layout, st)
                       : p->host.kind == ikgpu::KernelKind::Tree && !p->host.tree_extras()
                           ? ikgpu::launch_eval_tree(p->host, p->dev, B, q, q, nullptr, nullptr, oMf_out, layout, st)
                           : ikgpu::launch_eval_generic(p->gen, p->dev, B, q, q, nullptr, nullptr, oMf_out, layout, st);
        return launched(e, "launching the FK kernel");
    });
}

}  // extern "C"
