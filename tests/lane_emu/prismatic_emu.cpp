// prismatic_emu.cpp -- TEST HARNESS ONLY.  The per-lane chain programs of the gfx950 kernels (ik_amd/csrc/device/*.hpp) for chains WITH
// PRISMATIC JOINTS, compiled for the host and run one "lane" after another, for all seven jobs: the single solve and the stage kernels
// (as lane_emu.cpp), track, line, path, multi-start, goal set and solutions (as the *_emu.cpp next to this file, whose models of the
// cross-lane exchanges are restated here).  Three programs, chosen by the caller:
//   0  the runtime-parameter build that reads the joint-kind mask (SMASK = kSpecRuntimeKinds; what the stage kernels run) -- the
//      single solve and the stages only
//   1  the device's general build of a chain with a prismatic joint (SMASK = 1 << kSpecKinds, sin / cos by dsincos_fast)
//   2  the structure-specialised hot program, ChainStruct<code, mask of prismatic joints>, for the chains listed in HOT_SHAPES
// The older emulators match a hot program by the placement code alone and know no joint kinds; they stay what they were.
// Compiled by tests/ with g++ into its own shared object; libikgpu.so neither contains nor calls it (the product has no CPU path).
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "device/chain_kernel_body.hpp"
#include "device/chain_hot.hpp"
#include "ikgpu.h"
#include "model.hpp"
#include "problem.hpp"

namespace {

thread_local std::string g_err;

auto any_active = [](bool act) { return act; };

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, const ikdev::ChainDesc<NJ> &d, const ikgpu::ProblemHost &ph, const ikgpu_dls_params *prm, int layout,
          int64_t B, const double *q0, const double *targets, double *q_out, uint8_t *success, int32_t *iters) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.desc = &d;
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = layout; a.B = B; a.q0 = q0; a.targets = targets;
    a.q_out = q_out; a.success = success; a.iters = iters;
    if (!prm) return;
    a.prm.max_iterations = prm->max_iterations;
    a.prm.lam2 = prm->damping * prm->damping;
    a.prm.step_length = prm->step_length;
    a.prm.stop_sq_tol = prm->stop_sq_tol;
}

template <int NJ>
ikdev::ChainDesc<NJ> desc_of(const ikgpu::ProblemHost &ph) {
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    return d;
}

// ---- the programs: what differs between the general builds and the hot program, behind one set of names ---------------------------
template <int NJ_, int KT, int SM>
struct General {
    static constexpr int NJ = NJ_;
    ikdev::ChainDesc<NJ> d;
    explicit General(const ikgpu::ProblemHost &ph) : d(desc_of<NJ>(ph)) {}
    typedef ikdev::ChainKernelArgs<NJ> Args;
    void solve(const Args &a, int64_t b) const { ikdev::dls_chain_body<NJ, KT, SM>(a, d, b, any_active); }
    void track(const Args &a, int T, int64_t b) const { ikdev::dls_chain_track_body<NJ, KT, SM>(a, d, T, b, any_active); }
    int line(const Args &a, const ikdev::LineArgs &la, int64_t b) const { return ikdev::dls_chain_line_body<NJ, KT, SM>(a, d, la, b, any_active); }
    int path(const Args &a, const ikdev::PathArgs &pa, int64_t b) const { return ikdev::dls_chain_path_body<NJ, KT, SM>(a, d, pa, b, any_active); }
    void ms_lane(const Args &a, const ikdev::MultistartArgs &ms, int64_t b, int k, double (&q)[NJ], bool &ok, int &it, double &err) const {
        ikdev::dls_chain_multistart_lane<NJ, KT, SM>(a, ms, d, b, k, q, ok, it, err, any_active);
    }
    void gs_lane(const Args &a, const ikdev::GoalsetArgs &ga, int64_t b, int g, int k, double (&q)[NJ], bool &ok, int &it, double &err) const {
        ikdev::dls_chain_goalset_lane<NJ, KT, SM>(a, ga, d, b, g, k, q, ok, it, err, any_active);
    }
    template <class X, class Y>
    void gs_body(const Args &a, const ikdev::GoalsetArgs &ga, int64_t gid, X exchange, Y any) const {
        ikdev::dls_chain_goalset_body<NJ, KT, SM>(a, ga, d, gid, any_active, exchange, any);
    }
    void sol_lane(const Args &a, const ikdev::SolutionsArgs &sa, int64_t b, int k, double (&q)[NJ], bool &ok, int &it) const {
        ikdev::dls_chain_solutions_lane<NJ, KT, SM>(a, sa, d, b, k, q, ok, it, any_active);
    }
    void pass(const Args &a, const double *src, double *q_out, int64_t b, bool stepped) const { ikdev::chain_pass_through_into(a, src, q_out, b, stepped); }
};

template <int NJ_, class S>
struct Hot {
    static constexpr int NJ = NJ_;
    ikdev::ChainDesc<NJ> d;   // (the line and path bodies read the start pose from the chain table)
    ikdev::HotTable t{};
    explicit Hot(const ikgpu::ProblemHost &ph) : d(desc_of<NJ>(ph)) {
        const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
        if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
        std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    }
    typedef ikdev::ChainKernelArgs<NJ> Args;
    static bool never(const Args &a) { return a.prm.stop_sq_tol < 0.0; }
    void solve(const Args &a, int64_t b) const {
        if (never(a)) ikdev::hot_chain_body<NJ, S, true>(a, t, b, any_active);
        else ikdev::hot_chain_body<NJ, S, false>(a, t, b, any_active);
    }
    void track(const Args &a, int T, int64_t b) const {
        if (never(a)) ikdev::hot_track_body<NJ, S, true>(a, t, T, b, any_active);
        else ikdev::hot_track_body<NJ, S, false>(a, t, T, b, any_active);
    }
    int line(const Args &a, const ikdev::LineArgs &la, int64_t b) const { return ikdev::hot_line_body<NJ, S>(a, t, la, b, any_active); }
    int path(const Args &a, const ikdev::PathArgs &pa, int64_t b) const { return ikdev::hot_path_body<NJ, S>(a, t, pa, b, any_active); }
    void ms_lane(const Args &a, const ikdev::MultistartArgs &ms, int64_t b, int k, double (&q)[NJ], bool &ok, int &it, double &err) const {
        if (never(a)) ikdev::hot_multistart_lane<NJ, S, true>(a, ms, t, b, k, q, ok, it, err, any_active);
        else ikdev::hot_multistart_lane<NJ, S, false>(a, ms, t, b, k, q, ok, it, err, any_active);
    }
    void gs_lane(const Args &a, const ikdev::GoalsetArgs &ga, int64_t b, int g, int k, double (&q)[NJ], bool &ok, int &it, double &err) const {
        if (never(a)) ikdev::hot_goalset_lane<NJ, S, true>(a, ga, t, b, g, k, q, ok, it, err, any_active);
        else ikdev::hot_goalset_lane<NJ, S, false>(a, ga, t, b, g, k, q, ok, it, err, any_active);
    }
    template <class X, class Y>
    void gs_body(const Args &a, const ikdev::GoalsetArgs &ga, int64_t gid, X exchange, Y any) const {
        if (never(a)) ikdev::hot_goalset_body<NJ, S, true>(a, ga, t, gid, any_active, exchange, any);
        else ikdev::hot_goalset_body<NJ, S, false>(a, ga, t, gid, any_active, exchange, any);
    }
    void sol_lane(const Args &a, const ikdev::SolutionsArgs &sa, int64_t b, int k, double (&q)[NJ], bool &ok, int &it) const {
        ikdev::hot_solutions_lane<NJ, S>(a, sa, t, b, k, q, ok, it, any_active);
    }
    void pass(const Args &a, const double *src, double *q_out, int64_t b, bool stepped) const { ikdev::hot_pass_through_from(a, src, q_out, b, stepped); }
};

// The chains of tests/prismatic_common.py with a hot program: X(NJ, code0, code1, code2, mask of prismatic joints).  The codes are
// ikgpu::chain_structure's (prismatic_emu_structure prints them); a chain that is not listed has no hot program here.
#define HOT_SHAPES(X)                                                                                                    \
    X(7, 0x70000380001c0000ull, 0x70000380001c0000ull, 0x00000000003c0000ull, 0x24u) /* arm8 {j3, j6} / l7 */          \
    X(7, 0x70000380001c0000ull, 0x70000380001c0000ull, 0x00000000003c0000ull, 0x01u) /* arm8 {j1} / l7 */              \
    X(7, 0x70000380001c0000ull, 0x70000380001c0000ull, 0x00000000003c0000ull, 0x40u) /* arm8 {j7} / l7 */              \
    X(7, 0x24e570accea17665ull, 0x4675594a939a5656ull, 0x000002424ad1d956ull, 0x01u) /* ur5 on a rail / tool0 */       \
    X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull, 0x04u) /* ur5, prismatic elbow / tool0: UR5's own code */

// f(program) with the program the caller asked for; false when the chain has no such program here.
template <class F>
bool with_program(const ikgpu::ProblemHost &ph, int program, F f) {
    const int nj = ph.chain.nj, kt = ph.tasks[0].type;
    if (program == 2) {
        if (kt != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0]) || !ph.chain_struct.fits) return false;
        const ikgpu::ChainStructure &s = ph.chain_struct;
#define X(N, K0, K1, K2, PM)                                                                                             \
    if (nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2 && s.prismatic == static_cast<int>(PM)) {        \
        f(Hot<N, ikdev::ChainStruct<K0, K1, K2, PM>>(ph));                                                                \
        return true;                                                                                                      \
    }
        HOT_SHAPES(X)
#undef X
        return false;
    }
    // (program 0, the runtime-parameter build, runs the single solve and the stage kernels only: prismatic_emu_run)
    if (program != 1) return false;
    constexpr int kDev = 1 << ikdev::kSpecKinds;
#define X(N)                                                                            \
    if (nj == N) {                                                                      \
        if (kt == 2) f(General<N, 2, kDev>(ph));                                        \
        else if (kt == 0) f(General<N, 0, kDev>(ph));                                   \
        else f(General<N, 1, kDev>(ph));                                                \
        return true;                                                                    \
    }
    X(1) X(3) X(5) X(6) X(7) X(8)   // the chain lengths of tests/prismatic_common.py
#undef X
    return false;
}

ikgpu::ProblemHost analyse(const char *urdf, size_t len, const ikgpu_task *task, ikgpu::Model *model_out = nullptr) {
    ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
    ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
    if (ph.kind != ikgpu::KernelKind::Chain) throw std::runtime_error("not a chain problem: " + ph.kernel_name);
    if (model_out) *model_out = m;
    return ph;
}

// run(ph, draw mask) under the usual try / catch; 2: the chain has no such program here
template <class F>
int guarded(const char *urdf, size_t len, const ikgpu_task *task, int program, F run) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = analyse(urdf, len, task, &m);
        const std::vector<uint8_t> draw = ikgpu::multistart_draw_mask(m, ph);
        bool known = false;
        known = with_program(ph, program, [&](const auto &prog) { run(ph, prog, draw.data()); });
        if (!known) { g_err = "no program " + std::to_string(program) + " for " + ph.kernel_name; return 2; }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

int log2_of(int K) {
    int l = 0;
    while ((1 << l) < K) ++l;
    if (K < 1 || K > 64 || (1 << l) != K) throw std::runtime_error("group sizes must be powers of two up to 64");
    return l;
}

template <int NJ>
struct SolLane {
    double q[NJ];
    bool ok;
    int it;
    ikdev::SolutionsLane s;
};
template <int NJ>
struct SolFetch {   // what a lane of the group receives in step j (solutions_emu.cpp)
    const std::vector<SolLane<NJ>> *lanes;
    bool flag(int j, bool) const { return (*lanes)[static_cast<size_t>(j)].s.offer; }
    bool any(bool f) const { return f; }
    template <int N_>
    void q(int j, const double (&)[N_], double (&theirs)[N_]) const {
        for (int i = 0; i < N_; ++i) theirs[i] = (*lanes)[static_cast<size_t>(j)].q[i];
    }
};

}  // namespace

extern "C" {

const char *prismatic_emu_last_error(void) { return g_err.c_str(); }

// out[0] = chain length, out[1 .. 3] = the structure code, out[4] = the mask of prismatic joints, out[5] = LoopParams::idmask;
// support / draw [nq] (either may be null): ikgpu_problem_support and the entries a generated start draws.
int prismatic_emu_structure(const char *urdf, size_t len, const ikgpu_task *task, uint64_t *out, uint8_t *support, uint8_t *draw) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = analyse(urdf, len, task, &m);
        out[0] = static_cast<uint64_t>(ph.chain.nj);
        for (int i = 0; i < 3; ++i) out[1 + i] = ph.chain_struct.code[i];
        out[4] = static_cast<uint64_t>(ph.chain_struct.prismatic);
        out[5] = static_cast<uint64_t>(ikgpu::chain_kernel_mask(ph.chain));
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        for (int i = 0; i < m.nq; ++i) {
            if (support) support[i] = ph.q_in_chain[static_cast<size_t>(i)] ? 1 : 0;
            if (draw) draw[i] = mask[static_cast<size_t>(i)];
        }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// What ikgpu_multistart_starts defines, on host pointers: starts_out [K-1][nq x B] in `layout` (multistart_emu.cpp).
int prismatic_emu_starts(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int K, const double *q0, unsigned long long seed,
                         double *starts_out, int layout) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = analyse(urdf, len, task, &m);
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        for (int k = 1; k < K; ++k)
            for (int64_t b = 0; b < B; ++b)
                for (int i = 0; i < m.nq; ++i) {
                    const int64_t at = ikdev::at(layout, B, m.nq, i, b);
                    starts_out[static_cast<int64_t>(k - 1) * m.nq * B + at] =
                        mask[static_cast<size_t>(i)] ? ikdev::multistart_draw(seed, b, k, i, m.lower[static_cast<size_t>(i)], m.upper[static_cast<size_t>(i)]) : q0[at];
                }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// mode 0: ik::dls, 1: evaluate (e, dense J), 2: task-frame FK -- the stage kernels run the runtime-parameter build whatever `program`.
int prismatic_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int program, int mode, int64_t B, const double *q0, const double *targets,
                      const ikgpu_dls_params *prm, double *q_out, uint8_t *success, int32_t *iters, double *e_out, double *J_out, double *oMf_out,
                      int layout) {
    if (mode == 0 && program != 0)
        return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *) {
            typename std::decay_t<decltype(prog)>::Args a{};
            fill(a, prog.d, ph, prm, layout, B, q0, targets, q_out, success, iters);
            for (int64_t b = 0; b < B; ++b) prog.solve(a, b);
        });
    try {
        const ikgpu::ProblemHost ph = analyse(urdf, len, task);
        const int nj = ph.chain.nj, kt = task->type;
#define X(N)                                                                                                     \
    if (nj == N) {                                                                                               \
        const ikdev::ChainDesc<N> d = desc_of<N>(ph);                                                            \
        ikdev::ChainKernelArgs<N> a{};                                                                           \
        fill(a, d, ph, nullptr, layout, B, q0, targets, nullptr, nullptr, nullptr);                              \
        a.e_out = e_out; a.J_out = J_out; a.oMf_out = oMf_out;                                                   \
        if (mode == 0) fill(a, d, ph, prm, layout, B, q0, targets, q_out, success, iters);                       \
        for (int64_t b = 0; b < B; ++b) {                                                                        \
            if (mode == 0 && kt == 2) ikdev::dls_chain_body<N, 2, ikdev::kSpecRuntimeKinds>(a, d, b, any_active); \
            else if (mode == 0 && kt == 0) ikdev::dls_chain_body<N, 0, ikdev::kSpecRuntimeKinds>(a, d, b, any_active); \
            else if (mode == 0) ikdev::dls_chain_body<N, 1, ikdev::kSpecRuntimeKinds>(a, d, b, any_active);      \
            else if (mode == 2) ikdev::fk_chain_body<N, true>(a, d, b);                                          \
            else if (kt == 2) ikdev::eval_chain_body<N, 2, ikdev::kSpecRuntimeKinds>(a, d, b);                   \
            else if (kt == 0) ikdev::eval_chain_body<N, 0, ikdev::kSpecRuntimeKinds>(a, d, b);                   \
            else ikdev::eval_chain_body<N, 1, ikdev::kSpecRuntimeKinds>(a, d, b);                                \
        }                                                                                                        \
        return 0;                                                                                                \
    }
        X(1) X(3) X(5) X(6) X(7) X(8)
#undef X
        g_err = "shape not instantiated: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// targets [T][12 x B], q_traj [T][nq x B], success / iters [T][B] (track_emu.cpp)
int prismatic_emu_track(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int T, const double *q0, const double *targets,
                        const ikgpu_dls_params *prm, double *q_traj, uint8_t *success, int32_t *iters, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *) {
        typename std::decay_t<decltype(prog)>::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, targets, q_traj, success, iters);
        for (int64_t b = 0; b < B; ++b) prog.track(a, T, b);
    });
}

// goals [12 x B]; q_traj null: the waypoints alone into waypoints [T][12 x B] (kernels.hip path_targets_chain_kernel with P = 1); else
// ikgpu_dls_line_batch's outputs and visited [B], the waypoints the lane's loop went through (line_emu.cpp)
int prismatic_emu_line(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int T, const double *q0, const double *goals,
                       const ikgpu_dls_params *prm, double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached, int32_t *visited,
                       double *waypoints, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *) {
        typedef std::decay_t<decltype(prog)> P;
        typename P::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, goals, q_traj, success, iters);
        for (int64_t b = 0; b < B; ++b) {
            if (q_traj) {
                const int n = prog.line(a, ikdev::LineArgs{reached, T}, b);
                if (visited) visited[b] = n;
                continue;
            }
            double q[P::NJ], goal[12];
            ikdev::line_load(a, b, q, goal);
            ikdev::LineStart ls;
            ikdev::line_chain_start<true>(a, prog.d, q, goal, ls);
            for (int k = 0; k < T; ++k) {
                double t[12];
                ikdev::line_waypoint(ls, goal, k, T, t);
                for (int c = 0; c < 12; ++c) waypoints[static_cast<int64_t>(k) * 12 * B + ikdev::at(layout, B, 12, c, b)] = t[c];
            }
        }
    });
}

// vias [P][12 x B]; q_traj null: the waypoints alone into waypoints [P T][12 x B]; else ikgpu_dls_path_batch's outputs (path_emu.cpp)
int prismatic_emu_path(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int P_, int T, const double *q0, const double *vias,
                       const ikgpu_dls_params *prm, double max_joint_step, double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached,
                       int32_t *visited, double *waypoints, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *) {
        typedef std::decay_t<decltype(prog)> P;
        typename P::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, vias, q_traj, success, iters);
        for (int64_t b = 0; b < B; ++b) {
            if (q_traj) {
                const int n = prog.path(a, ikdev::PathArgs{reached, T, P_, max_joint_step}, b);
                if (visited) visited[b] = n;
                continue;
            }
            double q[P::NJ], via[12];
            ikdev::line_load(a, b, q, via);
            ikdev::LineStart ls;
            ikdev::line_chain_start<true>(a, prog.d, q, via, ls);
            for (int s = 0; s < P_; ++s) {
                if (s > 0) {
                    double next[12];
                    ikdev::load_target_raw(a, a.targets + static_cast<int64_t>(s) * 12 * B, b, next);
                    ikdev::line_start_from_pose(via, next, ls);
                    for (int c = 0; c < 12; ++c) via[c] = next[c];
                }
                for (int k = 0; k < T; ++k) {
                    double t[12];
                    ikdev::line_waypoint(ls, via, k, T, t);
                    for (int c = 0; c < 12; ++c) waypoints[(static_cast<int64_t>(s) * T + k) * 12 * B + ikdev::at(layout, B, 12, c, b)] = t[c];
                }
            }
        }
    });
}

// ikgpu_dls_multistart_batch on host pointers.  The butterfly of the selection is modelled from its own invariant, as in
// multistart_emu.cpp: before step s a lane holds the minimum over the aligned block of 1 << s lanes it belongs to.
int prismatic_emu_multistart(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int K, const double *q0, const double *starts,
                             unsigned long long seed, const double *targets, const ikgpu_dls_params *prm, double *q_out, uint8_t *success,
                             int32_t *iters, int32_t *winner, double *err_sq, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *draw) {
        typedef std::decay_t<decltype(prog)> P;
        constexpr int NJ = P::NJ;
        const int log2K = log2_of(K);
        typename P::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, targets, q_out, success, iters);
        const ikdev::MultistartArgs ms{starts, draw, seed, winner, err_sq, log2K};
        struct Lane { double q[NJ], err; bool ok; int it; unsigned long long key; };
        std::vector<Lane> lanes(static_cast<size_t>(K));
        for (int64_t b = 0; b < B; ++b) {
            for (int k = 0; k < K; ++k) {
                prog.ms_lane(a, ms, b, k, lanes[k].q, lanes[k].ok, lanes[k].it, lanes[k].err);
                lanes[k].key = ikdev::multistart_key(lanes[k].ok, lanes[k].err);
            }
            int stored = 0;
            for (int k = 0; k < K; ++k) {
                const int win = ikdev::multistart_select(log2K, lanes[k].key, k, [&](int m, unsigned long long &key, int &kk) {
                    const int partner = k ^ m, lo = partner & ~(m - 1);
                    int best = lo;
                    for (int x = lo + 1; x < lo + m; ++x)
                        if (lanes[x].key < lanes[best].key) best = x;
                    key = lanes[best].key;
                    kk = best;
                });
                if (win != k) continue;
                ikdev::multistart_store(a, ms, b, k, lanes[k].q, lanes[k].ok, lanes[k].it, lanes[k].err,
                                        [&](const double *src, bool stepped) { prog.pass(a, src, a.q_out, b, stepped); });
                ++stored;
            }
            if (stored != 1) throw std::runtime_error("the selection left " + std::to_string(stored) + " winners in a group");
        }
    });
}

// ikgpu_dls_goalset_batch on host pointers (goalset_emu.cpp: two passes, and one extra group past the batch for the tail lanes)
int prismatic_emu_goalset(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int G, int K, const double *q0,
                          const double *starts, unsigned long long seed, const double *goals, const ikgpu_dls_params *prm, double *q_out,
                          uint8_t *success, int32_t *iters, int32_t *goal, int32_t *start, double *err_sq, uint8_t *reachable, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *draw) {
        typedef std::decay_t<decltype(prog)> P;
        constexpr int NJ = P::NJ;
        const int log2G = log2_of(G), log2K = log2_of(K), log2J = log2G + log2K, J = 1 << log2J;
        if (J > 64) throw std::runtime_error("G K must be at most 64");
        typename P::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, goals, q_out, success, iters);
        const ikdev::GoalsetArgs ga{ikdev::MultistartArgs{starts, draw, seed, nullptr, err_sq, log2K}, goal, start, reachable, log2G};
        struct Lane { unsigned long long key; bool ok; };
        std::vector<Lane> lanes(static_cast<size_t>(J));
        for (int64_t prob = 0; prob <= B; ++prob) {
            const int64_t b = prob < B ? prob : B - 1;
            for (int j = 0; j < J; ++j) {
                double q[NJ], err;
                int it;
                prog.gs_lane(a, ga, b, j >> log2K, j & (K - 1), q, lanes[j].ok, it, err);
                lanes[j].key = ikdev::multistart_key(lanes[j].ok, err);
            }
            for (int j = 0; j < J; ++j)
                prog.gs_body(a, ga, (prob << log2J) + j,
                             [&lanes, j](int m, unsigned long long &key, int &jj) {
                                 const int partner = j ^ m, lo = partner & ~(m - 1);
                                 int best = lo;
                                 for (int x = lo + 1; x < lo + m; ++x)
                                     if (lanes[x].key < lanes[best].key) best = x;
                                 key = lanes[best].key;
                                 jj = best;
                             },
                             [&lanes, j](int l2K, bool flag) {
                                 const int n = 1 << l2K, lo = j & ~(n - 1);
                                 if (flag != lanes[j].ok) throw std::runtime_error("a lane's second solve disagrees with its first");
                                 bool any = false;
                                 for (int x = lo; x < lo + n; ++x) any = any || lanes[x].ok;
                                 return any;
                             });
        }
    });
}

// ikgpu_dls_solutions_batch on host pointers (solutions_emu.cpp)
int prismatic_emu_solutions(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int K, int N, const double *q0,
                            const double *starts, unsigned long long seed, const double *targets, const ikgpu_dls_params *prm, double sep,
                            double *q_sols, int32_t *count, int32_t *which, int32_t *iters, int layout) {
    return guarded(urdf, len, task, program, [&](const ikgpu::ProblemHost &ph, const auto &prog, const uint8_t *draw) {
        typedef std::decay_t<decltype(prog)> P;
        constexpr int NJ = P::NJ;
        const int log2K = log2_of(K);
        if (N < 1 || N > K) throw std::runtime_error("N must be 1 .. K");
        typename P::Args a{};
        fill(a, prog.d, ph, prm, layout, B, q0, targets, q_sols, nullptr, iters);
        const ikdev::SolutionsArgs sa{ikdev::MultistartArgs{starts, draw, seed, nullptr, nullptr, log2K}, count, which, sep, N};
        std::vector<SolLane<NJ>> lanes(static_cast<size_t>(K));
        for (int64_t b = 0; b < B; ++b) {
            for (int k = 0; k < K; ++k) {
                lanes[k].s = ikdev::SolutionsLane{};
                prog.sol_lane(a, sa, b, k, lanes[k].q, lanes[k].ok, lanes[k].it);
            }
            for (int j = 0; j < K; ++j) {
                for (int k = 0; k < K; ++k) ikdev::solutions_offer(lanes[k].s, lanes[k].ok, N);
                for (int k = 0; k < K; ++k) ikdev::solutions_take<NJ>(lanes[k].s, j, k, sep, lanes[k].q, SolFetch<NJ>{&lanes});
            }
            int kept = 0;
            for (int k = 0; k < K; ++k) {
                if (lanes[k].s.cnt != lanes[0].s.cnt) throw std::runtime_error("the lanes of a group disagree on the count");
                if (!lanes[k].s.kept) continue;
                if (lanes[k].s.slot != kept) throw std::runtime_error("the kept lanes' slots are not 0, 1, 2, ...");
                ++kept;
                ikdev::solutions_store(a, sa, b, k, lanes[k].s.slot, lanes[k].q, lanes[k].it,
                                       [&](const double *src, double *q_out, bool stepped) { prog.pass(a, src, q_out, b, stepped); });
            }
            if (kept != lanes[0].s.cnt || kept > N) throw std::runtime_error("the count is not the number of kept lanes");
            count[b] = lanes[0].s.cnt;
        }
    });
}

}  // extern "C"
