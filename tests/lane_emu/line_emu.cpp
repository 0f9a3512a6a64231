// line_emu.cpp -- TEST HARNESS ONLY.  Runs the per-lane programs of the gfx950 line kernels (dls_chain_line_body in
// ik_amd/csrc/device/chain_kernel_body.hpp, hot_line_body in device/chain_hot.hpp: a straight Cartesian line to one goal per problem,
// solved waypoint after waypoint with q on-chip) and the waypoint function behind ikgpu_line_targets (device/line.hpp) on the CPU, one
// "lane" after another, as track_emu.cpp does for the tracking programs.  Compiled by tests/ with g++ into its own shared object;
// libikgpu.so neither contains nor calls it (the product has no CPU path).
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

struct IO {
    int64_t B;
    int T;
    const double *q0, *goals;
    const ikgpu_dls_params *prm;
    double *q_traj;       // null: write the waypoints into `waypoints` instead of solving
    uint8_t *success;
    int32_t *iters, *reached, *visited;   // visited [B]: waypoints the lane's loop went through
    double *waypoints;    // [T][12 x B]
    int layout;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, const ikdev::ChainDesc<NJ> &d, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.desc = &d;
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.goals;
    a.q_out = io.q_traj; a.success = io.success; a.iters = io.iters;   // waypoint 0's slabs
    if (!io.prm) return;   // (the waypoints alone)
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
}

template <int NJ>
ikdev::ChainDesc<NJ> desc_of(const ikgpu::ProblemHost &ph) {
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    return d;
}

// the waypoints alone: what the kernel behind ikgpu_line_targets does for a chain problem (kernels.hip path_targets_chain_kernel with P = 1)
template <int NJ>
void run_waypoints(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainDesc<NJ> d = desc_of<NJ>(ph);
    ikdev::ChainKernelArgs<NJ> a{};
    fill(a, d, ph, io);
    for (int64_t b = 0; b < io.B; ++b) {
        double q[NJ], goal[12];
        ikdev::line_load(a, b, q, goal);
        ikdev::LineStart ls;
        ikdev::line_chain_start(a, d, q, goal, ls);
        for (int k = 0; k < io.T; ++k) {
            double t[12];
            ikdev::line_waypoint(ls, goal, k, io.T, t);
            for (int c = 0; c < 12; ++c) io.waypoints[static_cast<int64_t>(k) * 12 * io.B + ikdev::at(io.layout, io.B, 12, c, b)] = t[c];
        }
    }
}

template <int NJ, int KT>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    if (!io.q_traj) { run_waypoints<NJ>(ph, io); return; }
    const ikdev::ChainDesc<NJ> d = desc_of<NJ>(ph);
    ikdev::ChainKernelArgs<NJ> a{};
    fill(a, d, ph, io);
    const ikdev::LineArgs la{io.reached, io.T};
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const char *tr = std::getenv("LANE_EMU_TRIG");
    for (int64_t b = 0; b < io.B; ++b) {
        const int n = tr ? ikdev::dls_chain_line_body<NJ, KT, 0>(a, d, la, b, [](bool act) { return act; })
                         : ikdev::dls_chain_line_body<NJ, KT>(a, d, la, b, [](bool act) { return act; });
        if (io.visited) io.visited[b] = n;
    }
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainDesc<NJ> d = desc_of<NJ>(ph);
    ikdev::ChainKernelArgs<NJ> a{};
    fill(a, d, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    const ikdev::LineArgs la{io.reached, io.T};
    for (int64_t b = 0; b < io.B; ++b) {
        const int n = ikdev::hot_line_body<NJ, S>(a, t, la, b, [](bool act) { return act; });
        if (io.visited) io.visited[b] = n;
    }
}

// true when the problem was run by the hot program (LANE_EMU_HOT set, a Full task with unit weights, a known structure code)
bool try_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    if (!io.q_traj || !std::getenv("LANE_EMU_HOT") || ph.tasks[0].type != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0])) return false;
    const ikgpu::ChainStructure s = ikgpu::chain_structure(ph.chain);
    if (!s.fits) return false;
#define X(N, K0, K1, K2)                                                                      \
    if (ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) {         \
        run_chain_hot<N, K0, K1, K2>(ph, io);                                                 \
        return true;                                                                          \
    }
    X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull)
    X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull)
#undef X
    return false;
}

int run(const char *urdf, size_t len, const ikgpu_task *task, const IO &io) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        if (io.T < 1) { g_err = "the emulator takes T >= 1 (the entry point returns before any kernel otherwise)"; return 1; }
        if (try_chain_hot(ph, io)) return 0;
        if (io.q_traj && std::getenv("LANE_EMU_HOT")) { g_err = "no hot program for " + ph.kernel_name; return 2; }
        const int nj = ph.chain.nj, kt = task->type;
#define X(N)                                       \
    if (nj == N) {                                 \
        if (kt == 2) run_chain<N, 2>(ph, io);      \
        else if (kt == 0) run_chain<N, 0>(ph, io); \
        else run_chain<N, 1>(ph, io);              \
        return 0;                                  \
    }
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
        g_err = "shape not instantiated in the line emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // namespace

extern "C" {

const char *line_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, the layouts of ikgpu_line_targets (include/ikgpu.h): goals [12 x B], waypoints [T][12 x B].  One task on a fixed-base chain.
int line_emu_targets(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int T, const double *q0, const double *goals,
                     double *waypoints, int layout) {
    return run(urdf, len, task, IO{B, T, q0, goals, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, waypoints, layout});
}

// Host pointers, the layouts of ikgpu_dls_line_batch: q_traj [T][nq x B], success / iters [T][B], reached [B], visited [B] (each of
// the last four may be null).  Returns 2 when LANE_EMU_HOT is set and the chain has no hot program.
int line_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int T, const double *q0, const double *goals,
                 const ikgpu_dls_params *prm, double *q_traj, uint8_t *success, int32_t *iters, int32_t *reached, int32_t *visited, int layout) {
    return run(urdf, len, task, IO{B, T, q0, goals, prm, q_traj, success, iters, reached, visited, nullptr, layout});
}

}  // extern "C"
