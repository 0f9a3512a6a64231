// track_emu.cpp -- TEST HARNESS ONLY.  Runs the per-lane programs of the gfx950 tracking kernels (dls_chain_track_body in
// ik_amd/csrc/device/chain_kernel_body.hpp, hot_track_body in device/chain_hot.hpp: T chained ik::dls() calls with q on-chip between
// them) on the CPU, one "lane" after another, as lane_emu.cpp does for the single-solve programs.  Compiled by tests/ with g++ into its
// own shared object; libikgpu.so neither contains nor calls it (the product has no CPU path).
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
    const double *q0, *targets;
    const ikgpu_dls_params *prm;
    double *q_traj;
    uint8_t *success;
    int32_t *iters;
    int layout;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_traj; a.success = io.success; a.iters = io.iters;   // waypoint 0's slabs
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
}

template <int NJ, int KT>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    fill(a, ph, io);
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const char *tr = std::getenv("LANE_EMU_TRIG");
    for (int64_t b = 0; b < io.B; ++b) {
        if (tr) ikdev::dls_chain_track_body<NJ, KT, 0>(a, d, io.T, b, [](bool act) { return act; });
        else ikdev::dls_chain_track_body<NJ, KT>(a, d, io.T, b, [](bool act) { return act; });
    }
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    fill(a, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    for (int64_t b = 0; b < io.B; ++b) {
        if (io.prm->stop_sq_tol < 0.0) ikdev::hot_track_body<NJ, S, true>(a, t, io.T, b, [](bool act) { return act; });
        else ikdev::hot_track_body<NJ, S, false>(a, t, io.T, b, [](bool act) { return act; });
    }
}

// true when the problem was run by the hot program (LANE_EMU_HOT set, a Full task with unit weights, a known structure code)
bool try_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    if (!std::getenv("LANE_EMU_HOT") || ph.tasks[0].type != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0])) return false;
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

}  // namespace

extern "C" {

const char *track_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, the layouts of ikgpu_dls_track_batch (include/ikgpu.h): targets [T][12 x B], q_traj [T][nq x B], success / iters
// [T][B] (either may be null).  One task on a fixed-base chain.  Returns 2 when LANE_EMU_HOT is set and the chain has no hot program.
int track_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int T, const double *q0, const double *targets,
                  const ikgpu_dls_params *prm, double *q_traj, uint8_t *success, int32_t *iters, int layout) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        const IO io{B, T, q0, targets, prm, q_traj, success, iters, layout};
        if (try_chain_hot(ph, io)) return 0;
        if (std::getenv("LANE_EMU_HOT")) { g_err = "no hot program for " + ph.kernel_name; return 2; }
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
        g_err = "shape not instantiated in the tracking emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
