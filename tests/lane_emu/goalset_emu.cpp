// goalset_emu.cpp -- TEST HARNESS ONLY.  Runs the goal-set kernels' bodies (dls_chain_goalset_body in
// ik_amd/csrc/device/chain_kernel_body.hpp, hot_goalset_body in device/chain_hot.hpp; device/goalset.hpp) on the CPU, one "lane" after
// another, as multistart_emu.cpp does for the multi-start pieces.  Two passes per group: the lanes' own solves (dls_chain_goalset_lane /
// hot_goalset_lane) give every lane's key and success flag; then the BODY runs for every lane gid of the group -- its own solve again,
// the selection, the reachability flag, the stores -- with the two cross-lane functors answered from the first pass.  Compiled by tests/
// with g++ into its own shared object; libikgpu.so neither contains nor calls it (the product has no CPU path).
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
    int log2G, log2K;
    const double *q0, *starts;
    unsigned long long seed;
    const double *goals;
    const ikgpu_dls_params *prm;
    double *q_out;
    uint8_t *success;
    int32_t *iters;
    int32_t *goal, *start;
    double *err_sq;
    uint8_t *reachable;
    int layout;
    const uint8_t *draw;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, ikdev::GoalsetArgs &ga, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.goals;
    a.q_out = io.q_out; a.success = io.success; a.iters = io.iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    ga = ikdev::GoalsetArgs{ikdev::MultistartArgs{io.starts, io.draw, io.seed, nullptr, io.err_sq, io.log2K}, io.goal, io.start, io.reachable, io.log2G};
}

struct Lane {
    unsigned long long key;
    bool success;
};

// solve(b, g, k, lane): the lane's own part; body(gid, exchange, any): the whole body of lane gid.  Before step s of the butterfly a lane
// holds the minimum over the aligned block of 1 << s lanes it belongs to, so what lane l receives at step s is the minimum over the block
// of its partner l ^ (1 << s) (multistart_emu.cpp); the OR over a goal's K lanes is read from the first pass likewise.  One extra group
// past the batch stands for the tail lanes of the last wave: it must store nothing (the outputs have no room for it: the caller's canaries
// say so).
template <class Solve, class Body>
void run_groups(const IO &io, Solve solve, Body body) {
    const int log2J = io.log2G + io.log2K, J = 1 << log2J, K = 1 << io.log2K;
    std::vector<Lane> lanes(static_cast<size_t>(J));
    for (int64_t prob = 0; prob <= io.B; ++prob) {
        const int64_t b = prob < io.B ? prob : io.B - 1;
        for (int j = 0; j < J; ++j) solve(b, j >> io.log2K, j & (K - 1), lanes[j]);
        for (int j = 0; j < J; ++j) {
            body((prob << log2J) + j,
                 [&lanes, j](int m, unsigned long long &key, int &jj) {
                     const int partner = j ^ m, lo = partner & ~(m - 1);
                     int best = lo;
                     for (int x = lo + 1; x < lo + m; ++x)
                         if (lanes[x].key < lanes[best].key) best = x;
                     key = lanes[best].key;
                     jj = best;
                 },
                 [&lanes, j](int log2K, bool flag) {
                     const int n = 1 << log2K, lo = j & ~(n - 1);
                     if (flag != lanes[j].success) throw std::runtime_error("a lane's second solve disagrees with its first");
                     bool any = false;
                     for (int x = lo; x < lo + n; ++x) any = any || lanes[x].success;
                     return any;
                 });
        }
    }
}

template <int NJ, int KT>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::GoalsetArgs ga{};
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    fill(a, ga, ph, io);
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const bool tr = std::getenv("LANE_EMU_TRIG") != nullptr;
    auto any_active = [](bool act) { return act; };
    run_groups(io, [&](int64_t b, int g, int k, Lane &l) {
        double q[NJ], err_sq;
        int iters;
        if (tr) ikdev::dls_chain_goalset_lane<NJ, KT, 0>(a, ga, d, b, g, k, q, l.success, iters, err_sq, any_active);
        else ikdev::dls_chain_goalset_lane<NJ, KT>(a, ga, d, b, g, k, q, l.success, iters, err_sq, any_active);
        l.key = ikdev::multistart_key(l.success, err_sq);
    }, [&](int64_t gid, auto exchange, auto any) {
        if (tr) ikdev::dls_chain_goalset_body<NJ, KT, 0>(a, ga, d, gid, any_active, exchange, any);
        else ikdev::dls_chain_goalset_body<NJ, KT>(a, ga, d, gid, any_active, exchange, any);
    });
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::GoalsetArgs ga{};
    fill(a, ga, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    const bool never = io.prm->stop_sq_tol < 0.0;
    auto any_active = [](bool act) { return act; };
    run_groups(io, [&](int64_t b, int g, int k, Lane &l) {
        double q[NJ], err_sq;
        int iters;
        if (never) ikdev::hot_goalset_lane<NJ, S, true>(a, ga, t, b, g, k, q, l.success, iters, err_sq, any_active);
        else ikdev::hot_goalset_lane<NJ, S, false>(a, ga, t, b, g, k, q, l.success, iters, err_sq, any_active);
        l.key = ikdev::multistart_key(l.success, err_sq);
    }, [&](int64_t gid, auto exchange, auto any) {
        if (never) ikdev::hot_goalset_body<NJ, S, true>(a, ga, t, gid, any_active, exchange, any);
        else ikdev::hot_goalset_body<NJ, S, false>(a, ga, t, gid, any_active, exchange, any);
    });
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

const char *goalset_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, the layouts of ikgpu_dls_goalset_batch (include/ikgpu.h); G and K powers of two with G K <= 64 (G = K = 1 runs too: a group
// of one lane); starts / success / iters / goal / start / err_sq / reachable may be null.  One task on a fixed-base chain.  Returns 2 when
// LANE_EMU_HOT is set and the chain has no hot program.
int goalset_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int G, int K, const double *q0, const double *starts,
                    unsigned long long seed, const double *goals, const ikgpu_dls_params *prm, double *q_out, uint8_t *success, int32_t *iters,
                    int32_t *goal, int32_t *start, double *err_sq, uint8_t *reachable, int layout) {
    try {
        int log2G = 0, log2K = 0;
        while ((1 << log2G) < G) ++log2G;
        while ((1 << log2K) < K) ++log2K;
        if (G < 1 || K < 1 || (1 << log2G) != G || (1 << log2K) != K || G * K > 64) { g_err = "G and K must be powers of two with G K <= 64"; return 1; }
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        const IO io{B, log2G, log2K, q0, starts, seed, goals, prm, q_out, success, iters, goal, start, err_sq, reachable, layout, mask.data()};
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
        g_err = "shape not instantiated in the goal-set emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
