// solutions_emu.cpp -- TEST HARNESS ONLY.  Runs the pieces of the gfx950 solution-set kernels (device/solutions.hpp: solutions_offer,
// solutions_take; dls_chain_solutions_lane / solutions_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_solutions_lane in
// device/chain_hot.hpp) on the CPU, as multistart_emu.cpp does for the multi-start kernels.  The K lanes of a group are run STEP BY STEP:
// in step j every lane makes its offer, then every lane takes lane j's offer and entries -- what the cross-lane fetches of the device
// deliver, since a fetch reads the value the source lane holds at that point of the step.  Compiled by tests/ with g++ into its own
// shared object; libikgpu.so neither contains nor calls it (the product has no CPU path).
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
    int log2K, N;
    const double *q0, *starts;
    unsigned long long seed;
    const double *targets;
    const ikgpu_dls_params *prm;
    double sep;
    double *q_sols;
    int32_t *count, *which, *iters;
    int layout;
    const uint8_t *draw;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, ikdev::SolutionsArgs &sa, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_sols; a.success = nullptr; a.iters = io.iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    sa = ikdev::SolutionsArgs{ikdev::MultistartArgs{io.starts, io.draw, io.seed, nullptr, nullptr, io.log2K}, io.count, io.which, io.sep, io.N};
}

template <int NJ>
struct Lane {
    double q[NJ];
    bool success;
    int iters;
    ikdev::SolutionsLane s;
};

// What a lane of the group receives in step j.  any(): the ballot is over the wave; a group alone decides here -- the other groups of a
// wave can only make a lane fetch entries it then does not use.
template <int NJ>
struct Fetch {
    const std::vector<Lane<NJ>> *lanes;
    bool flag(int j, bool) const { return (*lanes)[static_cast<size_t>(j)].s.offer; }
    bool any(bool f) const { return f; }
    template <int N_>
    void q(int j, const double (&)[N_], double (&theirs)[N_]) const {
        for (int i = 0; i < N_; ++i) theirs[i] = (*lanes)[static_cast<size_t>(j)].q[i];
    }
};

template <int NJ, class Solve, class Store>
void run_groups(const IO &io, Solve solve, Store store) {
    const int K = 1 << io.log2K;
    std::vector<Lane<NJ>> lanes(static_cast<size_t>(K));
    for (int64_t b = 0; b < io.B; ++b) {
        for (int k = 0; k < K; ++k) {
            lanes[k].s = ikdev::SolutionsLane{};
            solve(b, k, lanes[k]);
        }
        for (int j = 0; j < K; ++j) {
            for (int k = 0; k < K; ++k) ikdev::solutions_offer(lanes[k].s, lanes[k].success, io.N);
            for (int k = 0; k < K; ++k) ikdev::solutions_take<NJ>(lanes[k].s, j, k, io.sep, lanes[k].q, Fetch<NJ>{&lanes});
        }
        int kept = 0;
        for (int k = 0; k < K; ++k) {
            if (lanes[k].s.cnt != lanes[0].s.cnt) throw std::runtime_error("the lanes of a group disagree on the count");
            if (!lanes[k].s.kept) continue;
            if (lanes[k].s.slot != kept) throw std::runtime_error("the kept lanes' slots are not 0, 1, 2, ...");
            ++kept;
            store(b, k, lanes[k]);
        }
        if (kept != lanes[0].s.cnt || kept > io.N) throw std::runtime_error("the count is not the number of kept lanes");
        io.count[b] = lanes[0].s.cnt;   // (lane 0 of the group)
    }
}

template <int NJ, int KT>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::SolutionsArgs sa{};
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    fill(a, sa, ph, io);
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const bool tr = std::getenv("LANE_EMU_TRIG") != nullptr;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        if (tr) ikdev::dls_chain_solutions_lane<NJ, KT, 0>(a, sa, d, b, k, l.q, l.success, l.iters, any);
        else ikdev::dls_chain_solutions_lane<NJ, KT>(a, sa, d, b, k, l.q, l.success, l.iters, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::solutions_store(a, sa, b, k, l.s.slot, l.q, l.iters,
                               [&](const double *src, double *q_out, bool stepped) { ikdev::chain_pass_through_into(a, src, q_out, b, stepped); });
    });
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::SolutionsArgs sa{};
    fill(a, sa, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        ikdev::hot_solutions_lane<NJ, S>(a, sa, t, b, k, l.q, l.success, l.iters, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::solutions_store(a, sa, b, k, l.s.slot, l.q, l.iters,
                               [&](const double *src, double *q_out, bool stepped) { ikdev::hot_pass_through_from(a, src, q_out, b, stepped); });
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

const char *solutions_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, the layouts of ikgpu_dls_solutions_batch (include/ikgpu.h); K a power of two in 2 .. 64, 1 <= N <= K; starts / which /
// iters may be null.  One task on a fixed-base chain.  Returns 2 when LANE_EMU_HOT is set and the chain has no hot program.
int solutions_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int K, int N, const double *q0, const double *starts,
                      unsigned long long seed, const double *targets, const ikgpu_dls_params *prm, double sep, double *q_sols, int32_t *count,
                      int32_t *which, int32_t *iters, int layout) {
    try {
        int log2K = 0;
        while ((1 << log2K) < K) ++log2K;
        if (K < 2 || K > 64 || (1 << log2K) != K) { g_err = "K must be a power of two in 2 .. 64"; return 1; }
        if (N < 1 || N > K) { g_err = "N must be 1 .. K"; return 1; }
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        const IO io{B, log2K, N, q0, starts, seed, targets, prm, sep, q_sols, count, which, iters, layout, mask.data()};
        if (try_chain_hot(ph, io)) return 0;
        if (std::getenv("LANE_EMU_HOT")) { g_err = "no hot program for " + ph.kernel_name; return 2; }
        const int nj = ph.chain.nj, kt = task->type;
#define X(N_)                                       \
    if (nj == N_) {                                 \
        if (kt == 2) run_chain<N_, 2>(ph, io);      \
        else if (kt == 0) run_chain<N_, 0>(ph, io); \
        else run_chain<N_, 1>(ph, io);              \
        return 0;                                   \
    }
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
        g_err = "shape not instantiated in the solution-set emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
