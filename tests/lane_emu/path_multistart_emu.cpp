// path_multistart_emu.cpp -- TEST HARNESS ONLY.  Runs the pieces of the gfx950 path multi-start kernels (dls_chain_path_multistart_lane,
// path_scout, path_multistart_key and path_multistart_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_path_multistart_lane in
// device/chain_hot.hpp: K starts per problem against the path's first pose, each start that entered scouting the path behind it without a
// trajectory store, the one that gets furthest stored) on the CPU, one "lane" after another in groups of K, as multistart_emu.cpp does
// for the multi-start pieces and path_emu.cpp for the path program.  The cross-lane exchange of the selection is modelled from the
// butterfly's own invariant (multistart_emu.cpp); a wave's trip count is the largest of its lanes' (a lane leaves its loops when it is
// dead, the wave when all are).  Compiled by tests/ with g++ into its own shared object; libikgpu.so neither contains nor calls it (the
// product has no CPU path).
#include <algorithm>
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
    int log2K, P, T;                    // P vias: via 0 and P - 1 segments behind it
    const double *q0, *starts;
    unsigned long long seed;
    const double *vias;                 // [P][12 x B]
    const ikgpu_dls_params *prm;
    double max_joint_step;
    double *q_entry;
    uint8_t *entry_success;
    int32_t *entry_iters, *winner;
    double *err_sq;
    int32_t *reached, *reached_all;     // [B], [K][B]
    int32_t *visited;                   // [ceil(B K / 64)]: waypoints each wave's loops went through
    int layout;
    const uint8_t *draw;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, ikdev::PathMultistartArgs &pm, const ikdev::ChainDesc<NJ> &d, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.desc = &d;
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.vias;
    a.q_out = io.q_entry; a.success = io.entry_success; a.iters = io.entry_iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    const int64_t N = static_cast<int64_t>(io.P - 1) * io.T;
    pm = ikdev::PathMultistartArgs{ikdev::MultistartArgs{io.starts, io.draw, io.seed, io.winner, io.err_sq, io.log2K}, io.reached, io.reached_all,
                                   N > 0 ? io.T : 0, N > 0 ? io.P - 1 : 0, io.max_joint_step};
}

template <int NJ>
ikdev::ChainDesc<NJ> desc_of(const ikgpu::ProblemHost &ph) {
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    return d;
}

template <int NJ>
struct Lane {
    double q[NJ], err_sq;
    bool success;
    int iters, reached;
    unsigned long long key;
};

// One group after another: `solve(b, k, lane)` is the lane's own part and returns its trip count; then every lane of the group stores its
// reached_all entry and runs multistart_select (multistart_emu.cpp run_groups: what a lane receives at step s of the butterfly is the
// minimum over its partner's aligned block); the winner stores.
template <int NJ, class Solve, class Store>
void run_groups(const IO &io, const ikdev::PathMultistartArgs &pm, Solve solve, Store store) {
    const int K = 1 << io.log2K;
    std::vector<Lane<NJ>> lanes(static_cast<size_t>(K));
    if (io.visited) std::fill(io.visited, io.visited + (io.B * K + 63) / 64, 0);
    for (int64_t b = 0; b < io.B; ++b) {
        for (int k = 0; k < K; ++k) {
            const int n = solve(b, k, lanes[k]);
            lanes[k].key = ikdev::path_multistart_key(pm, lanes[k].success, lanes[k].reached, lanes[k].err_sq);
            if (io.visited) io.visited[(b * K + k) / 64] = std::max(io.visited[(b * K + k) / 64], n);
            if (pm.reached_all) pm.reached_all[static_cast<int64_t>(k) * io.B + b] = lanes[k].reached;
        }
        int stored = 0;
        for (int k = 0; k < K; ++k) {
            const int win = ikdev::multistart_select(io.log2K, lanes[k].key, k, [&](int m, unsigned long long &key, int &kk) {
                const int partner = k ^ m, lo = partner & ~(m - 1);
                int best = lo;
                for (int x = lo + 1; x < lo + m; ++x)
                    if (lanes[x].key < lanes[best].key) best = x;
                key = lanes[best].key;
                kk = best;
            });
            if (win == k) {
                store(b, k, lanes[k]);
                ++stored;
            }
        }
        if (stored != 1) throw std::runtime_error("the selection left " + std::to_string(stored) + " winners in a group");
    }
}

template <int NJ, int KT>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainDesc<NJ> d = desc_of<NJ>(ph);
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::PathMultistartArgs pm{};
    fill(a, pm, d, ph, io);
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const bool tr = std::getenv("LANE_EMU_TRIG") != nullptr;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, pm, [&](int64_t b, int k, Lane<NJ> &l) {
        return tr ? ikdev::dls_chain_path_multistart_lane<NJ, KT, 0>(a, pm, d, b, k, l.q, l.success, l.iters, l.err_sq, l.reached, any)
                  : ikdev::dls_chain_path_multistart_lane<NJ, KT>(a, pm, d, b, k, l.q, l.success, l.iters, l.err_sq, l.reached, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::path_multistart_store(a, pm, b, k, l.q, l.success, l.iters, l.err_sq, l.reached,
                                     [&](const double *src, bool stepped) { ikdev::chain_pass_through_from(a, src, b, stepped); });
    });
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainDesc<NJ> d = desc_of<NJ>(ph);
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::PathMultistartArgs pm{};
    fill(a, pm, d, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, pm, [&](int64_t b, int k, Lane<NJ> &l) {
        return ikdev::hot_path_multistart_lane<NJ, S>(a, pm, t, b, k, l.q, l.success, l.iters, l.err_sq, l.reached, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::path_multistart_store(a, pm, b, k, l.q, l.success, l.iters, l.err_sq, l.reached,
                                     [&](const double *src, bool stepped) { ikdev::hot_pass_through_from(a, src, a.q_out, b, stepped); });
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

const char *path_multistart_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, the layouts of ikgpu_dls_path_multistart_batch (include/ikgpu.h) without the trajectory; K a power of two in 2 .. 64;
// P >= 1 vias, T >= 1 (the emulator of the kernel: the entry point's own refusals are not modelled); every output but q_entry may be
// null.  visited [ceil(B K / 64)].  One task on a fixed-base chain.  Returns 2 when LANE_EMU_HOT is set and the chain has no hot program.
int path_multistart_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int K, int P, int T, const double *q0,
                            const double *starts, unsigned long long seed, const double *vias, const ikgpu_dls_params *prm, double max_joint_step,
                            double *q_entry, uint8_t *entry_success, int32_t *entry_iters, int32_t *winner, double *err_sq, int32_t *reached,
                            int32_t *reached_all, int32_t *visited, int layout) {
    try {
        int log2K = 0;
        while ((1 << log2K) < K) ++log2K;
        if (K < 2 || K > 64 || (1 << log2K) != K) { g_err = "K must be a power of two in 2 .. 64"; return 1; }
        if (P < 1 || T < 0) { g_err = "the emulator takes P >= 1 and T >= 0"; return 1; }
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        const IO io{B, log2K, P, T, q0, starts, seed, vias, prm, max_joint_step, q_entry, entry_success, entry_iters, winner, err_sq,
                    reached, reached_all, visited, layout, mask.data()};
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
        g_err = "shape not instantiated in the path multi-start emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
