// pick_emu.cpp -- TEST HARNESS ONLY.  Runs the pieces of the gfx950 pick kernels (device/pick.hpp: the costs and the key;
// dls_chain_pick_lane / pick_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_pick_lane in device/chain_hot.hpp) on the CPU, one
// "lane" after another, as multistart_emu.cpp does for the multi-start kernels, next to the single-solve body of the same lane program
// (dls_chain_body / hot_chain_body) that the pick call is defined through.  Compiled by tests/ with g++ into its own shared object;
// libikgpu.so neither contains nor calls it (the product has no CPU path).
//
// program: 0  the runtime-parameter build (SMASK = -1; kSpecRuntimeKinds for a chain with a prismatic joint)
//          1  the device's general build (SMASK = 0; 1 << kSpecKinds for a chain with a prismatic joint)
//          2  the structure-specialised hot program, for the chains listed in HOT_SHAPES
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
    int log2K;   // -1: the single solve
    const double *q0, *starts;
    unsigned long long seed;
    const double *targets;
    const ikgpu_dls_params *prm;
    int rule;
    const double *q_ref, *w;   // w [nq] or null
    double *q_out;
    uint8_t *success;
    int32_t *iters;
    int32_t *winner;
    double *cost, *err_sq;
    int layout;
    const uint8_t *draw;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, ikdev::PickArgs &pk, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_out; a.success = io.success; a.iters = io.iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    pk = ikdev::PickArgs{};
    pk.ms = ikdev::MultistartArgs{io.starts, io.draw, io.seed, io.winner, io.err_sq, io.log2K};
    pk.q_ref = io.q_ref;
    pk.cost = io.cost;
    pk.rule = io.rule;
    for (int j = 0; j < ikdev::kPickMaxChain; ++j) pk.w[j] = (io.w && j < NJ) ? io.w[a.qidx[j]] : 1.0;   // (as ikgpu_dls_pick_batch folds it)
}

template <int NJ>
struct Lane {
    double q[NJ], err_sq, cost;
    bool success;
    int iters;
    unsigned long long key;
};

// One group, as multistart_emu.cpp run_groups: what lane l receives at step s of the butterfly is the minimum over the block of its
// partner l ^ (1 << s), computed from the lanes' initial keys.
template <int NJ, class Solve, class Store>
void run_groups(const IO &io, Solve solve, Store store) {
    const int K = 1 << io.log2K;
    std::vector<Lane<NJ>> lanes(static_cast<size_t>(K));
    for (int64_t b = 0; b < io.B; ++b) {
        for (int k = 0; k < K; ++k) {
            solve(b, k, lanes[k]);
            lanes[k].key = ikdev::pick_key(lanes[k].success, lanes[k].cost, lanes[k].err_sq);
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

template <int NJ, int KT, int SM>
void run_chain(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::PickArgs pk{};
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    fill(a, pk, ph, io);
    auto any = [](bool act) { return act; };
    if (io.log2K < 0) {
        for (int64_t b = 0; b < io.B; ++b) ikdev::dls_chain_body<NJ, KT, SM>(a, d, b, any);
        return;
    }
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        ikdev::dls_chain_pick_lane<NJ, KT, SM>(a, pk, d, b, k, l.q, l.success, l.iters, l.err_sq, l.cost, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::pick_store(a, pk, b, k, l.q, l.success, l.iters, l.err_sq, l.cost,
                          [&](const double *src, bool stepped) { ikdev::chain_pass_through_from(a, src, b, stepped); });
    });
}

template <int NJ, class S>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::PickArgs pk{};
    fill(a, pk, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    auto any = [](bool act) { return act; };
    if (io.log2K < 0) {
        for (int64_t b = 0; b < io.B; ++b) ikdev::hot_chain_body<NJ, S, false>(a, t, b, any);
        return;
    }
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        ikdev::hot_pick_lane<NJ, S>(a, pk, t, b, k, l.q, l.success, l.iters, l.err_sq, l.cost, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::pick_store(a, pk, b, k, l.q, l.success, l.iters, l.err_sq, l.cost,
                          [&](const double *src, bool stepped) { ikdev::hot_pass_through_from(a, src, a.q_out, b, stepped); });
    });
}

// X(NJ, code0, code1, code2, mask of prismatic joints): the Cassie leg, UR5, and UR5 on a rail (tests/prismatic_common.py)
#define HOT_SHAPES(X)                                                                    \
    X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull, 0x00u)     \
    X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull, 0x00u)     \
    X(7, 0x24e570accea17665ull, 0x4675594a939a5656ull, 0x000002424ad1d956ull, 0x01u)

int run(const char *urdf, size_t len, const ikgpu_task *task, int program, IO io) {
    ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
    const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
    if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
    if (io.prm->stop_sq_tol < 0.0) { g_err = "a pick needs a stop rule"; return 1; }
    const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
    io.draw = mask.data();
    const int nj = ph.chain.nj, kt = task->type;
    if (program == 2) {
        if (kt != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0])) { g_err = "the hot program takes a Full task with unit weights"; return 2; }
        const ikgpu::ChainStructure s = ikgpu::chain_structure(ph.chain);
#define X(N, K0, K1, K2, PM)                                                                                              \
    if (s.fits && nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2 && ph.chain.prismatic == static_cast<int>(PM)) { \
        run_chain_hot<N, ikdev::ChainStruct<K0, K1, K2, PM>>(ph, io);                                                     \
        return 0;                                                                                                         \
    }
        HOT_SHAPES(X)
#undef X
        g_err = "no hot program for " + ph.kernel_name;
        return 2;
    }
    const bool pris = ph.chain.prismatic != 0;
    constexpr int kDev = 1 << ikdev::kSpecKinds;
#define Y(N, KT)                                                                                  \
    if (nj == N && kt == KT) {                                                                    \
        if (program == 0 && !pris) run_chain<N, KT, -1>(ph, io);                                  \
        else if (program == 0) run_chain<N, KT, ikdev::kSpecRuntimeKinds>(ph, io);                \
        else if (!pris) run_chain<N, KT, 0>(ph, io);                                              \
        else run_chain<N, KT, kDev>(ph, io);                                                      \
        return 0;                                                                                 \
    }
    Y(6, 2) Y(7, 2) Y(6, 0) Y(7, 0)   // the chains of tests/test_pick_emulation.py: Full and Position tasks on 6 and 7 joints
#undef Y
    g_err = "shape not instantiated in the pick emulator: " + ph.kernel_name;
    return 1;
}

}  // namespace

extern "C" {

const char *pick_emu_last_error(void) { return g_err.c_str(); }

// The cost steps and the key of device/pick.hpp on plain arrays.  n entries: every one counts as a support entry.
double pick_emu_distance(int n, const double *w, const double *q, const double *ref) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc = ikdev::pick_distance_step(acc, w[i], q[i], ref[i]);
    return acc;
}
double pick_emu_max_distance(int n, const double *w, const double *q, const double *ref) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc = ikdev::pick_max_distance_step(acc, w[i], q[i], ref[i]);
    return acc;
}
double pick_emu_limit_margin(int n, const double *q, const double *lo, const double *hi) {
    double acc = 0.5;
    for (int i = 0; i < n; ++i) acc = ikdev::pick_margin_step(acc, q[i], lo[i], hi[i]);
    return ikdev::pick_margin_cost(acc);
}
// G: M x M row-major, its lower triangle is read; M is 3 or 6.
double pick_emu_manipulability(int M, const double *G) {
    if (M == 6) {
        double g[36];
        std::memcpy(g, G, sizeof g);
        return ikdev::pick_manipulability_cost(ikdev::pick_ldlt_det<6>(g));
    }
    double g[9];
    std::memcpy(g, G, sizeof g);
    return ikdev::pick_manipulability_cost(ikdev::pick_ldlt_det<3>(g));
}
unsigned long long pick_emu_key(int success, double cost, double err_sq) { return ikdev::pick_key(success != 0, cost, err_sq); }
// The winner of K lanes with these keys (multistart_select over the modelled butterfly): every lane must agree.
int pick_emu_select(int log2K, const unsigned long long *keys) {
    const int K = 1 << log2K;
    int agreed = -1;
    for (int k = 0; k < K; ++k) {
        const int win = ikdev::multistart_select(log2K, keys[k], k, [&](int m, unsigned long long &key, int &kk) {
            const int partner = k ^ m, lo = partner & ~(m - 1);
            int best = lo;
            for (int x = lo + 1; x < lo + m; ++x)
                if (keys[x] < keys[best]) best = x;
            key = keys[best];
            kk = best;
        });
        if (k > 0 && win != agreed) return -1;
        agreed = win;
    }
    return agreed;
}

// The support of the problem, [nq].
int pick_emu_support(const char *urdf, size_t len, const ikgpu_task *task, uint8_t *support) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        for (int i = 0; i < m.nq; ++i) support[i] = ph.q_in_chain[static_cast<size_t>(i)] ? 1 : 0;
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// What ikgpu_multistart_starts defines, on host pointers: starts_out [K-1][nq x B] in `layout`.
int pick_emu_starts(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int K, const double *q0, unsigned long long seed,
                    double *starts_out, int layout) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
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

// The single solve of `program`, host pointers in `layout`: what ikgpu_dls_solve_batch writes.
int pick_emu_single(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, const double *q0, const double *targets,
                    const ikgpu_dls_params *prm, double *q_out, uint8_t *success, int32_t *iters, int layout) {
    try {
        return run(urdf, len, task, program, IO{B, -1, q0, nullptr, 0, targets, prm, 0, nullptr, nullptr, q_out, success, iters, nullptr, nullptr, nullptr, layout, nullptr});
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// Host pointers, the layouts of ikgpu_dls_pick_batch (include/ikgpu.h); K a power of two in 2 .. 64; starts / q_ref / w / success /
// iters / winner / cost / err_sq may be null.  One task on a fixed-base chain.  Returns 2 when the chain has no hot program.
int pick_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int program, int64_t B, int K, const double *q0, const double *starts,
                 unsigned long long seed, const double *targets, const ikgpu_dls_params *prm, int rule, const double *q_ref, const double *w,
                 double *q_out, uint8_t *success, int32_t *iters, int32_t *winner, double *cost, double *err_sq, int layout) {
    try {
        int log2K = 0;
        while ((1 << log2K) < K) ++log2K;
        if (K < 2 || K > 64 || (1 << log2K) != K) { g_err = "K must be a power of two in 2 .. 64"; return 1; }
        return run(urdf, len, task, program, IO{B, log2K, q0, starts, seed, targets, prm, rule, q_ref, w, q_out, success, iters, winner, cost, err_sq, layout, nullptr});
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
