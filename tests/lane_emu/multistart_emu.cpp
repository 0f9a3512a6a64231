// multistart_emu.cpp -- TEST HARNESS ONLY.  Runs the pieces of the gfx950 multi-start kernels (device/multistart.hpp: the draw, the key,
// the selection; dls_chain_multistart_lane / multistart_store in ik_amd/csrc/device/chain_kernel_body.hpp, hot_multistart_lane in
// device/chain_hot.hpp) on the CPU, one "lane" after another, as lane_emu.cpp does for the single-solve programs.  The cross-lane
// exchange of the selection is modelled from the butterfly's own invariant (below).  Compiled by tests/ with g++ into its own shared
// object; libikgpu.so neither contains nor calls it (the product has no CPU path).
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
    int log2K;
    const double *q0, *starts;
    unsigned long long seed;
    const double *targets;
    const ikgpu_dls_params *prm;
    double *q_out;
    uint8_t *success;
    int32_t *iters;
    int32_t *winner;
    double *err_sq;
    int layout;
    const uint8_t *draw;
};

template <int NJ>
void fill(ikdev::ChainKernelArgs<NJ> &a, ikdev::MultistartArgs &ms, const ikgpu::ProblemHost &ph, const IO &io) {
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_out; a.success = io.success; a.iters = io.iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    ms = ikdev::MultistartArgs{io.starts, io.draw, io.seed, io.winner, io.err_sq, io.log2K};
}

template <int NJ>
struct Lane {
    double q[NJ], err_sq;
    bool success;
    int iters;
    unsigned long long key;
};

// One group: `solve(b, k, lane)` is the lane's own part; then every lane runs multistart_select.  Before step s of the butterfly a lane
// holds the minimum over the aligned block of 1 << s lanes it belongs to, so what lane l receives at step s is the minimum over the
// block of its partner l ^ (1 << s): computed here from the lanes' initial keys.
template <int NJ, class Solve, class Store>
void run_groups(const IO &io, Solve solve, Store store) {
    const int K = 1 << io.log2K;
    std::vector<Lane<NJ>> lanes(static_cast<size_t>(K));
    for (int64_t b = 0; b < io.B; ++b) {
        for (int k = 0; k < K; ++k) {
            solve(b, k, lanes[k]);
            lanes[k].key = ikdev::multistart_key(lanes[k].success, lanes[k].err_sq);
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
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::MultistartArgs ms{};
    ikdev::ChainDesc<NJ> d{};
    const std::vector<double> t = ikgpu::chain_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    fill(a, ms, ph, io);
    // LANE_EMU_TRIG set: the device's general build (SMASK = 0); unset: the runtime-parameter build (SMASK = -1) -- as lane_emu.cpp
    const bool tr = std::getenv("LANE_EMU_TRIG") != nullptr;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        if (tr) ikdev::dls_chain_multistart_lane<NJ, KT, 0>(a, ms, d, b, k, l.q, l.success, l.iters, l.err_sq, any);
        else ikdev::dls_chain_multistart_lane<NJ, KT>(a, ms, d, b, k, l.q, l.success, l.iters, l.err_sq, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::multistart_store(a, ms, b, k, l.q, l.success, l.iters, l.err_sq,
                                [&](const double *src, bool stepped) { ikdev::chain_pass_through_from(a, src, b, stepped); });
    });
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_chain_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikdev::MultistartArgs ms{};
    fill(a, ms, ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    const bool never = io.prm->stop_sq_tol < 0.0;
    auto any = [](bool act) { return act; };
    run_groups<NJ>(io, [&](int64_t b, int k, Lane<NJ> &l) {
        if (never) ikdev::hot_multistart_lane<NJ, S, true>(a, ms, t, b, k, l.q, l.success, l.iters, l.err_sq, any);
        else ikdev::hot_multistart_lane<NJ, S, false>(a, ms, t, b, k, l.q, l.success, l.iters, l.err_sq, any);
    }, [&](int64_t b, int k, const Lane<NJ> &l) {
        ikdev::multistart_store(a, ms, b, k, l.q, l.success, l.iters, l.err_sq,
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

const char *multistart_emu_last_error(void) { return g_err.c_str(); }

// u of (seed, b, k, i): the emulator's copy of the draw (device/multistart.hpp)
double multistart_emu_uniform(unsigned long long seed, int64_t b, int k, int i) { return ikdev::multistart_uniform(seed, b, k, i); }

// The entries a generated start draws, [nq], and the problem's support, [nq] (either may be null).  Any model, free-flyer or not.
int multistart_emu_mask(const char *urdf, size_t len, int free_flyer, const ikgpu_task *tasks, int ntasks, uint8_t *draw, uint8_t *support) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, free_flyer != 0);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, tasks, ntasks, false);
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        for (int i = 0; i < m.nq; ++i) {
            if (draw) draw[i] = mask[static_cast<size_t>(i)];
            if (support) support[i] = ph.q_in_chain[static_cast<size_t>(i)] ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// What ikgpu_multistart_starts defines, on host pointers: starts_out [K-1][nq x B] in `layout`.
int multistart_emu_starts(const char *urdf, size_t len, int free_flyer, const ikgpu_task *tasks, int ntasks, int64_t B, int K, const double *q0,
                          unsigned long long seed, double *starts_out, int layout) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, free_flyer != 0);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, tasks, ntasks, false);
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

// Host pointers, the layouts of ikgpu_dls_multistart_batch (include/ikgpu.h); K a power of two in 2 .. 64; starts / success / iters /
// winner / err_sq may be null.  One task on a fixed-base chain.  Returns 2 when LANE_EMU_HOT is set and the chain has no hot program.
int multistart_emu_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, int K, const double *q0, const double *starts,
                       unsigned long long seed, const double *targets, const ikgpu_dls_params *prm, double *q_out, uint8_t *success,
                       int32_t *iters, int32_t *winner, double *err_sq, int layout) {
    try {
        int log2K = 0;
        while ((1 << log2K) < K) ++log2K;
        if (K < 2 || K > 64 || (1 << log2K) != K) { g_err = "K must be a power of two in 2 .. 64"; return 1; }
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain) { g_err = "not a chain problem: " + ph.kernel_name; return 1; }
        const std::vector<uint8_t> mask = ikgpu::multistart_draw_mask(m, ph);
        const IO io{B, log2K, q0, starts, seed, targets, prm, q_out, success, iters, winner, err_sq, layout, mask.data()};
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
        g_err = "shape not instantiated in the multi-start emulator: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
