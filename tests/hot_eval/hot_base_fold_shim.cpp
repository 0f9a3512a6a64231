// hot_base_fold_shim.cpp -- TEST HARNESS ONLY.  The two forms of hot_evaluate of the structure-specialised chain program
// (ik_amd/csrc/device/chain_hot.hpp) side by side on the CPU -- the default one on the world target, and BASE_FOLDED on
// hot_fold_base's P_0^-1 oMt -- and one never-stop hot_dls solve, for the two structure codes kernels_hot.hip instantiates, arm7, the
// chains of tests/hot_fold_common.py and the ones tests/test_hot_base_fold_host.py adds.  Compiled by that test with g++ into its own
// shared object; libikgpu.so neither contains nor calls it.  A chain whose code is not in the list below is refused with the X(...)
// line to add.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "device/chain_hot.hpp"
#include "ikgpu.h"
#include "model.hpp"
#include "problem.hpp"

namespace {

thread_local std::string g_err;

struct Out {
    double *e, *col, *e_folded, *col_folded, *q_next;   // [B][6], [B][NJ][6], the same of the folded form, [B][nq]
};

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run(const ikgpu::ProblemHost &ph, int64_t B, const double *q, const double *targets, int iterations, double lam2, const Out &o) {
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    ikdev::ChainKernelArgs<NJ> a{};
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.layout = 1; a.B = B; a.q0 = q; a.targets = targets;
    a.prm.max_iterations = iterations; a.prm.lam2 = lam2; a.prm.step_length = 1.0; a.prm.stop_sq_tol = -1.0;
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    for (int64_t b = 0; b < B; ++b) {
        double qj[NJ], oMt[12], oM0[12], e[6], col[NJ][6];
        for (int j = 0; j < NJ; ++j) qj[j] = q[b * a.nq + a.qidx[j]];
        ikdev::load_target(a, b, oMt);
        ikdev::hot_evaluate<NJ, S>(t, qj, oMt, e, col);
        for (int r = 0; r < 6; ++r) o.e[6 * b + r] = e[r];
        for (int j = 0; j < NJ; ++j)
            for (int r = 0; r < 6; ++r) o.col[6 * NJ * b + 6 * j + r] = col[j][r];
        ikdev::hot_fold_base<S>(t, oMt, oM0);
        ikdev::hot_evaluate<NJ, S, true>(t, qj, oM0, e, col);
        for (int r = 0; r < 6; ++r) o.e_folded[6 * b + r] = e[r];
        for (int j = 0; j < NJ; ++j)
            for (int r = 0; r < 6; ++r) o.col_folded[6 * NJ * b + 6 * j + r] = col[j][r];
        // the never-stop solve of `iterations` steps from the same q (the chain's entries; the others are copied)
        int iters;
        bool success;
        ikdev::hot_dls<NJ, S, true>(t, a.prm, qj, oMt, iters, success, [](bool act) { return act; });
        for (int i = 0; i < a.nq; ++i) o.q_next[b * a.nq + i] = q[b * a.nq + i];
        for (int j = 0; j < NJ; ++j) o.q_next[b * a.nq + a.qidx[j]] = qj[j];
    }
}

}  // namespace

extern "C" {

const char *hot_base_fold_last_error(void) { return g_err.c_str(); }

// q: [B][nq], targets: [B][12] (rotation row-major, then translation), one Full task with unit weights.  Out: e [B][6] and col
// [B][NJ][6] (hot_evaluate's error and its own columns) in the default form and in the folded one, q_next [B][nq] (q after `iterations`
// never-stop DLS steps with damping^2 = lam2 and step length 1), *nj.
int hot_base_fold_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, const double *q, const double *targets, int iterations,
                      double lam2, double *e_out, double *col_out, double *e_folded, double *col_folded, double *q_next, int *nj) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain || ph.tasks[0].type != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0]))
            throw std::runtime_error("not a chain problem with one Full task of unit weights");
        const ikgpu::ChainStructure s = ikgpu::chain_structure(ph.chain);
        if (!s.fits) throw std::runtime_error("the chain has no structure code");
        *nj = ph.chain.nj;
        const Out o{e_out, col_out, e_folded, col_folded, q_next};
#define X(N, K0, K1, K2)                                                                      \
    if (ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) {         \
        run<N, K0, K1, K2>(ph, B, q, targets, iterations, lam2, o);                           \
        return 0;                                                                             \
    }
        X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull)   // Cassie leg
        X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull)   // UR5 / UR10
        // the chains of tests/hot_fold_common.py
        X(2, 0x700003cacadc0000ull, 0x0000000000000000ull, 0x0000000000000000ull)   // run2_whole
        X(4, 0x79595b80001c0000ull, 0x00000380001c0000ull, 0x0000000000000000ull)   // run2_middle
        X(5, 0x79595b80001c0000ull, 0x70000380001e5656ull, 0x0000000000000000ull)   // run3_middle
        X(5, 0x700003cacadc0000ull, 0x700003cacadc0000ull, 0x0000000000000000ull)   // run2_twice
        X(3, 0x70000380001c0000ull, 0x00000000001c0000ull, 0x0000000000000000ull)   // no_run
        // arm7, and the chains of tests/test_hot_base_fold_host.py
        X(7, 0x70000380001c0000ull, 0x70000380001c0000ull, 0x00000380001c0000ull)   // arm7: every placement general
        X(3, 0x7000038000025656ull, 0x00000000001c0000ull, 0x0000000000000000ull)   // identity_base
        X(3, 0x70000380001e5656ull, 0x00000000001c0000ull, 0x0000000000000000ull)   // shifted_base
#undef X
        char line[160];
        std::snprintf(line, sizeof line, "structure code not instantiated in the shim: X(%d, 0x%016llxull, 0x%016llxull, 0x%016llxull)", ph.chain.nj,
                      (unsigned long long)s.code[0], (unsigned long long)s.code[1], (unsigned long long)s.code[2]);
        throw std::runtime_error(line);
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
