// hot_eval_shim.cpp -- TEST HARNESS ONLY.  Exposes hot_evaluate of the structure-specialised chain program
// (ik_amd/csrc/device/chain_hot.hpp) on the CPU for the structure codes kernels_hot.hip instantiates, so that its error vector and
// Jacobian columns can be compared with the oracle's, stage-wise, in the GPU-less build container.  Compiled by
// tests/test_hot_evaluate.py with g++ into its own shared object; libikgpu.so neither contains nor calls it.
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

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run(const ikgpu::ProblemHost &ph, int64_t B, const double *q, const double *targets, double *e_out, double *J_out, double *col_out,
         int *leader_out) {
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    ikdev::ChainKernelArgs<NJ> a{};
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.layout = 1; a.B = B; a.q0 = q; a.targets = targets;
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    for (int j = 0; j < NJ; ++j) leader_out[j] = ikdev::ChainRuns<S, NJ>::value.leader[j];
    for (int64_t b = 0; b < B; ++b) {
        double qj[NJ], oMt[12], e[6], col[NJ][6];
        for (int j = 0; j < NJ; ++j) qj[j] = q[b * a.nq + a.qidx[j]];
        ikdev::load_target(a, b, oMt);
        ikdev::hot_evaluate<NJ, S>(t, qj, oMt, e, col);
        for (int r = 0; r < 6; ++r) e_out[6 * b + r] = e[r];
        for (int k = 0; k < 6 * a.nv; ++k) J_out[6 * a.nv * b + k] = 0.0;
        for (int j = 0; j < NJ; ++j)
            for (int r = 0; r < 6; ++r) {
                J_out[6 * a.nv * b + r * a.nv + a.vidx[j]] = -col[j][r];   // col: the negated task Jacobian columns
                col_out[6 * NJ * b + 6 * j + r] = col[j][r];
            }
    }
}

}  // namespace

extern "C" {

const char *hot_eval_last_error(void) { return g_err.c_str(); }

// q: [B][nq], targets: [B][12] (rotation row-major, then translation), one Full task with unit weights.  Out: e [B][6], J [B][6][nv]
// (the task Jacobian, as the oracle returns it), col [B][NJ][6] (hot_evaluate's own columns), leader [NJ] (ChainRuns), *nj.
int hot_eval_run(const char *urdf, size_t len, const ikgpu_task *task, int64_t B, const double *q, const double *targets, double *e_out,
                 double *J_out, double *col_out, int *leader_out, int *nj) {
    try {
        ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
        ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
        if (ph.kind != ikgpu::KernelKind::Chain || ph.tasks[0].type != IKGPU_FULL || !ikgpu::task_has_unit_weights(ph.tasks[0]))
            throw std::runtime_error("not a chain problem with one Full task of unit weights");
        const ikgpu::ChainStructure s = ikgpu::chain_structure(ph.chain);
        if (!s.fits) throw std::runtime_error("the chain has no structure code");
        *nj = ph.chain.nj;
#define X(N, K0, K1, K2)                                                                      \
    if (ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) {         \
        run<N, K0, K1, K2>(ph, B, q, targets, e_out, J_out, col_out, leader_out);             \
        return 0;                                                                             \
    }
        X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull)   // Cassie leg
        X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull)   // UR5 / UR10
#undef X
        throw std::runtime_error("structure code not instantiated in the shim: " + ph.kernel_name);
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
