// tree_emu.cpp -- TEST HARNESS ONLY.  The per-lane program of the free-flyer tree kernels (ik_amd/csrc/device/tree_kernel_body.hpp) on
// the CPU, one "lane" after another, in the compile-time build the LAUNCHER would pick: the build comes from problem.cpp
// select_tree_build and its SPEC from tree_build.hpp with_tree_spec, the two functions kernels.hip run_dls_tree dispatches on -- no
// environment switch.  Around the lane program it hands over what the kernel wrapper (kernels.hip dls_tree_kernel) does: the first
// problem of the lane's 128-lane workgroup where the build addresses targets through LaneRows, and a column for the outside joints
// where the wrapper keeps them in LDS.  Compiled by tests/ with g++ into its own shared object; libikgpu.so neither contains nor calls it.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "device/tree_kernel_body.hpp"
#include "ikgpu.h"
#include "model.hpp"
#include "problem.hpp"
#include "tree_build.hpp"

namespace {

thread_local std::string g_err;
constexpr int kTreeBlock = 128;   // kernels.hip: two waves per workgroup

template <int NJ>
struct HostPark {  // the device parks chain 0's factor in LDS; the host keeps a copy
    mutable ikdev::LegFactor<NJ> saved;
    void store(const ikdev::LegFactor<NJ> &F) const { saved = F; }
    void load(ikdev::LegFactor<NJ> &F) const {
        for (int e = 0; e < NJ * (NJ + 1) / 2; ++e) F.L[e] = saved.L[e];
        for (int j = 0; j < NJ; ++j) {
            for (int c = 0; c < 6; ++c) F.W[j][c] = saved.W[j][c];
            F.u[j] = saved.u[j];
        }
    }
};

struct IO {
    int64_t B;
    const double *q0, *targets;
    const ikgpu_dls_params *prm;
    double pik_lambda1;
    double *q_out;
    uint8_t *success;
    int32_t *iters;
    int layout;
};

template <int NJ, int NCH>
void run_tree(const ikgpu::ProblemHost &ph, const ikgpu::TreeBuild &build, const IO &io) {
    ikdev::TreeKernelArgs<NJ, NCH> a{};
    ikdev::TreeDesc<NJ, NCH> d{};
    const std::vector<double> t = ikgpu::tree_desc_table(ph);
    if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("tree desc table size mismatch");
    std::memcpy(&d, t.data(), sizeof d);
    const ikgpu::TreeArgsHost h = ikgpu::tree_args(ph);
    for (int c = 0; c < NCH; ++c)
        for (int j = 0; j < NJ; ++j) { a.qidx[c][j] = h.qidx[c][j]; a.vidx[c][j] = h.vidx[c][j]; }
    for (int s = 0; s < 3; ++s) { a.tslot[s] = h.tslot[s]; a.trow[s] = h.trow[s]; a.tdim[s] = h.tdim[s]; a.trow0[s] = h.trow0[s]; }
    a.prm.prio[0] = h.prio[0]; a.prm.prio[1] = h.prio[1]; a.prm.prioP = h.prio[2]; a.prm.hasP = h.hasP;
    a.prm.idmask[0] = h.idmask[0]; a.prm.idmask[1] = h.idmask[1]; a.prm.idmaskP = h.idmaskP;
    a.prm.unit[0] = h.unit[0]; a.prm.unit[1] = h.unit[1]; a.prm.unitP = h.unit[2];
    a.prm.ref_base[0] = h.ref_base[0]; a.prm.ref_base[1] = h.ref_base[1];
    a.prm.align_chain = h.align_chain; a.prm.align_axis = h.align_axis; a.prm.align_slot = h.align_slot;
    a.prm.align_prio = h.align_prio; a.prm.align_w = h.align_w;
    a.prm.fixed_base = h.fixed_base;
    a.prm.cons_on = h.cons_on; a.prm.cons_type = h.cons_type;
    a.prm.post_on = h.post_on; a.prm.post_prio = h.post_prio; a.prm.post_n = h.post_n;
    for (int k = 0; k < h.post_n; ++k) {
        a.prm.post_q[k] = h.post_q[k]; a.prm.post_slot[k] = h.post_slot[k]; a.prm.post_w[k] = h.post_w[k]; a.prm.post_m[k] = h.post_m[k];
    }
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j < 8; ++j) { a.prm.postc_slot[c][j] = h.postc_slot[c][j]; a.prm.postc_w[c][j] = h.postc_w[c][j]; a.prm.postc_m[c][j] = h.postc_m[c][j]; }
    a.nq = ph.nq; a.nv = ph.nv; a.ntasks = ph.ntasks;
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_out; a.success = io.success; a.iters = io.iters;
    a.prm.max_iterations = io.prm->max_iterations;
    a.prm.lam2 = io.prm->damping * io.prm->damping;
    a.prm.step_length = io.prm->step_length;
    a.prm.stop_sq_tol = io.prm->stop_sq_tol;
    if (build.extras == ikgpu::TreeBuild::kPik) { a.prm.pik_on = 1; a.prm.pik_lam2_1 = io.pik_lambda1 * io.pik_lambda1; }
    // the lane's own column for the outside joints, their targets and the chain's posture targets, one row after another (the device
    // keeps [row][lane] in LDS: dynamic LDS in the one-chain posture build, the idle park buffer in the posture + constraint build
    // while 2 post_n + NJ rows fit it, else the lane's column of q_out)
    std::vector<double> column(static_cast<size_t>(2 * ikdev::kMaxPostOut + NJ), 0.0);
    const bool built = ikgpu::with_tree_spec<NJ, NCH>(build, [&](auto spec) {
        constexpr int SPEC = decltype(spec)::value;
        constexpr bool kPostCons = SPEC > 0 && NCH > 1 && (SPEC & ikdev::kSpecPostCons) == ikdev::kSpecPostCons;
        constexpr bool kRows = SPEC >= 0 && (kPostCons || (ikdev::spec_is_general(SPEC) && (SPEC & (1 << ikdev::kSpecGen)) == 0));
        double *post_lane = (SPEC > 0 && ikdev::spec_has_posture(SPEC) && NCH == 1) ? column.data() : nullptr;
        if (kPostCons && a.prm.cons_on && 2 * a.prm.post_n + NJ <= NJ * (NJ + 1) / 2 + NJ * 6 + NJ) post_lane = column.data();
        for (int64_t b = 0; b < io.B; ++b)
            ikdev::dls_tree_body<NJ, NCH, SPEC>(a, d, b, HostPark<NJ>{}, [](bool act) { return act; }, post_lane, int64_t{1},
                                                kRows ? b / kTreeBlock * kTreeBlock : int64_t{-1});
    });
    if (!built) throw std::runtime_error("the shape has no such build");
}

}  // namespace

extern "C" {

const char *tree_emu_last_error(void) { return g_err.c_str(); }

// Host pointers, same layouts as include/ikgpu.h.  tasks in stacking order.  pik_lambda1 > 0: level 1 of a two-level ik::pik rides on
// the solve (prm->damping is lambda_0).  build_out: the selection's name (problem.hpp tree_build_name) of the build that ran.
int tree_emu_run(const char *urdf, size_t len, int free_flyer, const ikgpu_task *tasks, int ntasks, const ikgpu_task *cons, int ncons,
                 int64_t B, const double *q0, const double *targets, const ikgpu_dls_params *prm, double pik_lambda1, double *q_out,
                 uint8_t *success, int32_t *iters, int layout, char *build_out, size_t cap) {
    try {
        const ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, free_flyer != 0);
        const ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, tasks, ntasks, false, cons, ncons);
        if (ph.kind != ikgpu::KernelKind::Tree) { g_err = "the problem did not map onto the tree kernel: " + ph.kernel_name; return 1; }
        const ikgpu::TreeBuild build = ikgpu::select_tree_build(ph, *prm, pik_lambda1 > 0.0);
        if (!build.launchable) { g_err = "no launchable build: " + ph.kernel_name; return 1; }
        if (build_out && cap) {
            std::strncpy(build_out, ikgpu::tree_build_name(build).c_str(), cap - 1);
            build_out[cap - 1] = '\0';
        }
        const IO io{B, q0, targets, prm, pik_lambda1, q_out, success, iters, layout};
        const int nj = ph.chain.nj, nch = ph.chainB.nj > 0 ? 2 : 1;
        if (nj == 7 && nch == 2) { run_tree<7, 2>(ph, build, io); return 0; }
        if (nj == 7 && nch == 1) { run_tree<7, 1>(ph, build, io); return 0; }
        if (nj == 6 && nch == 2) { run_tree<6, 2>(ph, build, io); return 0; }
        if (nj == 6 && nch == 1) { run_tree<6, 1>(ph, build, io); return 0; }
        g_err = "tree shape without a compiled kernel: " + ph.kernel_name;
        return 1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"
