// pass_plan_shim.cpp -- TEST HARNESS ONLY.  The plan of the entries of q outside the chain (ik_amd/csrc/device/chain_kernel_body.hpp
// PassPlan) on the CPU: what the host builder makes of a problem (problem.cpp fill_pass_plan), and the bodies that read it --
// hot_pass_through_from, chain_pass_through_into, the general dls_chain_body and the hot program's hot_chain_body -- run lane after lane
// with and without it on the same inputs.  Compiled by tests/test_pass_plan_host.py with g++ into its own shared object; libikgpu.so
// neither contains nor calls it.  With -DPASS_PLAN_SHIM_MAIN it is a stand-alone program (for the host sanitizers): it reads nothing and
// runs every body on a model of its own, with and without the plan, and compares the bits.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "device/chain_hot.hpp"
#include "device/chain_kernel_body.hpp"
#include "ikgpu.h"
#include "model.hpp"
#include "problem.hpp"

namespace {

thread_local std::string g_err;

enum Body { kHotFrom = 0, kGeneralInto = 1, kGeneralSolve = 2, kHotSolve = 3 };

struct IO {
    int body, with_plan, layout;
    int64_t B;
    const double *q0, *targets;
    int max_iterations;
    double stop_sq_tol;
    const uint8_t *stepped;   // [B], bodies kHotFrom / kGeneralInto
    double *q_out;
    uint8_t *success;
    int32_t *iters;
};

template <int NJ>
ikdev::ChainKernelArgs<NJ> make_args(const ikgpu::ProblemHost &ph, const IO &io) {
    ikdev::ChainKernelArgs<NJ> a{};
    ikgpu::fill_chain_args(ph, a.ref_pl, a.qidx, a.vidx, &a.nq, &a.nv, &a.prm.priority, &a.prm.idmask, &a.prm.unit_weights);
    a.lower = ph.lower.data(); a.upper = ph.upper.data(); a.q_in_chain = ph.q_in_chain.data();
    if (io.with_plan) a.pass.state = ikgpu::fill_pass_plan(ph, ikdev::kPassPlanMax, a.pass.idx, a.pass.lo, a.pass.hi);
    a.layout = io.layout; a.B = io.B; a.q0 = io.q0; a.targets = io.targets;
    a.q_out = io.q_out; a.success = io.success; a.iters = io.iters;
    a.prm.max_iterations = io.max_iterations; a.prm.lam2 = 1e-4; a.prm.step_length = 1.0; a.prm.stop_sq_tol = io.stop_sq_tol;
    return a;
}

template <int NJ>
void run_plain(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainKernelArgs<NJ> a = make_args<NJ>(ph, io);
    if (io.body == kGeneralSolve) {
        ikdev::ChainDesc<NJ> d{};
        const std::vector<double> t = ikgpu::chain_desc_table(ph);
        if (t.size() * sizeof(double) != sizeof d) throw std::runtime_error("chain desc table size mismatch");
        std::memcpy(&d, t.data(), sizeof d);
        for (int64_t b = 0; b < io.B; ++b) ikdev::dls_chain_body<NJ, 2>(a, d, b, [](bool act) { return act; });
        return;
    }
    for (int64_t b = 0; b < io.B; ++b) {
        if (io.body == kHotFrom) ikdev::hot_pass_through_from(a, a.q0, a.q_out, b, io.stepped[b] != 0);
        else ikdev::chain_pass_through_into(a, a.q0, a.q_out, b, io.stepped[b] != 0);
    }
}

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
void run_hot(const ikgpu::ProblemHost &ph, const IO &io) {
    const ikdev::ChainKernelArgs<NJ> a = make_args<NJ>(ph, io);
    ikdev::HotTable t{};
    const std::vector<double> tab = ikgpu::chain_hot_table(ph.chain);
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) throw std::runtime_error("compact table too long");
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
    typedef ikdev::ChainStruct<C0, C1, C2> S;
    for (int64_t b = 0; b < io.B; ++b) {
        if (io.stop_sq_tol < 0.0) ikdev::hot_chain_body<NJ, S, true>(a, t, b, [](bool act) { return act; });
        else ikdev::hot_chain_body<NJ, S, false>(a, t, b, [](bool act) { return act; });
    }
}

ikgpu::ProblemHost analyse(const char *urdf, size_t len, const ikgpu_task *task) {
    ikgpu::Model m = ikgpu::Model::from_urdf(urdf, len, false);
    ikgpu::ProblemHost ph = ikgpu::analyse_problem(m, task, 1, false);
    if (ph.kind != ikgpu::KernelKind::Chain || ph.tasks[0].type != IKGPU_FULL) throw std::runtime_error("not a chain problem with one Full task");
    return ph;
}

void run(const ikgpu::ProblemHost &ph, const IO &io) {
    if (io.body == kHotSolve) {
        const ikgpu::ChainStructure s = ikgpu::chain_structure(ph.chain);
#define X(N, K0, K1, K2)                                                                                \
    if (s.fits && ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) {         \
        run_hot<N, K0, K1, K2>(ph, io);                                                                 \
        return;                                                                                         \
    }
        X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull)   // Cassie leg
        X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull)   // UR5 / UR10
#undef X
        throw std::runtime_error("structure code not instantiated in the shim");
    }
#define X(N) \
    if (ph.chain.nj == N) { run_plain<N>(ph, io); return; }
    X(3) X(6) X(7)
#undef X
    throw std::runtime_error("chain length not instantiated in the shim");
}

}  // namespace

extern "C" {

const char *pass_plan_last_error(void) { return g_err.c_str(); }
int pass_plan_max(void) { return ikdev::kPassPlanMax; }

// The plan fill_pass_plan makes of the problem (under the caller's environment), and what it was made from.  idx / lo / hi:
// [pass_plan_max()], in_chain / lower / upper: [nq] (at most 64).
int pass_plan_build(const char *urdf, size_t len, const ikgpu_task *task, int *state, int *idx, double *lo, double *hi, uint8_t *in_chain,
                    double *lower, double *upper, int *nq, int *nj) {
    try {
        const ikgpu::ProblemHost ph = analyse(urdf, len, task);
        if (ph.nq > 64) throw std::runtime_error("more than 64 entries of q");
        ikdev::PassPlan p{};
        p.state = ikgpu::fill_pass_plan(ph, ikdev::kPassPlanMax, p.idx, p.lo, p.hi);
        *state = p.state;
        for (int k = 0; k < ikdev::kPassPlanMax; ++k) { idx[k] = p.idx[k]; lo[k] = p.lo[k]; hi[k] = p.hi[k]; }
        for (int i = 0; i < ph.nq; ++i) { in_chain[i] = ph.q_in_chain[i]; lower[i] = ph.lower[i]; upper[i] = ph.upper[i]; }
        *nq = ph.nq;
        *nj = ph.chain.nj;
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

// One body over B problems.  body: 0 hot_pass_through_from, 1 chain_pass_through_into (both: stepped[b] per problem, q_out's chain entries
// are left alone), 2 dls_chain_body (general program), 3 hot_chain_body (never-stop when stop_sq_tol < 0).  q0 / q_out: nq x B in
// `layout` (0 SoA, 1 AoS), targets 12 x B likewise.
int pass_plan_run(const char *urdf, size_t len, const ikgpu_task *task, int body, int with_plan, int layout, int64_t B, const double *q0,
                  const double *targets, int max_iterations, double stop_sq_tol, const uint8_t *stepped, double *q_out, uint8_t *success,
                  int32_t *iters) {
    try {
        const ikgpu::ProblemHost ph = analyse(urdf, len, task);
        run(ph, IO{body, with_plan, layout, B, q0, targets, max_iterations, stop_sq_tol, stepped, q_out, success, iters});
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return 1;
    }
}

}  // extern "C"

#ifdef PASS_PLAN_SHIM_MAIN
// A fixed base, a chain of three joints to `tool` and a side branch of n_side joints that the chain does not take.
static std::string side_branch_urdf(int n_side) {
    std::string o = "<?xml version=\"1.0\"?>\n<robot name=\"side\">\n  <link name=\"base\"/>\n  <link name=\"tool\"/>\n";
    char line[512];
    for (int j = 1; j <= 3; ++j) { std::snprintf(line, sizeof line, "  <link name=\"l%d\"/>\n", j); o += line; }
    for (int j = 1; j <= n_side; ++j) { std::snprintf(line, sizeof line, "  <link name=\"s%d\"/>\n", j); o += line; }
    for (int j = 1; j <= 3; ++j) {
        std::snprintf(line, sizeof line,
                      "  <joint name=\"j%d\" type=\"revolute\"><origin rpy=\"0.3 -0.4 0.2\" xyz=\"0.05 -0.02 0.2\"/><axis xyz=\"0 0 1\"/>"
                      "<parent link=\"%s\"/><child link=\"l%d\"/><limit lower=\"-2.5\" upper=\"2.5\"/></joint>\n",
                      j, j == 1 ? "base" : ("l" + std::to_string(j - 1)).c_str(), j);
        o += line;
    }
    for (int j = 1; j <= n_side; ++j) {
        std::snprintf(line, sizeof line,
                      "  <joint name=\"sj%d\" type=\"revolute\"><origin rpy=\"0 0 0\" xyz=\"0.1 0 0\"/><axis xyz=\"0 0 1\"/>"
                      "<parent link=\"%s\"/><child link=\"s%d\"/><limit lower=\"%g\" upper=\"%g\"/></joint>\n",
                      j, j == 1 ? "base" : ("s" + std::to_string(j - 1)).c_str(), j, -0.1 * j, 0.05 * j);
        o += line;
    }
    o += "  <joint name=\"tool_joint\" type=\"fixed\"><origin rpy=\"0.2 -0.1 0.3\" xyz=\"0.03 0.02 0.14\"/><parent link=\"l3\"/><child link=\"tool\"/></joint>\n</robot>\n";
    return o;
}

int main() {
    int bad = 0;
    for (int n_side : {0, 5, 16, 17}) {
        const std::string urdf = side_branch_urdf(n_side);
        const ikgpu::Model m = ikgpu::Model::from_urdf(urdf.data(), urdf.size(), false);
        ikgpu_task task{};
        task.frame = m.frame_id("tool");
        task.type = IKGPU_FULL;
        for (double &w : task.weight) w = 1.0;
        const int nq = 3 + n_side;
        const int64_t B = 67;
        std::vector<double> q0(static_cast<size_t>(nq * B)), tg(static_cast<size_t>(12 * B), 0.0);
        std::vector<uint8_t> stepped(static_cast<size_t>(B));
        for (int64_t b = 0; b < B; ++b) {
            stepped[b] = b % 3 != 0;
            for (int i = 0; i < nq; ++i) q0[b * nq + i] = 0.37 * ((b * 31 + i * 17) % 23 - 11);   // partly outside the limits
            const double id[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0.05, 0.4};
            std::memcpy(&tg[12 * b], id, sizeof id);
        }
        for (int body : {0, 1, 2}) {
            std::vector<double> out[2];
            std::vector<uint8_t> ok[2];
            std::vector<int32_t> it[2];
            for (int plan = 0; plan < 2; ++plan) {
                out[plan].assign(q0.size(), -7.0);
                ok[plan].assign(static_cast<size_t>(B), 9);
                it[plan].assign(static_cast<size_t>(B), -9);
                if (pass_plan_run(urdf.data(), urdf.size(), &task, body, plan, 1, B, q0.data(), tg.data(), 2, 1e-3, stepped.data(), out[plan].data(),
                                  ok[plan].data(), it[plan].data())) {
                    std::fprintf(stderr, "n_side %d body %d plan %d: %s\n", n_side, body, plan, pass_plan_last_error());
                    return 2;
                }
            }
            const bool same = std::memcmp(out[0].data(), out[1].data(), out[0].size() * sizeof(double)) == 0 && ok[0] == ok[1] && it[0] == it[1];
            std::printf("side branch of %2d, body %d: %s\n", n_side, body, same ? "equal bits" : "DIFFERENT");
            bad += same ? 0 : 1;
        }
    }
    return bad ? 1 : 0;
}
#endif
