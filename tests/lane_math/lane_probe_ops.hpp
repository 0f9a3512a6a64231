// lane_probe_ops.hpp -- one wrapper per lane primitive of ik_amd/csrc/device/{lane_math,line,tree_solver,chain_hot}.hpp, for the
// probe that runs ONE of them per launch (tests/lane_math/lane_probe.hip on the device, under each of the product's three
// translation-unit recipes; tests/lane_math/lane_probe_host.cpp under g++).  A wrapper takes one lane's inputs as doubles and writes
// one lane's outputs as doubles.  The table below -- name, inputs, outputs -- is the only list of the operations: the device
// program, the host shim and the Python side (through `--list`) all read it.
#pragma once
#include "device/lane_math.hpp"
#include "device/line.hpp"
#include "device/tree_solver.hpp"   // quat_to_R, freeflyer_integrate; brings device/chain_hot.hpp (hot_sincos and the LDS table)

namespace lane_probe {
using namespace ikdev;

// ---- scalars -----------------------------------------------------------------------------------------------------------------
IKD_FN void op_drcp(const double *a, double *o) { o[0] = drcp(a[0]); }
IKD_FN void op_drsqrt(const double *a, double *o) { o[0] = drsqrt(a[0]); }
IKD_FN void op_dsqrt(const double *a, double *o) { o[0] = dsqrt(a[0]); }
IKD_FN void op_dacos(const double *a, double *o) { o[0] = dacos(a[0]); }
// dfma3 (inline assembly on the device) and the builtin on the same operands
IKD_FN void op_dfma3(const double *a, double *o) {
    o[0] = dfma3(a[0], a[1], a[2]);
    o[1] = __builtin_fma(a[0], a[1], a[2]);
}
IKD_FN void op_dsincos(const double *a, double *o) { dsincos(a[0], o[0], o[1]); }
IKD_FN void op_dsincos_fast(const double *a, double *o) { dsincos_fast(a[0], o[0], o[1]); }
IKD_FN void op_dsincos_bounded2(const double *a, double *o) { dsincos_bounded<2>(a[0], o[0], o[1]); }
IKD_FN void op_dsincos_bounded3(const double *a, double *o) { dsincos_bounded<3>(a[0], o[0], o[1]); }
IKD_FN void op_dsincos_hot(const double *a, double *o) { dsincos_hot(a[0], o[0], o[1]); }

// ---- the table routine as the hot kernels reach it: hot_sincos<NJ> on the caller's table object (LDS on the device) -------------
// outputs: s[NJ], c[NJ], residual[NJ], index[NJ] (as a double)
template <int NJ, class Tab>
IKD_FN void op_sincos_lut(const Tab &t, const double *a, double *o) {
    double phi[NJ], sn[NJ], cs[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) phi[j] = a[j];
    hot_sincos<NJ>(t, phi, sn, cs);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        double r;
        int idx;
        dsincos_lut_reduce(phi[j], r, idx);
        o[j] = sn[j];
        o[NJ + j] = cs[j];
        o[2 * NJ + j] = r;
        o[3 * NJ + j] = static_cast<double>(idx);
    }
}

// ---- log6 / Jlog6: in Re[9] pe[3]; out e[6] A[9] and Bm[9] or C[9] -------------------------------------------------------------
IKD_FN void log6_pack(const LogAndJlog &lj, const double *third, double *o) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = lj.e[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o[6 + k] = lj.A[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o[15 + k] = third[k];
}
IKD_FN void log6_unpack(const double *a, double (&Re)[9], double (&pe)[3]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Re[k] = a[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pe[k] = a[9 + k];
}
IKD_FN void op_log6_inv(const double *a, double *o) {
    double Re[9], pe[3];
    log6_unpack(a, Re, pe);
    LogAndJlog lj;
    log6_and_jlog6_inv(Re, pe, lj);
    log6_pack(lj, lj.Bm, o);
}
template <bool WITH_BM, bool LEAN>
IKD_FN void log6_hot_any(const double *a, double *o) {
    double Re[9], pe[3], Cm[9];
    log6_unpack(a, Re, pe);
    LogAndJlog lj;
    log6_and_jlog6_hot<WITH_BM, LEAN>(Re, pe, lj, &Cm);
    log6_pack(lj, WITH_BM ? lj.Bm : Cm, o);
}
IKD_FN void op_log6_hot_bm(const double *a, double *o) { log6_hot_any<true, false>(a, o); }
IKD_FN void op_log6_hot_c(const double *a, double *o) { log6_hot_any<false, false>(a, o); }        // the tree program
IKD_FN void op_log6_hot_lean_c(const double *a, double *o) { log6_hot_any<false, true>(a, o); }    // the hot chain program
IKD_FN void op_log6_hot_lean_bm(const double *a, double *o) { log6_hot_any<true, true>(a, o); }

// ---- solves: in G[M*M] (row-major, symmetric) b[M]; out x[M] -------------------------------------------------------------------
template <int M, bool LDLT>
IKD_FN void solve_any(const double *a, double *o) {
    double G[M * M], b[M], x[M];
#pragma unroll
    for (int k = 0; k < M * M; ++k) G[k] = a[k];
#pragma unroll
    for (int k = 0; k < M; ++k) b[k] = a[M * M + k];
    if (LDLT) ldlt_solve<M>(G, b, x);
    else chol_solve<M>(G, b, x);
#pragma unroll
    for (int k = 0; k < M; ++k) o[k] = x[k];
}
IKD_FN void op_ldlt_solve3(const double *a, double *o) { solve_any<3, true>(a, o); }
IKD_FN void op_ldlt_solve6(const double *a, double *o) { solve_any<6, true>(a, o); }
IKD_FN void op_chol_solve6(const double *a, double *o) { solve_any<6, false>(a, o); }

// ---- device/line.hpp -----------------------------------------------------------------------------------------------------------
IKD_FN void op_log3(const double *a, double *o) {
    double R[9], w[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a[k];
    log3(R, w);
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}
IKD_FN void op_exp3(const double *a, double *o) {
    double w[3] = {a[0], a[1], a[2]}, R[9];
    exp3(w, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
}
// in from[12] goal[12]; out w[3] then waypoints k = 0 .. T-1, twelve values each
template <int T>
IKD_FN void line_any(const double *a, double *o) {
    double from[12], goal[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { from[k] = a[k]; goal[k] = a[12 + k]; }
    LineStart ls;
    line_start_from_pose(from, goal, ls);
    o[0] = ls.w[0]; o[1] = ls.w[1]; o[2] = ls.w[2];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        double t[12];
        line_waypoint(ls, goal, k, T, t);
#pragma unroll
        for (int m = 0; m < 12; ++m) o[3 + 12 * k + m] = t[m];
    }
}
IKD_FN void op_line_t1(const double *a, double *o) { line_any<1>(a, o); }
IKD_FN void op_line_t3(const double *a, double *o) { line_any<3>(a, o); }
IKD_FN void op_line_t8(const double *a, double *o) { line_any<8>(a, o); }

// ---- device/tree_solver.hpp ----------------------------------------------------------------------------------------------------
IKD_FN void op_quat_to_R(const double *a, double *o) {
    double qb[7], R[9];
#pragma unroll
    for (int k = 0; k < 7; ++k) qb[k] = a[k];
    quat_to_R(qb, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
}
// in qb[7] v[6]; R1 = quat_to_R(qb) as every caller forms it; out the new qb[7]
IKD_FN void op_freeflyer_integrate(const double *a, double *o) {
    double qb[7], v[6], R1[9], out[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) qb[k] = a[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = a[7 + k];
    quat_to_R(qb, R1);
    freeflyer_integrate(qb, R1, v, out);
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = out[k];
}

}  // namespace lane_probe

// X(name, n_in, n_out): a plain wrapper op_<name>(in, out)
#define LANE_PROBE_OPS(X)          \
    X(drcp, 1, 1)                  \
    X(drsqrt, 1, 1)                \
    X(dsqrt, 1, 1)                 \
    X(dacos, 1, 1)                 \
    X(dfma3, 3, 2)                 \
    X(dsincos, 1, 2)               \
    X(dsincos_fast, 1, 2)          \
    X(dsincos_bounded2, 1, 2)      \
    X(dsincos_bounded3, 1, 2)      \
    X(dsincos_hot, 1, 2)           \
    X(log6_inv, 12, 24)            \
    X(log6_hot_bm, 12, 24)         \
    X(log6_hot_c, 12, 24)          \
    X(log6_hot_lean_c, 12, 24)     \
    X(log6_hot_lean_bm, 12, 24)    \
    X(ldlt_solve3, 12, 3)          \
    X(ldlt_solve6, 42, 6)          \
    X(chol_solve6, 42, 6)          \
    X(log3, 9, 3)                  \
    X(exp3, 3, 9)                  \
    X(line_t1, 24, 15)             \
    X(line_t3, 24, 39)             \
    X(line_t8, 24, 99)             \
    X(quat_to_R, 7, 9)             \
    X(freeflyer_integrate, 13, 7)
// X(name, NJ): op_sincos_lut<NJ> on the caller's table; NJ inputs, 4 NJ outputs
#define LANE_PROBE_LUT_OPS(X) \
    X(dsincos_lut1, 1)        \
    X(dsincos_lut7, 7)

namespace lane_probe {
struct OpInfo {
    const char *name;
    int n_in, n_out;
};
#define LANE_PROBE_ROW(name, ni, no) {#name, ni, no},
#define LANE_PROBE_LUT_ROW(name, nj) {#name, nj, 4 * nj},
static const OpInfo kOps[] = {LANE_PROBE_OPS(LANE_PROBE_ROW) LANE_PROBE_LUT_OPS(LANE_PROBE_LUT_ROW)};
#undef LANE_PROBE_ROW
#undef LANE_PROBE_LUT_ROW
constexpr int kNumOps = static_cast<int>(sizeof(kOps) / sizeof(kOps[0]));
}  // namespace lane_probe
