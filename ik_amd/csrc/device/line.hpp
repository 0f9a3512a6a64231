// line.hpp -- the waypoints of a straight Cartesian line (include/ikgpu.h ikgpu_line_targets, ikgpu_dls_line_batch): the start pose of
// a task frame in its reference frame, the rotation logarithm and exponential, and waypoint k of T between the start and the goal --
// and of a path through via poses (ikgpu_path_targets, ikgpu_dls_path_batch): the start of a later segment from the previous via, the
// path kernels' arguments and the joint-step test.
//
// ONE source of this arithmetic: the kernels behind ikgpu_line_targets (kernels.hip) and the fused line bodies (dls_chain_line_body in
// chain_kernel_body.hpp, hot_line_body in chain_hot.hpp) call the functions below and nothing else, which is what makes the fused launch
// return the bits of ikgpu_dls_track_batch on ikgpu_line_targets -- as multistart_draw (multistart.hpp) does for the generated starts.
// Written with explicit dfma and no additions of a literal zero, so that the translation units that fold signed zeros (kernels_hot.hip,
// the run-time compiled hot build) compute the same bits as kernels.hip.
#pragma once
#include "lane_math.hpp"

namespace ikdev {

// What the line kernels take after the solve's arguments.
struct LineArgs {
    int32_t *reached;   // [B] or null: waypoints met before the first failure (T: the goal was reached)
    int T;              // waypoints, >= 1
};

// w = log3(R), |w| = theta in [0, pi]: the rotation part of log6_and_jlog6_inv (lane_math.hpp; formulas SURVEY.md App. A.3), the
// same scalars in the same order.  Near theta = pi the axis is ill-conditioned (the alternative formula recovers it from the
// diagonal): callers split such moves.
IKD_FN void log3(const double (&R)[9], double (&w)[3]) {
    const double tr = R[0] + R[4] + R[8];
    double x = (tr - 1.0) * 0.5;
    x = dmin(1.0, dmax(-1.0, x));  // tr >= 3 -> theta = 0 ; tr <= -1 -> theta = pi
    const double theta = dacos(x);
    const double omc = 1.0 - x;
    const double st = dsqrt(dmax(0.0, omc * (1.0 + x)));   // sin(theta), theta in [0, pi]
    const double fac = 0.5 * dsel(theta > kTaylorPrec3, theta * drcp(st), 1.0);
    w[0] = fac * (R[7] - R[5]);
    w[1] = fac * (R[2] - R[6]);
    w[2] = fac * (R[3] - R[1]);
    const bool near_pi = theta >= kPi - 1e-2;
    if (IKD_NEAR_PI_GATE(near_pi)) {
        const double cphi = -x;
        const double beta_pi = theta * theta * drcp(1.0 + cphi);
        const double t0 = (R[0] + cphi) * beta_pi, t1 = (R[4] + cphi) * beta_pi, t2 = (R[8] + cphi) * beta_pi;
        const double a0 = dsel(R[7] > R[5], 1.0, -1.0) * dsel(t0 > 0.0, dsqrt(dmax(t0, 0.0)), 0.0);
        const double a1 = dsel(R[2] > R[6], 1.0, -1.0) * dsel(t1 > 0.0, dsqrt(dmax(t1, 0.0)), 0.0);
        const double a2 = dsel(R[3] > R[1], 1.0, -1.0) * dsel(t2 > 0.0, dsqrt(dmax(t2, 0.0)), 0.0);
        w[0] = dsel(near_pi, a0, w[0]);
        w[1] = dsel(near_pi, a1, w[1]);
        w[2] = dsel(near_pi, a2, w[2]);
    }
}

// R = exp3(w) (Rodrigues): (1 - cos t)/t^2 w w^T + sin t / t skew(w) + cos t I, Taylor forms below t = eps^(1/4).
IKD_FN void exp3(const double (&w)[3], double (&R)[9]) {
    const double t2 = dot(w, w);
    const double t = dsqrt(t2);
    const bool small = t < kTaylorPrec3;
    double s, c;
    dsincos(t, s, c);
    const double inv_t = drcp(dmax(t, 0x1p-200));   // (the floor keeps the discarded arms finite at t = 0, as log6_and_jlog6_hot's)
    const double a_wxv = dsel(small, dfma(t2, -1.0 / 24.0, 0.5), (1.0 - c) * (inv_t * inv_t));
    const double a_v = dsel(small, dfma(t2, -1.0 / 6.0, 1.0), s * inv_t);
    const double diag = dsel(small, dfma(t2, -0.5, 1.0), c);
    const double u[3] = {a_wxv * w[0], a_wxv * w[1], a_wxv * w[2]};
    const double v[3] = {a_v * w[0], a_v * w[1], a_v * w[2]};
    R[0] = dfma(u[0], w[0], diag);
    R[4] = dfma(u[1], w[1], diag);
    R[8] = dfma(u[2], w[2], diag);
    R[1] = dfma(u[0], w[1], -v[2]);
    R[3] = dfma(u[1], w[0], v[2]);
    R[2] = dfma(u[0], w[2], v[1]);
    R[6] = dfma(u[2], w[0], -v[1]);
    R[5] = dfma(u[1], w[2], -v[0]);
    R[7] = dfma(u[2], w[1], v[0]);
}

// World placement of a chain's task frame at q: the arithmetic of the stage kernel (chain_kernel_body.hpp fk_chain_body: dsincos, the
// run-time placement mask), on the lane's own copy of the chain entries.  KINDS: read the joint-kind mask (chain_solver.hpp kKindShift).
template <int NJ, bool KINDS = false, class Desc>
IKD_FN void line_chain_fk(const Desc &d, int idmask, const double (&q)[NJ], double (&R)[9], double (&p)[3]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = d.pl[0][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = d.pl[0][9 + k];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j > 0) se3_compose_const(R, p, d.pl[j], ((idmask >> j) & 1) != 0);
        bool slides = false;
        if constexpr (KINDS) slides = ((idmask >> (16 + j)) & 1) != 0;
        if (slides) {
            p[0] = dfma(q[j], R[2], p[0]);
            p[1] = dfma(q[j], R[5], p[1]);
            p[2] = dfma(q[j], R[8], p[2]);
        } else {
            double s, c;
            dsincos(q[j], s, c);
            rot_z_right(R, s, c);
        }
    }
    se3_compose_const(R, p, d.frame_pl, ((idmask >> NJ) & 1) != 0);
}

// A line from M0 = (R0, p0) = oMr^-1 oMf(q0) -- the pose of the task frame in its reference frame at the start -- to the goal
// M1 = (R1, p1): what a lane keeps between waypoints.  w = log3(R0^T R1).
struct LineStart {
    double R0[9], p0[3], w[3];
};

// ref: world placement oMr of the reference frame (12 values, rotation row-major then translation); (Rf, pf) = oMf(q0); goal: M1.
template <class RefPtr>
IKD_FN void line_start(RefPtr ref, const double (&Rf)[9], const double (&pf)[3], const double (&goal)[12], LineStart &s) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s.R0[3 * i + j] = dfma(ref[i], Rf[j], dfma(ref[3 + i], Rf[3 + j], ref[6 + i] * Rf[6 + j]));
    const double dp[3] = {pf[0] - ref[9], pf[1] - ref[10], pf[2] - ref[11]};
#pragma unroll
    for (int i = 0; i < 3; ++i) s.p0[i] = dfma(ref[i], dp[0], dfma(ref[3 + i], dp[1], ref[6 + i] * dp[2]));
    double Rrel[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rrel[3 * i + j] = dfma(s.R0[i], goal[j], dfma(s.R0[3 + i], goal[3 + j], s.R0[6 + i] * goal[6 + j]));
    log3(Rrel, s.w);
}

// The start of a segment from a GIVEN pose -- segment s >= 1 of a path (include/ikgpu.h ikgpu_path_targets) starts at via s - 1's own
// twelve values: (R0, p0) = from, w = log3(R0^T R1), the last product of line_start in the same expressions.  The one source for the
// kernels behind ikgpu_path_targets and the fused path bodies (dls_chain_path_body, hot_path_body).
IKD_FN void line_start_from_pose(const double (&from)[12], const double (&goal)[12], LineStart &s) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s.R0[k] = from[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) s.p0[i] = from[9 + i];
    double Rrel[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rrel[3 * i + j] = dfma(s.R0[i], goal[j], dfma(s.R0[3 + i], goal[3 + j], s.R0[6 + i] * goal[6 + j]));
    log3(Rrel, s.w);
}

// What the path kernels take after the solve's arguments (include/ikgpu.h ikgpu_dls_path_batch): P segments of T waypoints each.
struct PathArgs {
    int32_t *reached;        // [B] or null: waypoints met before the first one that was not (P * T: the whole path)
    int T, P;                // waypoints per segment >= 1, segments >= 1
    double max_joint_step;   // 0: no joint-step rule; else a waypoint is met only when no chain entry moved by more than this
};

// "Some entry of the support moved by more than max_step between the start of the solve and its result": one subtraction, fabs and a
// compare per entry, on plain entries (no distance modulo 2 pi), as solutions_near (solutions.hpp).  max_step == 0: the rule is off.
template <int NJ>
IKD_FN bool path_jumped(const double (&q)[NJ], const double (&q_prev)[NJ], double max_step) {
    bool jumped = false;
#pragma unroll
    for (int i = 0; i < NJ; ++i) jumped = jumped || __builtin_fabs(q[i] - q_prev[i]) > max_step;
    return jumped && max_step != 0.0;
}

// Waypoint k of T (0 <= k < T), s = (k + 1) / T: R = R0 exp3(s w), p = p0 + s (p1 - p0) -- a straight line of the frame origin at
// constant angular velocity; waypoint T - 1 is the goal's own twelve values.
IKD_FN void line_waypoint(const LineStart &ls, const double (&goal)[12], int k, int T, double (&t)[12]) {
    const double s = static_cast<double>(k + 1) / static_cast<double>(T);
    const double sw[3] = {s * ls.w[0], s * ls.w[1], s * ls.w[2]};
    double E[9];
    exp3(sw, E);
    const bool last = k + 1 >= T;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double r = dfma(ls.R0[3 * i], E[j], dfma(ls.R0[3 * i + 1], E[3 + j], ls.R0[3 * i + 2] * E[6 + j]));
            t[3 * i + j] = last ? goal[3 * i + j] : r;
        }
        const double p = dfma(s, goal[9 + i] - ls.p0[i], ls.p0[i]);
        t[9 + i] = last ? goal[9 + i] : p;
    }
}

}  // namespace ikdev
