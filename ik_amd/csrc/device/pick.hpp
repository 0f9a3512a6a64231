// pick.hpp -- what the pick solve (include/ikgpu.h ikgpu_dls_pick_batch) shares between its kernels, the loop that stands in for them and
// the CPU lane emulator under tests/: the arguments, the four costs a converged start is ranked by, and the key.  The multi-start call
// returns the lowest-index start that met the stop rule; a caller who runs K starts usually wants a particular one -- the configuration
// closest to where the arm is, the one furthest from its limits, the best-conditioned one (TRAC-IK's Distance / Manip solve types).
// The K starts, their lane mapping and the selection across lanes are the multi-start call's (device/multistart.hpp); only the key differs.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#include "lane_math.hpp"
#include "multistart.hpp"

namespace ikdev {

enum : int { PICK_DISTANCE = 0, PICK_MAX_DISTANCE = 1, PICK_LIMIT_MARGIN = 2, PICK_MANIPULABILITY = 3 };  // == ikgpu_pick_rule

constexpr int kPickMaxChain = 8;   // the longest chain a chain kernel is built for (kernels.hip IKGPU_FOR_NJ)

// What a pick kernel takes besides the single solve's arguments.
struct PickArgs {
    MultistartArgs ms;          // the starts, the draw, winner / err_sq and log2 K: the multi-start kernel's
    const double *q_ref;        // [nq x B] in the batch layout, or null: q0            (DISTANCE, MAX_DISTANCE)
    double *cost;               // [B] or null
    double w[kPickMaxChain];    // the weight of chain joint j's entry of q             (DISTANCE, MAX_DISTANCE)
    int rule;
};

// What a path multi-start kernel takes besides the single solve's arguments (include/ikgpu.h ikgpu_dls_path_multistart_batch): the K
// starts solve against via 0 (a.targets' slab 0), every start that entered follows the P segments of T waypoints through the slabs
// behind it, and the start that gets furthest is stored -- pick_key with cost = P T - reached.
struct PathMultistartArgs {
    MultistartArgs ms;          // the starts, the draw, winner / err_sq and log2 K: the multi-start kernel's
    int32_t *reached;           // [B] or null: the winner's count, 0 when its entry failed
    int32_t *reached_all;       // [K][B] or null: every start's count, -1 where the entry failed
    int T, P;                   // waypoints per segment >= 0, segments behind via 0 >= 0
    double max_joint_step;      // the path kernels' (line.hpp path_jumped)
};

// finite, read from the bits: the hot kernels are built with -fno-honor-nans / -fno-honor-infinities
IKD_FN bool pick_finite(double x) { return (multistart_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// ---- the costs, one support entry at a time (the kernels walk the chain, the loop's cost kernel walks q) -----------------------------
// DISTANCE: sum_i w_i (q_i - ref_i)^2, from 0.
IKD_FN double pick_distance_step(double acc, double w, double q, double ref) {
    const double d = q - ref;
    return dfma(w * d, d, acc);
}
// MAX_DISTANCE: max_i w_i |q_i - ref_i|, from 0.
IKD_FN double pick_max_distance_step(double acc, double w, double q, double ref) { return dmax(acc, w * __builtin_fabs(q - ref)); }
// LIMIT_MARGIN: the relative margin min_i min(q_i - lo_i, hi_i - q_i) / (hi_i - lo_i) over the entries with finite limits lo < hi and a
// finite range hi - lo (a free-flyer's entries carry -+DBL_MAX: no range), from 0.5 (no entry within its limits has more: a support
// without such an entry costs 0); the cost is pick_margin_cost of the result.
IKD_FN double pick_margin_step(double acc, double q, double lo, double hi) {
    const double range = hi - lo;
    const bool bounded = pick_finite(lo) && pick_finite(hi) && lo < hi && pick_finite(range);
    const double m = dmin(q - lo, hi - q) * drcp(bounded ? range : 1.0);
    return bounded ? dmin(acc, m) : acc;
}
IKD_FN double pick_margin_cost(double margin) { return 0.5 - margin; }
// MANIPULABILITY: 1 / sqrt(det G), G = J J^T + damping^2 I given by its lower triangle; det G is the product of the pivots of the
// unpivoted L D L^T the solver forms (lane_math.hpp ldlt_solve: the same elimination, without a right-hand side).  G is destroyed.
template <int M>
IKD_FN double pick_ldlt_det(double (&G)[M * M]) {
    double det = 1.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        det = det * G[k * M + k];
        const double inv = drcp(G[k * M + k]);
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            const double l = G[i * M + k] * inv;
#pragma unroll
            for (int j = k + 1; j <= i; ++j) G[i * M + j] = dfma(-l, G[j * M + k], G[i * M + j]);
        }
    }
    return det;
}
IKD_FN double pick_manipulability_cost(double det) { return drsqrt(det); }

// The rank of one start's result as ONE unsigned integer, smaller is better (multistart_key with the cost in place of 0): the bit
// pattern of the cost for a start that met the stop rule, else bit 63 set over the bit pattern of its error.  Both are non-negative, so
// the patterns order as the values do; a non-finite or negative-signed one ranks as +infinity.
IKD_FN unsigned long long pick_key(bool success, double cost, double err_sq) {
    const unsigned long long inf = 0x7ff0000000000000ull;
    unsigned long long u = multistart_bits(success ? cost : err_sq);
    if ((u & inf) == inf || (u >> 63) != 0ull) u = inf;
    return success ? u : ((1ull << 63) | u);
}

}  // namespace ikdev
