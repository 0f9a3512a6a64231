// solutions.hpp -- what the solution-set solve (include/ikgpu.h ikgpu_dls_solutions_batch) shares between its kernels and the CPU lane
// emulator under tests/: the greedy set of distinct converged starts among the K starts of one problem.  The starts, the draw and the
// lane mapping are the multi-start solve's (device/multistart.hpp: K starts of a problem are K neighbouring lanes of one wave; ik::dls is
// a local method, reference ik/ik/dls.cpp:10, :73, ik/ik/dls.hpp:27); what differs is the cross-lane step after the loop: instead of one
// winner, every converged start that is separated from the ones kept before it is stored, up to N of them.
#pragma once
#include "multistart.hpp"

namespace ikdev {

// What a solution-set kernel takes besides the single solve's arguments.
struct SolutionsArgs {
    MultistartArgs ms;          // starts, draw, seed, log2K as the multi-start kernels read them (winner / err_sq: null, not read)
    int32_t *count;             // [B] the number of starts kept
    int32_t *which;             // [N][B] or null: the index of the start in each slot
    double sep;                 // two starts are the same solution when every chain entry differs by less than this
    int N;                      // at most this many are kept
};

// A lane's part of the state of its group's set.  The set is built in K steps, step j deciding start j: `cnt` is the number kept among the
// starts before the current step (the same in every lane of a group), `dropped` says a kept start before this one lies within sep of it.
struct SolutionsLane {
    int cnt = 0, slot = 0;      // slot: where this lane's start goes once kept
    bool offer = false, kept = false, dropped = false;
};

// Step j, first piece, every lane: would this lane's start be kept if it were decided now?  Final for lane j, whose predecessors are all
// decided; the other lanes' offers are not read in this step.
IKD_FN void solutions_offer(SolutionsLane &s, bool success, int N) { s.offer = success && !s.dropped && s.cnt < N; }

// "No entry differs by sep or more": one subtraction, fabs and a compare per entry -- the rule of include/ikgpu.h on the chain entries,
// which are the problem's support.
template <int NJ>
IKD_FN bool solutions_near(const double (&q)[NJ], const double (&qj)[NJ], double sep) {
    bool near = true;
#pragma unroll
    for (int i = 0; i < NJ; ++i) near = near && !(__builtin_fabs(q[i] - qj[i]) >= sep);
    return near;
}

// Step j, second piece, every lane (k: this lane's start).  fetch.flag(j, offer) is the offer of lane j of this lane's group,
// fetch.any(f) whether f holds in any lane of the wave (wave-uniform), fetch.q(j, q, qj) the chain entries of lane j of this lane's group.
template <int NJ, class Fetch>
IKD_FN void solutions_take(SolutionsLane &s, int j, int k, double sep, const double (&q)[NJ], Fetch fetch) {
    const bool kept_j = fetch.flag(j, s.offer);
    if (k == j) { s.kept = kept_j; s.slot = s.cnt; }
    if (fetch.any(kept_j)) {   // (a step that keeps nothing anywhere in the wave moves no entries)
        double qj[NJ];
        fetch.q(j, q, qj);
        if (k > j && kept_j && solutions_near<NJ>(q, qj, sep)) s.dropped = true;
    }
    s.cnt += kept_j ? 1 : 0;
}

// The K steps, as the kernels run them: K x (one flag through the cross-lane network, one ballot, and for a kept start its NJ entries in
// two 32-bit halves each); no LDS, no atomics.
template <int NJ, class Fetch>
IKD_FN void solutions_select(SolutionsLane &s, int log2K, int k, int N, double sep, bool success, const double (&q)[NJ], Fetch fetch) {
    for (int j = 0; j < (1 << log2K); ++j) {
        solutions_offer(s, success, N);
        solutions_take<NJ>(s, j, k, sep, q, fetch);
    }
}

// The fetches on the device.  base: the first lane of this lane's group within the wave, lane & ~(K - 1).
struct SolutionsShuffle {
    int base;
    IKD_FN bool flag(int j, bool offer) const {
#if IKD_ON_DEVICE
        return __shfl(offer ? 1 : 0, base + j) != 0;
#else
        (void)j;
        return offer;
#endif
    }
    IKD_FN bool any(bool f) const {
#if IKD_ON_DEVICE
        return __any(f ? 1 : 0) != 0;
#else
        return f;
#endif
    }
    template <int NJ>
    IKD_FN void q(int j, const double (&mine)[NJ], double (&theirs)[NJ]) const {
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
#if IKD_ON_DEVICE
            const unsigned long long u = multistart_bits(mine[i]);
            const unsigned lo = __shfl(static_cast<unsigned>(u), base + j), hi = __shfl(static_cast<unsigned>(u >> 32), base + j);
            const unsigned long long v = (static_cast<unsigned long long>(hi) << 32) | lo;
            __builtin_memcpy(&theirs[i], &v, sizeof v);
#else
            (void)j;
            theirs[i] = mine[i];
#endif
        }
    }
};

}  // namespace ikdev
