// goalset.hpp -- what the goal-set solve (include/ikgpu.h ikgpu_dls_goalset_batch) adds to the multi-start one (multistart.hpp): a problem
// has G = 1 << log2G alternative goals as well as K = 1 << log2K starts, and its G x K candidates are neighbouring lanes of one wave.
// Candidate j = g * K + k is start k solved against goal g; the key, the selection and the draw of a start are multistart.hpp's, over
// log2G + log2K butterfly steps on (key, j).  Shared by the kernels and the CPU lane emulator under tests/.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#include "multistart.hpp"

namespace ikdev {

// What a goal-set kernel takes besides the single solve's arguments (whose `targets` holds the G slabs of goals, [G][12 x B]).
// ms.winner is not written: the winner is reported as goal = j / K and start = j % K.
struct GoalsetArgs {
    MultistartArgs ms;          // the starts (they do not depend on the goal), err_sq, log2K
    int32_t *goal;              // [B] or null
    int32_t *start;             // [B] or null
    uint8_t *reachable;         // [G][B] or null: 1 where some start of goal g met the stop rule
    int log2G;
};

// any(m, flag): the OR of `flag` over the K lanes of this lane's goal (the lanes whose index within the wave differs from this lane's in
// the low log2K bits only), in every one of them.  On the device: one wave ballot, masked to the subgroup.
struct GoalsetBallot {
    IKD_FN bool operator()(int log2K, bool flag) const {
#if IKD_ON_DEVICE
        const unsigned long long votes = __ballot(flag);
        const int lane = static_cast<int>(threadIdx.x) & 63, K = 1 << log2K;
        const unsigned long long group = (K == 64 ? ~0ull : ((1ull << K) - 1ull)) << (lane & ~(K - 1));
        return (votes & group) != 0ull;
#else
        (void)log2K;
        return flag;
#endif
    }
};

}  // namespace ikdev
