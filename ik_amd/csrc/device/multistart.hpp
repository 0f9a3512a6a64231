// multistart.hpp -- what the multi-start solve (include/ikgpu.h ikgpu_dls_multistart_batch) shares between its kernels and the CPU lane
// emulator under tests/: the draw of a generated start, the key a start is ranked by, and the selection among the K starts of one
// problem.  ik::dls is a local method and the reference says so itself (ik/ik/dls.cpp:10 "todo - if limited convergence, try random
// walk", dls.cpp:73 "If issues, perform random restart"; dls_parameters::random_restart, ik/ik/dls.hpp:27, is read by nothing): K starts
// of one problem are K neighbouring lanes of one wave here, solved side by side and compared across lanes.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#include "lane_math.hpp"

namespace ikdev {

// What a multi-start kernel takes besides the single solve's arguments.  K = 1 << log2K starts per problem.
struct MultistartArgs {
    const double *starts;       // [K-1][nq x B] caller's starts 1 .. K-1, or null: generated from `seed`
    const uint8_t *draw;        // [nq] 1 where a generated start draws the entry (multistart_draw), 0 where it keeps q0's
    unsigned long long seed;
    int32_t *winner;            // [B] or null
    double *err_sq;             // [B] or null
    int log2K;
};

IKD_FN unsigned long long multistart_mix(unsigned long long z) {   // (the splitmix64 finaliser)
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// u in [0, 1) of entry i of start k of problem b: a function of (seed, b, k, i) only -- not of B, K, the layout or the build.
IKD_FN double multistart_uniform(unsigned long long seed, int64_t b, int k, int i) {
    unsigned long long h = multistart_mix(seed + 0x9E3779B97F4A7C15ull);
    h = multistart_mix(h + static_cast<unsigned long long>(b));
    h = multistart_mix(h + static_cast<unsigned long long>(k));
    h = multistart_mix(h + static_cast<unsigned long long>(i));
    return static_cast<double>(h >> 11) * 0x1.0p-53;
}

// Entry i of generated start k >= 1 of problem b, for an entry with finite limits lo < hi: uniform in [lo, hi].
IKD_FN double multistart_draw(unsigned long long seed, int64_t b, int k, int i, double lo, double hi) {
    return dmin(hi, dmax(dfma(multistart_uniform(seed, b, k, i), hi - lo, lo), lo));
}

IKD_FN unsigned long long multistart_bits(double x) {
    unsigned long long u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}

// The rank of one start's result as ONE unsigned integer, smaller is better: 0 for a start that met the stop rule, else bit 63 set
// over the bit pattern of its error (a sum of squares: non-negative, so the patterns order as the values do).  A non-finite error
// ranks as +infinity.  Read from the bits: the kernels are built with -fno-honor-nans / -fno-honor-infinities.
IKD_FN unsigned long long multistart_key(bool success, double err_sq) {
    const unsigned long long inf = 0x7ff0000000000000ull;
    unsigned long long u = multistart_bits(err_sq);
    if ((u & inf) == inf || (u >> 63) != 0ull) u = inf;
    return success ? 0ull : ((1ull << 63) | u);
}

// The start with the smallest (key, index) among the K = 1 << log2K lanes of a group, in every lane of the group: a butterfly of log2K
// steps.  exchange(m, key, k) replaces (key, k) by those of the lane whose index within the wave differs in bit m.
template <class Exchange>
IKD_FN int multistart_select(int log2K, unsigned long long key, int k, Exchange exchange) {
    for (int s = 0; s < log2K; ++s) {
        unsigned long long okey = key;
        int ok = k;
        exchange(1 << s, okey, ok);
        const bool take = okey < key || (okey == key && ok < k);
        key = take ? okey : key;
        k = take ? ok : k;
    }
    return k;
}

// The exchange on the device: two 32-bit halves of the key and the index through the cross-lane network.
struct MultistartShuffle {
    IKD_FN void operator()(int m, unsigned long long &key, int &k) const {
#if IKD_ON_DEVICE
        const unsigned lo = __shfl_xor(static_cast<unsigned>(key), m), hi = __shfl_xor(static_cast<unsigned>(key >> 32), m);
        key = (static_cast<unsigned long long>(hi) << 32) | lo;
        k = __shfl_xor(k, m);
#else
        (void)m; (void)key; (void)k;
#endif
    }
};

}  // namespace ikdev
