// The hot chain kernel for structure codes that are compiled at run time (rtc.cpp), for tools/kernel_stats.py: the all-general 7-joint
// chain of fixtures/models/arm7.kin.urdf (no structural entry, no run: 96 placement values parked in accumulation registers) and the
// same chain with its placements 4 and 5 made identity rotations -- a run of three joints, folded by hot_evaluate; and a chain with a
// prismatic joint: a UR5 on a linear rail along x (fixtures/models/ur5.kin.urdf with its world_joint made prismatic; joint 0 slides).
// Compile-only.
#include <hip/hip_runtime.h>

#include "device/chain_hot.hpp"

using namespace ikdev;

constexpr uint64_t kGeneral = 7ull << 18;   // nine general rotation entries, three non-zero translation components
constexpr uint64_t identity_rotation() {
    uint64_t v = 7ull << 18;
    for (int e = 0; e < 9; ++e) v |= static_cast<uint64_t>((e == 0 || e == 4 || e == 8) ? kEntOne : kEntZero) << (2 * e);
    return v;
}
constexpr uint64_t kIdentity = identity_rotation();
constexpr uint64_t word(uint64_t a, uint64_t b, uint64_t c) { return a | (b << kStructBits) | (c << (2 * kStructBits)); }

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP>
__global__ __launch_bounds__(64) void hot_rtc_shape_kernel(const ChainKernelArgs<NJ> a, const HotTable t) {
    hot_kernel_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t);
}
template __global__ void hot_rtc_shape_kernel<7, word(kGeneral, kGeneral, kGeneral), word(kGeneral, kGeneral, kGeneral), word(kGeneral, kGeneral, 0), true>(
    const ChainKernelArgs<7>, const HotTable);
template __global__ void hot_rtc_shape_kernel<7, word(kGeneral, kGeneral, kGeneral), word(kGeneral, kIdentity, kIdentity), word(kGeneral, kGeneral, 0), true>(
    const ChainKernelArgs<7>, const HotTable);

// (a kernel template of its own: the two above keep their names)
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, unsigned PM, bool NEVERSTOP>
__global__ __launch_bounds__(64) void hot_rtc_prismatic_kernel(const ChainKernelArgs<NJ> a, const HotTable t) {
    hot_kernel_entry<NJ, ChainStruct<C0, C1, C2, PM>, NEVERSTOP>(a, t);
}
template __global__ void hot_rtc_prismatic_kernel<7, 0x24e570accea17665ull, 0x4675594a939a5656ull, 0x000002424ad1d956ull, 0x01u, true>(
    const ChainKernelArgs<7>, const HotTable);
