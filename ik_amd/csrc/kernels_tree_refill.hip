// kernels_tree_refill.hip -- the free-flyer tree kernels under lane refill (device/tree_kernel_body.hpp TreeRefill): the stop-rule
// mode of BASELINE.json's config 3 (Cassie full body) and of the general tree build on batches larger than the machine.  Persistent
// two-wave workgroups (the LDS park of chain 0's factor is per wave, as in kernels.hip); a lane whose visitor fired (reference
// ik/ik/visitor.hpp:15-21, ik/ik/dls.cpp:61-64) or whose iteration count reached max_iterations (dls.cpp:76-77) stores its result
// and takes the next unsolved problem; results are bit-identical to the lock-step kernels' (same lane program).
// A separate translation unit: the tree kernels are the slowest to compile.
#include "kernels.hpp"

#include <algorithm>

#include "device/tree_kernel_body.hpp"

namespace ikgpu {
namespace {

using ikdev::HotMask;
using ikdev::LdsPark;
using ikdev::TreeDesc;
using ikdev::TreeKernelArgs;

constexpr int kTreeWaves = 2;
constexpr int kTreeBlock = 64 * kTreeWaves;

template <int NJ, int NCH, int SPEC>
__global__ __launch_bounds__(kTreeBlock) void dls_tree_refill_kernel(const TreeKernelArgs<NJ, NCH> a, unsigned long long *queue, int chunk) {
    __shared__ double lds_park[kTreeWaves][NCH > 1 ? LdsPark<NJ>::kEntries : 1][64];
    __shared__ double lds_desc[sizeof(TreeDesc<NJ, NCH>) / sizeof(double)];
    {
        constexpr int kWords = sizeof(TreeDesc<NJ, NCH>) / sizeof(double);
        const double *g = reinterpret_cast<const double *>(a.desc);
        for (int i = threadIdx.x; i < kWords; i += kTreeBlock) lds_desc[i] = g[i];
        __syncthreads();
    }
    const TreeDesc<NJ, NCH> &d = *reinterpret_cast<const TreeDesc<NJ, NCH> *>(lds_desc);
    LdsPark<NJ> park{lds_park[threadIdx.x / 64], static_cast<int>(threadIdx.x % 64)};
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * kTreeWaves + threadIdx.x / 64;
    ikdev::dls_tree_refill_body<NJ, NCH, SPEC>(a, d, wave, static_cast<int64_t>(gridDim.x) * kTreeWaves, park, queue, chunk);
}

// The refill twin of each lock-step build (kernels.hip run_dls_tree), whose lane program it must share to return the same bits:
// TreeBuild::kRefillHot (mask, unit weights, base task at a translation: all folded), kRefillMask (the placement mask folded only),
// kRefillFold (the mask next to the general extras: base-relative references, alignment row, fixed base), kRefillGeneral.
// Instantiated for NJ = 7 only (problem.cpp select_tree_build names a twin for no other shape).
template <int NJ, int NCH>
const void *refill_kernel(int refill) {
    if constexpr (NJ != 7) {
        return nullptr;
    } else {
        constexpr int kMask = HotMask<NJ>::value;
        constexpr int kHot = kMask | (1 << ikdev::kSpecUnit) | (1 << ikdev::kSpecUnitP) | (1 << ikdev::kSpecIdP);
        constexpr int kFold = kMask | (1 << ikdev::kSpecGen);
        return refill == TreeBuild::kRefillHot    ? reinterpret_cast<const void *>(dls_tree_refill_kernel<NJ, NCH, kHot>)
               : refill == TreeBuild::kRefillMask ? reinterpret_cast<const void *>(dls_tree_refill_kernel<NJ, NCH, kMask>)
               : refill == TreeBuild::kRefillFold ? reinterpret_cast<const void *>(dls_tree_refill_kernel<NJ, NCH, kFold>)
               : refill == TreeBuild::kRefillGeneral ? reinterpret_cast<const void *>(dls_tree_refill_kernel<NJ, NCH, 0>)
                                                     : nullptr;
    }
}

}  // namespace

// Resident waves of the refill twin of a tree problem's lock-step build (kernels.hpp run_stop_rule); 0 where it has none
// (TreeBuild::kRefillNone: posture rows, a constraint, an ik::pik level, shapes other than NJ = 7).  Persistent workgroups of two waves: what the device
// holds, one wave per SIMD until every lane has >= 8 problems (kernels.hip refill_resident).
template <int NJ, int NCH>
int64_t tree_refill_waves(int refill, int64_t B) {
    const void *kernel = refill_kernel<NJ, NCH>(refill);
    if (!kernel) return 0;
    const int64_t occ_waves = persistent_grid(kernel, kTreeBlock, 0, INT64_MAX) * kTreeWaves;
    const int64_t waves = refill_resident(occ_waves, B);
    return std::max<int64_t>(kTreeWaves, waves / kTreeWaves * kTreeWaves);
}

// The refill twin `refill` on `waves` resident waves (tree_refill_waves), `a` the lock-step launch's argument block.
template <int NJ, int NCH>
hipError_t launch_tree_refill_build(const TreeKernelArgs<NJ, NCH> &a, int refill, int64_t waves, unsigned long long *queue, int chunk,
                                    hipStream_t stream) {
    void *args[] = {const_cast<TreeKernelArgs<NJ, NCH> *>(&a), &queue, &chunk};
    return hipLaunchKernel(refill_kernel<NJ, NCH>(refill), dim3(static_cast<unsigned>(waves / kTreeWaves)), dim3(kTreeBlock), args, 0, stream);
}

#define X(N, C)                                                                                                                        \
    template int64_t tree_refill_waves<N, C>(int, int64_t);                                                                            \
    template hipError_t launch_tree_refill_build<N, C>(const TreeKernelArgs<N, C> &, int, int64_t, unsigned long long *, int, hipStream_t);
X(7, 2) X(7, 1) X(6, 2) X(6, 1)
#undef X

}  // namespace ikgpu
