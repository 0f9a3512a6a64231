// tree_build.hpp -- from a TreeBuild (problem.hpp select_tree_build) to the SPEC template argument of ikdev::dls_tree_body: the one
// mapping the launcher (kernels.hip run_dls_tree) and the CPU lane emulator (tests/lane_emu/tree_emu.cpp) instantiate from, so that
// neither can run a build the selection did not name.
#pragma once
#include <type_traits>

#include "device/tree_kernel_body.hpp"
#include "problem.hpp"

namespace ikgpu {

// Calls f(std::integral_constant<int, SPEC>{}) with the SPEC of build `b` on shape (NJ, NCH) and returns true; false when the shape
// has no such build (the constraint builds exist for two chains only).  The general builds exist twice where the shape's placement
// mask is known: with it folded (bit kSpecGen next to the mask) and without.
template <int NJ, int NCH, class F>
bool with_tree_spec(const TreeBuild &b, F &&f) {
    constexpr int kMask = ikdev::HotMask<NJ>::value;
    constexpr int kHot = kMask | (1 << ikdev::kSpecUnit) | (1 << ikdev::kSpecUnitP) | (1 << ikdev::kSpecIdP);
#define IKGPU_TREE_SPEC(V) (f(std::integral_constant<int, (V)>{}), true)
#define IKGPU_TREE_GENERAL(FLAGS) \
    (b.folded ? IKGPU_TREE_SPEC(kMask != 0 ? ((FLAGS) | kMask | (1 << ikdev::kSpecGen)) : (FLAGS)) : IKGPU_TREE_SPEC(FLAGS))
    switch (b.build) {
    case TreeBuild::kHotNever: return IKGPU_TREE_SPEC(kHot | (1 << ikdev::kSpecNever));
    case TreeBuild::kHot: return IKGPU_TREE_SPEC(kHot);
    case TreeBuild::kMask: return IKGPU_TREE_SPEC(kMask != 0 ? kMask : kHot);
    default: break;
    }
    switch (b.extras) {
    case TreeBuild::kPik: return IKGPU_TREE_GENERAL((1 << ikdev::kSpecPik));
    case TreeBuild::kPostureConstraint:
        if constexpr (NCH == 2) return IKGPU_TREE_GENERAL(ikdev::kSpecPostCons);
        else return false;
    case TreeBuild::kConstraint:
        if constexpr (NCH == 2) return IKGPU_TREE_GENERAL((1 << ikdev::kSpecCons));
        else return false;
    case TreeBuild::kPosture: return IKGPU_TREE_GENERAL((1 << ikdev::kSpecPost));
    default: return IKGPU_TREE_GENERAL(0);
    }
#undef IKGPU_TREE_GENERAL
#undef IKGPU_TREE_SPEC
}

}  // namespace ikgpu
