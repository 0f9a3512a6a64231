// kernels_hot.hip -- the structure-specialised builds of the headline chain kernel (device/chain_hot.hpp): one Full FrameTask
// with unit weights on a fixed-base serial chain, i.e. BASELINE.json's configs 1, 2, 4 (Cassie leg) and 5 (UR arm).
//
// This translation unit is compiled with -fno-signed-zeros -fno-honor-nans -fno-honor-infinities (see the Makefile): the lane
// program multiplies by LITERAL 0.0 / +-1.0 where a placement entry is structurally zero / one, and those flags let the
// compiler fold such products (x * 0.0 -> 0.0 needs "no NaN, no signed zero") -- no reassociation, no reciprocal or
// approximate maths, contraction as in kernels.hip: on finite data the results are the bits of the full products.
//
// The instantiation list is generated: tools/print_struct_codes.cpp prints the placement-structure code (ikgpu::chain_structure)
// of the fixture models' chains.  A chain whose code is not in the list runs on the general chain kernel (kernels.hip).
#include "kernels.hpp"

#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "device/chain_hot.hpp"

namespace ikgpu {
namespace {

constexpr int kBlock = 64;  // one wave64 per workgroup: 1024 workgroups at B = 65536 cover 256 CUs x 4 SIMDs.  Every entry of chain_hot.hpp
                            // relies on it: the 16 KB sin / cos table in static LDS is filled by one wave, 16 entries per lane, without a barrier

using ikdev::ChainKernelArgs;
using ikdev::ChainStruct;
using ikdev::HotTable;

template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_kernel(const ChainKernelArgs<NJ> a, const HotTable t) {
    ikdev::hot_kernel_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t);
}

// The same program with lane refill (device/chain_kernel_body.hpp chain_refill_loop): the stop-rule mode on batches larger than the machine.
// Two waves per SIMD asked for (<= 256 registers): a wave that refills waits for its gathered loads (~2 us, most iterations have a
// lane that finishes) and the other wave of the SIMD computes meanwhile.
#ifndef IKGPU_HOT_REFILL_WAVES
#define IKGPU_HOT_REFILL_WAVES 2   // (tools/build_variant.sh onewave -DIKGPU_HOT_REFILL_WAVES=1: the A/B of DESIGN.md section 3.1)
#endif
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock, IKGPU_HOT_REFILL_WAVES) void dls_chain_hot_refill_kernel(const ChainKernelArgs<NJ> a, const HotTable t, unsigned long long *queue, int chunk) {
    ikdev::hot_refill_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, queue, chunk);
}

// T chained solves per problem in one launch, q in registers between them (device/chain_hot.hpp hot_track_body; include/ikgpu.h
// ikgpu_dls_track_batch).  Always lock-step per waypoint; no queue slot, no worklist, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_track_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const int T) {
    ikdev::hot_track_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, T);
}

// K starts per problem in one launch, the best one stored (device/chain_hot.hpp hot_multistart_body; include/ikgpu.h
// ikgpu_dls_multistart_batch): lane gid serves problem gid / K with start gid % K.  Lock-step; no LDS beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_multistart_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::MultistartArgs ms) {
    ikdev::hot_multistart_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, ms);
}

// K starts per problem in one launch, the converged one with the smallest cost stored (device/chain_hot.hpp hot_pick_body; include/ikgpu.h
// ikgpu_dls_pick_batch): the multi-start kernel's lane mapping, one instantiation for the four rules.  Stop rule only; lock-step; no LDS
// beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_pick_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::PickArgs pk) {
    ikdev::hot_pick_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pk);
}

// K starts per problem in one launch against via 0, each scouting the path behind it without a trajectory store, the one that gets
// furthest stored (device/chain_hot.hpp hot_path_multistart_body; include/ikgpu.h ikgpu_dls_path_multistart_batch): the multi-start
// kernel's lane mapping.  Stop rule only; lock-step per solve; no LDS beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_path_multistart_kernel(const ChainKernelArgs<NJ> a, const HotTable t,
                                                                               const ikdev::PathMultistartArgs pm) {
    ikdev::hot_path_multistart_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pm);
}

// G goals and K starts per problem in one launch, the best candidate stored (device/chain_hot.hpp hot_goalset_body; include/ikgpu.h
// ikgpu_dls_goalset_batch): lane gid serves problem gid / (G K) with goal (gid / K) % G and start gid % K.  Lock-step; no LDS, no queue
// slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_goalset_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::GoalsetArgs ga) {
    ikdev::hot_goalset_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, ga);
}

// K starts per problem in one launch, the distinct converged ones stored (device/chain_hot.hpp hot_solutions_body; include/ikgpu.h
// ikgpu_dls_solutions_batch): the multi-start kernel's lane mapping.  Stop rule only; lock-step; no LDS beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_solutions_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::SolutionsArgs sa) {
    ikdev::hot_solutions_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, sa);
}

// A straight Cartesian line to one goal per problem in one launch (device/chain_hot.hpp hot_line_body; include/ikgpu.h
// ikgpu_dls_line_batch).  Stop rule only; lock-step per waypoint; no LDS beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_line_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::LineArgs la) {
    ikdev::hot_line_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, la);
}

// A Cartesian path through P vias per problem with the joint-step rule in one launch (device/chain_hot.hpp hot_path_body; include/ikgpu.h
// ikgpu_dls_path_batch).  Stop rule only; lock-step per waypoint; no LDS beyond the sin / cos table, no queue slot, no allocation.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
__global__ __launch_bounds__(kBlock) void dls_chain_hot_path_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const ikdev::PathArgs pa) {
    ikdev::hot_path_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pa);
}

// X(NJ, code0, code1, code2)
#define IKGPU_HOT_SHAPES(X)                                                                                                   \
    X(7, 0x04f0208cce8c7664ull, 0x395959cacad65656ull, 0x000001cacace5656ull) /* Cassie leg: Left / RightFootFront, 22 values */ \
    X(6, 0x695959272b925656ull, 0x47655a33aaca549cull, 0x0000000000121256ull) /* UR5 / UR10 tool0, 14 values */

}  // namespace

// The hot program's preconditions: one Full FrameTask with unit weights on a chain whose structure code fits three words.
static bool chain_hot_eligible(const ProblemHost &ph) {
    if (ph.kind != KernelKind::Chain || ph.ntasks != 1 || ph.tasks[0].type != IKGPU_FULL || !task_has_unit_weights(ph.tasks[0])) return false;
    const char *env = std::getenv("IKGPU_CHAIN_HOT");
    if (env && std::strcmp(env, "0") == 0) return false;   // A/B switch: the general chain kernel
    return ph.chain_struct.fits;
}

bool chain_hot_built(const ProblemHost &ph) {
    if (!chain_hot_eligible(ph)) return false;
    const ChainStructure &s = ph.chain_struct;
    // The pre-built programs are chains of revolute joints.  The structure code does not say which joints slide: a UR5 whose elbow
    // is prismatic has UR5's code, and takes the run-time compiled build (whose key carries the mask) like any other chain.
    if (!s.fits || s.prismatic != 0) return false;
#define X(N, K0, K1, K2) \
    if (ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) return true;
    IKGPU_HOT_SHAPES(X)
#undef X
    return false;
}

int select_chain_build(const ProblemHost &ph, bool compile) {
    if (chain_hot_built(ph)) return 1;
    if (chain_hot_eligible(ph) && rtc_chain_hot_available(ph, compile)) return 2;
    return 0;
}

std::string chain_kernel_name(const ProblemHost &ph) {
    std::string n = ph.kernel_name;
    const size_t cut = n.rfind(',');
    if (cut == std::string::npos) return n;
    return n.substr(0, cut) + (ph.chain_build == 1 ? ",hot>" : ph.chain_build == 2 ? ",hot-rtc>" : ",general>");
}

namespace {

// One pre-built shape: the kernel the job asks for, on the never-stop visitor's own instantiation when the call has no stop rule.
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
hipError_t launch_hot_shape(const ProblemHost &ph, const DeviceTables &dt, const BatchIO &io, const ChainJob &job, const ikgpu_dls_params &prm,
                            hipStream_t stream, const HotTable &t) {
    ChainKernelArgs<NJ> a{};
    fill_chain_kernel_args(a, ph, dt);
    fill_solve_args(a, io, prm);
    const dim3 grid(static_cast<unsigned>((job.lanes(io.B) + kBlock - 1) / kBlock)), block(kBlock);
    auto launch = [&](auto never) -> hipError_t {
        constexpr bool NEVER = decltype(never)::value;
        if (job.kind == ChainJob::Track) {
            hipLaunchKernelGGL((dls_chain_hot_track_kernel<NJ, C0, C1, C2, NEVER>), grid, block, 0, stream, a, t, job.T);
        } else if (job.kind == ChainJob::Multistart) {
            hipLaunchKernelGGL((dls_chain_hot_multistart_kernel<NJ, C0, C1, C2, NEVER>), grid, block, 0, stream, a, t, job.ms);
        } else if (job.kind == ChainJob::Goalset) {
            hipLaunchKernelGGL((dls_chain_hot_goalset_kernel<NJ, C0, C1, C2, NEVER>), grid, block, 0, stream, a, t, job.goal);
        } else if (job.kind == ChainJob::Solutions) {
            if constexpr (NEVER) return hipErrorInvalidValue;   // (no start converges without a stop rule: the entry point refuses the call)
            else hipLaunchKernelGGL((dls_chain_hot_solutions_kernel<NJ, C0, C1, C2>), grid, block, 0, stream, a, t, job.sol);
        } else if (job.kind == ChainJob::Pick) {
            if constexpr (NEVER) return hipErrorInvalidValue;   // (likewise)
            else hipLaunchKernelGGL((dls_chain_hot_pick_kernel<NJ, C0, C1, C2>), grid, block, 0, stream, a, t, job.pick);
        } else if (job.kind == ChainJob::PathMultistart) {
            if constexpr (NEVER) return hipErrorInvalidValue;   // (likewise)
            else hipLaunchKernelGGL((dls_chain_hot_path_multistart_kernel<NJ, C0, C1, C2>), grid, block, 0, stream, a, t, job.pms);
        } else if (job.kind == ChainJob::Line) {
            if constexpr (NEVER) return hipErrorInvalidValue;   // (nothing is ever reached without a stop rule: refused likewise)
            else hipLaunchKernelGGL((dls_chain_hot_line_kernel<NJ, C0, C1, C2>), grid, block, 0, stream, a, t, job.line);
        } else if (job.kind == ChainJob::Path) {
            if constexpr (NEVER) return hipErrorInvalidValue;   // (likewise)
            else hipLaunchKernelGGL((dls_chain_hot_path_kernel<NJ, C0, C1, C2>), grid, block, 0, stream, a, t, job.path);
        } else if constexpr (NEVER) {
            hipLaunchKernelGGL((dls_chain_hot_kernel<NJ, C0, C1, C2, true>), grid, block, 0, stream, a, t);
        } else {
            const int64_t rgrid = refill_grid(reinterpret_cast<const void *>(dls_chain_hot_refill_kernel<NJ, C0, C1, C2>), io.B);
            return run_stop_rule(dt.queues, io, prm, stream, a, false, rgrid, PassThrough{&ph, &dt}, [&] {
                hipLaunchKernelGGL((dls_chain_hot_kernel<NJ, C0, C1, C2, false>), grid, block, 0, stream, a, t);
                return hipGetLastError();
            }, [&](unsigned long long *queue, int chunk) {
                hipLaunchKernelGGL((dls_chain_hot_refill_kernel<NJ, C0, C1, C2>), dim3(static_cast<unsigned>(rgrid)), block, 0, stream, a, t, queue, chunk);
                return hipGetLastError();
            });
        }
        return hipGetLastError();
    };
    return prm.stop_sq_tol < 0.0 ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace

hipError_t launch_dls_chain_hot(const ProblemHost &ph, const DeviceTables &dt, const BatchIO &io, const ChainJob &job, const ikgpu_dls_params &prm,
                                hipStream_t stream) {
    if (ph.chain_build == 2) return rtc_launch_chain_hot(ph, dt, io, job, prm, stream);
    const ChainStructure &s = ph.chain_struct;
    const std::vector<double> &tab = ph.chain_hot;
    HotTable t{};
    if (tab.size() > static_cast<size_t>(ikdev::kHotTableMax)) return hipErrorInvalidValue;
    std::memcpy(t.v, tab.data(), tab.size() * sizeof(double));
#define X(N, K0, K1, K2) \
    if (ph.chain.nj == N && s.code[0] == K0 && s.code[1] == K1 && s.code[2] == K2) return launch_hot_shape<N, K0, K1, K2>(ph, dt, io, job, prm, stream, t);
    IKGPU_HOT_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}

}  // namespace ikgpu
