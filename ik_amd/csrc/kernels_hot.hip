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

// The lock-step jobs of kernels.hpp IKGPU_CHAIN_JOBS on the hot program, one overload per tail argument: the job's entry of
// device/chain_hot.hpp, on the never-stop visitor's own instantiation where the job has one (with_chain_job asks for no other).
#define IKGPU_HOT_JOB_KERNEL(TAIL)                                               \
    template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2, bool NEVERSTOP> \
    __global__ __launch_bounds__(kBlock) void dls_chain_hot_job_kernel(const ChainKernelArgs<NJ> a, const HotTable t, const TAIL)
IKGPU_HOT_JOB_KERNEL(int T) { ikdev::hot_track_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, T); }
IKGPU_HOT_JOB_KERNEL(ikdev::MultistartArgs ms) { ikdev::hot_multistart_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, ms); }
IKGPU_HOT_JOB_KERNEL(ikdev::GoalsetArgs ga) { ikdev::hot_goalset_entry<NJ, ChainStruct<C0, C1, C2>, NEVERSTOP>(a, t, ga); }
#define IKGPU_HOT_STOP_RULE_ONLY static_assert(!NEVERSTOP, "a job that needs a stop rule has no never-stop kernel");
IKGPU_HOT_JOB_KERNEL(ikdev::SolutionsArgs sa) { IKGPU_HOT_STOP_RULE_ONLY ikdev::hot_solutions_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, sa); }
IKGPU_HOT_JOB_KERNEL(ikdev::LineArgs la) { IKGPU_HOT_STOP_RULE_ONLY ikdev::hot_line_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, la); }
IKGPU_HOT_JOB_KERNEL(ikdev::PathArgs pa) { IKGPU_HOT_STOP_RULE_ONLY ikdev::hot_path_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pa); }
IKGPU_HOT_JOB_KERNEL(ikdev::PickArgs pk) { IKGPU_HOT_STOP_RULE_ONLY ikdev::hot_pick_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pk); }
IKGPU_HOT_JOB_KERNEL(ikdev::PathMultistartArgs pm) { IKGPU_HOT_STOP_RULE_ONLY ikdev::hot_path_multistart_entry<NJ, ChainStruct<C0, C1, C2>>(a, t, pm); }
#undef IKGPU_HOT_STOP_RULE_ONLY
#undef IKGPU_HOT_JOB_KERNEL

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

// One pre-built shape: the kernel the job asks for, on the never-stop visitor's own instantiation when the call has no stop rule
// (solve: the lambda; every other job: with_chain_job, which refuses a never-stop call of a job without that form).
template <int NJ, uint64_t C0, uint64_t C1, uint64_t C2>
hipError_t launch_hot_shape(const ProblemHost &ph, const DeviceTables &dt, const BatchIO &io, const ChainJob &job, const ikgpu_dls_params &prm,
                            hipStream_t stream, const HotTable &t) {
    ChainKernelArgs<NJ> a{};
    fill_chain_kernel_args(a, ph, dt);
    fill_solve_args(a, io, prm);
    const dim3 grid(static_cast<unsigned>((job.lanes(io.B) + kBlock - 1) / kBlock)), block(kBlock);
    auto launch = [&](auto never) -> hipError_t {
        constexpr bool NEVER = decltype(never)::value;
        if constexpr (NEVER) {
            hipLaunchKernelGGL((dls_chain_hot_kernel<NJ, C0, C1, C2, true>), grid, block, 0, stream, a, t);
            return hipGetLastError();
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
    };
    const bool never_stop = prm.stop_sq_tol < 0.0;
    if (job.kind == ChainJob::Solve) return never_stop ? launch(std::true_type{}) : launch(std::false_type{});
    return with_chain_job(job, never_stop, [&](auto rule, auto never) -> hipError_t {
        // (the overload of dls_chain_hot_job_kernel that takes the job's tail)
        hipLaunchKernelGGL((dls_chain_hot_job_kernel<NJ, C0, C1, C2, decltype(never)::value>), grid, block, 0, stream, a, t, decltype(rule)::tail(job));
        return hipGetLastError();
    });
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
