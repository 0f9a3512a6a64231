// chain_hot.hpp -- the headline lane program: ik::dls() for ONE problem with one Full FrameTask (unit weights, reference
// frame fixed in the world) on a serial chain of NJ <= 7 revolute or prismatic joints, specialised at compile time on the STRUCTURE of the
// chain's constant placements.
//
// Same algorithm as device/chain_solver.hpp (which stays the program of every other chain problem; the reference path it
// restates is cited there: ik/ik/dls.cpp:5-78, data.cpp:25-58, frame.hpp:37-62,152-182, common.hpp:53-56, visitor.hpp:15-21),
// with the Jacobian columns built in the task frame, tip to base (hot_evaluate): the two builds differ by rounding.
// What differs is what a lone wave pays for: measured on gfx950
// (tools/issue_probe.hip, profiles/r02_issue_probe.csv) a wave that has its SIMD to itself -- the situation at the metric's
// batch, 65536 problems = 1024 waves on 1024 SIMDs -- issues ONE instruction of any kind every 4 cycles (VALU, SALU, s_nop,
// s_waitcnt alike; 16 for an FP64 transcendental, 8 for v_mov_b64) and a dependent FP64 instruction can follow its producer
// in the next slot.  The iteration therefore costs 4 cycles x (number of instructions) + the scalar-load waits, and nothing
// else: instruction-level parallelism buys nothing, every instruction removed buys 4 cycles.  Hence:
//
//  * Placement structure as a template argument.  Joint placements in URDFs are mostly axis permutations (rpy multiples of
//    pi/2) and translations along one or two axes.  The host classifies every entry of every placement of the chain --
//    rotation entries: exactly 0, exactly +1, exactly -1, or general; translation: which components are exactly zero --
//    into a 21-bit code (ChainStruct).  For a structural entry the lane program uses the LITERAL 0.0 / +-1.0, and the translation
//    unit is compiled with -fno-signed-zeros -fno-honor-nans -fno-honor-infinities (no reassociation, no reciprocal maths:
//    results stay bit-identical on finite data) so that x * 0.0, x * 1.0, x + 0.0 fold away: a near-permutation placement costs
//    6-15 instructions instead of 36.  No robot constant is compiled in: the non-structural values (22 doubles for a
//    Cassie leg instead of 96) arrive in the kernel-argument segment and stay in registers for the whole loop -- no table
//    loads, no s_waitcnt inside the iteration.  A model whose code has no instantiation runs on chain_solver.hpp.
//  * The visitor that never stops (the metric's fixed-iteration mode) is its own instantiation: no `active` selects, no
//    stop-test arithmetic.
//  * The task Jacobian in the task frame, tip to base (hot_evaluate).  The reference defines J = -Jlog6(tMf) J_local with the frame
//    Jacobian in the LOCAL frame; walking the chain from the task frame towards the base yields the columns of J_local directly
//    (third row of the running rotation, and R^T (e_z x p)).  The world-frame form of chain_solver.hpp pays for the detour: the
//    frame rotation folded into both Jlog6 blocks (54 multiply-adds), org_j - p and a full cross product per joint, and three
//    multiply-adds per non-zero translation component of a right-multiplied placement where the left-multiplied one adds.  Issue
//    slots per iteration of the evaluation (tools/hot_phase_count.py): Cassie leg 743 -> 641, UR5 / UR10 653 -> 611.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#include "chain_kernel_body.hpp"

namespace ikdev {

// 21 bits per placement i = 0 .. NJ (i = NJ: last joint frame -> task frame), three placements per 64-bit word:
//   bits 0-17   nine 2-bit classes of the rotation entries, row-major: 0 general (a table value), 1 exactly 0, 2 exactly +1,
//               3 exactly -1   (URDF rpy values are decimal approximations of pi/2, so a "permutation" placement usually
//               keeps a few entries of 1e-12 .. 1e-16: those stay general and exact -- nothing is snapped)
//   bits 18-20  translation component k is non-zero
constexpr int kStructBits = 21;
constexpr int kStructPerWord = 3;
enum : unsigned { kEntGeneral = 0, kEntZero = 1, kEntOne = 2, kEntMinusOne = 3 };

// PM: bit j set when joint j is PRISMATIC -- it slides along its local z where a revolute joint turns about it (chain_solver.hpp).
// 0, the default, is a chain of revolute joints: the type every such chain had before prismatic joints were taken.
template <uint64_t C0, uint64_t C1, uint64_t C2, unsigned PM = 0>
struct ChainStruct {
    static constexpr unsigned kPrismatic = PM;
    static constexpr bool prismatic(int j) { return j >= 0 && ((PM >> j) & 1u) != 0; }
    static constexpr uint64_t word(int w) { return w == 0 ? C0 : (w == 1 ? C1 : C2); }
    static constexpr unsigned code(int i) { return static_cast<unsigned>((word(i / kStructPerWord) >> (kStructBits * (i % kStructPerWord))) & 0x1fffffu); }
    static constexpr unsigned ent(int i, int e) { return (code(i) >> (2 * e)) & 3u; }           // e = 3 m + k
    static constexpr bool tnz(int i, int k) { return ((code(i) >> (18 + k)) & 1u) != 0; }
    static constexpr int ngen_before(int i, int e) { return e == 0 ? 0 : ngen_before(i, e - 1) + (ent(i, e - 1) == kEntGeneral ? 1 : 0); }
    static constexpr int count(int i) { return ngen_before(i, 9) + (tnz(i, 0) ? 1 : 0) + (tnz(i, 1) ? 1 : 0) + (tnz(i, 2) ? 1 : 0); }
    // position of placement i's values in the compact table: [general rotation entries, row-major][non-zero translation entries]
    static constexpr int offset(int i) { return i == 0 ? 0 : offset(i - 1) + count(i - 1); }
    static constexpr int rot_at(int i, int e) { return offset(i) + ngen_before(i, e); }
    static constexpr int trans_at(int i, int k) {
        return offset(i) + ngen_before(i, 9) + (k > 0 && tnz(i, 0) ? 1 : 0) + (k > 1 && tnz(i, 1) ? 1 : 0);
    }
    static constexpr double literal(int i, int e) { return ent(i, e) == kEntOne ? 1.0 : (ent(i, e) == kEntMinusOne ? -1.0 : 0.0); }
    // Joint j (>= 1) turns about the SAME world axis as joint j - 1 when its placement has an exactly-identity rotation (R * Rz leaves
    // the third column of R alone).  leader(j): the first joint of j's run of parallel axes; members(L): how many joints L leads.
    // A prismatic joint has no angle to share: it is a run of its own and ends the run below it (leader(j) = j for it and for j + 1).
    static constexpr bool identity_rotation(int i) {
        return ent(i, 0) == kEntOne && ent(i, 4) == kEntOne && ent(i, 8) == kEntOne && ent(i, 1) == kEntZero && ent(i, 2) == kEntZero &&
               ent(i, 3) == kEntZero && ent(i, 5) == kEntZero && ent(i, 6) == kEntZero && ent(i, 7) == kEntZero;
    }
    static constexpr int leader(int j) { return (j > 0 && identity_rotation(j) && !prismatic(j) && !prismatic(j - 1)) ? leader(j - 1) : j; }
    static constexpr int members(int L, int nj) { return nj <= 0 ? 0 : members(L, nj - 1) + (leader(nj - 1) == L ? 1 : 0); }
};

// The shortest run of parallel joints that hot_evaluate walks in the run's own frame ("folds").  From the static counts of the
// iteration loop (v_mov_b64 two issue slots, a transcendental four): each member after the first saves the 16
// instructions that rotate rows 0, 1 of R and p, and pays one addition for its angle sum and one extra multiply-add per in-plane
// translation component; forming lin_j and A lin_j costs 6 + 9 = 15 per member unfolded against 6 per member and 18 once per run
// folded (A r0, A r1), which is even at two joints (30 = 30) and ahead from three.  A run of two therefore already pays, and the
// listing agrees: UR5 / UR10 (one run of two) 1049 -> 1035 slots with no copy added and ten registers fewer.  A run of one has
// nothing to fold; 1 here would only send every joint down the folded path for no gain.
// Known cost: in a chain whose table is parked in accumulation registers (kHotTableVgprMax) the allocator spills around the
// theta -> pi arm of log3 once a run is folded -- the all-general 7-joint chain with a run of three: executed path 1419 -> 1356 slots,
// that arm 116 -> 251 -- so a wave of such a chain that enters the arm (a lane within 1e-2 of pi) pays more than before.
constexpr int kHotFoldMinRun = 2;

// leader / members as compile-time tables (indexed by the unrolled joint loops: a constant index into a constant array folds;
// the recursive constexpr functions above, called with a loop variable, would be emitted as real calls)
// folded[j]: joint j's run is walked in the run's own frame by hot_evaluate (a run of at least kHotFoldMinRun joints); tip[j]: j is
// the tip-side end of its run (the member the tip-to-base walk meets first); any_folded: the chain has a folded run.
template <class S, int NJ>
struct ChainRuns {
    struct Table { int leader[8], members[8]; bool folded[8], tip[8], prismatic[8], any_folded; };
    static constexpr Table make() {
        Table t{};
        for (int j = 0; j < 8; ++j) { t.leader[j] = j < NJ ? S::leader(j) : j; t.members[j] = 0; t.prismatic[j] = j < NJ && S::prismatic(j); }
        for (int j = 0; j < NJ; ++j) ++t.members[t.leader[j]];
        for (int j = 0; j < 8; ++j) {
            t.folded[j] = t.members[t.leader[j]] >= kHotFoldMinRun;
            t.tip[j] = j == t.leader[j] + t.members[t.leader[j]] - 1;
            if (j < NJ && t.folded[j]) t.any_folded = true;
        }
        return t;
    }
    static constexpr Table value = make();
};

constexpr int kHotTableMax = 112;  // doubles in the kernel-argument copy of the compact table (values, then lo[NJ], hi[NJ]): 8 x 12 + 2 x 7 when nothing is structural

// Placement values (S::offset(NJ + 1) doubles) up to which hot_park_table's copy of the table stays in vector registers next to the
// loop's own live registers: the built-in structure codes have at most 36 (Cassie leg: 22) and stay, the all-general 7-joint chain
// has 96 and is parked in accumulation registers by the compiler (compile-only assembly, tools/kernel_stats.py).  The bound sits
// between the two observed classes -- nothing between 36 and 96 has been built --; it is the one place that says which class a chain
// is in, and hot_evaluate asks it.
constexpr int kHotTableVgprMax = 48;

struct HotTable {
    double v[kHotTableMax];
};

// ---- the table of dsincos_lut (lane_math.hpp) as the lane programs reach it: through their Tab argument --------------------------
// A plain HotTable (the host emulators and shims under tests/) reads the header's array where it stands.  The kernels pass a
// HotTableLds, which carries a pointer to the workgroup's copy in LDS beside v[]: one ds_read_b128 per angle, on the one pipe these
// kernels otherwise leave idle.  Both read the same 2048 doubles, so every job and both stop-rule modes compute the same bits.
// DEVICE code that hands the lane program a plain HotTable does not compile (the overload is deleted there): an entry that forgets
// IKD_HOT_LUT_DECLARE must not fall back to reading the table from HBM unnoticed.  The phase probes of tools/, which wrap single
// functions in kernels of their own, ask for that path by name: IKD_HOT_LUT_FROM_HBM, defined ahead of this header.
struct HotLutNoStage {};
#if IKD_HIP_LANG
typedef double SinCosPair __attribute__((ext_vector_type(2)));   // {sin, cos}, 16 bytes
// the header's literals, device-resident, once per translation unit: what the entries stage into LDS (mathematical constants, the
// same on every call)
static __device__ const double kSinCosLutDevice[2 * IKD_SINCOS_LUT_SIZE] __attribute__((aligned(16), unused)) = {IKD_SINCOS_LUT_VALUES};
struct HotTableLds : HotTable {
    SinCosPair *lut;   // IKD_SINCOS_LUT_SIZE entries of static __shared__ memory (IKD_HOT_LUT_DECLARE), filled by hot_lut_commit
};
constexpr int kHotLutPerLane = IKD_SINCOS_LUT_SIZE / 64;   // one wave64 per workgroup: 16 entries of 16 bytes per lane
struct HotLutStage { SinCosPair v[kHotLutPerLane]; };
// The fill in two halves, so that a body can put its own loads from HBM between them: hot_lut_issue starts the 16 loads of this lane
// (entries lane + 64 i: consecutive lanes read consecutive 16 bytes), hot_lut_commit writes them to LDS.  A body calls the first ahead
// of its q0 and target loads and the second behind them -- one round trip to HBM for all of it -- and in front of its pass-through
// stores.  One wave per workgroup: LDS serves a wave's accesses in order, so the reads that follow see the writes of every lane
// without a barrier; the fence keeps the compiler from moving a read above them.
__device__ __forceinline__ HotLutStage hot_lut_issue(const HotTableLds &) {
    HotLutStage st;
    const SinCosPair *src = reinterpret_cast<const SinCosPair *>(kSinCosLutDevice);
    const int lane = static_cast<int>(threadIdx.x) & 63;
#pragma unroll
    for (int i = 0; i < kHotLutPerLane; ++i) st.v[i] = src[lane + 64 * i];
    return st;
}
__device__ __forceinline__ void hot_lut_commit(const HotTableLds &t, const HotLutStage &st) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
#pragma unroll
    for (int i = 0; i < kHotLutPerLane; ++i) t.lut[lane + 64 * i] = st.v[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void hot_lut_fetch(const HotTableLds &t, int idx, double &S, double &C) {
    const SinCosPair e = t.lut[idx];
    S = e.x;
    C = e.y;
}
// in a kernel entry: the 16 KB table and the table object `tv` that carries it
#define IKD_HOT_LUT_DECLARE(tv)                                       \
    __shared__ SinCosPair ikd_hot_lut[IKD_SINCOS_LUT_SIZE];           \
    HotTableLds tv;                                                   \
    tv.lut = ikd_hot_lut
#endif
IKD_FN HotLutNoStage hot_lut_issue(const HotTable &) { return HotLutNoStage{}; }
IKD_FN void hot_lut_commit(const HotTable &, const HotLutNoStage &) {}
#if IKD_ON_DEVICE && !defined(IKD_HOT_LUT_FROM_HBM)
void hot_lut_fetch(const HotTable &, int idx, double &S, double &C) = delete;
#else
IKD_FN void hot_lut_fetch(const HotTable &, int idx, double &S, double &C) {
#if IKD_ON_DEVICE
    S = kSinCosLutDevice[2 * idx];
    C = kSinCosLutDevice[2 * idx + 1];
#else
    S = kSinCosLutHost[2 * idx];
    C = kSinCosLutHost[2 * idx + 1];
#endif
}
#endif

// sin and cos of NJ angles at once, the form the hot loops run (hot_evaluate; tools/hot_phase_count.hip counts this very function):
// dsincos_lut in its pieces, ordered by hand because a lone wave hides the table read behind nothing else -- every reduction and
// index, then the NJ reads in the order the tip-to-base walk consumes them, then the residual polynomials, which need nothing from
// the table, then the combinations.
// PM: the chain's prismatic joints (ChainStruct) -- no angle, so nothing is computed for them and sn / cs stay unset there.
template <int NJ, unsigned PM = 0, class Tab>
IKD_FN void hot_sincos(const Tab &t, const double (&phi)[NJ], double (&sn)[NJ], double (&cs)[NJ]) {
    double res[NJ], tS[NJ], tC[NJ], sl[NJ], cm1[NJ];
    int idx[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (!((PM >> j) & 1u)) dsincos_lut_reduce(phi[j], res[j], idx[j]);
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j)
        if (!((PM >> j) & 1u)) hot_lut_fetch(t, idx[j], tS[j], tC[j]);
    IKD_SCHED_FENCE();   // (left alone the scheduler issues the reads behind the polynomials and waits for them at once)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (!((PM >> j) & 1u)) dsincos_lut_poly(res[j], sl[j], cm1[j]);
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j)
        if (!((PM >> j) & 1u)) dsincos_lut_combine(tS[j], tC[j], sl[j], cm1[j], sn[j], cs[j]);
}

// entry e = 3 m + k of placement I's rotation: the literal 0.0 / +-1.0 when structural, else its table value
template <class S, int I, class Tab>
IKD_FN double hot_rot(const Tab &t, int e) {
    return S::ent(I, e) == kEntGeneral ? t.v[S::rot_at(I, e)] : S::literal(I, e);
}

// (R, p) <- placement I * (R, p), a LEFT composition: R' = Rc R, p' = Rc p + tc.  Written as the general product; with literal zeros
// and ones in it the compiler folds the multiplications by 1 and (under -fno-signed-zeros -fno-honor-nans) by 0 away: same bits as
// the full product on finite data.  The translation is the innermost addend: under a near-permutation Rc it is one addition per
// non-zero component (composed from the right it went through the running rotation, three multiply-adds per component), and an
// identity Rc leaves R -- its third row in particular -- the very same values.
template <class S, int I, class Tab>
IKD_FN void hot_compose_left(double (&R)[9], double (&p)[3], const Tab &t) {
    double Ro[9], po[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ro[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = p[k];
    // row by row of Rc: three entries of R' and one of p' per row
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double c0 = hot_rot<S, I>(t, 3 * r), c1 = hot_rot<S, I>(t, 3 * r + 1), c2 = hot_rot<S, I>(t, 3 * r + 2);
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * r + k] = dfma(c0, Ro[k], dfma(c1, Ro[3 + k], c2 * Ro[6 + k]));
        const double last = S::tnz(I, r) ? dfma(c2, po[2], t.v[S::trans_at(I, r)]) : c2 * po[2];
        p[r] = dfma(c0, po[0], dfma(c1, po[1], last));
    }
}

// The base placement P_0 = (Rc, tc) is constant, and fMt = oMf^-1 oMt = (Rz(q_0) P_1 ... P_NJ)^-1 (P_0^-1 oMt): the target can carry
// P_0^-1 once per solve instead of the walk composing P_0 in every iteration.  oM0 = P_0^-1 oMt: R' = Rc^T R_t, p' = Rc^T (p_t - tc),
// with Rc read through hot_rot so that literal 0 / +-1 entries fold as in hot_compose_left.  hot_evaluate<.., BASE_FOLDED = true>
// takes oM0 where the default form takes oMt; e and the columns see P_0^-1 oMt rounded once, so the two forms differ by rounding.
// Applied where a lane takes a target (hot_dls at entry, the refill loop's hook), never per iteration.
template <class S, class Tab>
IKD_FN void hot_fold_base(const Tab &t, const double (&oMt)[12], double (&oM0)[12]) {
    double c[9], dp[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = hot_rot<S, 0>(t, k);
#pragma unroll
    for (int k = 0; k < 3; ++k) dp[k] = S::tnz(0, k) ? oMt[9 + k] - t.v[S::trans_at(0, k)] : oMt[9 + k];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) oM0[3 * i + j] = dfma(c[i], oMt[j], dfma(c[3 + i], oMt[3 + j], c[6 + i] * oMt[6 + j]));
        oM0[9 + i] = dfma(c[i], dp[0], dfma(c[3 + i], dp[1], c[6 + i] * dp[2]));
    }
}

// e = log6(fMt) (6) and the NEGATED task Jacobian columns col[j] = Jlog6(tMf) J_local(:, j) at q (KT_FULL, unit weights; the
// reference defines J = -Jlog6 J_local with the frame Jacobian in the LOCAL frame, ik/ik/frame.hpp:162-166).  oMt: target placement
// in the world.  The chain oMf = P_0 Rz(q_0) P_1 Rz(q_1) ... P_{NJ-1} Rz(q_{NJ-1}) P_NJ is walked from the TIP to the base: the running
// Y = (R, p) = [Rz(q_j)] P_{j+1} ... P_NJ maps task-frame coordinates into joint j's frame, so joint j's column of J_local is read off
// it directly -- the unit twist about z carried to the task frame by Y^-1:  angular part R^T e_z, the third row of R;  linear part
// R^T (e_z x p).  (chain_solver.hpp walks base to tip in the world frame and then rotates everything into the task frame: there the
// frame rotation is folded into both Jlog6 blocks, 54 multiply-adds, and every column pays org_j - p and a full cross product.)
// INVARIANT hot_gram and hot_step rely on: inside a run of identity-rotation placements (S::leader) the angular parts ang[j], and so
// col[j][3..5], are the SAME values for every member -- rot_z_left leaves row 2 of R alone and an identity Rc folds away in
// hot_compose_left, so the members read the same registers.
// FOLDED RUNS (ChainRuns::folded, runs of at least kHotFoldMinRun joints).  Between the members of a run the placements are pure
// translations, so the walk stays in the frame it entered the run with and Y is materialised once, at the run's leader:
//  * rows 0 and 1 of R at the run's entry, r0 and r1, serve every member the way row 2 does -- R is simply not touched until the
//    leader; ang[j] is still row 2 of R, the very same registers for every member, and the invariant above holds unchanged;
//  * the running translation is kept in the entry frame, p~ = Rz(-phi_j) p with phi_j the SUM of the run's angles from its tip-side
//    member down to j, and is what differs from member to member:  lin_j = R^T (e_z x p) = p~0 r1 - p~1 r0;  joint j's own rotation
//    leaves p~ alone and its translation enters as p~ += Rz(-phi_j) t_j -- two multiply-adds per non-zero in-plane component, one
//    addition along the axis; a member without in-plane translation needs no sin / cos at all;
//  * A lin_j = p~0 (A r1) - p~1 (A r0): the two products are formed once per run and lin_j itself never;
//  * at the leader (R, p) <- P_L Rz(phi_L) (R, p~): the same rot_z_left and hot_compose_left as for a lone joint.
// The step, the joint limits and q stay per joint (hot_step); only sin and cos take phi_j.  Argument of dsincos_lut: its one-word
// reduction by 2 pi leaves an error of 3.9e-17 |x|.  Every joint of a chain problem is a bounded revolute (continuous joints go to
// the generic kernel) and q is clipped to its limits after every step, so from the second evaluation on |phi_j| <= the sum of the
// run's max(|lo|, |hi|).  Nothing bounds a URDF's limits (or the caller's q0, which the first evaluation sees unclipped), so this is
// no guarantee, only the scale of the error: under the ASSUMPTION of at most a full turn either way per joint a whole chain of seven
// reaches 44 rad and 1.7e-15, below the 2e-15 of the kernels, which holds up to |phi| = 51 rad; limits of +-100 rad on a run of seven
// give |phi| = 700 and 2.7e-14.  The folded form's error thus grows with the run's SUM where the unfolded one grew with each joint's own
// angle.  The second word of 2 pi (dsincos_fast) would not change that: phi_j is a rounded sum, each of its additions is off by up to
// half an ulp of |phi| (5.5e-17 .. 1.1e-16 |phi|), more than the dropped word's 3.9e-17 |phi|.  So the one-word reduction stays.
// (The bounds above were written for dsincos_hot's 2e-15; dsincos_lut has the same reduction and 3.4e-16 of its own, lane_math.hpp.)
// BASE_FOLDED: oMt is hot_fold_base's P_0^-1 oMt and joint 0 -- alone or as the leader of a folded run -- ends the walk with its own
// rotation, no hot_compose_left<S, 0>.  The columns are read off Y before that composition either way: the same expressions.
template <int NJ, class S, bool BASE_FOLDED = false, class Tab>
IKD_FN void hot_evaluate(const Tab &t, const double (&q)[NJ], const double (&oMt)[12], double (&e)[6], double (&col)[NJ][6]) {
    constexpr typename ChainRuns<S, NJ>::Table kRuns = ChainRuns<S, NJ>::value;
    // the NJ sin / cos first: independent of the chain.  A member of a folded run takes phi_j.
    double phi[NJ], sn[NJ], cs[NJ];
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) phi[j] = (kRuns.folded[j] && !kRuns.tip[j]) ? phi[j + 1 < NJ ? j + 1 : j] + q[j] : q[j];
    hot_sincos<NJ, S::kPrismatic>(t, phi, sn, cs);

    double ang[NJ][3], lin[NJ][3];
    double rows[NJ][6], pt[NJ][2];   // folded runs: rows 0 and 1 of R at the run's entry (by leader), p~0 and p~1 (by member)
    double R[9], p[3];
    // placement NJ: last joint frame -> task frame
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = hot_rot<S, NJ>(t, k);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = S::tnz(NJ, k) ? t.v[S::trans_at(NJ, k)] : 0.0;

    // A chain with more than kHotTableVgprMax placement values has its table parked in accumulation registers (hot_park_table: more
    // values than the vector registers hold).  The rotation of Y and its translation are two independent dependency chains, and the compiler was seen to
    // run the translation chain a few hundred instructions after the rotation chain -- fetching every entry of every Rc twice
    // (arm7: 338 v_accvgpr_read per iteration instead of 220).  Pinning p and one entry of R after each joint keeps the two together.
    // Not for the structural chains: their table stays in vector registers, and a pin keeps a literal entry from folding.
    constexpr bool kPinWalk = S::offset(NJ + 1) > kHotTableVgprMax;
    // joint J: its local column from Y (the same before and after the joint's own rotation), then Y <- P_J Rz(q_J) Y
#define IKD_HOT_JOINT(J)                                                                                   \
    if (J < NJ) {                                                                                          \
        constexpr int jj = J < NJ ? J : 0;                                                                 \
        ang[jj][0] = R[6]; ang[jj][1] = R[7]; ang[jj][2] = R[8];                                           \
        if (kRuns.prismatic[jj]) {                                                                         \
            /* the unit translation along z carried to the task frame: linear part R^T e_z, no angular part (the column loop    \
               below never reads ang of a prismatic joint); then Y <- P_J Trans_z(q_J) Y */                \
            lin[jj][0] = R[6]; lin[jj][1] = R[7]; lin[jj][2] = R[8];                                       \
            p[2] += q[jj];                                                                                 \
            if (!(BASE_FOLDED && jj == 0)) hot_compose_left<S, jj>(R, p, t);                               \
            if (kPinWalk) { IKD_PIN(p[0]); IKD_PIN(p[1]); IKD_PIN(p[2]); IKD_PIN(R[0]); }                  \
        } else if (!kRuns.folded[jj]) {                                                                    \
            lin[jj][0] = dfma(p[0], R[3], -(p[1] * R[0]));                                                 \
            lin[jj][1] = dfma(p[0], R[4], -(p[1] * R[1]));                                                 \
            lin[jj][2] = dfma(p[0], R[5], -(p[1] * R[2]));                                                 \
            rot_z_left(R, p, sn[jj], cs[jj]);                                                              \
            if (!(BASE_FOLDED && jj == 0)) hot_compose_left<S, jj>(R, p, t);                               \
            if (kPinWalk) { IKD_PIN(p[0]); IKD_PIN(p[1]); IKD_PIN(p[2]); IKD_PIN(R[0]); }                  \
        } else {                                                                                           \
            /* (R, p) = (R at the run's entry, p~): A lin_j = p~0 (A r1) - p~1 (A r0) once A is known */   \
            pt[jj][0] = p[0]; pt[jj][1] = p[1];                                                            \
            if (kRuns.leader[jj] != jj) {                                                                  \
                /* p~ += Rz(-phi_j) t_j: the member's placement is a pure translation */                   \
                if (S::tnz(jj, 0)) {                                                                       \
                    const double t0 = t.v[S::trans_at(jj, 0)];                                             \
                    p[0] = dfma(cs[jj], t0, p[0]); p[1] = dfma(-sn[jj], t0, p[1]);                         \
                }                                                                                          \
                if (S::tnz(jj, 1)) {                                                                       \
                    const double t1 = t.v[S::trans_at(jj, 1)];                                             \
                    p[0] = dfma(sn[jj], t1, p[0]); p[1] = dfma(cs[jj], t1, p[1]);                          \
                }                                                                                          \
                if (S::tnz(jj, 2)) p[2] += t.v[S::trans_at(jj, 2)];                                        \
            } else {                                                                                       \
                /* the leader: Y is materialised, (R, p) <- P_L Rz(phi_L) (R, p~) */                       \
                _Pragma("unroll") for (int k = 0; k < 6; ++k) rows[jj][k] = R[k];                          \
                rot_z_left(R, p, sn[jj], cs[jj]);                                                          \
                if (!(BASE_FOLDED && jj == 0)) hot_compose_left<S, jj>(R, p, t);                           \
                if (kPinWalk) { IKD_PIN(p[0]); IKD_PIN(p[1]); IKD_PIN(p[2]); IKD_PIN(R[0]); }              \
            }                                                                                              \
        }                                                                                                  \
    }
    IKD_HOT_JOINT(6) IKD_HOT_JOINT(5) IKD_HOT_JOINT(4) IKD_HOT_JOINT(3) IKD_HOT_JOINT(2) IKD_HOT_JOINT(1) IKD_HOT_JOINT(0)
#undef IKD_HOT_JOINT

    // In a folded run R does not depend on the members' own sin / cos -- only p~ does -- and the compiler was seen to sink those past
    // the branch inside log6, away from the others: the two polynomial constants that each sin / cos takes through a vector register
    // (v_mov_b64, 8 cycles of issue each) were then copied twice per iteration (Cassie leg: 5 v_mov_b64 in the loop, with the pin 3,
    // the unfolded loop's own; the leader's rows[][] = R[] is a copy in the source only: R is not written inside a run, and the
    // built kernels hold r0, r1 in the registers R had -- a fact of the listings, tools/kernel_stats.py, not of the source).  A folded member needs no kPinWalk pin: it has no rotation chain for p to drift away from (the
    // all-general 7-joint chain with three of its placements made identity: the same listing with and without).
    if (kRuns.any_folded) { IKD_PIN(p[0]); IKD_PIN(p[1]); }
    // (R, p) = oMf;  fMt = oMf^-1 oMt
    double Re[9], pe[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Re[3 * i + j] = dfma(R[i], oMt[j], dfma(R[3 + i], oMt[3 + j], R[6 + i] * oMt[6 + j]));
    {
        const double dp[3] = {oMt[9] - p[0], oMt[10] - p[1], oMt[11] - p[2]};
        rotT_vec(R, dp, pe);
    }
    LogAndJlog lj;
    double Cm[9];
    log6_and_jlog6_hot<false, true>(Re, pe, lj, &Cm);
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = lj.e[i];

    // folded runs: A r0 and A r1, once per run
    double Ar0[NJ][3], Ar1[NJ][3];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (kRuns.folded[j] && kRuns.leader[j] == j) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Ar0[j][i] = dfma(lj.A[3 * i], rows[j][0], dfma(lj.A[3 * i + 1], rows[j][1], lj.A[3 * i + 2] * rows[j][2]));
                Ar1[j][i] = dfma(lj.A[3 * i], rows[j][3], dfma(lj.A[3 * i + 1], rows[j][4], lj.A[3 * i + 2] * rows[j][5]));
            }
        }

    // Jlog6(tMf) = [A  C A; 0  A] on the local columns [lin_j; ang_j]:  beta_j = A ang_j (shared by a run of parallel joints),
    // top = A lin_j + C beta_j.  The product C A is never formed.  In a folded run A lin_j = p~0 (A r1) - p~1 (A r0).
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (kRuns.prismatic[j]) {   // [A lin_j ; 0]: beta_j = 0, written as the literal
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                col[j][i] = dfma(lj.A[3 * i], lin[j][0], dfma(lj.A[3 * i + 1], lin[j][1], lj.A[3 * i + 2] * lin[j][2]));
                col[j][3 + i] = 0.0;
            }
            continue;
        }
        double beta[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) beta[i] = dfma(lj.A[3 * i], ang[j][0], dfma(lj.A[3 * i + 1], ang[j][1], lj.A[3 * i + 2] * ang[j][2]));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            // the beta terms first: consecutive joints with parallel axes share them
            const double cb = dfma(Cm[3 * i], beta[0], dfma(Cm[3 * i + 1], beta[1], Cm[3 * i + 2] * beta[2]));
            if (!kRuns.folded[j])
            col[j][i] = dfma(lj.A[3 * i], lin[j][0], dfma(lj.A[3 * i + 1], lin[j][1], dfma(lj.A[3 * i + 2], lin[j][2], cb)));
            else
                col[j][i] = dfma(pt[j][0], Ar1[kRuns.leader[j]][i], dfma(-pt[j][1], Ar0[kRuns.leader[j]][i], cb));
            col[j][3 + i] = beta[i];
        }
    }
}

// Gram matrix G = J J^T + lam2 I (lower triangle) from the negated task Jacobian columns.
template <int NJ, class S>
IKD_FN void hot_gram(const double (&col)[NJ][6], double lam2, double (&G)[36]) {
    constexpr int M = 6;
    constexpr typename ChainRuns<S, NJ>::Table kRuns = ChainRuns<S, NJ>::value;
            // Gram matrix.  Joints of one run of parallel axes (S::leader) share their bottom (angular) rows: col[j][3..5] = A ang_j is
            // the same vector for all of them (hot_evaluate's invariant), so  sum_j col[j][3+a] col[j][3+b] = n c_a c_b  and  sum_j col[j][3+a] col[j][b] =
            // c_a (sum_j col[j][b])  within a run -- 102 instead of 147 multiply-adds for a Cassie leg (runs of 1, 1 and 5 joints).
                    double top_sum[NJ][3], nbot[NJ][3];
    #pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (kRuns.leader[j] == j) {
    #pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        top_sum[j][b] = col[j][b];
                        nbot[j][b] = kRuns.members[j] > 1 ? static_cast<double>(kRuns.members[j]) * col[j][3 + b] : col[j][3 + b];
                    }
                } else {
    #pragma unroll
                    for (int b = 0; b < 3; ++b) top_sum[kRuns.leader[j]][b] += col[j][b];
                }
            }
    #pragma unroll
            for (int a = 0; a < 3; ++a)
    #pragma unroll
                for (int b = 0; b <= a; ++b) {
                    double s = (a == b) ? lam2 : 0.0;
    #pragma unroll
                    for (int j = 0; j < NJ; ++j) s = dfma(col[j][a], col[j][b], s);
                    G[a * M + b] = s;
                }
    #pragma unroll
            for (int a = 3; a < 6; ++a) {
    #pragma unroll
                for (int b = 0; b < 3; ++b) {
                    double s = 0.0;
    #pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        if (kRuns.leader[j] == j && !kRuns.prismatic[j]) s = dfma(col[j][a], top_sum[j][b], s);   // (a prismatic column has no angular rows)
                    G[a * M + b] = s;
                }
    #pragma unroll
                for (int b = 3; b <= a; ++b) {
                    double s = (a == b) ? lam2 : 0.0;
    #pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        if (kRuns.leader[j] == j && !kRuns.prismatic[j]) s = dfma(nbot[j][a - 3], col[j][b], s);
                    G[a * M + b] = s;
                }
            }
}

// q <- clip(q + step_length dq), dq = -J^T y = +col^T y (reference ik/ik/dls.cpp:52-53,67-71) where `take`; q stays elsewhere.
template <int NJ, class S, class Tab>
IKD_FN void hot_step(const Tab &t, const LoopParams &prm, const double (&col)[NJ][6], const double (&y)[6], double (&q)[NJ], bool take) {
    constexpr int kLim = S::offset(NJ + 1);  // lo[NJ], hi[NJ] follow the placement values
    constexpr typename ChainRuns<S, NJ>::Table kRuns = ChainRuns<S, NJ>::value;
    double ang[NJ];   // the angular part of col_j^T y, shared by a run of parallel axes
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (kRuns.leader[j] == j && !kRuns.prismatic[j]) ang[j] = dfma(col[j][3], y[3], dfma(col[j][4], y[4], col[j][5] * y[5]));
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        double s = kRuns.prismatic[j] ? 0.0 : ang[kRuns.leader[j]];
#pragma unroll
        for (int a = 0; a < 3; ++a) s = dfma(col[j][a], y[a], s);
        const double qn = dfma(prm.step_length, s, q[j]);  // dq_j = -J_task(:, j)^T y = +col_j^T y
        const double qc = dmin(t.v[kLim + NJ + j], dmax(qn, t.v[kLim + j]));
        q[j] = take ? qc : q[j];
    }
}

// One full solve.  q: in = q0 (chain joints), out = result.  oMt: the target in the world; it is carried into joint 0's frame once, at
// entry, and every iteration evaluates in the BASE_FOLDED form.  NEVERSTOP: the visitor never stops (stop_sq_tol < 0): every
// lane takes exactly max_iterations steps.  active: false for a lane that takes no part in this solve (chain_solver.hpp chain_dls).
template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn>
IKD_FN void hot_dls(const Tab &t, const LoopParams &prm, double (&q)[NJ], const double (&oMt)[12], int &iters_out,
                    bool &success_out, AnyFn any_active, bool active = true) {
    constexpr int M = 6;
    bool success = false;
    int iters = prm.max_iterations;
    double oM0[12];   // the target in joint 0's frame: P_0 leaves the loop (hot_fold_base)
    hot_fold_base<S>(t, oMt, oM0);
#pragma unroll 1
    for (int it = 0; it < prm.max_iterations; ++it) {
        double e[M], col[NJ][M];
        hot_evaluate<NJ, S, true>(t, q, oM0, e, col);

        double G[M * M];
        hot_gram<NJ, S>(col, prm.lam2, G);
        double y[M];
        ldlt_solve<M>(G, e, y);

        if (!NEVERSTOP) {
            double e0sq = 0.0;
            if (prm.priority == 0) {
#pragma unroll
                for (int a = 0; a < M; ++a) e0sq = dfma(e[a], e[a], e0sq);
            }
            const bool stop_now = active && (prm.stop_sq_tol >= 0.0) && (e0sq < prm.stop_sq_tol);
            if (stop_now) { success = true; iters = it; }
            active = active && !stop_now;
        }
        hot_step<NJ, S>(t, prm, col, y, q, NEVERSTOP || active);
        if (!NEVERSTOP && !any_active(active)) break;
    }
    iters_out = (NEVERSTOP || success) ? iters : iterations_taken(any_active, prm.max_iterations);   // (chain_solver.hpp chain_dls)
    success_out = success;
}

// Entries of q outside the task support: dq = 0 there, so the loop only ever clips them to the limits (reference
// ik/ik/dls.cpp:71 clips the whole q after each step; no step is taken when the solve stops at iteration 0).
// With the plan of the kernel arguments (chain_kernel_body.hpp PassPlan) which entries they are and their limits are wave-uniform
// values of the argument segment: the per-lane loads of all of them are issued together (pass_plan_issue), then clamped and stored
// (pass_plan_finish) -- one trip to memory.  hot_chain_body and hot_track_body issue the loads of their first never-stop solve
// themselves, beside the ones of q0, the target and the sin / cos table.
// Without a plan: sixteen entries at a time over the problem's tables in HBM, the loads of a group ahead of its first store (one entry
// per pass -- load, wait, store; the next load cannot move above a store that might alias it -- cost one HBM round trip per entry).
// The tables may alias q_out as far as the compiler knows, so their reads are VECTOR loads at wave-uniform addresses, and
// `&& !a.q_in_chain[i]` is a branch per entry with a wait on its flag in front: the group's per-lane loads leave only behind the last
// of those waits (a listing of the never-stop NJ = 7 kernel: fifteen dependent round trips, then one more for the loads).
template <int NJ>
IKD_FN void hot_pass_through_from(const ChainKernelArgs<NJ> &a, const double *q_src, double *q_out, int64_t b, bool stepped) {
    const ChainStrides st = chain_strides(a);
    if (a.pass.state != 0) {
        PassStage s;
        pass_plan_issue(a, st, q_src, b, s);
        pass_plan_finish(a, st, s, q_out, b, stepped);
        return;
    }
    constexpr int kGroup = 16;   // (a Cassie model's sixteen entries in ONE pass: with groups of eight the second group's loads waited
                                 // for the first group's stores -- a second HBM round trip in the prologue)
    for (int i0 = 0; i0 < a.nq; i0 += kGroup) {
        double v[kGroup], lo[kGroup], hi[kGroup];
        bool out[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const int i = i0 + k < a.nq ? i0 + k : a.nq - 1;
            out[k] = i0 + k < a.nq && !a.q_in_chain[i];
            lo[k] = a.lower[i];
            hi[k] = a.upper[i];
        }
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const int i = i0 + k < a.nq ? i0 + k : a.nq - 1;
            v[k] = q_src[at(st.elem, st.q_prob, i, b)];
        }
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const double c = dmin(hi[k], dmax(v[k], lo[k]));
            if (out[k]) q_out[at(st.elem, st.q_prob, i0 + k, b)] = stepped ? c : v[k];
        }
    }
}
template <int NJ>
IKD_FN void hot_pass_through_to(const ChainKernelArgs<NJ> &a, double *q_out, int64_t b, bool stepped) { hot_pass_through_from(a, a.q0, q_out, b, stepped); }
template <int NJ>
IKD_FN void hot_pass_through(const ChainKernelArgs<NJ> &a, int64_t b, bool stepped) { hot_pass_through_to(a, a.q_out, b, stepped); }

#if IKD_HIP_LANG
// The hot program under lane refill (chain_kernel_body.hpp chain_refill_loop): the stop-rule mode for batches larger than the machine.
template <int NJ, class S, class Tab>
__device__ __forceinline__ void hot_refill_body(const ChainKernelArgs<NJ> &a, const Tab &t, unsigned long long *queue, int chunk) {
    // The sin / cos table is filled by the loop's stage hook: only by a wave that has work (with every problem stopped in the first
    // phase the whole grid leaves at once, and a fill there would be the launch's entire cost), its loads in flight beside the first
    // round's q and target loads as in hot_chain_body.
    struct Stage {
        const Tab &t;
        decltype(hot_lut_issue(t)) st;
        __device__ __forceinline__ void issue() { st = hot_lut_issue(t); }
        __device__ __forceinline__ void commit() { hot_lut_commit(t, st); }
    };
    // (the loop's oMt holds P_0^-1 oMt: folded by the hook below where a lane takes a target, as hot_dls folds at entry -- the same bits)
    chain_refill_loop<NJ>(a, queue, chunk, [&](double (&q)[NJ], const double (&oMt)[12], bool have) {
        constexpr int M = 6;
        double e[M], col[NJ][M];
        hot_evaluate<NJ, S, true>(t, q, oMt, e, col);
        double G[M * M];
        hot_gram<NJ, S>(col, a.prm.lam2, G);
        double y[M];
        ldlt_solve<M>(G, e, y);
        double e0sq = 0.0;
        if (a.prm.priority == 0) {
#pragma unroll
            for (int k = 0; k < M; ++k) e0sq = dfma(e[k], e[k], e0sq);
        }
        const bool stop_now = have && (a.prm.stop_sq_tol >= 0.0) && (e0sq < a.prm.stop_sq_tol);
        hot_step<NJ, S>(t, a.prm, col, y, q, !stop_now);
        return stop_now;
    }, [&](double (&oMt)[12]) {
        double w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = oMt[k];
        hot_fold_base<S>(t, w, oMt);
    }, Stage{t, {}});
}
#endif

// B independent ik::dls() calls, lane `gid`: load, solve, store -- dls_chain_body (chain_kernel_body.hpp) with the hot program.
// wave_start: the measurement build's stamp of the kernel's first instruction (hot_kernel_entry); unused otherwise.
template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn>
IKD_FN void hot_chain_body(const ChainKernelArgs<NJ> &a, const Tab &t, int64_t gid, AnyFn any_active, long long wave_start = 0) {
    const ChainStrides st = chain_strides(a);
#if defined(IKGPU_HOT_STAMP) && IKD_ON_DEVICE
    const long long rs = wave_start;   // wave start, 100 MHz ticks
#endif
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const auto lut_stage = hot_lut_issue(t);   // the sin / cos table's loads travel with the ones of q0 and the target (hot_lut_issue)
    double q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(st.elem, st.q_prob, a.qidx[j], b)];
    // (load_target in its two halves, the same expressions: the raw loads leave ahead of the plan's scalar reads)
    double raw[12], oMt[12];
    load_target_raw(a, a.targets, b, raw);
    // never-stop, with a plan: the loads of the entries outside the chain travel with them too -- the prologue's one trip to memory
    const bool planned = NEVERSTOP && a.pass.state != 0;
    PassStage pass_stage;
    if (NEVERSTOP) pass_plan_issue<true>(a, st, a.q0, b, pass_stage);   // (no branch among the prologue's loads: pass_plan_issue)
    compose_target(a, raw, oMt);
    hot_lut_commit(t, lut_stage);
    if (NEVERSTOP) pass_plan_settle(pass_stage);
    // The visitor never stops: every lane takes max_iterations steps, so what happens to the entries outside the support is
    // known before the loop -- copy them now (the stores drain while the loop runs) instead of after it (4 us of epilogue).
    if (NEVERSTOP && valid) {
        if (planned) pass_plan_finish(a, st, pass_stage, a.q_out, b, a.prm.max_iterations > 0);
        else hot_pass_through(a, b, a.prm.max_iterations > 0);
    }
    int iters;
    bool success;
#if defined(IKGPU_HOT_STAMP) && IKD_ON_DEVICE
    // measurement build (tools/build_variant.sh stamp -DIKGPU_HOT_STAMP): lanes 0 / 1 of every wave return the iteration loop's
    // duration in shader clocks (s_memtime) and in 100 MHz ticks (s_memrealtime) through `iters`
    const long long c0 = __builtin_readcyclecounter(), r0 = wall_clock64();
#endif
    hot_dls<NJ, S, NEVERSTOP>(t, a.prm, q, oMt, iters, success, any_active);
#if defined(IKGPU_HOT_STAMP) && IKD_ON_DEVICE
    const long long c1 = __builtin_readcyclecounter(), r1 = wall_clock64();
    const int stamp_loop_cycles = static_cast<int>(c1 - c0), stamp_loop_ticks = static_cast<int>(r1 - r0);
    const int stamp_pre_ticks = static_cast<int>(r0 - rs);
    const int stamp_true_iters = iters;
#endif
    if (!NEVERSTOP && a.append_count)   // (first phase of a two-phase solve)
        append_unfinished(a.append_list, a.append_count, valid && !success && iters < a.prm.max_iterations, b);
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) a.q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
    if (!NEVERSTOP) hot_pass_through(a, b, iters > 0);
    if (a.success) a.success[b] = success ? 1 : 0;
#if defined(IKGPU_HOT_STAMP) && IKD_ON_DEVICE
    // lanes 0..5 of every wave: loop cycles, loop ticks, prologue ticks (wave start -> loop), epilogue ticks (loop end -> here,
    // the stores issued), absolute start and end ticks (low 31 bits)
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const long long re = wall_clock64();
        const int lane = threadIdx.x % 64;
        iters = lane == 0 ? stamp_loop_cycles : lane == 1 ? stamp_loop_ticks : lane == 2 ? stamp_pre_ticks
              : lane == 3 ? static_cast<int>(re - r1) : lane == 4 ? static_cast<int>(rs & 0x7fffffff)
              : lane == 5 ? static_cast<int>(re & 0x7fffffff) : stamp_true_iters;
    }
#endif
    if (a.iters) a.iters[b] = iters;
}

// T chained solves of lane `gid`'s problem with q in registers between them -- dls_chain_track_body (chain_kernel_body.hpp: the
// definition, the slab layout, the rule for the entries outside the chain) with the hot program.  The raw target of waypoint k + 1
// is in flight during the iteration loop of waypoint k and composed after it: twelve doubles parked, nothing of them in the loop.
template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn>
IKD_FN void hot_track_body(const ChainKernelArgs<NJ> &a, const Tab &t, int T, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B, t_slab = 12 * a.B;
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    double q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(st.elem, st.q_prob, a.qidx[j], b)];
    // (never-stop, with a plan: the first waypoint's loads of the entries outside the chain are issued here -- hot_chain_body; the later
    // waypoints load theirs again, in front of their loop)
    const bool planned = NEVERSTOP && a.pass.state != 0;
    PassStage pass_stage;
    if (NEVERSTOP) pass_plan_issue<true>(a, st, a.q0, b, pass_stage);
    // Order per waypoint: solve k, compose target k + 1 (its loads were issued before solve k began), store slab k, THEN issue the loads
    // of target k + 2.  The wait that consumes a prefetched target therefore never has a store of this waypoint in front of it (loads
    // and stores share one counter on gfx950: behind a store the wait would be for the store's acknowledgement, once per waypoint).
    double next[12], oMt[12];
    if (T > 0) {
        load_target_raw(a, a.targets, b, next);
        compose_target(a, next, oMt);
    }
    if (T > 1) load_target_raw(a, a.targets + t_slab, b, next);
    hot_lut_commit(t, lut_stage);
    if (NEVERSTOP) pass_plan_settle(pass_stage);
    bool stepped = NEVERSTOP && a.prm.max_iterations > 0;   // (never-stop: every waypoint takes max_iterations steps, known here)
    if (planned && valid && T > 0) pass_plan_finish(a, st, pass_stage, a.q_out, b, stepped);   // (ahead of the waypoint loop: the staged values end here)
    for (int k = 0; k < T; ++k) {
        double *q_out = a.q_out + k * q_slab;
        if (NEVERSTOP && valid && !(planned && k == 0)) hot_pass_through_to(a, q_out, b, stepped);   // the stores drain while the loop runs (hot_chain_body)
        int iters;
        bool success;
        hot_dls<NJ, S, NEVERSTOP>(t, a.prm, q, oMt, iters, success, any_active);   // (any_active by value: a fresh count per waypoint)
        stepped = stepped || iters > 0;
        if (k + 1 < T) compose_target(a, next, oMt);
        if (valid) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
            if (a.success) a.success[k * a.B + b] = success ? 1 : 0;
            if (a.iters) a.iters[k * a.B + b] = iters;
            if (!NEVERSTOP) hot_pass_through_to(a, q_out, b, stepped);
        }
        if (k + 2 < T) load_target_raw(a, a.targets + (k + 2) * t_slab, b, next);
    }
}

// A straight Cartesian line to one goal per problem -- dls_chain_line_body (chain_kernel_body.hpp: the definition, the lane's order of
// work, which slabs are written) with the hot program.  The start pose comes from the chain table in HBM (a.desc, the stage kernels'
// FK), not from the compact table: once per launch, and the bits of ikgpu_line_targets.  Between waypoints the lane parks q, the start
// pose, the rotation vector and the goal (27 doubles); nothing is loaded per waypoint, so no wait stands between two solves.
template <int NJ, class S, class Tab, class AnyFn>
IKD_FN int hot_line_body(const ChainKernelArgs<NJ> &a, const Tab &t, const LineArgs &la, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B;
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    double q[NJ], goal[12];
    line_load(a, b, q, goal);
    hot_lut_commit(t, lut_stage);
    LineStart ls;
    typedef const IKD_CONST_AS ChainDesc<NJ> ConstDesc;   // scalar loads from HBM, as the general chain kernels
    line_chain_start<S::kPrismatic != 0>(a, *(ConstDesc *)a.desc, q, goal, ls);
    bool alive = true, stepped = false;
    int reached = 0, k = 0;
    for (; k < la.T && IKD_ANY(alive); ++k) {
        double w[12], oMt[12];
        line_waypoint(ls, goal, k, la.T, w);
        compose_target(a, w, oMt);
        int iters;
        bool success;
        hot_dls<NJ, S, false>(t, a.prm, q, oMt, iters, success, any_active, alive);   // (any_active by value: a fresh count per waypoint)
        stepped = stepped || (alive && iters > 0);
        if (valid && alive) {
            double *q_out = a.q_out + k * q_slab;
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
            if (a.success) a.success[k * a.B + b] = success ? 1 : 0;
            if (a.iters) a.iters[k * a.B + b] = iters;
            hot_pass_through_to(a, q_out, b, stepped);
        }
        alive = alive && success;
        reached += alive ? 1 : 0;
    }
    if (valid && la.reached) la.reached[b] = reached;
    return k;
}

// A Cartesian path through P vias per problem with the joint-step rule -- dls_chain_path_body (chain_kernel_body.hpp: the definition, the
// met rule, the lane's order of work, which slabs are written) with the hot program.  Between waypoints the lane parks q and q_prev
// (2 NJ doubles), the segment's start pose, its rotation vector and the current via (27 doubles); via s + 1 (twelve more) is in flight
// during the last solve of segment s only and consumed right after it, in front of that waypoint's stores.
template <int NJ, class S, class Tab, class AnyFn>
IKD_FN int hot_path_body(const ChainKernelArgs<NJ> &a, const Tab &t, const PathArgs &pa, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B, t_slab = 12 * a.B;
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    double q[NJ], q_prev[NJ], via[12], next[12];
    line_load(a, b, q, via);
    hot_lut_commit(t, lut_stage);
    LineStart ls;
    typedef const IKD_CONST_AS ChainDesc<NJ> ConstDesc;   // scalar loads from HBM, as the general chain kernels
    line_chain_start<S::kPrismatic != 0>(a, *(ConstDesc *)a.desc, q, via, ls);
    bool alive = true, stepped = false;
    int reached = 0;
    int64_t n = 0;
    for (int s = 0; s < pa.P && IKD_ANY(alive); ++s) {
        for (int k = 0; k < pa.T && IKD_ANY(alive); ++k, ++n) {
            double w[12], oMt[12];
            line_waypoint(ls, via, k, pa.T, w);
            compose_target(a, w, oMt);
            const bool turn = k + 1 == pa.T && s + 1 < pa.P;   // the last waypoint of a segment that has a successor
            if (turn) load_target_raw(a, a.targets + (s + 1) * t_slab, b, next);
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_prev[j] = q[j];
            int iters;
            bool success;
            hot_dls<NJ, S, false>(t, a.prm, q, oMt, iters, success, any_active, alive);   // (any_active by value: a fresh count per waypoint)
            if (turn) {
                line_start_from_pose(via, next, ls);
#pragma unroll
                for (int c = 0; c < 12; ++c) via[c] = next[c];
            }
            stepped = stepped || (alive && iters > 0);
            if (valid && alive) {
                double *q_out = a.q_out + n * q_slab;
#pragma unroll
                for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
                if (a.success) a.success[n * a.B + b] = success ? 1 : 0;
                if (a.iters) a.iters[n * a.B + b] = iters;
                hot_pass_through_to(a, q_out, b, stepped);
            }
            alive = alive && success && !path_jumped<NJ>(q, q_prev, pa.max_joint_step);
            reached += alive ? 1 : 0;
        }
    }
    if (valid && pa.reached) pa.reached[b] = reached;
    return static_cast<int>(n);
}

// K starts per problem, the best one stored -- dls_chain_multistart_body (chain_kernel_body.hpp: the definition, the lane mapping, the
// three pieces) with the hot program: the unchanged hot_dls, then one more hot_evaluate at its result for the error alone (its Jacobian
// columns are dead code).
template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn>
IKD_FN void hot_multistart_lane(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, const Tab &t, int64_t b, int k, double (&q)[NJ],
                                bool &success, int &iters, double &err_sq, AnyFn any_active) {
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    multistart_load(a, ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    hot_lut_commit(t, lut_stage);
    hot_dls<NJ, S, NEVERSTOP>(t, a.prm, q, oMt, iters, success, any_active);
    double e[6], col[NJ][6], oM0[12];
    hot_fold_base<S>(t, oMt, oM0);   // (hot_dls's own fold again: the same values, and P_0 stays out of the loop's live registers)
    hot_evaluate<NJ, S, true>(t, q, oM0, e, col);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) err_sq = dfma(e[r], e[r], err_sq);
}

template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn, class Exchange>
IKD_FN void hot_multistart_body(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, const Tab &t, int64_t gid, AnyFn any_active,
                                Exchange exchange) {
    const int64_t prob = gid >> ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters;
    hot_multistart_lane<NJ, S, NEVERSTOP>(a, ms, t, b, k, q, success, iters, err_sq, any_active);
    const int win = multistart_select(ms.log2K, multistart_key(success, err_sq), k, exchange);
    if (valid && win == k)
        multistart_store(a, ms, b, k, q, success, iters, err_sq,
                         [&](const double *src, bool stepped) { hot_pass_through_from(a, src, a.q_out, b, stepped); });
}

// K starts per problem, the converged one with the smallest cost stored -- dls_chain_pick_body (chain_kernel_body.hpp: the definition,
// the lane mapping, the pieces) with the hot program: hot_multistart_lane's statements, then the cost at the result; the trailing
// evaluation's Jacobian columns and hot_gram are live under the MANIPULABILITY rule alone.  Always under a stop rule.
template <int NJ, class S, class Tab, class AnyFn>
IKD_FN void hot_pick_lane(const ChainKernelArgs<NJ> &a, const PickArgs &pk, const Tab &t, int64_t b, int k, double (&q)[NJ], bool &success,
                          int &iters, double &err_sq, double &cost, AnyFn any_active) {
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    multistart_load(a, pk.ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    hot_lut_commit(t, lut_stage);
    hot_dls<NJ, S, false>(t, a.prm, q, oMt, iters, success, any_active);
    double e[6], col[NJ][6], oM0[12];
    hot_fold_base<S>(t, oMt, oM0);   // (hot_dls's own fold again: the same values, and P_0 stays out of the loop's live registers)
    hot_evaluate<NJ, S, true>(t, q, oM0, e, col);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) err_sq = dfma(e[r], e[r], err_sq);
    cost = pick_chain_cost<6>(a, pk, b, q, [&](double (&G)[36]) { hot_gram<NJ, S>(col, a.prm.lam2, G); });
}

template <int NJ, class S, class Tab, class AnyFn, class Exchange>
IKD_FN void hot_pick_body(const ChainKernelArgs<NJ> &a, const PickArgs &pk, const Tab &t, int64_t gid, AnyFn any_active, Exchange exchange) {
    const int64_t prob = gid >> pk.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << pk.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq, cost;
    bool success;
    int iters;
    hot_pick_lane<NJ, S>(a, pk, t, b, k, q, success, iters, err_sq, cost, any_active);
    const int win = multistart_select(pk.ms.log2K, pick_key(success, cost, err_sq), k, exchange);
    if (valid && win == k)
        pick_store(a, pk, b, k, q, success, iters, err_sq, cost,
                   [&](const double *src, bool stepped) { hot_pass_through_from(a, src, a.q_out, b, stepped); });
}

// K starts per problem, the one whose branch carries the path furthest stored -- dls_chain_path_multistart_body (chain_kernel_body.hpp:
// the definition, the lane mapping, the scout, the pieces) with the hot program: hot_multistart_lane against via 0, then path_scout with
// hot_path_body's start and solve.  The entry result (NJ doubles, iters, err_sq) waits in registers across the path loop.
template <int NJ, class S, class Tab, class AnyFn>
IKD_FN int hot_path_multistart_lane(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, const Tab &t, int64_t b, int k, double (&q)[NJ],
                                    bool &success, int &iters, double &err_sq, int &reached, AnyFn any_active) {
    hot_multistart_lane<NJ, S, false>(a, pm.ms, t, b, k, q, success, iters, err_sq, any_active);
    IKD_PIN(err_sq);   // (formed here, not sunk behind the path loop: dls_chain_path_multistart_lane)
    double qp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) qp[j] = q[j];
    typedef const IKD_CONST_AS ChainDesc<NJ> ConstDesc;   // scalar loads from HBM, as the general chain kernels
    const int n = path_scout(
        a, pm, b, qp, success, reached,
        [&](const double (&q0)[NJ], const double (&via)[12], LineStart &ls) { line_chain_start<S::kPrismatic != 0>(a, *(ConstDesc *)a.desc, q0, via, ls); },
        [&](double (&qw)[NJ], const double (&oMt)[12], int &it, bool &ok, bool alive) {
            hot_dls<NJ, S, false>(t, a.prm, qw, oMt, it, ok, any_active, alive);   // (any_active by value: a fresh count per waypoint)
        });
    reached = success ? reached : -1;
    return n;
}

template <int NJ, class S, class Tab, class AnyFn, class Exchange>
IKD_FN void hot_path_multistart_body(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, const Tab &t, int64_t gid, AnyFn any_active,
                                     Exchange exchange) {
    const int64_t prob = gid >> pm.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << pm.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters, reached;
    (void)hot_path_multistart_lane<NJ, S>(a, pm, t, b, k, q, success, iters, err_sq, reached, any_active);
    if (valid && pm.reached_all) pm.reached_all[static_cast<int64_t>(k) * a.B + b] = reached;
    const int win = multistart_select(pm.ms.log2K, path_multistart_key(pm, success, reached, err_sq), k, exchange);
    if (valid && win == k)
        path_multistart_store(a, pm, b, k, q, success, iters, err_sq, reached,
                              [&](const double *src, bool stepped) { hot_pass_through_from(a, src, a.q_out, b, stepped); });
}

// G goals and K starts per problem, the best candidate stored -- dls_chain_goalset_body (chain_kernel_body.hpp: the definition, the lane
// mapping, the pieces) with the hot program: hot_multistart_lane with the target taken from slab g of the goals.
template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn>
IKD_FN void hot_goalset_lane(const ChainKernelArgs<NJ> &a, const GoalsetArgs &ga, const Tab &t, int64_t b, int g, int k, double (&q)[NJ],
                             bool &success, int &iters, double &err_sq, AnyFn any_active) {
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    multistart_load(a, ga.ms, b, k, q);
    double raw[12], oMt[12];
    load_target_raw(a, a.targets + static_cast<int64_t>(g) * 12 * a.B, b, raw);
    compose_target(a, raw, oMt);
    hot_lut_commit(t, lut_stage);
    hot_dls<NJ, S, NEVERSTOP>(t, a.prm, q, oMt, iters, success, any_active);
    double e[6], col[NJ][6], oM0[12];
    hot_fold_base<S>(t, oMt, oM0);   // (hot_dls's own fold again: the same values, and P_0 stays out of the loop's live registers)
    hot_evaluate<NJ, S, true>(t, q, oM0, e, col);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) err_sq = dfma(e[r], e[r], err_sq);
}

template <int NJ, class S, bool NEVERSTOP, class Tab, class AnyFn, class Exchange, class Any>
IKD_FN void hot_goalset_body(const ChainKernelArgs<NJ> &a, const GoalsetArgs &ga, const Tab &t, int64_t gid, AnyFn any_active, Exchange exchange,
                             Any any) {
    const int log2J = ga.log2G + ga.ms.log2K;
    const int64_t prob = gid >> log2J;
    const int j = static_cast<int>(gid & ((int64_t{1} << log2J) - 1));
    const int g = j >> ga.ms.log2K, k = j & ((1 << ga.ms.log2K) - 1);
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters;
    hot_goalset_lane<NJ, S, NEVERSTOP>(a, ga, t, b, g, k, q, success, iters, err_sq, any_active);
    const int win = multistart_select(log2J, multistart_key(success, err_sq), j, exchange);
    const bool reached = any(ga.ms.log2K, success);
    if (!valid) return;
    if (ga.reachable && k == 0) ga.reachable[static_cast<int64_t>(g) * a.B + b] = reached ? 1 : 0;
    if (win == j)
        goalset_store(a, ga, b, g, k, q, success, iters, err_sq,
                      [&](const double *src, bool stepped) { hot_pass_through_from(a, src, a.q_out, b, stepped); });
}

// K starts per problem, the distinct converged ones stored -- dls_chain_solutions_body (chain_kernel_body.hpp: the definition, the lane
// mapping, the three pieces) with the hot program: the unchanged hot_dls, always under a stop rule (without one no start converges).
template <int NJ, class S, class Tab, class AnyFn>
IKD_FN void hot_solutions_lane(const ChainKernelArgs<NJ> &a, const SolutionsArgs &sa, const Tab &t, int64_t b, int k, double (&q)[NJ],
                               bool &success, int &iters, AnyFn any_active) {
    const auto lut_stage = hot_lut_issue(t);   // (hot_chain_body)
    multistart_load(a, sa.ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    hot_lut_commit(t, lut_stage);
    hot_dls<NJ, S, false>(t, a.prm, q, oMt, iters, success, any_active);
}

template <int NJ, class S, class Tab, class AnyFn, class Fetch>
IKD_FN void hot_solutions_body(const ChainKernelArgs<NJ> &a, const SolutionsArgs &sa, const Tab &t, int64_t gid, AnyFn any_active, Fetch fetch) {
    const int64_t prob = gid >> sa.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << sa.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ];
    bool success;
    int iters;
    hot_solutions_lane<NJ, S>(a, sa, t, b, k, q, success, iters, any_active);
    SolutionsLane s;
    solutions_select<NJ>(s, sa.ms.log2K, k, sa.N, sa.sep, success, q, fetch);
    if (!valid) return;
    if (s.kept)
        solutions_store(a, sa, b, k, s.slot, q, iters,
                        [&](const double *src, double *q_out, bool stepped) { hot_pass_through_from(a, src, q_out, b, stepped); });
    if (k == 0) sa.count[b] = s.cnt;
}

#if IKD_HIP_LANG
// ---- kernel entries, shared by the instantiations compiled into the library (kernels_hot.hip) and the ones compiled at run time for
// a chain's own structure code (rtc.cpp) -----------------------------------------------------------------------------------------
#ifndef IKGPU_HOT_PIN_LO
// the placement values are parked in vector registers, the joint limits stay in scalar registers (A/B on one box, B = 65536:
// everything in VGPRs 0.1440 ms -- 22 v_accvgpr_read per iteration --, limits in SGPRs 0.1417 ms)
#define IKGPU_HOT_PIN_LO 0
#define IKGPU_HOT_PIN_HI (S::offset(NJ + 1))
#endif

// The compact table (<= 36 doubles for the fixture shapes, see kHotTableVgprMax) arrives in the kernel-argument segment and is parked
// in vector registers for the whole loop: in scalar registers it competes with the ~40 polynomial constants for the 100 SGPRs (31 v_readlane
// + 39 s_mov of spill code per iteration in the round-1 kernel); a lone wave has 512 VGPRs to itself.
template <int NJ, class S>
__device__ __forceinline__ void hot_park_table(const HotTable &t, HotTable &tv) {
    constexpr int kUsed = S::offset(NJ + 1) + 2 * NJ;
    static_assert(kUsed <= kHotTableMax, "compact table too long");
#pragma unroll
    for (int k = 0; k < kHotTableMax; ++k) {
        tv.v[k] = k < kUsed ? t.v[k] : 0.0;
        if (k >= IKGPU_HOT_PIN_LO && k < kUsed && k < IKGPU_HOT_PIN_HI) IKD_PIN(tv.v[k]);
    }
}

template <int NJ, class S, bool NEVERSTOP>
__device__ __forceinline__ void hot_kernel_entry(const ChainKernelArgs<NJ> &a, const HotTable &t) {
#if defined(IKGPU_HOT_STAMP)
    // measurement build: the wave's first stamp, as early as the compiler lets it stand.  The workgroup index passes through the
    // statement, so every per-lane address -- every load from HBM -- comes after it; the kernel-argument loads do not depend on it and
    // the compiler issues the first batch of them ahead (the listing says how many instructions and waits stand in front).
    long long wave_start;
    unsigned block = blockIdx.x;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wave_start), "+s"(block) : : "memory");
#else
    const long long wave_start = 0;
    const unsigned block = blockIdx.x;
#endif
    const int64_t gid = static_cast<int64_t>(block) * 64 + threadIdx.x;   // one wave64 per workgroup
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_chain_body<NJ, S, NEVERSTOP>(a, tv, gid, KeepGoing{a.leave_active, a.leave_after, 0}, wave_start);
}

template <int NJ, class S, bool NEVERSTOP>
__device__ __forceinline__ void hot_track_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, int T) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_track_body<NJ, S, NEVERSTOP>(a, tv, T, gid, KeepGoing{0, 0, 0});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_line_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const LineArgs &la) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    (void)hot_line_body<NJ, S>(a, tv, la, gid, KeepGoing{0, 0, 0});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_path_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const PathArgs &pa) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    (void)hot_path_body<NJ, S>(a, tv, pa, gid, KeepGoing{0, 0, 0});
}

template <int NJ, class S, bool NEVERSTOP>
__device__ __forceinline__ void hot_multistart_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const MultistartArgs &ms) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup: 64 / K whole problems
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_multistart_body<NJ, S, NEVERSTOP>(a, ms, tv, gid, KeepGoing{0, 0, 0}, MultistartShuffle{});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_pick_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const PickArgs &pk) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup: 64 / K whole problems
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_pick_body<NJ, S>(a, pk, tv, gid, KeepGoing{0, 0, 0}, MultistartShuffle{});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_path_multistart_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const PathMultistartArgs &pm) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup: 64 / K whole problems
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_path_multistart_body<NJ, S>(a, pm, tv, gid, KeepGoing{0, 0, 0}, MultistartShuffle{});
}

template <int NJ, class S, bool NEVERSTOP>
__device__ __forceinline__ void hot_goalset_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const GoalsetArgs &ga) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup: 64 / (G x K) whole problems
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_goalset_body<NJ, S, NEVERSTOP>(a, ga, tv, gid, KeepGoing{0, 0, 0}, MultistartShuffle{}, GoalsetBallot{});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_solutions_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, const SolutionsArgs &sa) {
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;   // one wave64 per workgroup: 64 / K whole problems
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    const int lane = static_cast<int>(threadIdx.x) & 63;
    hot_solutions_body<NJ, S>(a, sa, tv, gid, KeepGoing{0, 0, 0}, SolutionsShuffle{lane & ~((1 << sa.ms.log2K) - 1)});
}

template <int NJ, class S>
__device__ __forceinline__ void hot_refill_entry(const ChainKernelArgs<NJ> &a, const HotTable &t, unsigned long long *queue, int chunk) {
    IKD_HOT_LUT_DECLARE(tv);
    hot_park_table<NJ, S>(t, tv);
    hot_refill_body<NJ, S>(a, tv, queue, chunk);
}
#endif

}  // namespace ikdev
