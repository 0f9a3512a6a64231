// chain_kernel_body.hpp -- what ONE lane of the chain kernels does around the lane solver:
// load its problem from HBM, solve, store.  Shared by the __global__ wrappers (kernels.hip) and
// by the CPU lane emulator under tests/ (which runs it in a plain loop over b).
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#include "chain_solver.hpp"
#include "goalset.hpp"
#include "line.hpp"
#include "multistart.hpp"
#include "pick.hpp"
#include "solutions.hpp"

namespace ikdev {

enum : int { LAYOUT_SOA = 0, LAYOUT_AOS = 1 };  // == ikgpu_layout

// The entries of q OUTSIDE the chain as a plan carried in the kernel arguments: which they are and their limits, made once on the host
// from the problem's own copies (kernels.hpp fill_pass_plan).  A body that finds one reads no flag and no limit from memory -- they are
// wave-uniform values of the argument segment -- and issues the per-lane loads of every planned entry together, ahead of the first
// store (pass_plan_issue / pass_plan_finish below).
//   state == 0      no plan: a value-initialised ChainKernelArgs (the emulators and shims under tests/, the CPU oracle's fast path), more
//                   than kPassPlanMax entries outside the chain, or IKGPU_PASS_PLAN=0.  The bodies walk q_in_chain / lower / upper.
//   state == n + 1  n entries outside the chain, idx ascending; n == 0 (a chain that takes every entry of q, UR5) stores nothing.
//                   Slots n .. kPassPlanMax - 1 repeat slot n - 1 (entry 0 when n == 0, as in a value-initialised plan), so a load
//                   of any slot reads a valid address.
// 328 bytes; ChainKernelArgs<7> is 680 bytes with it, ChainKernelArgs<6> 672 (352 / 344 without), and a hot kernel's argument
// segment with its 984-byte table 1664 / 1656 bytes of the 4096 a launch may pass.
constexpr int kPassPlanMax = 16;
struct PassPlan {
    int state;
    int idx[kPassPlanMax];
    double lo[kPassPlanMax], hi[kPassPlanMax];
};

template <int NJ>
struct ChainKernelArgs {
    const ChainDesc<NJ> *desc;  // HBM copy of the chain table (uploaded at problem creation)
    LoopParams prm;
    double ref_pl[12];          // world placement of the task's (world-fixed) reference frame
    int qidx[NJ];               // index of each chain joint in q
    int vidx[NJ];               // ... and in the tangent vector
    int nq, nv, layout;
    int64_t B;
    const double *q0;
    const double *targets;
    double *q_out;
    uint8_t *success;
    int32_t *iters;
    const double *lower, *upper;  // [nq]
    const uint8_t *q_in_chain;    // [nq]
    double *e_out, *J_out, *oMf_out;  // stage kernels
    // second phase of a two-phase stop-rule solve (kernels.hip two_phase_*): the refill kernel walks a LIST of problems -- those the
    // lock-step first phase left unfinished -- continuing each from its iterate in q_out at the iteration count the first phase left
    // in iters[].  Null: the whole batch.
    const int32_t *worklist;
    const unsigned long long *count;   // (device) length of the list
    // ... and of its first phase: a wave of the lock-step kernel LEAVES its loop once no more than `leave_active` of its lanes are still
    // iterating (and at least `leave_after` iterations are done; KeepGoing below) and appends the problems it leaves unfinished
    // (append_unfinished below).  leave_active == 0: an ordinary lock-step solve.
    int leave_active, leave_after;
    int32_t *append_list;
    unsigned long long *append_count;
    PassPlan pass;   // the entries of q outside the chain (above); last, so that a value-initialised struct has none
};

// First phase of a two-phase solve: the lanes of a wave whose problem is still open after the lock-step iterations append its index to
// the list -- one atomic per wave.  Called by EVERY lane of the wave (tail lanes with open = false).
IKD_FN void append_unfinished(int32_t *list, unsigned long long *count, bool open, int64_t b) {
#if IKD_ON_DEVICE
    const unsigned long long mask = __ballot(open);
    if (mask == 0ull) return;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    unsigned long long base = 0;
    if (lane == __ffsll(static_cast<long long>(mask)) - 1) base = atomicAdd(count, static_cast<unsigned long long>(__popcll(mask)));
    const int src = __ffsll(static_cast<long long>(mask)) - 1;
    const unsigned lo = __shfl(static_cast<unsigned>(base), src), hi = __shfl(static_cast<unsigned>(base >> 32), src);
    base = (static_cast<unsigned long long>(hi) << 32) | lo;
    if (open) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = static_cast<int32_t>(b);
#else
    if (open) list[(*count)++] = static_cast<int32_t>(b);
#endif
}

IKD_FN int64_t at(int layout, int64_t B, int ncomp, int c, int64_t b) {
    return layout == LAYOUT_SOA ? static_cast<int64_t>(c) * B + b : b * ncomp + c;
}

// The same place through two strides, for the chain bodies: the layout is resolved ONCE per body into an element stride and a problem
// stride (SOA: B and 1; AOS: 1 and the number of components -- nq for q0 / q_out / starts, 12 for the targets), and entry c of problem
// b is one multiply-add away.  at() above chooses per access, and on a wave-uniform layout hipcc made a scalar BRANCH of every such
// choice: ~180 conditional branches (45-60 cycles each for a lone wave when taken) and as many flow blocks with a wait in front in the
// prologue of the hot kernels.  The strides are derived here, on the device, from the `layout` the launchers have always filled in --
// not carried in the kernel arguments: the host-side lane emulators under tests/ fill ChainKernelArgs themselves.  They are made
// opaque to the optimiser (IKD_OPAQUE_S) so that it cannot fold the multiply back into the choice.
struct ChainStrides {
    int64_t elem, q_prob, t_prob;
};
#if IKD_ON_DEVICE
#define IKD_OPAQUE_S(x) asm("" : "+s"(x))   // (not volatile: two bodies inlined into one kernel may share the values)
#else
#define IKD_OPAQUE_S(x) ((void)0)
#endif
template <class Args>
IKD_FN ChainStrides chain_strides(const Args &a) {
    const bool soa = a.layout == LAYOUT_SOA;
    ChainStrides s{soa ? a.B : int64_t{1}, soa ? int64_t{1} : static_cast<int64_t>(a.nq), soa ? int64_t{1} : int64_t{12}};
    IKD_OPAQUE_S(s.elem);
    IKD_OPAQUE_S(s.q_prob);
    IKD_OPAQUE_S(s.t_prob);
    return s;
}
IKD_FN int64_t at(int64_t elem, int64_t prob, int c, int64_t b) { return static_cast<int64_t>(c) * elem + b * prob; }

// oMt = oMr * target (reference ik/ik/frame.hpp:48); oMr is constant for a world-fixed reference.
template <int NJ>
IKD_FN void load_target(const ChainKernelArgs<NJ> &a, int64_t b, double (&oMt)[12]) {
    const ChainStrides st = chain_strides(a);
    double t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = a.targets[at(st.elem, st.t_prob, k, b)];
    const double *r = a.ref_pl;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            oMt[3 * i + j] = dfma(r[3 * i], t[j], dfma(r[3 * i + 1], t[3 + j], r[3 * i + 2] * t[6 + j]));
        oMt[9 + i] = dfma(r[3 * i], t[9], dfma(r[3 * i + 1], t[10], dfma(r[3 * i + 2], t[11], r[9 + i])));
    }
}

// ---- the entries of q outside the chain -------------------------------------------------------------------------------------------
// dq = 0 there, so a solve only ever clips them to the limits (reference ik/ik/dls.cpp:71 clips the whole q after each step; no step is
// taken when the solve stops at iteration 0): q_out = stepped ? min(hi, max(v, lo)) : v.
// Through the plan (PassPlan above), in two halves so that a body can put other work between them: pass_plan_issue starts the per-lane
// loads of every planned entry of column b of `src` -- nothing between them waits, and a plan without entries loads nothing --,
// pass_plan_finish clamps and stores.  Both only with a plan (a.pass.state != 0).
// Every slot is clamped in one straight run ahead of the stores, the spare slots too (they hold a copy of the last entry: loaded and
// clamped with the others, never stored): the limits then come in by a few wide scalar loads, not by a pair per store with a wait each.
struct PassStage {
    double v[kPassPlanMax];
};
// ALWAYS: the loads are issued whatever the plan says (without entries every slot names entry 0, a valid address, and nothing of it
// is stored).  For a prologue that has other loads in flight: a branch here would end the block they are scheduled in, and where its
// two arms meet again every later wait is for the arm with fewer loads behind it -- on the other arm, for the plan's loads as well.
template <bool ALWAYS = false, int NJ>
IKD_FN void pass_plan_issue(const ChainKernelArgs<NJ> &a, const ChainStrides &st, const double *src, int64_t b, PassStage &s) {
    if (ALWAYS || a.pass.state > 1) {
#pragma unroll
        for (int k = 0; k < kPassPlanMax; ++k) s.v[k] = src[at(st.elem, st.q_prob, a.pass.idx[k], b)];
    }
}
// What a body that issued the loads ahead of other work calls in EVERY lane before its iteration loop: the loaded values are taken
// here, whatever the plan says and whether or not the lane stores.  A load still in flight at the loop's entry on some path (a tail
// lane, a plan without entries) costs the loop a wait of its own where its registers are first written.
IKD_FN void pass_plan_settle(PassStage &s) {
#pragma unroll
    for (int k = 0; k < kPassPlanMax; ++k) IKD_PIN(s.v[k]);
}
template <int NJ>
IKD_FN void pass_plan_finish(const ChainKernelArgs<NJ> &a, const ChainStrides &st, const PassStage &s, double *q_out, int64_t b, bool stepped) {
    const int n = a.pass.state - 1;
    if (n <= 0) return;
    double w[kPassPlanMax];
#pragma unroll
    for (int k = 0; k < kPassPlanMax; ++k) {
        double v = s.v[k];
        IKD_PIN(v);   // the clamp stays HERE: moved up to the loads it would put their wait in front of whatever a body issues behind them
        const double c = dmin(a.pass.hi[k], dmax(v, a.pass.lo[k]));
        w[k] = stepped ? c : v;
    }
#pragma unroll
    for (int k = 0; k < kPassPlanMax; ++k)
        if (k < n) q_out[at(st.elem, st.q_prob, a.pass.idx[k], b)] = w[k];   // (wave-uniform test)
}

// The entries outside the chain of a solve started from column b of `src`, into q_out (a slab of its own for the jobs that have several).
// With a plan every load is issued before the first store; without one, an entry per pass over the problem's tables in HBM.
template <int NJ>
IKD_FN void chain_pass_through_into(const ChainKernelArgs<NJ> &a, const double *src, double *q_out, int64_t b, bool stepped) {
    const ChainStrides st = chain_strides(a);
    if (a.pass.state != 0) {
        PassStage s;
        pass_plan_issue(a, st, src, b, s);
        pass_plan_finish(a, st, s, q_out, b, stepped);
        return;
    }
    for (int i = 0; i < a.nq; ++i) {
        if (a.q_in_chain[i]) continue;
        const double v = src[at(st.elem, st.q_prob, i, b)];
        const double c = dmin(a.upper[i], dmax(v, a.lower[i]));
        q_out[at(st.elem, st.q_prob, i, b)] = stepped ? c : v;
    }
}
template <int NJ>
IKD_FN void chain_pass_through_from(const ChainKernelArgs<NJ> &a, const double *src, int64_t b, bool stepped) {
    chain_pass_through_into(a, src, a.q_out, b, stepped);
}

// B independent ik::dls() calls (reference ik/ik/dls.cpp:5-78), lane `gid`.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_body(const ChainKernelArgs<NJ> &a, const Desc &d, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing

    double q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(st.elem, st.q_prob, a.qidx[j], b)];
    double oMt[12];
    load_target(a, b, oMt);

    int iters;
    bool success;
    chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);

    // (wave-uniform test; a problem that ran out of iterations is finished, not open)
    if (a.append_count) append_unfinished(a.append_list, a.append_count, valid && !success && iters < a.prm.max_iterations, b);
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) a.q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
    // Entries outside the task support: dq = 0 there, so the loop only ever clamps them
    // (reference ik/ik/dls.cpp:71 clips the whole q after each step; no step is taken when iters == 0).
    chain_pass_through_from(a, a.q0, b, iters > 0);
    if (a.success) a.success[b] = success ? 1 : 0;
    if (a.iters) a.iters[b] = iters;
}

// ---- tracking: a SEQUENCE of T targets per problem in one launch (include/ikgpu.h ikgpu_dls_track_batch) ---------------------------
// Defined as T calls of the single solve, each started from the result of the one before (the reference's caller does exactly that,
// ik_ros/src/cassie.cpp:92-113: q_ = ik::dls(*ik_, q_, ...) on every tick).  Waypoints are outermost: slab k of targets / q_out /
// success / iters is what the single solve takes, so `a` holds the pointers of slab 0 and the strides below lead to slab k.
// load_target in two halves, so that the twelve loads of a later waypoint can be in flight during the iteration loop of waypoint k and
// consumed after it: the same expressions, the same bits.
template <int NJ>
IKD_FN void load_target_raw(const ChainKernelArgs<NJ> &a, const double *targets, int64_t b, double (&t)[12]) {
    const ChainStrides st = chain_strides(a);
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = targets[at(st.elem, st.t_prob, k, b)];
}
template <int NJ>
IKD_FN void compose_target(const ChainKernelArgs<NJ> &a, const double (&t)[12], double (&oMt)[12]) {
    const double *r = a.ref_pl;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            oMt[3 * i + j] = dfma(r[3 * i], t[j], dfma(r[3 * i + 1], t[3 + j], r[3 * i + 2] * t[6 + j]));
        oMt[9 + i] = dfma(r[3 * i], t[9], dfma(r[3 * i + 1], t[10], dfma(r[3 * i + 2], t[11], r[9 + i])));
    }
}

// T chained ik::dls() calls of lane `gid`'s problem with q on-chip between them.  The wave moves to the next waypoint when its last
// lane has stopped (any_active, a fresh copy per waypoint: lock-step per solve, as dls_chain_body).  Entries of q outside the chain:
// call k of the chain writes iters_k > 0 ? clip(previous) : previous, and clipping is idempotent, so slab k holds
// stepped ? clip(q0[i]) : q0[i] with stepped = "some waypoint <= k took a step" -- read from q0 only, never from an earlier slab.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_track_body(const ChainKernelArgs<NJ> &a, const Desc &d, int T, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B, t_slab = 12 * a.B;

    double q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(st.elem, st.q_prob, a.qidx[j], b)];
    // (order per waypoint: solve k, compose target k + 1, store slab k, issue the loads of target k + 2 -- see hot_track_body)
    double next[12], oMt[12];
    if (T > 0) {
        load_target_raw(a, a.targets, b, next);
        compose_target(a, next, oMt);
    }
    if (T > 1) load_target_raw(a, a.targets + t_slab, b, next);
    bool stepped = false;
    for (int k = 0; k < T; ++k) {
        int iters;
        bool success;
        chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);   // (any_active by value: a fresh count per waypoint)
        stepped = stepped || iters > 0;
        if (k + 1 < T) compose_target(a, next, oMt);
        if (valid) {
            double *q_out = a.q_out + k * q_slab;
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
            if (a.success) a.success[k * a.B + b] = success ? 1 : 0;
            if (a.iters) a.iters[k * a.B + b] = iters;
            chain_pass_through_into(a, a.q0, q_out, b, stepped);
        }
        if (k + 2 < T) load_target_raw(a, a.targets + (k + 2) * t_slab, b, next);
    }
}

// ---- line: follow a straight Cartesian line from the pose at q0 to ONE goal per problem (include/ikgpu.h ikgpu_dls_line_batch) ----------
// Defined as the tracking call above on the T waypoints of ikgpu_line_targets, a problem taking part in waypoint k only while all its
// earlier waypoints met the stop rule.  The lane loads q0 and its goal (twelve doubles, not T x 12), runs the stage kernels' FK at q0
// and forms the start pose and the rotation vector once (device/line.hpp: the source of ikgpu_line_targets too, hence the same bits);
// per waypoint it forms the raw target, hands it to compose_target where the tracking body hands a loaded one, and solves with q
// on-chip.  A lane whose line has failed enters the later waypoints inactive (chain_dls: its q stays, it keeps no other lane waiting)
// and stores nothing more; the wave leaves the waypoint loop once none of its lanes is alive.  Slabs 0 .. min(reached, T - 1) of a
// problem are written -- the failed waypoint's among them, success = 0 -- and hold the tracking call's bits; entries of q outside the
// chain as there.  Needs a stop rule (without one nothing is ever reached: the entry point refuses the call).
// Returns the waypoints this lane's wave went through (the host-side lane emulator reads it; a kernel ignores it).
template <int NJ>
IKD_FN void line_load(const ChainKernelArgs<NJ> &a, int64_t b, double (&q)[NJ], double (&goal)[12]) {
    const ChainStrides st = chain_strides(a);
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(st.elem, st.q_prob, a.qidx[j], b)];
    load_target_raw(a, a.targets, b, goal);
}
// The start of the line of a chain problem: FK at q from the chain table in HBM (a.desc), through scalar loads on the device.
template <bool KINDS = false, int NJ, class Desc>
IKD_FN void line_chain_start(const ChainKernelArgs<NJ> &a, const Desc &d, const double (&q)[NJ], const double (&goal)[12], LineStart &ls) {
    double Rf[9], pf[3];
    line_chain_fk<NJ, KINDS>(d, a.prm.idmask, q, Rf, pf);
    line_start(a.ref_pl, Rf, pf, goal, ls);
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN int dls_chain_line_body(const ChainKernelArgs<NJ> &a, const Desc &d, const LineArgs &la, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B;
    double q[NJ], goal[12];
    line_load(a, b, q, goal);
    LineStart ls;
    line_chain_start<ReadsKinds<SMASK>::value>(a, d, q, goal, ls);
    bool alive = true, stepped = false;
    int reached = 0, k = 0;
    for (; k < la.T && IKD_ANY(alive); ++k) {
        double t[12], oMt[12];
        line_waypoint(ls, goal, k, la.T, t);
        compose_target(a, t, oMt);
        int iters;
        bool success;
        chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active, alive);   // (any_active by value: a fresh count per waypoint)
        stepped = stepped || (alive && iters > 0);
        if (valid && alive) {
            double *q_out = a.q_out + k * q_slab;
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
            if (a.success) a.success[k * a.B + b] = success ? 1 : 0;
            if (a.iters) a.iters[k * a.B + b] = iters;
            chain_pass_through_into(a, a.q0, q_out, b, stepped);
        }
        alive = alive && success;
        reached += alive ? 1 : 0;
    }
    if (valid && la.reached) la.reached[b] = reached;
    return k;
}

// ---- path: a Cartesian path through P via poses per problem, T waypoints per segment, with a joint-step rule (include/ikgpu.h
// ikgpu_dls_path_batch) ----------------------------------------------------------------------------------------------------------------
// Defined as the tracking call on the P x T waypoints of ikgpu_path_targets: segment 0 is the line above (from the pose at q0 to via 0),
// segment s >= 1 runs from via s - 1's own twelve values to via s (line_start_from_pose).  A problem takes part in waypoint n = s T + k
// only while all its earlier waypoints were MET: the solve met the stop rule and, with max_joint_step > 0, no chain entry moved by
// more than max_joint_step from the configuration the solve started from (path_jumped: q0 for n = 0, the result of waypoint n - 1
// after that).  a.targets holds the P slabs of vias.  Between waypoints the lane parks q, q_prev (NJ entries each), the segment's start
// pose, its rotation vector and the current via; the twelve loads of via s + 1 are issued before the LAST solve of segment s and
// consumed right after it, in front of that waypoint's stores -- no load waits between two solves and no store stands in front of the
// wait (hot_track_body's order).  Dead lanes, the written slabs and the entries of q outside the chain: as the line body; the failing
// slab carries the solve's own flag, so success = 1 there says "reached, but through a jump".
// Returns the waypoints this lane's wave went through (the host-side lane emulator reads it; a kernel ignores it).
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN int dls_chain_path_body(const ChainKernelArgs<NJ> &a, const Desc &d, const PathArgs &pa, int64_t gid, AnyFn any_active) {
    const ChainStrides st = chain_strides(a);
    const bool valid = gid < a.B;
    const int64_t b = valid ? gid : a.B - 1;  // tail lanes shadow the last problem and store nothing
    const int64_t q_slab = static_cast<int64_t>(a.nq) * a.B, t_slab = 12 * a.B;
    double q[NJ], q_prev[NJ], via[12], next[12];
    line_load(a, b, q, via);
    LineStart ls;
    line_chain_start<ReadsKinds<SMASK>::value>(a, d, q, via, ls);
    bool alive = true, stepped = false;
    int reached = 0;
    int64_t n = 0;
    for (int s = 0; s < pa.P && IKD_ANY(alive); ++s) {
        for (int k = 0; k < pa.T && IKD_ANY(alive); ++k, ++n) {
            double t[12], oMt[12];
            line_waypoint(ls, via, k, pa.T, t);
            compose_target(a, t, oMt);
            const bool turn = k + 1 == pa.T && s + 1 < pa.P;   // the last waypoint of a segment that has a successor
            if (turn) load_target_raw(a, a.targets + (s + 1) * t_slab, b, next);
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_prev[j] = q[j];
            int iters;
            bool success;
            chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active, alive);   // (any_active by value: a fresh count per waypoint)
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
                chain_pass_through_into(a, a.q0, q_out, b, stepped);
            }
            alive = alive && success && !path_jumped<NJ>(q, q_prev, pa.max_joint_step);
            reached += alive ? 1 : 0;
        }
    }
    if (valid && pa.reached) pa.reached[b] = reached;
    return static_cast<int>(n);
}

// ---- multi-start: K starts per problem in one launch, the best one stored (include/ikgpu.h ikgpu_dls_multistart_batch) ----------------
// Defined through K calls of the single solve from K starts (start 0: the caller's q0; start k >= 1: slab k - 1 of the caller's
// `starts`, or drawn from the seed -- device/multistart.hpp) and the error ikgpu_evaluate_batch defines at each result; ik::dls is a
// local method (reference ik/ik/dls.cpp:10, :73; ik/ik/dls.hpp:27).  Lane gid serves problem gid >> log2K with start gid & (K - 1): the
// K starts of a problem are neighbouring lanes of one wave.  Three pieces, so that the CPU lane emulator can run them lane after lane:
// the lane's own solve (below, and hot_multistart_lane), the selection (multistart_select) and the winner's stores (multistart_store).

// Where start k of a problem reads entry i from: q0 (start 0, and the entries a generated start does not draw) or the caller's slab.
template <int NJ>
IKD_FN const double *multistart_source(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, int k) {
    return (k == 0 || !ms.starts) ? a.q0 : ms.starts + static_cast<int64_t>(k - 1) * a.nq * a.B;
}

// The chain entries of start k of problem b.
template <int NJ>
IKD_FN void multistart_load(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, int64_t b, int k, double (&q)[NJ]) {
    const ChainStrides st = chain_strides(a);
    const double *src = multistart_source(a, ms, k);
    const bool generated = k > 0 && !ms.starts;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = a.qidx[j];
        const double v = src[at(st.elem, st.q_prob, i, b)];
        const double r = multistart_draw(ms.seed, b, k, i, a.lower[i], a.upper[i]);
        q[j] = (generated && ms.draw[i]) ? r : v;
    }
}

// One start: the single solve's loop, unchanged, then one more evaluation at its result for the error alone.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_multistart_lane(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, const Desc &d, int64_t b, int k,
                                      double (&q)[NJ], bool &success, int &iters, double &err_sq, AnyFn any_active) {
    constexpr int M = TaskDim<KT>::value;
    multistart_load(a, ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);
    double e[M], col[NJ][M], Rf[9], pf[3];
    chain_evaluate<NJ, KT, SMASK>(d, q, oMt, a.prm.idmask, a.prm.unit_weights != 0, e, col, Rf, pf);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) err_sq = dfma(e[r], e[r], err_sq);
}

// The winning lane's stores: what the single solve from start k writes, over all nq entries, and the two outputs of the selection.
// pass(src, stepped) writes the entries outside the chain from the start's own column.
template <int NJ, class Pass>
IKD_FN void multistart_store(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, int64_t b, int k, const double (&q)[NJ], bool success,
                             int iters, double err_sq, Pass pass) {
    const ChainStrides st = chain_strides(a);
#pragma unroll
    for (int j = 0; j < NJ; ++j) a.q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
    pass(multistart_source(a, ms, k), iters > 0);
    if (a.success) a.success[b] = success ? 1 : 0;
    if (a.iters) a.iters[b] = iters;
    if (ms.winner) ms.winner[b] = k;
    if (ms.err_sq) ms.err_sq[b] = err_sq;
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn, class Exchange>
IKD_FN void dls_chain_multistart_body(const ChainKernelArgs<NJ> &a, const MultistartArgs &ms, const Desc &d, int64_t gid, AnyFn any_active,
                                      Exchange exchange) {
    const int64_t prob = gid >> ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters;
    dls_chain_multistart_lane<NJ, KT, SMASK>(a, ms, d, b, k, q, success, iters, err_sq, any_active);
    const int win = multistart_select(ms.log2K, multistart_key(success, err_sq), k, exchange);
    if (valid && win == k)
        multistart_store(a, ms, b, k, q, success, iters, err_sq, [&](const double *src, bool stepped) { chain_pass_through_from(a, src, b, stepped); });
}

// ---- pick: K starts per problem in one launch, the converged one with the smallest cost stored (include/ikgpu.h ikgpu_dls_pick_batch) ----
// Defined through the K single solves of the multi-start call (the same starts, the same lane mapping, the same error) and a cost
// at each result (device/pick.hpp): the key orders (met the stop rule, cost | error, k).  The multi-start pieces again; the trailing
// evaluation's Jacobian is read by the MANIPULABILITY rule alone.  Always under a stop rule (without one no start converges and the
// rule could never act: the entry point refuses the call).

// The cost of a chain problem's start from its chain entries q: the support of a chain problem is its chain.  gram(G) fills the lower
// triangle of J J^T + damping^2 I at q (the build's own Gram matrix of the trailing evaluation).  pk.rule is wave-uniform.
template <int M, int NJ, class Gram>
IKD_FN double pick_chain_cost(const ChainKernelArgs<NJ> &a, const PickArgs &pk, int64_t b, const double (&q)[NJ], Gram gram) {
    static_assert(NJ <= kPickMaxChain, "PickArgs::w is too short for this chain");
    if (pk.rule == PICK_MANIPULABILITY) {
        double G[M * M];
        gram(G);
        return pick_manipulability_cost(pick_ldlt_det<M>(G));
    }
    if (pk.rule == PICK_LIMIT_MARGIN) {
        double margin = 0.5;
#pragma unroll
        for (int j = 0; j < NJ; ++j) margin = pick_margin_step(margin, q[j], a.lower[a.qidx[j]], a.upper[a.qidx[j]]);
        return pick_margin_cost(margin);
    }
    const ChainStrides st = chain_strides(a);
    const double *ref = pk.q_ref ? pk.q_ref : a.q0;
    double r[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] = ref[at(st.elem, st.q_prob, a.qidx[j], b)];
    double cost = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        cost = pk.rule == PICK_DISTANCE ? pick_distance_step(cost, pk.w[j], q[j], r[j]) : pick_max_distance_step(cost, pk.w[j], q[j], r[j]);
    return cost;
}

// One start: the multi-start lane (dls_chain_multistart_lane: the same statements), then the cost at its result.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_pick_lane(const ChainKernelArgs<NJ> &a, const PickArgs &pk, const Desc &d, int64_t b, int k, double (&q)[NJ], bool &success,
                                int &iters, double &err_sq, double &cost, AnyFn any_active) {
    constexpr int M = TaskDim<KT>::value;
    multistart_load(a, pk.ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);
    double e[M], col[NJ][M], Rf[9], pf[3];
    chain_evaluate<NJ, KT, SMASK>(d, q, oMt, a.prm.idmask, a.prm.unit_weights != 0, e, col, Rf, pf);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) err_sq = dfma(e[r], e[r], err_sq);
    // MANIPULABILITY is defined on the Jacobian ikgpu_evaluate_batch returns at q: evaluated once more in the stage kernels' own form
    // (eval_chain_body: accurate sin / cos, run-time mask and weights), under that rule alone.  The loop's form differs from it by rounding
    // that a Position or Orientation task amplifies without bound -- its unconstrained rotation error may lie near pi, where the
    // coefficients of log6's Jacobian cancel -- and the cost would then depend on the build.
    cost = pick_chain_cost<M>(a, pk, b, q, [&](double (&G)[M * M]) {   // (chain_iteration's Gram matrix)
        constexpr int kStage = ReadsKinds<SMASK>::value ? kSpecRuntimeKinds : -1;
        double es[M], cs[NJ][M], Rs[9], ps[3];
        chain_evaluate<NJ, KT, kStage>(d, q, oMt, a.prm.idmask, a.prm.unit_weights != 0, es, cs, Rs, ps);
#pragma unroll
        for (int r = 0; r < M; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                double s = (r == c) ? a.prm.lam2 : 0.0;
#pragma unroll
                for (int j = 0; j < NJ; ++j) s = dfma(cs[j][r], cs[j][c], s);
                G[r * M + c] = s;
            }
    });
}

// The winning lane's stores: multistart_store and the winner's cost.
template <int NJ, class Pass>
IKD_FN void pick_store(const ChainKernelArgs<NJ> &a, const PickArgs &pk, int64_t b, int k, const double (&q)[NJ], bool success, int iters,
                       double err_sq, double cost, Pass pass) {
    multistart_store(a, pk.ms, b, k, q, success, iters, err_sq, pass);
    if (pk.cost) pk.cost[b] = cost;
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn, class Exchange>
IKD_FN void dls_chain_pick_body(const ChainKernelArgs<NJ> &a, const PickArgs &pk, const Desc &d, int64_t gid, AnyFn any_active, Exchange exchange) {
    const int64_t prob = gid >> pk.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << pk.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq, cost;
    bool success;
    int iters;
    dls_chain_pick_lane<NJ, KT, SMASK>(a, pk, d, b, k, q, success, iters, err_sq, cost, any_active);
    const int win = multistart_select(pk.ms.log2K, pick_key(success, cost, err_sq), k, exchange);
    if (valid && win == k)
        pick_store(a, pk, b, k, q, success, iters, err_sq, cost, [&](const double *src, bool stepped) { chain_pass_through_from(a, src, b, stepped); });
}

// ---- path multi-start: K starts per problem in one launch, the one whose branch carries the path furthest stored (include/ikgpu.h
// ikgpu_dls_path_multistart_batch) -------------------------------------------------------------------------------------------------------
// Defined through the K single solves of the multi-start call against via 0 (a.targets' slab 0: the same starts, the same lane mapping,
// the same error) and, from each result that met the stop rule, the path call through the P slabs behind via 0 (dls_chain_path_body
// with q0 = that result: segment 0 runs from the frame's pose there).  The key orders (entered, P T - reached | error, k): pick_key.
// The SCOUT: a lane follows the path with no trajectory store at all -- chain_dls, alive, path_jumped and the via prefetch in the path
// body's order, so `reached` holds that call's bits -- while its entry result (NJ doubles, iters, err_sq) waits in registers; a lane
// whose entry failed is dead from the start and the wave leaves once none of its lanes is alive.  The winner's trajectory is a second,
// ordinary path launch from q_entry: 1 / K of the lanes, one buffer.

// The path loop of dls_chain_path_body / hot_path_body from q without its stores: start(q, via, ls) is the build's line_chain_start,
// solve(q, oMt, iters, success, alive) its loop.  q is left at the last result; returns the waypoints the lane's wave went through.
template <int NJ, class Start, class Solve>
IKD_FN int path_scout(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, int64_t b, double (&q)[NJ], bool alive, int &reached, Start start,
                      Solve solve) {
    const int64_t t_slab = 12 * a.B;
    const double *vias = a.targets + t_slab;   // slab s of the path call
    reached = 0;
    int n = 0;
    if (pm.P < 1 || pm.T < 1) return n;   // (wave-uniform: no slab behind via 0 is read)
    double q_prev[NJ], via[12], next[12];
    load_target_raw(a, vias, b, via);
    LineStart ls;
    start(q, via, ls);
    for (int s = 0; s < pm.P && IKD_ANY(alive); ++s) {
        for (int k = 0; k < pm.T && IKD_ANY(alive); ++k, ++n) {
            double t[12], oMt[12];
            line_waypoint(ls, via, k, pm.T, t);
            compose_target(a, t, oMt);
            const bool turn = k + 1 == pm.T && s + 1 < pm.P;   // the last waypoint of a segment that has a successor
            if (turn) load_target_raw(a, vias + (s + 1) * t_slab, b, next);
#pragma unroll
            for (int j = 0; j < NJ; ++j) q_prev[j] = q[j];
            int iters;
            bool success;
            solve(q, oMt, iters, success, alive);
            if (turn) {
                line_start_from_pose(via, next, ls);
#pragma unroll
                for (int c = 0; c < 12; ++c) via[c] = next[c];
            }
            alive = alive && success && !path_jumped<NJ>(q, q_prev, pm.max_joint_step);
            reached += alive ? 1 : 0;
        }
    }
    return n;
}

// What a start is ranked by: pick_key with the waypoints it did NOT reach as the cost (an exact small integer in a double).
IKD_FN unsigned long long path_multistart_key(const PathMultistartArgs &pm, bool success, int reached, double err_sq) {
    const int64_t N = static_cast<int64_t>(pm.P) * pm.T;
    return pick_key(success, static_cast<double>(N - (success ? reached : 0)), err_sq);
}

// One start: the multi-start lane against via 0 (dls_chain_multistart_lane: the same statements), then the scout from a copy of its
// result.  reached = -1 for a start whose entry failed.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN int dls_chain_path_multistart_lane(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, const Desc &d, int64_t b, int k,
                                          double (&q)[NJ], bool &success, int &iters, double &err_sq, int &reached, AnyFn any_active) {
    dls_chain_multistart_lane<NJ, KT, SMASK>(a, pm.ms, d, b, k, q, success, iters, err_sq, any_active);
    IKD_PIN(err_sq);   // the error is formed HERE: sunk to its use behind the path loop, the trailing evaluation's inputs would wait with it
    double qp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) qp[j] = q[j];
    const int n = path_scout(
        a, pm, b, qp, success, reached,
        [&](const double (&q0)[NJ], const double (&via)[12], LineStart &ls) { line_chain_start<ReadsKinds<SMASK>::value>(a, d, q0, via, ls); },
        [&](double (&qw)[NJ], const double (&oMt)[12], int &it, bool &ok, bool alive) {
            chain_dls<NJ, KT, SMASK>(d, a.prm, qw, oMt, it, ok, any_active, alive);   // (any_active by value: a fresh count per waypoint)
        });
    reached = success ? reached : -1;
    return n;
}

// The winning lane's stores: multistart_store (q_entry over all nq entries, the flags, winner, err_sq) and the winner's count.
template <int NJ, class Pass>
IKD_FN void path_multistart_store(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, int64_t b, int k, const double (&q)[NJ], bool success,
                                  int iters, double err_sq, int reached, Pass pass) {
    multistart_store(a, pm.ms, b, k, q, success, iters, err_sq, pass);
    if (pm.reached) pm.reached[b] = success ? reached : 0;
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn, class Exchange>
IKD_FN void dls_chain_path_multistart_body(const ChainKernelArgs<NJ> &a, const PathMultistartArgs &pm, const Desc &d, int64_t gid, AnyFn any_active,
                                           Exchange exchange) {
    const int64_t prob = gid >> pm.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << pm.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters, reached;
    (void)dls_chain_path_multistart_lane<NJ, KT, SMASK>(a, pm, d, b, k, q, success, iters, err_sq, reached, any_active);
    if (valid && pm.reached_all) pm.reached_all[static_cast<int64_t>(k) * a.B + b] = reached;
    const int win = multistart_select(pm.ms.log2K, path_multistart_key(pm, success, reached, err_sq), k, exchange);
    if (valid && win == k)
        path_multistart_store(a, pm, b, k, q, success, iters, err_sq, reached,
                              [&](const double *src, bool stepped) { chain_pass_through_from(a, src, b, stepped); });
}

// ---- goal set: G alternative goals and K starts per problem in one launch, the best candidate stored (include/ikgpu.h
// ikgpu_dls_goalset_batch) ------------------------------------------------------------------------------------------------------------
// Defined through the G x K single solves "start k against goal g" (the starts are the multi-start call's and do not depend on the goal;
// slab g of `a.targets` is what the single solve takes as its targets) and the error ikgpu_evaluate_batch defines at each result.  Lane
// gid serves problem gid >> (log2G + log2K) with candidate j = the low bits, goal j >> log2K, start j & (K - 1): a problem's candidates
// are neighbouring lanes of one wave, a goal's K starts neighbours within them.  The key orders (met the stop rule, error, j), so among
// the candidates that met the stop rule the lowest goal wins and within it the lowest start.  The same three pieces as multi-start, and
// `any`, the OR over a goal's K lanes, for the reachability flags (device/goalset.hpp GoalsetBallot).

// One candidate: the multi-start lane's code with the target taken from slab g -- load_target in its two halves, the same expressions.
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_goalset_lane(const ChainKernelArgs<NJ> &a, const GoalsetArgs &ga, const Desc &d, int64_t b, int g, int k, double (&q)[NJ],
                                   bool &success, int &iters, double &err_sq, AnyFn any_active) {
    constexpr int M = TaskDim<KT>::value;
    multistart_load(a, ga.ms, b, k, q);
    double t[12], oMt[12];
    load_target_raw(a, a.targets + static_cast<int64_t>(g) * 12 * a.B, b, t);
    compose_target(a, t, oMt);
    chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);
    double e[M], col[NJ][M], Rf[9], pf[3];
    chain_evaluate<NJ, KT, SMASK>(d, q, oMt, a.prm.idmask, a.prm.unit_weights != 0, e, col, Rf, pf);
    err_sq = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) err_sq = dfma(e[r], e[r], err_sq);
}

// The winning lane's stores: multistart_store (ms.winner is null in a goal-set call) and the winner's two indices.
template <int NJ, class Pass>
IKD_FN void goalset_store(const ChainKernelArgs<NJ> &a, const GoalsetArgs &ga, int64_t b, int g, int k, const double (&q)[NJ], bool success,
                          int iters, double err_sq, Pass pass) {
    multistart_store(a, ga.ms, b, k, q, success, iters, err_sq, pass);
    if (ga.goal) ga.goal[b] = g;
    if (ga.start) ga.start[b] = k;
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn, class Exchange, class Any>
IKD_FN void dls_chain_goalset_body(const ChainKernelArgs<NJ> &a, const GoalsetArgs &ga, const Desc &d, int64_t gid, AnyFn any_active,
                                   Exchange exchange, Any any) {
    const int log2J = ga.log2G + ga.ms.log2K;
    const int64_t prob = gid >> log2J;
    const int j = static_cast<int>(gid & ((int64_t{1} << log2J) - 1));
    const int g = j >> ga.ms.log2K, k = j & ((1 << ga.ms.log2K) - 1);
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ], err_sq;
    bool success;
    int iters;
    dls_chain_goalset_lane<NJ, KT, SMASK>(a, ga, d, b, g, k, q, success, iters, err_sq, any_active);
    const int win = multistart_select(log2J, multistart_key(success, err_sq), j, exchange);
    const bool reached = any(ga.ms.log2K, success);
    if (!valid) return;
    if (ga.reachable && k == 0) ga.reachable[static_cast<int64_t>(g) * a.B + b] = reached ? 1 : 0;
    if (win == j)
        goalset_store(a, ga, b, g, k, q, success, iters, err_sq, [&](const double *src, bool stepped) { chain_pass_through_from(a, src, b, stepped); });
}

// ---- solution set: K starts per problem in one launch, the distinct converged ones stored (include/ikgpu.h ikgpu_dls_solutions_batch) ---
// Defined through the K single solves of the multi-start call (the same starts, the same lane mapping: lane gid serves problem
// gid >> log2K with start gid & (K - 1)) and the greedy rule of device/solutions.hpp over their results: start k is kept when it met the
// stop rule, fewer than N are kept, and some chain entry differs by sep or more from every start kept before it.  Three pieces again: the
// lane's own solve, the K steps of the set (solutions_offer / solutions_take) and a kept lane's stores (solutions_store).

// One start: the single solve's loop, unchanged.  (Only converged starts matter: no evaluation after it.)
template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn>
IKD_FN void dls_chain_solutions_lane(const ChainKernelArgs<NJ> &a, const SolutionsArgs &sa, const Desc &d, int64_t b, int k, double (&q)[NJ],
                                     bool &success, int &iters, AnyFn any_active) {
    multistart_load(a, sa.ms, b, k, q);
    double oMt[12];
    load_target(a, b, oMt);
    chain_dls<NJ, KT, SMASK>(d, a.prm, q, oMt, iters, success, any_active);
}

// A kept lane's stores into slab `slot` of q_sols (a.q_out) / which / iters (a.iters): what the single solve from start k writes, over
// all nq entries.  pass(src, q_out, stepped) writes the entries outside the chain from the start's own column; it goes FIRST: its loads
// are the only ones after the loop, and behind a store their wait would be for the store's acknowledgement as well (loads and stores
// share one counter on gfx950).
template <int NJ, class Pass>
IKD_FN void solutions_store(const ChainKernelArgs<NJ> &a, const SolutionsArgs &sa, int64_t b, int k, int slot, const double (&q)[NJ], int iters,
                            Pass pass) {
    const ChainStrides st = chain_strides(a);
    double *q_out = a.q_out + static_cast<int64_t>(slot) * a.nq * a.B;
    pass(multistart_source(a, sa.ms, k), q_out, iters > 0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
    if (sa.which) sa.which[slot * a.B + b] = k;
    if (a.iters) a.iters[slot * a.B + b] = iters;
}

template <int NJ, int KT, int SMASK = -1, class Desc, class AnyFn, class Fetch>
IKD_FN void dls_chain_solutions_body(const ChainKernelArgs<NJ> &a, const SolutionsArgs &sa, const Desc &d, int64_t gid, AnyFn any_active,
                                     Fetch fetch) {
    const int64_t prob = gid >> sa.ms.log2K;
    const int k = static_cast<int>(gid & ((int64_t{1} << sa.ms.log2K) - 1));
    const bool valid = prob < a.B;
    const int64_t b = valid ? prob : a.B - 1;  // tail lanes (whole groups) shadow the last problem and store nothing
    double q[NJ];
    bool success;
    int iters;
    dls_chain_solutions_lane<NJ, KT, SMASK>(a, sa, d, b, k, q, success, iters, any_active);
    SolutionsLane s;
    solutions_select<NJ>(s, sa.ms.log2K, k, sa.N, sa.sep, success, q, fetch);
    if (!valid) return;
    if (s.kept)
        solutions_store(a, sa, b, k, s.slot, q, iters,
                        [&](const double *src, double *q_out, bool stepped) { chain_pass_through_into(a, src, q_out, b, stepped); });
    if (k == 0) sa.count[b] = s.cnt;
}

#if IKD_HIP_LANG
// ---- lane refill: the stop-rule mode without lock-step divergence ----------------------------------------------------------------
// With the reference's default visitor (ik/ik/visitor.hpp:15-21) a problem stops after a handful of iterations or never
// (max_iterations, ik/ik/dls.cpp:76-77); in the lock-step kernels a wave runs until its LAST lane stops, so one lane that never
// converges keeps 63 finished ones idle.  Here a wave is persistent: a lane whose visitor fired (or whose iteration count reached
// max_iterations) stores its result and takes the next unsolved problem from the launch's queue head; the wave leaves when the
// queue is exhausted and every lane is idle.  A lane's state is (q, target, it): the iteration is the same code as the lock-step
// loop's, so results are bit-identical whatever the batch composition.  Worth it when the batch is larger than the machine
// (B > resident lanes); at B = resident lanes every problem has its own lane anyway and the launch lasts as long as its slowest problem.
//
// queue[0]: head -- problems handed out (in chunks) beyond the first (static) round, queue[1]: waves that have left; the last wave out
// zeroes both, so the next launch on the same stream finds the slot clean (host: QueuePool in kernels.hpp).
// iterate(q, oMt, have) runs ONE iteration of this lane's problem in place and returns "the visitor stopped it before the step".
// on_target(oMt) is called once where a lane takes a target -- the first round and every refill --, in place: the hot program carries the
// target into joint 0's frame there (chain_hot.hpp hot_fold_base); the default does nothing.
// stage: what a wave that HAS work sets up once, around its first round of loads -- issue() in front of them, commit() behind them and
// ahead of the first iteration (the hot program fills its sin / cos table in LDS there, chain_hot.hpp); a wave without a share of the
// first round leaves before either.  The default does nothing.
struct KeepTarget {
    __device__ __forceinline__ void operator()(double (&)[12]) const {}
};
struct NoStage {
    __device__ __forceinline__ void issue() {}
    __device__ __forceinline__ void commit() {}
};
template <int NJ, class IterFn, class TargetFn = KeepTarget, class StageFn = NoStage>
__device__ __forceinline__ void chain_refill_loop(const ChainKernelArgs<NJ> &a, unsigned long long *queue, int chunk_and_batch, IterFn iterate,
                                                  TargetFn on_target = TargetFn{}, StageFn stage = StageFn{}) {
    const ChainStrides st = chain_strides(a);
    const int lane = static_cast<int>(threadIdx.x) & 63;                 // one wave per workgroup
    const int64_t first_round = static_cast<int64_t>(gridDim.x) * 64;
    // work items: the batch's problems, or (second phase) the entries of the worklist; `b` is always a PROBLEM index
    const bool listed = a.worklist != nullptr;
    const int64_t nwork = listed ? static_cast<int64_t>(*a.count) : a.B;
    const double *qsrc = listed ? a.q_out : a.q0;
    auto problem = [&](int64_t w) { return listed ? static_cast<int64_t>(a.worklist[w]) : w; };
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    bool have = w0 < nwork;
    double q[NJ], oMt[12];
    int64_t b = 0;
    int it = 0;
    const int max_it = a.prm.max_iterations;                             // >= 1: the host sends max_iterations == 0 to the lock-step kernel
    // Waves without a share of the first round never touch the queue: they leave at once, and the slot's bookkeeping below counts the
    // others only.  (An EMPTY list -- every problem stopped in the first phase -- costs the launch and one load per wave: the slot is
    // still zero.  A thousand arrivals on one address took ~15 us, a quarter of a near-target solve.)
    const int64_t working = (nwork + 63) / 64 < static_cast<int64_t>(gridDim.x) ? (nwork + 63) / 64 : static_cast<int64_t>(gridDim.x);
    if (static_cast<int64_t>(blockIdx.x) >= working) return;
    stage.issue();
    b = problem(have ? w0 : 0);                                          // idle lanes shadow a valid problem
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = qsrc[at(st.elem, st.q_prob, a.qidx[j], b)];
    load_target(a, b, oMt);
    stage.commit();
    on_target(oMt);
    if (listed) it = a.iters[b];                                         // (the iterations the first phase took over this problem)
    // The wave's own reserve [pool_lo, pool_hi) of unsolved problems (wave-uniform): finished lanes are served from it, and only when
    // it runs dry does the wave pull `chunk` (>= 64) more from the launch's head.  One atomic per finished LANE-GROUP on one address
    // saturated the memory-side atomic unit (measured: ~30-70 M same-address atomics/s device-wide, every refill waiting ~30 us).
    int64_t pool_lo = 0, pool_hi = 0;
    bool exhausted = first_round >= nwork;                               // the head has passed the end of the batch
    // Refill events are BATCHED: a finished lane stores its result at once and then waits until `batch` lanes of the wave are idle
    // (or no lane is active any more) -- one ballot, one reserve update and one round trip of loads per event instead of per
    // iteration.  With targets near the start every lane is done within two or three iterations, an event per iteration cost
    // as much as the iterations themselves (round 3: refill 1.5-2x slower than lock-step there); with far targets the wave's
    // stragglers set the pace either way.  chunk_and_batch: chunk | batch << 16 (kernels.hip refill_chunk).
    const int batch = chunk_and_batch >> 16, chunk = chunk_and_batch & 0xffff;
    while (__any(have)) {
        const bool stop_now = iterate(q, oMt, have) && have;
        ++it;
        const bool done = have && (stop_now || it >= max_it);
        if (done) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) a.q_out[at(st.elem, st.q_prob, a.qidx[j], b)] = q[j];
            if (a.success) a.success[b] = stop_now ? 1 : 0;
            a.iters[b] = stop_now ? it - 1 : max_it;                     // never null here: the pass-through kernel reads it
            have = false;
        }
        const unsigned long long mask = __ballot(!have);                 // idle lanes: finished (or never had a problem)
        const int need = __popcll(mask);
        const bool supply = pool_hi > pool_lo || !exhausted;             // (wave-uniform)
        if (supply && (need >= batch || need == 64)) {
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            const int64_t avail = pool_hi - pool_lo;
            int64_t nb = pool_lo + rank;                                 // ranks below `avail` are served from the reserve
            bool got = rank < avail;
            if (avail < need && !exhausted) {                            // wave-uniform: pull the next chunk, serve the other ranks from it
                unsigned long long v = 0;
                if (lane == 0) v = atomicAdd(queue, static_cast<unsigned long long>(chunk));
                const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
                const int64_t nlo = first_round + static_cast<int64_t>((static_cast<unsigned long long>(hi) << 32) | lo);
                const int64_t nhi = nlo + chunk < nwork ? nlo + chunk : nwork;
                exhausted = nlo + chunk >= nwork;
                if (rank >= avail) { nb = nlo + (rank - avail); got = nb < nhi; }
                pool_lo = nlo + (need - avail);
                pool_hi = nhi > pool_lo ? nhi : pool_lo;
            } else {
                pool_lo += need < avail ? need : avail;
            }
            if (!have && got) {
                have = true;
                b = problem(nb);
#pragma unroll
                for (int j = 0; j < NJ; ++j) q[j] = qsrc[at(st.elem, st.q_prob, a.qidx[j], b)];
                load_target(a, b, oMt);
                on_target(oMt);
                it = listed ? a.iters[b] : 0;
            }
        }
    }
    // the last wave out resets the slot (every wave's atomics on queue[0] are ordered before its own arrival on queue[1])
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(queue + 1, 1ull) == static_cast<unsigned long long>(working) - 1ull) {
            queue[0] = 0ull;
            queue[1] = 0ull;
            queue[2] = 0ull;   // (the two-phase worklist's length)
            __threadfence();
        }
    }
}

// The general chain program under lane refill (device/chain_solver.hpp chain_dls, one iteration at a time).
template <int NJ, int KT, int SMASK, class Desc>
__device__ __forceinline__ void dls_chain_refill_body(const ChainKernelArgs<NJ> &a, const Desc &d_in, unsigned long long *queue, int chunk) {
    const Desc *dp = &d_in;
    chain_refill_loop<NJ>(a, queue, chunk, [&](double (&q)[NJ], const double (&oMt)[12], bool) {
        asm volatile("" ::: "memory");
        if constexpr (!std::is_same<Desc, ChainDesc<NJ>>::value) IKD_LAUNDER(dp);   // see chain_dls
        return chain_iteration<NJ, KT, SMASK>(*dp, a.prm, q, oMt, true);
    });
}

#endif  // IKD_HIP_LANG

// evaluate_problem_data + stacking (reference ik/ik/data.cpp:25-58, ik/ik/dls.cpp:18-24):
// e [M x B], dense J [M x nv x B] (zero outside the support, as the reference's zero-initialised
// frame Jacobian, ik/ik/frame.hpp:110).
template <int NJ, int KT, int SMASK = -1>
IKD_FN void eval_chain_body(const ChainKernelArgs<NJ> &a, const ChainDesc<NJ> &d, int64_t b) {
    constexpr int M = TaskDim<KT>::value;
    if (b >= a.B) return;
    double q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = a.q0[at(a.layout, a.B, a.nq, a.qidx[j], b)];
    double oMt[12];
    load_target(a, b, oMt);
    double e[M], col[NJ][M], Rf[9], pf[3];
    chain_evaluate<NJ, KT, SMASK>(d, q, oMt, a.prm.idmask, a.prm.unit_weights != 0, e, col, Rf, pf);
#pragma unroll
    for (int r = 0; r < M; ++r) a.e_out[at(a.layout, a.B, M, r, b)] = e[r];
    if (a.J_out) {
        for (int r = 0; r < M; ++r)
            for (int c = 0; c < a.nv; ++c) a.J_out[at(a.layout, a.B, M * a.nv, r * a.nv + c, b)] = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < M; ++r) a.J_out[at(a.layout, a.B, M * a.nv, r * a.nv + a.vidx[j], b)] = -col[j][r];
    }
}

// World placement of the task frame (reference ik/ik/data.cpp:28-29, one entry of data.oMf).
template <int NJ, bool KINDS = false>
IKD_FN void fk_chain_body(const ChainKernelArgs<NJ> &a, const ChainDesc<NJ> &d, int64_t b) {
    if (b >= a.B) return;
    double R[9], p[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = d.pl[0][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = d.pl[0][9 + k];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j > 0) se3_compose_const(R, p, d.pl[j], (a.prm.idmask >> j) & 1);
        const double qj = a.q0[at(a.layout, a.B, a.nq, a.qidx[j], b)];
        bool slides = false;
        if constexpr (KINDS) slides = ((a.prm.idmask >> (kKindShift + j)) & 1) != 0;
        if (slides) {
            p[0] = dfma(qj, R[2], p[0]);
            p[1] = dfma(qj, R[5], p[1]);
            p[2] = dfma(qj, R[8], p[2]);
        } else {
            double s, c;
            dsincos(qj, s, c);
            rot_z_right(R, s, c);
        }
    }
    se3_compose_const(R, p, d.frame_pl, (a.prm.idmask >> NJ) & 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.oMf_out[at(a.layout, a.B, 12, k, b)] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.oMf_out[at(a.layout, a.B, 12, 9 + k, b)] = p[k];
}

}  // namespace ikdev
