// trace_plan.h -- which traversal kernel a launch gets: a pure function of the hierarchy's sizes, the queue and the tuning (no HIP
// here).  exec::trace() (hip/trace.hip) launches what the plan says, the CPU debugging harness (tests/hostsim/exec.h) follows its
// `form`, rdr_debug_trace_plan (capi.cpp) shows it to tests/test_trace_plan.py.  Every form returns the same hits: a slip in a rule
// changes speed only, so each rule stands here once, next to the measurement that set its threshold.
#pragma once
#include "bvh.h"
#include "tuning.h"

namespace exec {
struct TraceFacts { int num_nodes, stack_need, wide_stack_need; bool has_wide; };      // what trace() reads off rt::BvhD
inline TraceFacts trace_facts(const rt::BvhD &bvh) { return {bvh.num_nodes, bvh.stack_need, bvh.wide_stack_need, bvh.wide != nullptr}; }

enum class TraceForm { Wide = 0, Refill = 1, Plain = 2 };       // trace_wide_kernel / trace_refill_kernel / trace_kernel
struct TracePlan {
    TraceForm form;
    int stack;                  // per-lane stack entries of the instantiation (Refill, 16: the hybrid LDS + scratch stack)
    bool short_index, stage_top, sorted, counting;      // 16-bit entries; top levels in LDS (Plain); octant order (Refill); instrumented
    int blocks;                 // grid size, 256 threads each
    int rays_per_lane, idle_min, steps, sort_mode;      // Refill only (0 otherwise)
};
constexpr int kWideStackMax = 48;
template <int N> int first_tier(int need, const int (&tiers)[N]) {      // the smallest tier that covers `need`, else the last
    for (int t : tiers) if (need <= t) return t;
    return tiers[N - 1];
}

// n > 0: the queue's host-side bound (Count::upper); `counting`: TraceStats::counting; both query kinds follow the same rules
inline TracePlan plan_trace(const TraceFacts &f, int n, bool /*any*/, bool coherent, bool counting, const rdr::Tuning &tune) {
    TracePlan p{};
    p.blocks = (n + 255) / 256;
    p.counting = counting;      // (the refilling kernel has no instrumented variant: chosen only when this is off)
    // Which form of the hierarchy: queues of up to RDR_WIDE_MAX rays (default 2^19) walk the 4-wide records (measured,
    // tools/trace_ab.py, profiles/r3_notes.md: half the dependent steps per ray pays where a launch is one or two waves per
    // SIMD -- closest-hit 0.119 -> 0.102 ms, any-hit 0.078 -> 0.066 ms per 65 k / 50 k rays; on queues of a million rays and
    // more both forms issue the same number of vector instructions per wave and the binary records, at 8 instead of 5 waves
    // per SIMD, are 0-10 % ahead).  RDR_TUNE_TRACE_BINARY: never the wide records.
    if (!tune.has(RDR_TUNE_TRACE_BINARY) && f.has_wide && f.wide_stack_need <= kWideStackMax && n <= tune.wide_max) {
        static constexpr int tiers[] = {12, 16, 20, 24, 32, kWideStackMax};
        p.form = TraceForm::Wide;
        p.stack = first_tier(f.wide_stack_need, tiers);
        return p;
    }
    // lanes refilled from the wave's own chunk of the queue (see trace_refill_kernel): queues sized for >= 2^22 lanes that the
    // caller does not mark coherent.  (The queue's host-side bound decides: a launch sized for 2^22 lanes -- four samples of a
    // 1024 x 1024 frame, the edge sub-paths' two lanes per slot -- still holds 1.5-3.3 M rays after the compactions; choosing the
    // rays per lane in the kernel from the actual count was measured too and is slower, 61.8 vs 62.5 Msamples/s.)
    // rdr_tuning: RDR_TUNE_REFILL_OFF never; refill_* those parameters; RDR_TUNE_REFILL_ALL every queue (tools/trace_ab.py).
    const bool refill = !tune.has(RDR_TUNE_REFILL_OFF) && (tune.has(RDR_TUNE_REFILL_ALL) || (!coherent && n >= (1 << 22)));
    const int k = refill ? tune.refill_k : 0;          // rays per lane
    const bool short_index = f.num_nodes < 65536;
    if (k >= 1 && !counting && f.stack_need <= rt::kTraverseStack) {
        p.form = TraceForm::Refill;
        if (short_index && f.stack_need <= 24) { p.stack = 24; p.short_index = true; }
        // the hybrid stack (16 LDS entries + scratch: six workgroups per CU) for every hierarchy too big for the 16-bit column:
        // 0.92 M triangles 2.39 -> 2.73, 3.7 M 2.02 -> 2.33 G rays/s against the 32-entry tier.  RDR_TRACE_HYBRID=0: the tiers.
        else if (tune.trace_hybrid) p.stack = 16;
        // big hierarchies (int entries): 32 entries where that covers the tree -- 40 KiB of LDS per workgroup instead of 49: four
        // workgroups per CU instead of three (a hierarchy beyond the L2 is latency-bound: more waves, profiles/r6_notes.md)
        else p.stack = f.stack_need <= 32 ? 32 : rt::kTraverseStack;
        p.rays_per_lane = k; p.idle_min = tune.refill_idle; p.steps = tune.refill_steps;
        p.sort_mode = tune.refill_sort;       // rdr_tuning::refill_order: 0 queue order, 1 octant (default), 2 octant x axis
        p.sorted = p.sort_mode > 0 && k == 4;
        p.blocks = (int)(((long long)n + 256 * k - 1) / (256 * k));       // a workgroup's 4 x 64 lanes take k rays each
        return p;
    }
    static constexpr int tiers[] = {16, 24, 32, rt::kTraverseStack};
    p.form = TraceForm::Plain;
    p.stack = first_tier(f.stack_need, tiers);
    p.short_index = short_index;
    // Staging pays on big queues (closest-hit 0.330 -> 0.321 ms per 956 k rays); on a 256 x 256 frame the 8 KiB copy + barrier per
    // 256 rays costs more than the L1-hot top levels save (optimisation-loop iteration +2 ms).  RDR_TUNE_TRACE_NO_LDS_TOP: never.
    p.stage_top = !tune.has(RDR_TUNE_TRACE_NO_LDS_TOP) && n >= (1 << 18);
    return p;
}
} // namespace exec
