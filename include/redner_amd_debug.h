/* redner_amd_debug.h -- test hooks of the C ABI that came after redner_amd.h was fixed at its present set of functions.  Include
 * this header instead of redner_amd.h (it includes it); the functions live in the same library, follow the same conventions
 * (rdr_last_error, the calling thread's device) and are bound by redner_amd/_capi.py from its DEBUG_SIGNATURES table.
 * tests/test_lane_park.py compares this header, that table and the library's exports with one another. */
#ifndef REDNER_AMD_DEBUG_H
#define REDNER_AMD_DEBUG_H

#include "redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: the lane park alone (csrc/lane_park.h: RDR_PARK_DECL -- per-lane state of a stage body kept in LDS columns across a
 * stretch that needs the registers).  ONE stage of `num_lanes` lanes; lane i -- unless active[i] == 0: it returns before the park
 * is declared, as the idle lanes of the production stages do -- parks in[K i .. K i + K) through every typed form (double, V3, V2,
 * double[4]), adds half of in[K i + k] on top of columns k = 10 .. 15, and fetches everything back in the opposite order into
 * out[K i .. K i + K).  K = *columns on return: the widest park a shipped stage declares (a call with num_lanes = 0
 * only reports it).  in / out: HOST memory, K doubles per lane; `out` is uploaded first, so the doubles of inactive lanes come
 * back untouched. */
int rdr_debug_lane_park(int num_lanes, const uint8_t *active, const double *in, double *out, int32_t *columns);

/* Test hook: rdr_scene_trace with every input of the launch plan (csrc/trace_plan.h) in the caller's hands, so that one process
 * can run every traversal kernel.  `tuning` as in rdr_render_options (null: the defaults); `coherent` as the render stages pass
 * it; trace_hybrid: -1 keeps the process's setting (RDR_TRACE_HYBRID), 0 / 1 override it -- the one plan input that is no field
 * of rdr_tuning; device_count (may be null): an int in the Scene's memory, the queue then holds min(*device_count, num_rays)
 * rays and the slots of `hits` from there on are not written.  Counting kernels are selected by rdr_trace_stats_enable, as for
 * rdr_scene_trace.  rays / hits: the Scene's memory, num_rays records (0 .. 2^24).  rdr_debug_scene_trace_plan with the same
 * num_rays, any_hit, coherent, counting and tuning reports the launch this makes when trace_hybrid is -1; with an override
 * only the refilling kernel's int-entry tier changes (trace_plan.h: stack 16 with the hybrid stack, else 32 up to a need of
 * 32 and 40 beyond), which the caller derives (tests/test_trace_tiers.py). */
int rdr_debug_scene_trace(const rdr_scene *scene, const float *rays, int32_t *hits, int num_rays, int any_hit, int coherent,
                          const rdr_tuning *tuning, int trace_hybrid, const int32_t *device_count);

/* Test hook, host arithmetic in every build: how many stack entries each ray uses.  The host builder (csrc/bvh.cpp) builds the
 * hierarchy of the Scene's meshes afresh -- what rdr_debug_bvh_check compares the kernels' build with -- and every ray of
 * host_rays (HOST memory, num_rays records of 8 floats) walks it with rt::traverse (wide = 0) or rt::traverse_wide (wide = 1)
 * over a stack pre-filled with a value no walk pushes; max_entries[i] = the highest stack index ray i wrote, plus one (0: it
 * pushed nothing, or the slot is dead).  max_entries[num_rays .. num_rays + 3] = {node records, stack_need, 4-wide records,
 * wide_stack_need} of that hierarchy: num_rays + 4 ints in all. */
int rdr_debug_trace_occupancy(const rdr_scene *scene, const float *host_rays, int num_rays, int any_hit, int wide,
                              int32_t *max_entries);

#ifdef __cplusplus
}
#endif

#endif
