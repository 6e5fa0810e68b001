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

#ifdef __cplusplus
}
#endif

#endif
