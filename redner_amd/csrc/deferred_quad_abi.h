/* deferred_quad_abi.h -- a companion header of the C ABI: rectangular area lights in deferred shading, the closed-form diffuse
 * irradiance of a uniformly emitting quad (Lambert's contour integral, clipped to the horizon) evaluated on a G-buffer, and its
 * gradient.  Include this header instead of include/redner_amd.h (it includes it); the functions live in the same library,
 * follow the same conventions (rdr_last_error, rdr_set_stream, device memory of gpu_index) and are bound by redner_amd/_capi.py
 * from its CSRC_HEADERS table.  It stands here and not under include/ because the set of files there, and the functions each
 * declares, are pinned (tests/test_capi.py); tests/test_deferred_quad.py compares this header, that table and the libraries'
 * exports with one another. */
#ifndef REDNER_AMD_DEFERRED_QUAD_ABI_H
#define REDNER_AMD_DEFERRED_QUAD_ABI_H

#include "../../include/redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* csrc/deferred_quad.h pins the meaning and the order of the fp32 operations.  Per texel of the oversampled G-buffer, with
 * position p, shading normal n as stored and albedo a, and per quad with corners q0..q3 in perimeter order, radiance L[3] and
 * the flag two_sided (the emitting side of a one-sided quad is that of cross(q1 - q0, q3 - q0)):
 *   nn = n.n, nh = n / sqrt(nn)            nothing unless 0 < nn < inf (background texels have n = 0) and p is finite
 *   r_i = q_i - p, h_i = nh.r_i            i = 0..3
 *   S = 0; for edge i = 0..3 from A = r_i to B = r_{(i+1)%4}:
 *       neither end has h > 0: nothing;  one end has: the other is replaced by x = A + (B - A) hA / (hA - hB),
 *       the EXIT point when A is up, the ENTRY point when B is;  S += edge(A', B')
 *   if some edge crossed: S += edge(exit, entry)                   (the arc along the horizon)
 *   edge(A, B) = atan2(|c|, A.B) (c.nh) / |c|, c = B x A;  0 unless c.c > 0
 *   F = (two_sided ? |S| : max(S, 0)) / 2
 *   texel_rgb[k] += L[k] (a[k] / pi) F
 * and the image [num_images, height, width, 3] is the mean over each aa_samples x aa_samples block (no alpha channel).  F / pi
 * is the view factor; a quad that fills the hemisphere gives rgb = L a.  The normal is normalised (rdr_deferred_shade's point
 * light uses it as stored).  The quad is expected to be planar and convex.
 *   desc          the description of rdr_deferred_shade.  Read: num_images, height, width, aa_samples, alpha, gpu_index,
 *                 num_lights (the number of quads), image_light_range (image n is lit by the rows [range[2n], range[2n+1]) of
 *                 `quads`; an empty range is legal) and light_type: light_type[q] is 0 for a one-sided quad and 1 for a
 *                 two-sided one; anything else is an error.  occluders, visibility, ao_occluders, ao_words and ao_rays must be
 *                 zero: nothing is traced.
 *   g_buffer      [num_images, height * aa, width * aa, 9 + alpha]: position 3, shading normal 3, albedo 3[, alpha, not read]
 *   quads         [num_lights][16]: [0..11] q0..q3, [12..14] L, [15] unused (its gradient is exactly 0); rows are 64 bytes
 * rdr_deferred_quad writes every element of image.  rdr_deferred_quad_backward writes every element of d_g_buffer (all nine
 * channels; the alpha channel is 0) and of d_quads, from the upstream gradient d_image [num_images, height, width, 3].  The
 * derivatives are those of the expression above: the conditions are constants; max(S, 0) passes half the gradient at S == 0;
 * |S| passes sign(S), 0 at 0; x is differentiated through hA and hB; no gradient of a gated texel or edge is anything but 0.
 * The quad gradients are fp64 partial sums per workgroup folded in a fixed order and rounded once: no atomics, the same bits
 * from run to run.  Pointers are DEVICE memory of gpu_index (a negative gpu_index: host memory, accepted by the CPU debugging
 * harness only); with alpha the G-buffers must be 8-byte aligned.  Everything is checked before anything is launched; launches
 * are ordered on the rdr_set_stream stream; both calls synchronise before returning.  Return 0 on success. */
int rdr_deferred_quad(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, float *image);
int rdr_deferred_quad_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, const float *d_image,
                               float *d_g_buffer, float *d_quads);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_DEFERRED_QUAD_ABI_H */
