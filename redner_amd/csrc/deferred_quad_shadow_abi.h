/* deferred_quad_shadow_abi.h -- a companion header of the C ABI: soft shadows for the rectangular area lights of
 * deferred_quad_abi.h.  The exact unshadowed irradiance F of rdr_deferred_quad is multiplied, per texel and quad, by a visibility
 * factor V = sum_k w_k vis_k / sum_k w_k over K fixed, stratified points of the quad, each tested by one any-hit ray over an
 * occluder scene and weighted by the unshadowed integrand w_k at that point: the ratio estimator of Heitz et al. 2018, "Combining
 * analytic direct illumination and stochastic shadows".  With nothing in the way the image is bit for bit rdr_deferred_quad's; a
 * penumbra carries no noise from the form factor itself; the only error is in the visibility fraction.  V is a CONSTANT of the
 * gradient, like the visibility bits and the ambient-occlusion factor of rdr_deferred_shade: the backward call reads the saved
 * factors, traces nothing and differentiates nothing across a shadow boundary.
 * Include this header instead of include/redner_amd.h (it includes it, through deferred_quad_abi.h); the functions live in the
 * same library, follow the same conventions and are bound by redner_amd/_capi.py from its CSRC_HEADERS table.  It stands here
 * and not under include/ for the reason deferred_quad_abi.h gives; tests/test_deferred_quad_shadows.py compares this header,
 * that table and the libraries' exports with one another. */
#ifndef REDNER_AMD_DEFERRED_QUAD_SHADOW_ABI_H
#define REDNER_AMD_DEFERRED_QUAD_SHADOW_ABI_H

#include "deferred_quad_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE RULE, in the order of the fp32 operations (dot and cross products as in csrc/deferred_quad.h; everything is fp32 unless
 * said otherwise).  K = shadow_rays, 1 .. 32.
 *   texel, quad   as in rdr_deferred_quad: position p, nh = n / sqrt(n.n), the texel gated by the same test (0 < n.n < inf,
 *                 p.p < inf); corners q0..q3, the flag two_sided, emitting side cross(q1 - q0, q3 - q0).
 *   sample table  uv[16][K][2], which the HOST computes in fp64 and rounds once to fp32 (no table arithmetic runs in a kernel).
 *                 For sample k of rotation j:  u = (k + ((j & 3) + 0.5) / 4) / K,
 *                                              v = radinv2(k) + ((j >> 2) + 0.5) / (4 K'),
 *                 radinv2 the base-2 radical inverse, K' the smallest power of two >= K.  Both lie strictly inside (0, 1); the
 *                 points are jittered within their strata, and the 16 rotations of a 4 x 4 block of texels interleave.  The
 *                 rotation of a texel is j = (x & 3) + 4 (y & 3), x and y its column and row in ITS image of the G-buffer (not
 *                 in a chunk of the pass): the rule of rdr_deferred_shade's ambient occlusion.
 *   point         a = q1 - q0,  b = q3 - q0,  g = (q2 - q1) - b
 *                 s = ((q0 + u a) + v b) + (u v) g
 *                 J = cross(a + v g, b + u g)          (constant for a parallelogram; carrying it makes the weights right for
 *                                                       any planar convex quad, with no square root)
 *   weight        d = s - p,  r2 = d.d,  cs = d.nh,  dj = d.J,  ce = two_sided ? |dj| : -dj
 *                 w = (cs ce) / (r2 r2)
 *                 The sample COUNTS iff r2 > 0, cs > 0, ce > 0, w is finite and positive, and every float of its ray is finite.
 *                 (The mean of w over the unit square is F, for a texel with the whole quad above its horizon.)
 *   ray           origin p,  dir = d / sqrtf(r2),  tmin = 1e-3f,  tmax = (1 - 1e-3f) sqrtf(r2): the offsets of the shadow rays of
 *                 rdr_deferred_shade, so the emitter's own mesh in the occluder scene is never hit.
 *   word          bit k is set iff sample k does not count or its ray found no triangle in (tmin, tmax); bits at and above K are 0.
 *                 A texel with no counting sample has the full mask; so has a background texel, a NaN texel, and every texel of
 *                 an image whose occluder is NULL.
 *   factor        den = sum of w_k over the counting samples, num = sum of w_k over the counting samples whose bit is set, both
 *                 summed for k = 0 .. K - 1 in that order, starting at +0.
 *                 V = (den > 0 and den finite) ? num / den : 1.  With every bit set num and den are the same bits: V == 1 exactly.
 *   shading       forward, F V stands where F stands in rdr_deferred_quad's  rgb[k] += (L[k] (a[k] / pi)) F;  in the adjoint dF is
 *                 multiplied by V, and F V stands in the albedo and radiance terms.  F * 1 == F: an unshadowed texel gives the
 *                 bits of rdr_deferred_quad, forward and backward.
 * The estimator is BIASED: E[num / den] is not E[num] / E[den]; the bias falls as 1 / K.
 *
 *   desc          the description of rdr_deferred_quad.  Forward: `occluders` is required, [num_images] scene handles of which
 *                 single entries may be NULL (that image is not shadowed: full words, factors 1), every scene on gpu_index;
 *                 `visibility` is required: the words, written here; ao_occluders, ao_words and ao_rays must be zero.
 *                 Backward: occluders and visibility must be zero as well (nothing is traced, the words are not read).
 *   shadow_rays   K, 1 .. 32
 *   factors       [pairs][height * aa][width * aa] floats, as are the words of desc->visibility (32-bit): pairs is the sum of the
 *                 images' range lengths, and the pair of quad l of image n is (the sum of the earlier images' lengths) +
 *                 l - range[2n].  The forward call writes every word and every factor; the backward call reads the factors.
 *                 A call whose pairs x texels does not fit a 32-bit signed index is refused.
 *   g_buffer, quads, image, d_image, d_g_buffer, d_quads    as in deferred_quad_abi.h
 * One pass per (image, quad, chunk of texels) over the call's stream: the texels with a counting sample are listed, their K rays
 * go into one ray-major queue, one any-hit launch answers them, and one lane per listed texel stores its word and factor.  The
 * host reads no count back; the scratch is bounded by the chunk, whatever the number of quads.  Everything is checked before
 * anything is launched; both calls synchronise before returning.  Return 0 on success; rdr_last_error has the text otherwise. */
int rdr_deferred_quad_shadowed(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, int shadow_rays,
                               float *factors, float *image);
int rdr_deferred_quad_shadowed_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads,
                                        const float *factors, const float *d_image, float *d_g_buffer, float *d_quads);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_DEFERRED_QUAD_SHADOW_ABI_H */
