/* deferred_specular_abi.h -- a companion header of the C ABI: specular highlights in deferred shading, the specular half of the
 * path tracer's BSDF (Blinn-Phong distribution, Smith shadowing, Schlick Fresnel; csrc/bsdf.h) evaluated on a G-buffer under the
 * point, spot and directional rows of rdr_deferred_shade's light table, and its gradient.  Include this header instead of
 * include/redner_amd.h (it includes it); the functions live in the same library, follow the same conventions (rdr_last_error,
 * rdr_set_stream, device memory of gpu_index) and are bound by redner_amd/_capi.py from its CSRC_HEADERS table.  It stands here
 * and not under include/ because the set of files there, and the functions each declares, are pinned (tests/test_capi.py);
 * tests/test_deferred_specular.py compares this header, that table and the libraries' exports with one another. */
#ifndef REDNER_AMD_DEFERRED_SPECULAR_ABI_H
#define REDNER_AMD_DEFERRED_SPECULAR_ABI_H

#include "../../include/redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* csrc/deferred_specular.h pins the meaning and the order of the fp32 operations.  Per texel of the oversampled G-buffer, with
 * position p, shading normal n as stored, specular reflectance ks[3], roughness rho, and the eye of the texel's image:
 *   nn = n.n, nh = n / sqrt(nn)                  no specular unless 0 < nn < inf (background texels have n = 0)
 *   v = (eye - p) / |eye - p|, cv = nh.v         no specular unless cv > 0
 *   per light (l, E):  point        d = pos - p, l = d / |d|, E = I / d.d
 *                      spot         l as point, s = -sdir / |sdir|, E = I pow(max(l.s, 0), e_spot)
 *                      directional  l = -dir / |dir|, E = I
 *                      ambient rows and SH rows add no specular; their parameter gradients from these calls are exactly 0
 *   cl = nh.l                                    no specular unless cl > 1e-3
 *   m = (v + l) / |v + l|, cm = nh.m             no specular unless cm > 0
 *   r = max(rho, 1e-3), e = max(2 / r - 2, 0), D = pow(cm, e) (e + 2) / (2 pi)
 *   G1(c): t = sqrt(max(1 / (c c) - 1, 0)); t == 0: 1; a = 1 / (sqrt(r) t); a >= 1.6: 1;
 *          else (3.535 a + 2.181 a a) / (1 + 2.276 a + 2.577 a a);      G = G1(cv) G1(cl)
 *   F_k = k_k + (1 - k_k) pow(max(1 - |m.l|, 0), 5), k_k = max(ks_k, 0)
 *   texel_rgb[k] += E_k F_k D G / (4 cv)
 * and the image [num_images, height, width, 3] is the mean over each aa_samples x aa_samples block (no alpha channel).
 *   desc          the description of rdr_deferred_shade (sizes, alpha, the light table's types and ranges, gpu_index).  occluders,
 *                 ao_occluders, ao_words and ao_rays must be zero: nothing is traced.  `visibility`, optional, is READ in both
 *                 calls: the words rdr_deferred_shade wrote; a light whose bit (row - range[2n]) is clear adds nothing to the
 *                 texel nor to any gradient.  With `visibility`, an image may have at most 32 lights.
 *   g_buffer      [num_images, height * aa, width * aa, 9 + alpha]: the diffuse pass's own buffer; p and n are read
 *   material      [num_images, height * aa, width * aa, 4]: ks rgb, then roughness; 16-byte aligned
 *   eye           [num_images, 3]
 *   light_params  [num_lights, 10], as for rdr_deferred_shade
 * rdr_deferred_specular writes every element of image.  rdr_deferred_specular_backward writes every element of d_g_buffer (the
 * position and normal channels; the albedo and alpha channels are 0), d_material, d_eye and d_light_params, from the upstream
 * gradient d_image [num_images, height, width, 3].  The derivatives are those of the expression above: every max(x, 0) and the
 * roughness floor pass half the gradient at the tie; the conditions and the visibility bits are constants; no gradient of a
 * gated texel is anything but 0.  The light and eye gradients are fp64 partial sums per workgroup folded in a fixed order and
 * rounded once: no atomics, the same bits from run to run.  Pointers are DEVICE memory of gpu_index (a negative gpu_index: host
 * memory, accepted by the CPU debugging harness only); with alpha the G-buffers must be 8-byte aligned.  Everything is checked
 * before anything is launched; launches are ordered on the rdr_set_stream stream; both calls synchronise before returning.
 * Return 0 on success. */
int rdr_deferred_specular(const rdr_deferred_desc *desc, const float *g_buffer, const float *material, const float *eye,
                          const float *light_params, float *image);
int rdr_deferred_specular_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *material, const float *eye,
                                   const float *light_params, const float *d_image, float *d_g_buffer, float *d_material,
                                   float *d_eye, float *d_light_params);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_DEFERRED_SPECULAR_ABI_H */
