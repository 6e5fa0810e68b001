/* redner_amd_image.h -- the image utilities of the C ABI that came after redner_amd.h was fixed at its present set of functions:
 * the Gaussian pyramid loss.  Include this header instead of redner_amd.h (it includes it); the functions live in the same library,
 * follow the same conventions (rdr_last_error, rdr_set_stream, device memory of gpu_index) and are bound by redner_amd/_capi.py
 * from its IMAGE_SIGNATURES table.  tests/test_pyramid_loss.py compares this header, that table and the library's exports with
 * one another. */
#ifndef REDNER_AMD_IMAGE_H
#define REDNER_AMD_IMAGE_H

#include "redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The Gaussian image pyramid loss that the reference's optimisation scripts end in, and its gradient (csrc/pyramid_loss.h, which
 * pins the meaning, the arithmetic and the summation orders).  image, target [batch, height, width, channels] fp32, contiguous;
 * num_levels = L >= 1 with min(height, width) >> (L - 1) >= 1, at most 16.
 *   D_0 = image - target, clamped to [-clamp, clamp] when clamp > 0 (clamp == 0: not clamped); level l + 1, of size
 *   floor(H_l / 2) x floor(W_l / 2), is D_l filtered with the 7 x 7 Gaussian a (x) a at ZERO padding 3 and averaged over 2 x 2
 *   (an odd side drops the filtered image's last row / column); a = [w3 + w4, w2, w1, w0, w1, w2, w3 + w4],
 *   w_k = exp(-k^2 / 2) / sum_{k = -4 .. 4} exp(-k^2 / 2), rounded to fp32;
 *   loss = sum_l weights[l] * sum(D_l^2) / ((height / 2^l) * (width / 2^l)), true division.  weights: HOST [L], NULL = all 1.
 *   rdr_pyramid_loss_scratch   floats the two calls need: `forward_floats` (scratch of rdr_pyramid_loss) and `backward_floats`
 *                              (scratch of rdr_pyramid_loss_backward).  Either may be NULL.
 *   rdr_pyramid_loss_plan      the launch plan: `tiled_levels` = T, the leading levels done by the tiled kernels (level 0 always;
 *                              a later level while it has more than `small_floats` floats per image); one workgroup per image
 *                              does the levels T .. L - 1.  Either may be NULL.
 *   rdr_pyramid_loss           writes loss[0] (fp32) and, unless NULL, terms[L] (fp64: the per-level terms, summed over the
 *                              batch).  Afterwards the start of `scratch` holds D_1 .. D_{L-1}, level l as [batch, H_l, W_l,
 *                              channels] with every level padded to a multiple of 64 floats: what the backward call takes as
 *                              `saved`.  T + 2 launches (T + 1 when T == L).
 *   rdr_pyramid_loss_backward  writes every element of d_image and, unless NULL, of d_target (= -d_image):
 *                              upstream[0] * d loss / d image, from the same image, target, weights and clamp and the forward
 *                              call's `saved` (at least the levels; not modified).  upstream: one float in DEVICE memory.
 *                              T + 1 launches (T when T == L).
 * The calls fail (rdr_last_error) for a size that is not positive, a side above 32768, more than 65535 images or 2^30 floats,
 * too many levels, a negative clamp, a required pointer that is NULL, or scratch / saved that is NULL, too short or (forward) not
 * aligned to 8 bytes.  Pointers are DEVICE memory of gpu_index unless marked HOST; a negative gpu_index means host memory and is
 * accepted by the CPU debugging harness only.  The library allocates nothing; launches are ordered on the rdr_set_stream stream
 * and NOT synchronised.  fp32 arithmetic in a fixed order, fp64 sums of squares in a fixed order rounded to fp32 once, gathers
 * only, no atomics: bitwise reproducible from run to run, and the harness computes the same bits as the kernels.
 * Return 0 on success. */
int rdr_pyramid_loss_scratch(int batch, int height, int width, int channels, int num_levels, int64_t *forward_floats,
                             int64_t *backward_floats);
int rdr_pyramid_loss_plan(int batch, int height, int width, int channels, int num_levels, int *tiled_levels, int *small_floats);
int rdr_pyramid_loss(const float *image, const float *target, int batch, int height, int width, int channels, int num_levels,
                     const float *weights, float clamp, float *loss, double *terms, float *scratch, int64_t scratch_floats,
                     int gpu_index);
int rdr_pyramid_loss_backward(const float *image, const float *target, int batch, int height, int width, int channels,
                              int num_levels, const float *weights, float clamp, const float *saved, int64_t saved_floats,
                              const float *upstream, float *d_image, float *d_target, float *scratch, int64_t scratch_floats,
                              int gpu_index);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_IMAGE_H */
