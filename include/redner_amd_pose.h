/* redner_amd_pose.h -- the third companion header of the C ABI: the rigid pose of the reference's pose-estimation scripts (the
 * rotation matrix of three Euler angles; rotate vertex sets about a centre and translate them) and its gradient.  Include this
 * header instead of redner_amd.h (it includes it); the functions live in the same library, follow the same conventions
 * (rdr_last_error, rdr_set_stream, device memory of gpu_index) and are bound by redner_amd/_capi.py from its POSE_SIGNATURES
 * table.  tests/test_pose.py compares this header, that table and the library's exports with one another. */
#ifndef REDNER_AMD_POSE_H
#define REDNER_AMD_POSE_H

#include "redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* csrc/pose.h pins the meaning, the arithmetic and the summation order.  angles = (theta, phi, psi), translation, center: [3]
 * fp32; matrix [3, 3] fp32, row-major: R = Rz(psi) (Ry(phi) Rx(theta)) in the convention of pyredner.gen_rotate_matrix, formed in
 * fp64 from glibc-exact sines and cosines and rounded once.  num_sets = K in [1, 16] vertex sets; counts: HOST [K], every one at
 * least 1, 2^30 vertices at most in all; vertices, out, d_out, d_vertices: HOST tables of K pointers to [counts[k], 3] fp32.
 *   out_k = (v_k - c) R^T + c + translation;  c = center, or, when center is NULL, the mean over all the vertices of all the sets
 *   (an fp64 sum in a fixed order, rounded once).
 *   rdr_pose_scratch             floats of scratch of rdr_pose_vertices with center == NULL (`forward_floats`; a given centre needs
 *                                none) and of rdr_pose_vertices_backward (`backward_floats`).  Either may be NULL.
 *   rdr_pose_plan                the launch plan of these set sizes: a set is cut into chunks of `chunk_vertices` vertices, and
 *                                `workgroups` = min(chunks, `max_workgroups`) workgroups own the chunks round-robin.  Any may be NULL.
 *   rdr_rotate_matrix            writes matrix[9].  One launch.
 *   rdr_rotate_matrix_backward   writes d_angles[3] = d_matrix : dR / d angles.  One launch.
 *   rdr_pose_vertices            writes every element of every out[k] and saved[12]: R, then the centre that was used.  Two
 *                                launches, one when a centre is given.
 *   rdr_pose_vertices_backward   from the same vertices and angles and the forward call's `saved`; own_center != 0 when that call
 *                                had center == NULL.  d_out[k] == NULL counts as zeros.  Writes d_angles[3], d_translation[3],
 *                                d_center[3] (own_center == 0; otherwise it may be NULL and is not written) and every element of
 *                                every d_vertices[k] that is not NULL (d_vertices itself may be NULL).  Two launches.
 * The calls fail (rdr_last_error) for a number of sets outside [1, 16], a count below 1, a required pointer that is NULL, or
 * scratch that is NULL, too short or not aligned to 8 bytes.  Pointers are DEVICE memory of gpu_index unless marked HOST; a
 * negative gpu_index means host memory and is accepted by the CPU debugging harness only.  The library allocates nothing;
 * launches are ordered on the rdr_set_stream stream and NOT synchronised: angles, translation, center and saved are read on the
 * device.  fp64 sums in a fixed order, no atomics: bitwise reproducible from run to run, the same bits in both builds and in the
 * harness.  Return 0 on success. */
int rdr_pose_scratch(int num_sets, const int *counts, int64_t *forward_floats, int64_t *backward_floats);
int rdr_pose_plan(int num_sets, const int *counts, int *chunk_vertices, int *max_workgroups, int *workgroups);
int rdr_rotate_matrix(const float *angles, float *matrix, int gpu_index);
int rdr_rotate_matrix_backward(const float *angles, const float *d_matrix, float *d_angles, int gpu_index);
int rdr_pose_vertices(int num_sets, const float *const *vertices, const int *counts, const float *angles, const float *translation,
                      const float *center, float *const *out, float *saved, float *scratch, int64_t scratch_floats, int gpu_index);
int rdr_pose_vertices_backward(int num_sets, const float *const *vertices, const int *counts, const float *angles, const float *saved,
                               int own_center, const float *const *d_out, float *const *d_vertices, float *d_angles,
                               float *d_translation, float *d_center, float *scratch, int64_t scratch_floats, int gpu_index);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_POSE_H */
