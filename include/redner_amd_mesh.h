/* redner_amd_mesh.h -- the mesh utilities of the C ABI that came after redner_amd.h was fixed at its present set of functions:
 * Laplacian smoothing.  Include this header instead of redner_amd.h (it includes it); the functions live in the same library,
 * follow the same conventions (rdr_last_error, rdr_set_stream, device memory of the plan's place) and are bound by
 * redner_amd/_capi.py from its MESH_SIGNATURES table.  tests/test_mesh_smooth.py compares this header, that table and the
 * library's exports with one another. */
#ifndef REDNER_AMD_MESH_H
#define REDNER_AMD_MESH_H

#include "redner_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Laplacian smoothing of a triangle mesh (pyredner/shape.py:130-277, bound_vertices and smooth) on the plan of
 * redner_amd.h, rdr_mesh_topology_create (csrc/mesh_smooth.h, which pins the meaning, the arithmetic and the summation order).  control [V] fp32, NULL = all 1.
 *   rdr_mesh_boundary            writes bound [V]: 1 where the signed sum of the opposite edges' index differences over the
 *                                vertex's corners is 0 (an interior or isolated vertex), 0 on an open rim.  Integer arithmetic.
 *   rdr_mesh_smooth_scratch      floats the buffers of a scheme need: `forward_floats` (scratch of rdr_mesh_laplacian and of
 *                                rdr_mesh_smooth), `backward_floats` (scratch of rdr_mesh_laplacian_backward), `saved_floats`
 *                                (what the forward call saves: C [V, 3], then W [V]).  Any of the three may be NULL.
 *   rdr_mesh_laplacian           writes every element of shift [V, 3] = (C / W) * control and of saved; 0 where W == 0.
 *   rdr_mesh_laplacian_backward  writes every element of d_vertices [V, 3] from d_shift [V, 3], the vertices, the same control
 *                                and `saved` of the forward call.  control is a constant.
 *   rdr_mesh_smooth              `iterations` (>= 1) steps vertices = vertices + shift * lmd; writes every element of
 *                                vertices_out [V, 3], which may be vertices_in.
 * Memory, scratch, ordering and reproducibility as for rdr_vertex_normal: two launches per step and each way (rdr_mesh_boundary:
 * one), nothing allocated, NOT synchronised, no float atomics.  Return 0 on success. */
typedef enum { rdr_smooth_weighting_reciprocal = 0, rdr_smooth_weighting_uniform = 1, rdr_smooth_weighting_cotangent = 2 } rdr_smooth_weighting;
int rdr_mesh_boundary(const rdr_mesh_topology *topology, float *bound);
int rdr_mesh_smooth_scratch(const rdr_mesh_topology *topology, int scheme, int64_t *forward_floats, int64_t *backward_floats,
                            int64_t *saved_floats);
int rdr_mesh_laplacian(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *control, float *shift,
                       float *saved, float *scratch, int64_t scratch_floats);
int rdr_mesh_laplacian_backward(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *control,
                                const float *saved, const float *d_shift, float *d_vertices, float *scratch, int64_t scratch_floats);
int rdr_mesh_smooth(const rdr_mesh_topology *topology, int scheme, const float *vertices_in, const float *control, float lmd,
                    int iterations, float *vertices_out, float *scratch, int64_t scratch_floats);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_MESH_H */
