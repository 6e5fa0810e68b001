// mesh_smooth.h -- Laplacian smoothing of a triangle mesh: the displacement, its vertex adjoint, the in-place step and the
// boundary mask (rdr_mesh_boundary / rdr_mesh_laplacian / rdr_mesh_laplacian_backward / rdr_mesh_smooth).
//
// The meaning is that of pyredner/shape.py:130-277 (bound_vertices, smooth).  vertices [V, 3] fp32, indices [T, 3] int32,
// control [V] fp32 (NULL = all 1).  Corner c = 3 f + k is corner k of face f; its sides e1, e2, their unit vectors a, b and
// the predicates `live` (|e1| |e2| > 0) and `spread` (live, and the sides do not coincide) are vnrm::corner_of, its angle is
// vnrm::corner_angle and cot = 1 / tan(angle) is vnrm::cotangent_of (vertex_normal.h: the bodies are called, not restated).
//
// Every vertex i gets a vector sum C_i and a scalar sum W_i (the reference's total_weight_contrib has three equal columns):
//   'reciprocal'  a live corner at vertex i adds  a + b  to C_i and  1 / |e1| + 1 / |e2|  to W_i
//   'uniform'     a live corner at vertex i adds  e1 + e2  to C_i and  2  to W_i
//   'cotangent'   a spread corner i of a face adds  w = (p[i+2] - p[i+1]) * cot  to C of vertex i + 1 and  -w  to C of vertex
//                 i + 2, and  cot  to W of both
// A corner that is not live (not spread, for 'cotangent') adds nothing.  (As for the normals, a corner of a zero-area face whose
// sides point in opposite directions IS spread: it adds, like the reference, with cot = 1 / tan(fp32 pi), and its gradient is 0.)  Then
//   shift_i = (C_i / W_i) * control_i       in fp32, in that order; 0 where W_i == 0 (an isolated vertex, a vertex of
//                                           degenerate corners only): such a vertex does not move.  (The reference: NaN.)
//   smooth:   v_i = v_i + shift_i * lmd     lmd an fp32 number; two roundings, no contraction
//   bound[i] = 1 where the sum over the corners c = 3 f + k at i of  indices[3 f + (k+2) % 3] - indices[3 f + (k+1) % 3]  is 0,
//              otherwise 0.  Summed in int64: exact for any mesh (the reference sums the same integers in fp32).
//
// ARITHMETIC AND ORDER are those of vertex_normal.h: per-corner terms in fp32, operation by operation, no contraction; the
// per-vertex sums in fp64 IN ASCENDING CORNER ID over the plan's row, rounded once to fp32.  For 'cotangent' corner c = 3 f + k
// brings two addends, in this order: + w and + cot of corner (k + 2) % 3, then - w and + cot of corner (k + 1) % 3, of face f.
//
// THE ADJOINT (control is a constant).  With g = d loss / d shift:  dC_i = g_i control_i / W_i,
// dW_i = -(g_i . C_i) control_i / W_i^2, both 0 where W_i == 0; evaluated in fp64 at the fp32 vertices from the saved fp32 sums
// (saved = C [V, 3], then W [V]).  The corner terms are differentiated in their closed forms, cot = (e1 . e2) / |e1 x e2|
// (vnrm::cotangent_corner_adjoint with u = h . (p2 - p1) + dW_{i+1} + dW_{i+2}, h = dC_{i+1} - dC_{i+2}); which corners count is
// decided by the fp32 predicates of the forward pass, recomputed.  One record per corner; vnrm::vertex_gather sums them.
//
// KERNELS.  One lane per item, 256 lanes per workgroup, grid ceil(n / 256).
//   ms_face_kernel<SCHEME>           a face: per corner 3 floats for C and 1 for W                                   -> scratch
//   ms_vertex_kernel<SCHEME, APPLY>  a vertex: gathers its row in order; writes shift and saved, or with APPLY
//                                    vertices_out = vertices_in + shift * lmd (in place is allowed: a vertex touches its own
//                                    row only, and the face kernel of that step has finished)
//   ms_boundary_kernel               a vertex: the integer sum over its row                                          -> bound
//   ms_face_adjoint_kernel<SCHEME>   a face: one d_position record per corner; summed by vnrm::vn_gather_kernel     -> d_vertices
// Gathers and plain stores only: no float atomics, no buffer that must be zero, every element of every output is written,
// bitwise reproducible.  The library allocates nothing per call and does not synchronise; the plan (vnrm::Topology) is read only.
// The per-item bodies are shared with the plain loops of the CPU harness.
#pragma once
#include "../../include/redner_amd_mesh.h"
#include "vertex_normal.h"

namespace rdr {
namespace msm {

using vnrm::D3;
using vnrm::F3;
using vnrm::Topology;

constexpr int kReciprocal = rdr_smooth_weighting_reciprocal, kUniform = rdr_smooth_weighting_uniform,
              kCotangent = rdr_smooth_weighting_cotangent;

// ---- the forward pass, per item --------------------------------------------------------------------------------------------
// A face: rec[4 c ..] = what corner c adds (C: 3 floats, W: 1).  For 'cotangent' it is (w, cot) of corner c, which goes to the
// OTHER two vertices of the face.
template <int SCHEME>
RDR_FN void face_forward(const float *vertices, const int *indices, int f, float *rec) {
    const size_t c0 = (size_t)3 * f;
    F3 p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = vnrm::load3(vertices + (size_t)3 * indices[c0 + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const F3 p1 = p[(k + 1) % 3], p2 = p[(k + 2) % 3];
        const vnrm::Corner c = vnrm::corner_of(p[k], p1, p2);
        F3 add{0.f, 0.f, 0.f};
        float weight = 0.f;
        if (SCHEME == kCotangent) {
            if (c.spread) {
                weight = vnrm::cotangent_of(vnrm::corner_angle(c));
                add = (p2 - p1) * weight;
            }
        } else if (c.live) {
            const F3 e1 = p1 - p[k], e2 = p2 - p[k];
            if (SCHEME == kReciprocal) {
                add = c.a + c.b;
                weight = 1.0f / vnrm::length(e1) + 1.0f / vnrm::length(e2);
            } else {
                add = e1 + e2;
                weight = 2.0f;
            }
        }
        float *r = rec + 4 * (c0 + k);
        vnrm::store3(r, add);
        r[3] = weight;
    }
}

// The two sums of a vertex, rounded once: gathered over its row in the canonical order.
struct Sums { F3 c; float w; };
template <int SCHEME>
RDR_FN Sums vertex_sums(const int *offsets, const int *corners, const float *rec, int v) {
    D3 sc{0.0, 0.0, 0.0};
    double sw = 0.0;
    for (int j = offsets[v]; j < offsets[v + 1]; ++j) {
        const int c = corners[j];
        if (SCHEME != kCotangent) {
            const float *r = rec + (size_t)4 * c;
            sc.x += (double)r[0]; sc.y += (double)r[1]; sc.z += (double)r[2];
            sw += (double)r[3];
        } else {
            const int f = c / 3, k = c - 3 * f;
            const float *plus = rec + 4 * ((size_t)3 * f + (k + 2) % 3), *minus = rec + 4 * ((size_t)3 * f + (k + 1) % 3);
            sc.x += (double)plus[0]; sc.y += (double)plus[1]; sc.z += (double)plus[2];
            sw += (double)plus[3];
            sc.x -= (double)minus[0]; sc.y -= (double)minus[1]; sc.z -= (double)minus[2];
            sw += (double)minus[3];
        }
    }
    return Sums{vnrm::narrow(sc), (float)sw};
}
// what moves: the fp32 predicate the adjoint recomputes from the saved W
RDR_FN bool moves(float w) { return w != 0.f; }

// A vertex.  !APPLY: writes shift [V, 3] and saved (C [V, 3], then W [V]).  APPLY: writes vertices_out[v] = vertices_in[v] +
// shift * lmd, and nothing else (vertices_out may be vertices_in).
template <int SCHEME, bool APPLY>
RDR_FN void vertex_forward(const int *offsets, const int *corners, const float *rec, const float *control, int v, int num_vertices,
                           float *shift, float *saved, const float *vertices_in, float lmd, float *vertices_out) {
    const Sums s = vertex_sums<SCHEME>(offsets, corners, rec, v);
    F3 move{0.f, 0.f, 0.f};
    if (moves(s.w)) move = (s.c / s.w) * (control ? control[v] : 1.0f);
    if (!APPLY) {
        vnrm::store3(shift + (size_t)3 * v, move);
        vnrm::store3(saved + (size_t)3 * v, s.c);
        saved[(size_t)3 * num_vertices + v] = s.w;
    } else {
        vnrm::store3(vertices_out + (size_t)3 * v, vnrm::load3(vertices_in + (size_t)3 * v) + move * lmd);
    }
}

// A vertex: bound[v] from the integer sum over its row
RDR_FN void vertex_boundary(const int *offsets, const int *corners, const int *indices, int v, float *bound) {
    long long sum = 0;
    for (int j = offsets[v]; j < offsets[v + 1]; ++j) {
        const int c = corners[j], f = c / 3, k = c - 3 * f;
        sum += (long long)indices[(size_t)3 * f + (k + 2) % 3] - (long long)indices[(size_t)3 * f + (k + 1) % 3];
    }
    bound[v] = sum == 0 ? 1.0f : 0.0f;
}

// ---- the adjoint, per item ---------------------------------------------------------------------------------------------------
// (dC, dW) of vertex v: the adjoint of shift = (C / W) * control
struct SumGrad { D3 c; double w; };
RDR_FN SumGrad vertex_adjoint(const float *saved, const float *control, const float *d_shift, int v, int num_vertices) {
    SumGrad d{D3{0.0, 0.0, 0.0}, 0.0};
    const float w = saved[(size_t)3 * num_vertices + v];
    if (!moves(w)) return d;
    const D3 g = vnrm::widen(vnrm::load3(d_shift + (size_t)3 * v)), C = vnrm::widen(vnrm::load3(saved + (size_t)3 * v));
    const double W = (double)w, ctl = control ? (double)control[v] : 1.0;
    d.c = g * (ctl / W);
    d.w = -vnrm::dot(g, C) * ctl / (W * W);
    return d;
}

// A face: rec[3 c ..] = d loss / d position of the vertex at corner c through this face (all three corners' terms).
template <int SCHEME>
RDR_FN void face_adjoint(const float *vertices, const int *indices, const float *saved, const float *control, const float *d_shift,
                         int num_vertices, int f, float *rec) {
    const size_t c0 = (size_t)3 * f;
    const D3 zero{0.0, 0.0, 0.0};
    F3 p[3];
    D3 P[3], dp[3] = {zero, zero, zero};
    SumGrad d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = indices[c0 + k];
        p[k] = vnrm::load3(vertices + (size_t)3 * v);
        P[k] = vnrm::widen(p[k]);
        d[k] = vertex_adjoint(saved, control, d_shift, v, num_vertices);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const vnrm::Corner c = vnrm::corner_of(p[k], p[k1], p[k2]);
        if (SCHEME == kCotangent) {
            // corner k: (h . (p2 - p1) + dW_{k+1} + dW_{k+2}) (e1 . e2) / |e1 x e2|, h = dC_{k+1} - dC_{k+2}
            if (!c.spread) continue;
            const D3 h = d[k1].c - d[k2].c;
            vnrm::cotangent_corner_adjoint(P, k, h, vnrm::dot(h, P[k2] - P[k1]) + d[k1].w + d[k2].w, dp);
        } else {
            if (!c.live) continue;
            D3 de1 = d[k].c, de2 = d[k].c;                       // 'uniform': dC_k . (e1 + e2); W is a constant
            if (SCHEME == kReciprocal) {
                // dC_k . (e1 / |e1| + e2 / |e2|) + dW_k (1 / |e1| + 1 / |e2|)
                const D3 e1 = P[k1] - P[k], e2 = P[k2] - P[k];
                const double q1 = vnrm::dot(e1, e1), q2 = vnrm::dot(e2, e2), i1 = 1.0 / sqrt(q1), i2 = 1.0 / sqrt(q2);
                const D3 a = e1 * i1, b = e2 * i2;
                de1 = (d[k].c - a * vnrm::dot(a, d[k].c)) * i1 - a * (d[k].w / q1);
                de2 = (d[k].c - b * vnrm::dot(b, d[k].c)) * i2 - b * (d[k].w / q2);
            }
            dp[k1] = dp[k1] + de1;
            dp[k2] = dp[k2] + de2;
            dp[k] = dp[k] - (de1 + de2);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) vnrm::store3(rec + 3 * (c0 + k), vnrm::narrow(dp[k]));
}

#if !defined(RDR_HOSTSIM)
template <int SCHEME>
__global__ void __launch_bounds__(256) ms_face_kernel(const float *__restrict__ vertices, const int *__restrict__ indices,
                                                      int num_triangles, float *__restrict__ rec) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)num_triangles) face_forward<SCHEME>(vertices, indices, (int)f, rec);
}
// (vertices_in and vertices_out may be the same memory: neither is __restrict__)
template <int SCHEME, bool APPLY>
__global__ void __launch_bounds__(256) ms_vertex_kernel(const int *__restrict__ offsets, const int *__restrict__ corners,
                                                        const float *__restrict__ rec, const float *__restrict__ control,
                                                        int num_vertices, float *__restrict__ shift, float *__restrict__ saved,
                                                        const float *vertices_in, float lmd, float *vertices_out) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)num_vertices)
        vertex_forward<SCHEME, APPLY>(offsets, corners, rec, control, (int)v, num_vertices, shift, saved, vertices_in, lmd, vertices_out);
}
__global__ void __launch_bounds__(256) ms_boundary_kernel(const int *__restrict__ offsets, const int *__restrict__ corners,
                                                          const int *__restrict__ indices, int num_vertices,
                                                          float *__restrict__ bound) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)num_vertices) vertex_boundary(offsets, corners, indices, (int)v, bound);
}
template <int SCHEME>
__global__ void __launch_bounds__(256) ms_face_adjoint_kernel(const float *__restrict__ vertices, const int *__restrict__ indices,
                                                              const float *__restrict__ saved, const float *__restrict__ control,
                                                              const float *__restrict__ d_shift, int num_vertices,
                                                              int num_triangles, float *__restrict__ rec) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)num_triangles) face_adjoint<SCHEME>(vertices, indices, saved, control, d_shift, num_vertices, (int)f, rec);
}
#endif

inline int scheme_of(int scheme, const char *who) {
    if (scheme != kReciprocal && scheme != kUniform && scheme != kCotangent)
        throw std::runtime_error(std::string(who) + ": unknown weighting scheme " + std::to_string(scheme));
    return scheme;
}
// floats: the corner records of the forward pass and of a smoothing step / of the adjoint / what the forward pass saves
inline size_t forward_scratch_floats(const Topology &t) { return (size_t)12 * t.num_triangles; }
inline size_t backward_scratch_floats(const Topology &t) { return (size_t)9 * t.num_triangles; }
inline size_t saved_floats(const Topology &t) { return (size_t)4 * t.num_vertices; }

// rdr_mesh_boundary: writes every element of bound [V]; stream-ordered, not synchronised
inline void boundary(const Topology &t, float *bound) {
    if (!bound) throw std::runtime_error("rdr_mesh_boundary: bound is required");
#if !defined(RDR_HOSTSIM)
    hipLaunchKernelGGL(ms_boundary_kernel, exec::grid_of(t.num_vertices), dim3(256), 0, exec::ctx().stream, t.offsets, t.corners,
                       t.indices, t.num_vertices, bound);
    exec::check(hipGetLastError(), "ms_boundary launch");
#else
    for (int v = 0; v < t.num_vertices; ++v) vertex_boundary(t.offsets, t.corners, t.indices, v, bound);
#endif
}

// one pass: the face records of `vertices_in`, then every vertex
template <int SCHEME, bool APPLY>
inline void forward_impl(const Topology &t, const float *control, float *shift, float *saved, const float *vertices_in, float lmd,
                         float *vertices_out, float *rec) {
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (t.num_triangles > 0) {
        hipLaunchKernelGGL(ms_face_kernel<SCHEME>, exec::grid_of(t.num_triangles), dim3(256), 0, stream, vertices_in, t.indices,
                           t.num_triangles, rec);
        exec::check(hipGetLastError(), "ms_face launch");
    }
    hipLaunchKernelGGL((ms_vertex_kernel<SCHEME, APPLY>), exec::grid_of(t.num_vertices), dim3(256), 0, stream, t.offsets, t.corners,
                       (const float *)rec, control, t.num_vertices, shift, saved, vertices_in, lmd, vertices_out);
    exec::check(hipGetLastError(), "ms_vertex launch");
#else
    for (int f = 0; f < t.num_triangles; ++f) face_forward<SCHEME>(vertices_in, t.indices, f, rec);
    for (int v = 0; v < t.num_vertices; ++v)
        vertex_forward<SCHEME, APPLY>(t.offsets, t.corners, rec, control, v, t.num_vertices, shift, saved, vertices_in, lmd, vertices_out);
#endif
}

template <int SCHEME>
inline void backward_impl(const Topology &t, const float *vertices, const float *control, const float *saved, const float *d_shift,
                          float *d_vertices, float *rec) {
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (t.num_triangles > 0) {
        hipLaunchKernelGGL(ms_face_adjoint_kernel<SCHEME>, exec::grid_of(t.num_triangles), dim3(256), 0, stream, vertices, t.indices,
                           saved, control, d_shift, t.num_vertices, t.num_triangles, rec);
        exec::check(hipGetLastError(), "ms_face_adjoint launch");
    }
    hipLaunchKernelGGL(vnrm::vn_gather_kernel, exec::grid_of(t.num_vertices), dim3(256), 0, stream, t.offsets, t.corners,
                       (const float *)rec, t.num_vertices, d_vertices);
    exec::check(hipGetLastError(), "vn_gather launch");
#else
    for (int f = 0; f < t.num_triangles; ++f) face_adjoint<SCHEME>(vertices, t.indices, saved, control, d_shift, t.num_vertices, f, rec);
    for (int v = 0; v < t.num_vertices; ++v) vnrm::vertex_gather(t.offsets, t.corners, rec, v, d_vertices);
#endif
}

// rdr_mesh_laplacian: writes every element of shift [V, 3] and of saved; stream-ordered, not synchronised
inline void laplacian(const Topology &t, int scheme, const float *vertices, const float *control, float *shift, float *saved,
                      float *scratch, size_t scratch_count) {
    scheme_of(scheme, "rdr_mesh_laplacian");
    if (!vertices || !shift || !saved) throw std::runtime_error("rdr_mesh_laplacian: vertices, shift and saved are required");
    need_scratch("rdr_mesh_laplacian", forward_scratch_floats(t), scratch, scratch_count);
    if (scheme == kReciprocal) forward_impl<kReciprocal, false>(t, control, shift, saved, vertices, 0.f, nullptr, scratch);
    else if (scheme == kUniform) forward_impl<kUniform, false>(t, control, shift, saved, vertices, 0.f, nullptr, scratch);
    else forward_impl<kCotangent, false>(t, control, shift, saved, vertices, 0.f, nullptr, scratch);
}

// rdr_mesh_laplacian_backward: writes every element of d_vertices [V, 3]; stream-ordered, not synchronised
inline void laplacian_backward(const Topology &t, int scheme, const float *vertices, const float *control, const float *saved,
                               const float *d_shift, float *d_vertices, float *scratch, size_t scratch_count) {
    scheme_of(scheme, "rdr_mesh_laplacian_backward");
    if (!vertices || !saved || !d_shift || !d_vertices)
        throw std::runtime_error("rdr_mesh_laplacian_backward: vertices, saved, d_shift and d_vertices are required");
    need_scratch("rdr_mesh_laplacian_backward", backward_scratch_floats(t), scratch, scratch_count);
    if (scheme == kReciprocal) backward_impl<kReciprocal>(t, vertices, control, saved, d_shift, d_vertices, scratch);
    else if (scheme == kUniform) backward_impl<kUniform>(t, vertices, control, saved, d_shift, d_vertices, scratch);
    else backward_impl<kCotangent>(t, vertices, control, saved, d_shift, d_vertices, scratch);
}

// rdr_mesh_smooth: `iterations` steps v = v + shift(v) * lmd; the first reads vertices_in, every step writes every element of
// vertices_out [V, 3] (which may be vertices_in), the later ones in place.  Stream-ordered, not synchronised.
inline void smooth(const Topology &t, int scheme, const float *vertices_in, const float *control, float lmd, int iterations,
                   float *vertices_out, float *scratch, size_t scratch_count) {
    scheme_of(scheme, "rdr_mesh_smooth");
    if (iterations < 1) throw std::runtime_error("rdr_mesh_smooth: iterations must be at least 1");
    if (!vertices_in || !vertices_out) throw std::runtime_error("rdr_mesh_smooth: vertices_in and vertices_out are required");
    need_scratch("rdr_mesh_smooth", forward_scratch_floats(t), scratch, scratch_count);
    for (int it = 0; it < iterations; ++it) {
        const float *from = it == 0 ? vertices_in : vertices_out;
        if (scheme == kReciprocal) forward_impl<kReciprocal, true>(t, control, nullptr, nullptr, from, lmd, vertices_out, scratch);
        else if (scheme == kUniform) forward_impl<kUniform, true>(t, control, nullptr, nullptr, from, lmd, vertices_out, scratch);
        else forward_impl<kCotangent, true>(t, control, nullptr, nullptr, from, lmd, vertices_out, scratch);
    }
}

} // namespace msm
} // namespace rdr
