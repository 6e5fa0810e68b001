// pose.h -- the rigid pose of the reference's pose-estimation scripts and its gradient: the rotation matrix of three Euler angles
// (rdr_rotate_matrix / rdr_rotate_matrix_backward) and "rotate every vertex set about a centre, then translate"
// (rdr_pose_vertices / rdr_pose_vertices_backward).
//
// THE MEANING.  angles = (theta, phi, psi), translation t, centre c: [3] fp32; K <= kMaxSets vertex sets v_k [N_k, 3] fp32, N_k >= 1.
//   R = Rz(psi) (Ry(phi) Rx(theta)) in the convention of pyredner/transform.py (gen_rotate_matrix): with s / c for sin / cos,
//       R = [ c_psi c_phi ,  c_psi s_phi s_theta - s_psi c_theta ,  -c_psi s_phi c_theta - s_psi s_theta ]
//           [ s_psi c_phi ,  s_psi s_phi s_theta + c_psi c_theta ,  -s_psi s_phi c_theta + c_psi s_theta ]
//           [ s_phi       ,  -c_phi s_theta                      ,   c_phi c_theta                       ]
//   out_k = (v_k - c) R^T + c + t for every set; c is given, or (own centre) the mean over ALL the vertices of all the sets.
//
// THE ARITHMETIC.
//   * The six sines and cosines are gm::sin / gm::cos (libm_exact.h) of double(angle), called by name in every build: the harness
//     and both product libraries form the same bits.  The nine entries are formed in fp64 in the order `rotation` writes them
//     (products left to right, then the one addition or subtraction) and each is rounded to fp32 ONCE; the three derivative
//     matrices dR / d theta, dR / d phi, dR / d psi (`rotation_derivative`) are formed the same way and stay fp64.
//   * Own centre: the fp64 sum of the fp32 coordinates in THE FIXED ORDER below, divided by the total count, rounded to fp32 once.
//   * Forward, fp32, no contraction (pose_vertex):   d = v - c;   out_i = (((R_i0 d_0 + R_i1 d_1) + R_i2 d_2) + c_i) + t_i.
//   * Backward, g the upstream gradient (a set without one counts as zeros), d as above:
//       S_ij = sum_n g_ni d_nj,  G_i = sum_n g_ni      fp64 (a product of two fp32 numbers is exact there), THE FIXED ORDER
//       d_translation = fp32(G)
//       d_angles_k    = fp32(sum over (i, j) ascending, from 0.0, of dR_k,ij * S_ij)
//       E_j           = G_j - ((R_0j G_0 + R_1j G_1) + R_2j G_2)      fp64, R the fp32 entries widened
//       d_center      = fp32(E)                           (a given centre)
//       d_v_nj        = (g_n0 R_0j + g_n1 R_1j) + g_n2 R_2j   in fp32; own centre: + fp32(E_j / N_total), added last
//     rdr_rotate_matrix_backward: d_angles_k = fp32(sum over (i, j) ascending, from 0.0, of dR_k,ij * double(d_matrix_ij)).
//
// THE FIXED ORDER is a function of the set sizes only.  Set k is cut into ceil(N_k / kChunk) chunks of kChunk vertices (the last
// one may be partial); the chunks of all sets are numbered in ascending (set, chunk) order, C in all.  P = min(C, kMaxGroups)
// workgroups of kThreads lanes; workgroup w owns the chunks w, w + P, w + 2 P, ...
//   * in a chunk, lane t adds the vertices t, t + kThreads, ... of the chunk in ascending order, from 0.0 (lane_coords / lane_moments);
//   * the kThreads lane sums are folded by the tree  for s = kThreads / 2, ..., 1:  x[t] += x[t + s] for t < s;  x[0] is the chunk's sum;
//   * a workgroup adds its chunks' sums in ascending chunk order, from 0.0: its partial;
//   * the partials are added in ascending workgroup order, from 0.0 (fold).  Every quantity (3 coordinates, or the 12 sums S_00, S_01,
//     ..., S_22, G_0, G_1, G_2) has its own sum.
// No atomics; bitwise reproducible from run to run; the harness's plain loops add in exactly this order through the same bodies.
//
// THE LAUNCH PLAN (gfx950, wave64; the op is launch-bound at the sizes of the scripts' scenes, so the launches are the design).
//   forward   own centre: center_partial_kernel (P workgroups: the fp64 partials of the coordinates), then pose_kernel (P workgroups:
//             each folds the <= kMaxGroups partials itself, a few KB from L2, forms c and R and poses its chunks): 2 launches.
//             A given centre: pose_kernel alone.  All sets go in the same launches; the set table travels in the kernel arguments.
//   backward  moments_partial_kernel (P workgroups: the partials of the 12 sums), then pose_adjoint_kernel: every workgroup folds
//             them; workgroup 0 writes d_angles, d_translation, d_center; each writes d_v of its chunks of the sets that want one.
//             When no set wants a gradient it is one workgroup.  2 launches.
//   rotate    one launch of one wave each way.
// The outputs are written BY ELEMENT: lane t of a workgroup owns the floats 3 first + t, 3 first + t + kThreads, ... of a chunk, so a
// wave stores 256 contiguous bytes per instruction and loads the three coordinates of each element's vertex (neighbouring lanes
// share them).  16-byte vectors are not used: a lane's four floats would straddle two vertices, and a set (a tensor view) need not
// start on a 16-byte boundary.  The sums read by vertex (lane t owns the vertices t, t + kThreads, ...: the order above); a wave
// reads 768 contiguous bytes and uses every fetched line in full.  LDS holds the reduction tree and the few numbers a workgroup
// forms once (the folded sums, R, c, t, E / N).  Scratch is the caller's (the partials, fp64).
// `saved` [12] fp32 is written by the forward call: R (9), then the centre it used (3); the backward call reads the centre there.
#pragma once
#include "../../include/redner_amd_pose.h"
#include "arena.h"
#include "vecmath.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace rdr {
namespace pose {

constexpr int kMaxSets = 16;
constexpr int kThreads = 256;
constexpr int kChunk = 512;                     // vertices of a chunk
constexpr int kMaxGroups = 128;                 // P_max
constexpr int kCoords = 3, kMoments = 12;       // quantities of the two reductions

// the set table: what the kernels need of the K sets, passed by value
struct Table {
    const float *v[kMaxSets];                   // vertices
    const float *g[kMaxSets];                   // backward: the upstream gradient of out_k, nullptr = zeros
    float *o[kMaxSets];                         // forward: out_k; backward: d_v_k, nullptr = not wanted
    int count[kMaxSets];
    int chunk_off[kMaxSets + 1];                // the first chunk of set k; [num_sets] = C
    int num_sets, groups;                       // groups = P
    long long total;
};

RDR_FN int set_of(const Table &tb, int chunk) {
    int k = 0;
    while (k + 1 < tb.num_sets && chunk >= tb.chunk_off[k + 1]) ++k;
    return k;
}
// the vertices [first, last) of set k that chunk `chunk` holds
RDR_FN void chunk_range(const Table &tb, int chunk, int &k, int &first, int &last) {
    k = set_of(tb, chunk);
    first = (chunk - tb.chunk_off[k]) * kChunk;
    last = first + kChunk < tb.count[k] ? first + kChunk : tb.count[k];
}

// ---- the rotation ------------------------------------------------------------------------------------------------------------
struct Trig { double st, ct, sp, cp, ss, cs; };         // sin / cos of theta, phi, psi
RDR_FN Trig trig_of(const float *angles) {
    const double theta = (double)angles[0], phi = (double)angles[1], psi = (double)angles[2];
    return Trig{gm::sin(theta), gm::cos(theta), gm::sin(phi), gm::cos(phi), gm::sin(psi), gm::cos(psi)};
}
RDR_FN void rotation(const Trig &a, double *R) {
    R[0] = a.cs * a.cp;  R[1] = a.cs * a.sp * a.st - a.ss * a.ct;  R[2] = -(a.cs * a.sp) * a.ct - a.ss * a.st;
    R[3] = a.ss * a.cp;  R[4] = a.ss * a.sp * a.st + a.cs * a.ct;  R[5] = -(a.ss * a.sp) * a.ct + a.cs * a.st;
    R[6] = a.sp;         R[7] = -(a.cp * a.st);                    R[8] = a.cp * a.ct;
}
// dR / d angles[k]
RDR_FN void rotation_derivative(const Trig &a, int k, double *D) {
    if (k == 0) {
        D[0] = 0.0;  D[1] = a.cs * a.sp * a.ct + a.ss * a.st;  D[2] = a.cs * a.sp * a.st - a.ss * a.ct;
        D[3] = 0.0;  D[4] = a.ss * a.sp * a.ct - a.cs * a.st;  D[5] = a.ss * a.sp * a.st + a.cs * a.ct;
        D[6] = 0.0;  D[7] = -(a.cp * a.ct);                    D[8] = -(a.cp * a.st);
    } else if (k == 1) {
        D[0] = -(a.cs * a.sp);  D[1] = a.cs * a.cp * a.st;  D[2] = -(a.cs * a.cp) * a.ct;
        D[3] = -(a.ss * a.sp);  D[4] = a.ss * a.cp * a.st;  D[5] = -(a.ss * a.cp) * a.ct;
        D[6] = a.cp;            D[7] = a.sp * a.st;         D[8] = -(a.sp * a.ct);
    } else {
        D[0] = -(a.ss * a.cp);  D[1] = -(a.ss * a.sp) * a.st - a.cs * a.ct;  D[2] = a.ss * a.sp * a.ct - a.cs * a.st;
        D[3] = a.cs * a.cp;     D[4] = a.cs * a.sp * a.st - a.ss * a.ct;     D[5] = -(a.cs * a.sp) * a.ct - a.ss * a.st;
        D[6] = 0.0;             D[7] = 0.0;                                  D[8] = 0.0;
    }
}
RDR_FN void rotation_fp32(const Trig &a, float *R) {
    double R64[9];
    rotation(a, R64);
    for (int e = 0; e < 9; ++e) R[e] = (float)R64[e];
}
// d_angles[0 .. 3) = fp32(sum over (i, j) ascending of dR_k,ij * S_ij)
RDR_FN void angle_gradient(const Trig &a, const double *S, float *d_angles) {
    for (int k = 0; k < 3; ++k) {
        double D[9], sum = 0.0;
        rotation_derivative(a, k, D);
        for (int e = 0; e < 9; ++e) sum += D[e] * S[e];
        d_angles[k] = (float)sum;
    }
}
// E = G - R^T G
RDR_FN void center_gradient(const float *R, const double *G, double *E) {
    for (int j = 0; j < 3; ++j)
        E[j] = G[j] - (((double)R[j] * G[0] + (double)R[3 + j] * G[1]) + (double)R[6 + j] * G[2]);
}

// ---- per element and vertex -----------------------------------------------------------------------------------------------------
// coordinate i of the posed vertex v
RDR_FN float pose_element(const float *v, const float *R, const float *c, const float *t, int i) {
    const float d0 = v[0] - c[0], d1 = v[1] - c[1], d2 = v[2] - c[2];
    return (((R[3 * i] * d0 + R[3 * i + 1] * d1) + R[3 * i + 2] * d2) + c[i]) + t[i];
}
RDR_FN void pose_vertex(const float *v, const float *R, const float *c, const float *t, float *out) {
    for (int i = 0; i < 3; ++i) out[i] = pose_element(v, R, c, t, i);
}
// coordinate j of d_v of the vertex whose upstream gradient is g (nullptr: zeros); spread = nullptr: a given centre
RDR_FN float pose_element_adjoint(const float *g, const float *R, const float *spread, int j) {
    const float g0 = g ? g[0] : 0.f, g1 = g ? g[1] : 0.f, g2 = g ? g[2] : 0.f;
    const float r = (g0 * R[j] + g1 * R[3 + j]) + g2 * R[6 + j];
    return spread ? r + spread[j] : r;
}
RDR_FN void pose_vertex_adjoint(const float *g, const float *R, const float *spread, float *d_v) {
    for (int j = 0; j < 3; ++j) d_v[j] = pose_element_adjoint(g, R, spread, j);
}

// ---- per chunk and lane: the lane-strided sums ---------------------------------------------------------------------------------
RDR_FN void lane_coords(const float *v, int first, int last, int t, double *acc) {
    for (int q = 0; q < kCoords; ++q) acc[q] = 0.0;
    for (int n = first + t; n < last; n += kThreads)
        for (int q = 0; q < kCoords; ++q) acc[q] += (double)v[(size_t)3 * n + q];
}
RDR_FN void lane_moments(const float *v, const float *g, const float *c, int first, int last, int t, double *acc) {
    for (int q = 0; q < kMoments; ++q) acc[q] = 0.0;
    if (!g) return;
    for (int n = first + t; n < last; n += kThreads) {
        const float *p = v + (size_t)3 * n, *gn = g + (size_t)3 * n;
        const double d0 = (double)(p[0] - c[0]), d1 = (double)(p[1] - c[1]), d2 = (double)(p[2] - c[2]);
        for (int i = 0; i < 3; ++i) {
            const double gi = (double)gn[i];
            acc[3 * i] += gi * d0;
            acc[3 * i + 1] += gi * d1;
            acc[3 * i + 2] += gi * d2;
            acc[9 + i] += gi;
        }
    }
}
// sum[q] = the partials of quantity q in ascending workgroup order
RDR_FN double fold(const double *partial, int groups, int quantities, int q) {
    double s = 0.0;
    for (int w = 0; w < groups; ++w) s += partial[(size_t)w * quantities + q];
    return s;
}
RDR_FN void own_center(const double *sums, long long total, float *c) {
    for (int q = 0; q < 3; ++q) c[q] = (float)(sums[q] / (double)total);
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels ----------------------------------------------------------------------------------------------------------
// x[q][t] = acc[q] folded by the tree: afterwards x[q][0] is the sum over the lanes (every lane of the workgroup calls this)
template <int Q>
__device__ inline void tree(double (*x)[kThreads], const double *acc, int t) {
    for (int q = 0; q < Q; ++q) x[q][t] = acc[q];
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if (t < s)
            for (int q = 0; q < Q; ++q) x[q][t] += x[q][t + s];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) center_partial_kernel(Table tb, double *partial) {
    __shared__ double x[kCoords][kThreads];
    const int t = threadIdx.x, w = blockIdx.x, C = tb.chunk_off[tb.num_sets];
    double mine[kCoords] = {0.0, 0.0, 0.0};                // lane 0: this workgroup's partial
    for (int chunk = w; chunk < C; chunk += tb.groups) {
        int k, first, last;
        chunk_range(tb, chunk, k, first, last);
        double acc[kCoords];
        lane_coords(tb.v[k], first, last, t, acc);
        tree<kCoords>(x, acc, t);
        if (t == 0)
            for (int q = 0; q < kCoords; ++q) mine[q] += x[q][0];
        __syncthreads();
    }
    if (t == 0)
        for (int q = 0; q < kCoords; ++q) partial[(size_t)w * kCoords + q] = mine[q];
}

// OWN: the centre is the mean (partial holds the coordinates' partials); otherwise `center` is read
template <bool OWN>
__global__ void __launch_bounds__(kThreads) pose_kernel(Table tb, const float *angles, const float *translation, const float *center,
                                                        const double *partial, float *saved) {
    __shared__ double sums[kCoords];
    __shared__ float R[9], c[3], tr[3];
    const int t = threadIdx.x, w = blockIdx.x, C = tb.chunk_off[tb.num_sets];
    if (OWN && t < kCoords) sums[t] = fold(partial, tb.groups, kCoords, t);
    if (OWN) __syncthreads();
    if (t == 0) {
        rotation_fp32(trig_of(angles), R);
        if (OWN) own_center(sums, tb.total, c);
        else for (int q = 0; q < 3; ++q) c[q] = center[q];
        for (int q = 0; q < 3; ++q) tr[q] = translation[q];
        if (w == 0) {
            for (int e = 0; e < 9; ++e) saved[e] = R[e];
            for (int q = 0; q < 3; ++q) saved[9 + q] = c[q];
        }
    }
    __syncthreads();
    for (int chunk = w; chunk < C; chunk += tb.groups) {
        int k, first, last;
        chunk_range(tb, chunk, k, first, last);
        // by element: lane t writes the floats 3 first + t, + kThreads, ... of the chunk (a wave stores 256 contiguous bytes)
        const float *v = tb.v[k];
        float *o = tb.o[k];
        for (size_t e = (size_t)3 * first + t; e < (size_t)3 * last; e += kThreads) {
            const size_t n = e / 3;
            o[e] = pose_element(v + 3 * n, R, c, tr, (int)(e - 3 * n));
        }
    }
}

__global__ void __launch_bounds__(kThreads) moments_partial_kernel(Table tb, const float *saved, double *partial) {
    __shared__ double x[kMoments][kThreads];
    const int t = threadIdx.x, w = blockIdx.x, C = tb.chunk_off[tb.num_sets];
    const float c[3] = {saved[9], saved[10], saved[11]};
    double mine[kMoments];
    for (int q = 0; q < kMoments; ++q) mine[q] = 0.0;
    for (int chunk = w; chunk < C; chunk += tb.groups) {
        int k, first, last;
        chunk_range(tb, chunk, k, first, last);
        double acc[kMoments];
        lane_moments(tb.v[k], tb.g[k], c, first, last, t, acc);
        tree<kMoments>(x, acc, t);
        if (t == 0)
            for (int q = 0; q < kMoments; ++q) mine[q] += x[q][0];
        __syncthreads();
    }
    if (t == 0)
        for (int q = 0; q < kMoments; ++q) partial[(size_t)w * kMoments + q] = mine[q];
}

// P workgroups, or one when no set wants a gradient (tb.groups is the P of the partials either way)
template <bool OWN>
__global__ void __launch_bounds__(kThreads) pose_adjoint_kernel(Table tb, const float *angles, const double *partial, float *d_angles,
                                                                float *d_translation, float *d_center) {
    __shared__ double sums[kMoments];
    __shared__ float R[9], spread[3];
    const int t = threadIdx.x, w = blockIdx.x, C = tb.chunk_off[tb.num_sets];
    if (t < kMoments) sums[t] = fold(partial, tb.groups, kMoments, t);
    __syncthreads();
    if (t == 0) {
        const Trig a = trig_of(angles);
        double E[3];
        rotation_fp32(a, R);
        center_gradient(R, sums + 9, E);
        for (int q = 0; q < 3; ++q) spread[q] = (float)(E[q] / (double)tb.total);
        if (w == 0) {
            angle_gradient(a, sums, d_angles);
            for (int q = 0; q < 3; ++q) d_translation[q] = (float)sums[9 + q];
            if (!OWN)
                for (int q = 0; q < 3; ++q) d_center[q] = (float)E[q];
        }
    }
    __syncthreads();
    for (int chunk = w; chunk < C; chunk += gridDim.x) {
        int k, first, last;
        chunk_range(tb, chunk, k, first, last);
        if (!tb.o[k]) continue;
        const float *g = tb.g[k];
        float *o = tb.o[k];
        for (size_t e = (size_t)3 * first + t; e < (size_t)3 * last; e += kThreads) {
            const size_t n = e / 3;
            o[e] = pose_element_adjoint(g ? g + 3 * n : nullptr, R, OWN ? spread : nullptr, (int)(e - 3 * n));
        }
    }
}

__global__ void __launch_bounds__(64) rotate_matrix_kernel(const float *angles, float *matrix) {
    if (threadIdx.x == 0) rotation_fp32(trig_of(angles), matrix);
}
__global__ void __launch_bounds__(64) rotate_matrix_adjoint_kernel(const float *angles, const float *d_matrix, float *d_angles) {
    if (threadIdx.x == 0) {
        double S[9];
        for (int e = 0; e < 9; ++e) S[e] = (double)d_matrix[e];
        angle_gradient(trig_of(angles), S, d_angles);
    }
}
#else
// ---- the harness: the same sums as plain loops ---------------------------------------------------------------------------------
// partial[w * Q + q] for every workgroup w, lane sums by `lane(k, first, last, t, acc)`
template <int Q, class Lane>
inline void partials(const Table &tb, double *partial, Lane lane) {
    const int C = tb.chunk_off[tb.num_sets];
    std::vector<double> x((size_t)Q * kThreads);
    for (int w = 0; w < tb.groups; ++w) {
        double mine[Q];
        for (int q = 0; q < Q; ++q) mine[q] = 0.0;
        for (int chunk = w; chunk < C; chunk += tb.groups) {
            int k, first, last;
            chunk_range(tb, chunk, k, first, last);
            for (int t = 0; t < kThreads; ++t) {
                double acc[Q];
                lane(k, first, last, t, acc);
                for (int q = 0; q < Q; ++q) x[(size_t)q * kThreads + t] = acc[q];
            }
            for (int s = kThreads / 2; s >= 1; s >>= 1)
                for (int t = 0; t < s; ++t)
                    for (int q = 0; q < Q; ++q) x[(size_t)q * kThreads + t] += x[(size_t)q * kThreads + t + s];
            for (int q = 0; q < Q; ++q) mine[q] += x[(size_t)q * kThreads];
        }
        for (int q = 0; q < Q; ++q) partial[(size_t)w * Q + q] = mine[q];
    }
}
#endif

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the plan of a list of set sizes: chunk offsets, C, P
inline Table make_table(int num_sets, const int *counts, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (num_sets < 1 || num_sets > kMaxSets) fail("between 1 and " + std::to_string(kMaxSets) + " vertex sets, got " + std::to_string(num_sets));
    if (!counts) fail("counts is required");
    Table tb{};
    tb.num_sets = num_sets;
    long long chunks = 0;
    for (int k = 0; k < num_sets; ++k) {
        if (counts[k] < 1) fail("set " + std::to_string(k) + " has " + std::to_string(counts[k]) + " vertices: at least 1");
        tb.count[k] = counts[k];
        tb.chunk_off[k] = (int)chunks;
        chunks += (counts[k] + (long long)kChunk - 1) / kChunk;
        tb.total += counts[k];
    }
    if (tb.total > (long long)1 << 30) fail("more than 2^30 vertices");
    tb.chunk_off[num_sets] = (int)chunks;
    tb.groups = chunks < kMaxGroups ? (int)chunks : kMaxGroups;
    return tb;
}
// floats of scratch: the fp64 partials of the coordinates (own centre only; the query reports that case) / of the 12 sums
inline long long forward_floats(const Table &tb) { return 2LL * kCoords * tb.groups; }
inline long long backward_floats(const Table &tb) { return 2LL * kMoments * tb.groups; }

// rdr_rotate_matrix / rdr_rotate_matrix_backward; stream-ordered, not synchronised
inline void rotate_matrix(const float *angles, float *matrix) {
    if (!angles || !matrix) throw std::runtime_error("rdr_rotate_matrix: angles and matrix are required");
#if !defined(RDR_HOSTSIM)
    hipLaunchKernelGGL(rotate_matrix_kernel, dim3(1), dim3(64), 0, exec::ctx().stream, angles, matrix);
    exec::check(hipGetLastError(), "rotate_matrix launch");
#else
    rotation_fp32(trig_of(angles), matrix);
#endif
}
inline void rotate_matrix_backward(const float *angles, const float *d_matrix, float *d_angles) {
    if (!angles || !d_matrix || !d_angles) throw std::runtime_error("rdr_rotate_matrix_backward: angles, d_matrix and d_angles are required");
#if !defined(RDR_HOSTSIM)
    hipLaunchKernelGGL(rotate_matrix_adjoint_kernel, dim3(1), dim3(64), 0, exec::ctx().stream, angles, d_matrix, d_angles);
    exec::check(hipGetLastError(), "rotate_matrix adjoint launch");
#else
    double S[9];
    for (int e = 0; e < 9; ++e) S[e] = (double)d_matrix[e];
    angle_gradient(trig_of(angles), S, d_angles);
#endif
}

// rdr_pose_vertices: writes every element of every out_k and saved[12]; center == nullptr: the sets' own mean
inline void forward(Table tb, const float *const *vertices, const float *angles, const float *translation, const float *center,
                    float *const *out, float *saved, float *scratch, size_t scratch_count) {
    const char *who = "rdr_pose_vertices";
    if (!vertices || !out || !angles || !translation || !saved)
        throw std::runtime_error(std::string(who) + ": vertices, out, angles, translation and saved are required");
    for (int k = 0; k < tb.num_sets; ++k) {
        if (!vertices[k] || !out[k]) throw std::runtime_error(std::string(who) + ": vertices and out of every set are required");
        tb.v[k] = vertices[k];
        tb.o[k] = out[k];
    }
    const bool own = center == nullptr;
    if (own) need_scratch(who, (size_t)forward_floats(tb), scratch, scratch_count, true);
    double *partial = reinterpret_cast<double *>(scratch);
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (own) {
        hipLaunchKernelGGL(center_partial_kernel, dim3(tb.groups), dim3(kThreads), 0, stream, tb, partial);
        exec::check(hipGetLastError(), "pose centre launch");
        hipLaunchKernelGGL(pose_kernel<true>, dim3(tb.groups), dim3(kThreads), 0, stream, tb, angles, translation, center,
                           (const double *)partial, saved);
    } else {
        hipLaunchKernelGGL(pose_kernel<false>, dim3(tb.groups), dim3(kThreads), 0, stream, tb, angles, translation, center,
                           (const double *)partial, saved);
    }
    exec::check(hipGetLastError(), "pose launch");
#else
    float R[9], c[3];
    rotation_fp32(trig_of(angles), R);
    if (own) {
        partials<kCoords>(tb, partial, [&](int k, int first, int last, int t, double *acc) { lane_coords(tb.v[k], first, last, t, acc); });
        double sums[kCoords];
        for (int q = 0; q < kCoords; ++q) sums[q] = fold(partial, tb.groups, kCoords, q);
        own_center(sums, tb.total, c);
    } else {
        for (int q = 0; q < 3; ++q) c[q] = center[q];
    }
    for (int e = 0; e < 9; ++e) saved[e] = R[e];
    for (int q = 0; q < 3; ++q) saved[9 + q] = c[q];
    for (int k = 0; k < tb.num_sets; ++k)
        for (int n = 0; n < tb.count[k]; ++n) pose_vertex(tb.v[k] + (size_t)3 * n, R, c, translation, tb.o[k] + (size_t)3 * n);
#endif
}

// rdr_pose_vertices_backward: writes d_angles, d_translation, d_center (a given centre) and every element of every d_vertices[k]
// that is not nullptr; d_out[k] == nullptr counts as zeros
inline void backward(Table tb, const float *const *vertices, const float *angles, const float *saved, bool own,
                     const float *const *d_out, float *const *d_vertices, float *d_angles, float *d_translation, float *d_center,
                     float *scratch, size_t scratch_count) {
    const char *who = "rdr_pose_vertices_backward";
    if (!vertices || !d_out || !angles || !saved || !d_angles || !d_translation || (!own && !d_center))
        throw std::runtime_error(std::string(who) + ": vertices, d_out, angles, saved, d_angles, d_translation and (for a given "
                                 "centre) d_center are required");
    bool wanted = false;
    for (int k = 0; k < tb.num_sets; ++k) {
        if (!vertices[k]) throw std::runtime_error(std::string(who) + ": vertices of every set are required");
        tb.v[k] = vertices[k];
        tb.g[k] = d_out[k];
        tb.o[k] = d_vertices ? d_vertices[k] : nullptr;
        wanted = wanted || tb.o[k];
    }
    need_scratch(who, (size_t)backward_floats(tb), scratch, scratch_count, true);
    double *partial = reinterpret_cast<double *>(scratch);
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    hipLaunchKernelGGL(moments_partial_kernel, dim3(tb.groups), dim3(kThreads), 0, stream, tb, saved, partial);
    exec::check(hipGetLastError(), "pose moments launch");
    const dim3 grid(wanted ? tb.groups : 1);
    if (own)
        hipLaunchKernelGGL(pose_adjoint_kernel<true>, grid, dim3(kThreads), 0, stream, tb, angles, (const double *)partial, d_angles,
                           d_translation, d_center);
    else
        hipLaunchKernelGGL(pose_adjoint_kernel<false>, grid, dim3(kThreads), 0, stream, tb, angles, (const double *)partial, d_angles,
                           d_translation, d_center);
    exec::check(hipGetLastError(), "pose adjoint launch");
#else
    const float *c = saved + 9;
    partials<kMoments>(tb, partial,
                       [&](int k, int first, int last, int t, double *acc) { lane_moments(tb.v[k], tb.g[k], c, first, last, t, acc); });
    double sums[kMoments], E[3];
    for (int q = 0; q < kMoments; ++q) sums[q] = fold(partial, tb.groups, kMoments, q);
    const Trig a = trig_of(angles);
    float R[9], spread[3];
    rotation_fp32(a, R);
    center_gradient(R, sums + 9, E);
    for (int q = 0; q < 3; ++q) spread[q] = (float)(E[q] / (double)tb.total);
    angle_gradient(a, sums, d_angles);
    for (int q = 0; q < 3; ++q) d_translation[q] = (float)sums[9 + q];
    if (!own)
        for (int q = 0; q < 3; ++q) d_center[q] = (float)E[q];
    for (int k = 0; k < tb.num_sets; ++k) {
        if (!tb.o[k]) continue;
        for (int n = 0; n < tb.count[k]; ++n)
            pose_vertex_adjoint(tb.g[k] ? tb.g[k] + (size_t)3 * n : nullptr, R, own ? spread : nullptr, tb.o[k] + (size_t)3 * n);
    }
#endif
}

} // namespace pose
} // namespace rdr
