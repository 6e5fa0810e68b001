// vertex_normal.h -- smooth vertex normals of a triangle mesh and their vertex adjoint (rdr_mesh_topology_* / rdr_vertex_normal /
// rdr_vertex_normal_backward).
//
// The meaning is that of pyredner/shape.py:7-127 (compute_vertex_normal).  vertices [V, 3] fp32, indices [T, 3] int32,
// normals [V, 3] fp32.  Corner c = 3 f + k is corner k of face f; its vertex is indices[c], its sides are
// e1 = v[k+1] - v[k] and e2 = v[k+2] - v[k] (k + 1, k + 2 modulo 3), a = e1 / |e1|, b = e2 / |e2|.
//
//   'max' (Nelson Max's weights)
//     * the face's unit normal n is normalise(cross(a, b)) OF CORNER 0, or 0 when that cross product has length 0
//     * angle = 2 asin(0.5 |b - a|), or pi - 2 asin(0.5 |a + b|) when a . b < 0; the asin argument is clamped to [0, 1 - 1e-6]
//     * corner c adds n * (sin(angle) / (|e1| |e2|)) to its vertex; nothing when |e1| |e2| == 0
//     * normals[v] = sum / |sum|, or (0, 0, 1) when |sum| == 0 (an isolated vertex, a vertex of degenerate faces only)
//   'cotangent'
//     * corner i adds w_i = (v[i+2] - v[i+1]) * cot(angle_i) to vertex i + 1 and subtracts it from vertex i + 2
//     * the sum is negated unless dot(sum, normal_max) > 0; if its length is > 0.05 it is normalised, otherwise the 'max'
//       normal is the result.  So 'cotangent' computes both sums, and the gradient flows through the branch each vertex took.
//     * a corner with a zero-length side or with two coincident sides (a == b: angle 0, cot infinite) adds nothing.  (The
//       reference produces NaN there and fails its own assertion.)
//     * a corner of a zero-area face whose sides point in opposite directions (angle = fp32 pi) adds, like the reference,
//       (v[i+2] - v[i+1]) / tan(fp32 pi), about 1e7 times that edge; its gradient is 0 (|e1 x e2| == 0: a degenerate corner).
//
// ARITHMETIC.  The per-corner terms are fp32, operation by operation in the order of the reference's expressions (no
// contraction).  asin, sin and tan are evaluated in fp64 by the routines of libm_exact.h (asin x = atan2(x, sqrt((1 - x)(1 + x))),
// tan = sin / cos) and rounded to fp32: the same bits in both product libraries and in the CPU harness.  The per-vertex sums
// are carried in fp64 IN A FIXED ORDER and rounded once to fp32 before the normalisation, like GradStore does for gradients.
//
// THE ORDER is a function of `indices` only: a vertex sums its incident corners in ASCENDING CORNER ID 3 f + k (a vertex that
// a face lists twice has two corners of that face).  For 'cotangent' a corner c = 3 f + k contributes two addends, in this
// order: + w_{(k+2) mod 3}, then - w_{(k+1) mod 3}, of face f.  The same order sums the adjoint's per-corner records.
//
// THE PLAN (Topology) holds what depends on `indices` only: a copy of them, row offsets [V + 1] and the corner list in the
// order above (CSR).  It is built once per connectivity: valence count with INTEGER atomics, exclusive scan by one workgroup,
// scatter with integer atomics (any order inside a row), then every row is sorted in place by one lane -- corner ids are
// unique, so the result is the canonical order whatever the scatter did.  Rows of up to 32 corners use insertion sort, longer
// ones heap sort: O(n log n) for a hub of any valence.  Every index is validated by the counting kernel (one readback);
// no later kernel reads out of bounds.  The harness builds the same plan with a host counting sort.
//
// THE ADJOINT differentiates the closed forms the expressions above are equal to,
//     n sin(angle) / (|e1| |e2|) = M / (|e1|^2 |e2|^2),   cot(angle) = (e1 . e2) / |M|,   M = (v1 - v0) x (v2 - v0)
// (every corner of a face has the same e1 x e2; the clamp of asin is never active: its argument is at most sqrt(2) / 2), in
// fp64 at the fp32 vertices; which corners, faces and vertices are degenerate, flipped or fallen back is decided by the fp32
// predicates of the forward pass, recomputed from the vertices and the saved sums.  THE GRADIENT OF A DEGENERATE CORNER OR
// FACE IS 0 (a zero-length side, a zero-length cross product, coincident sides), and so is that of a vertex that takes
// (0, 0, 1); the reference returns NaN there (torch.where over a 0 / 0 branch).  DESIGN.md section 7.
//
// KERNELS.  One lane per item, 256 lanes per workgroup, grid ceil(n / 256), no cap.
//   forward    vn_face_kernel     a face: three corner records (the 'max' addend; for 'cotangent' also w_i)       -> scratch
//              vn_vertex_kernel   a vertex: gathers its row in order, normalises / flips / falls back             -> normals, saved
//   adjoint    vn_face_adjoint_kernel  a face: d_sum at its three vertices (the adjoint of normalise / flip / fallback, from
//                                 `saved` and d_normals), then one d_position record per corner                   -> scratch
//              vn_gather_kernel   a vertex: sums the records of its row in order                                  -> d_vertices
// Gathers and plain stores only: no float atomics, no buffer that must be zero, every element of every output is written,
// bitwise reproducible.  The library allocates nothing per call and does not synchronise.
// The per-item bodies are shared with the plain loops of the CPU harness.
#pragma once
#include "../../include/redner_amd.h"
#include "arena.h"
#include "vecmath.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace rdr {
namespace vnrm {

struct F3 { float x, y, z; };
struct D3 { double x, y, z; };

RDR_FN F3 load3(const float *p) { return F3{p[0], p[1], p[2]}; }
RDR_FN void store3(float *p, F3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
RDR_FN F3 operator+(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RDR_FN F3 operator-(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RDR_FN F3 operator-(F3 a) { return F3{-a.x, -a.y, -a.z}; }
RDR_FN F3 operator*(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
RDR_FN F3 operator/(F3 a, float s) { return F3{a.x / s, a.y / s, a.z / s}; }          // true divisions, like torch
RDR_FN float dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RDR_FN float length(F3 a) { return sqrtf(dot(a, a)); }
RDR_FN F3 cross(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

RDR_FN D3 widen(F3 a) { return D3{(double)a.x, (double)a.y, (double)a.z}; }
RDR_FN F3 narrow(D3 a) { return F3{(float)a.x, (float)a.y, (float)a.z}; }
RDR_FN D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RDR_FN D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RDR_FN D3 operator*(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
RDR_FN double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RDR_FN D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

constexpr float kPi = 3.14159265358979323846f;              // torch.tensor(math.pi)
constexpr float kAsinMax = (float)(1.0 - 1e-6);             // clamp(0, 1 - 1e-6) of an fp32 tensor
constexpr float kCotangentMinLength = 0.05f;
constexpr int kInsertionRow = 32;                           // rows up to this long: insertion sort; longer: heap sort

// ---- the forward pass, per item --------------------------------------------------------------------------------------------
// What the fp32 forward pass decides about corner k of a face (p0 = its vertex, p1, p2 the next two): shared by the adjoint.
struct Corner {
    F3 a, b;            // unit sides (valid when live)
    float e1e2;         // |e1| |e2|
    bool live;          // both sides have a length: the corner adds to the 'max' sum
    bool obtuse;        // a . b < 0
    float half_chord;   // 0.5 |b - a| (0.5 |a + b| when obtuse), clamped: the argument of asin
    bool spread;        // live and the two sides do not coincide: the corner adds to the 'cotangent' sum
};
RDR_FN Corner corner_of(F3 p0, F3 p1, F3 p2) {
    Corner c{};
    const F3 e1 = p1 - p0, e2 = p2 - p0;
    const float l1 = length(e1), l2 = length(e2);
    c.e1e2 = l1 * l2;
    c.live = c.e1e2 > 0.f;
    if (!c.live) return c;
    c.a = e1 / l1;
    c.b = e2 / l2;
    c.obtuse = dot(c.a, c.b) < 0.f;
    const float x = 0.5f * length(c.obtuse ? c.a + c.b : c.b - c.a);
    c.half_chord = x > kAsinMax ? kAsinMax : x;
    c.spread = c.obtuse || x > 0.f;
    return c;
}
// the face's unit normal from corner 0, or 0
RDR_FN F3 face_normal(const Corner &c0) {
    if (!c0.live) return F3{0.f, 0.f, 0.f};
    const F3 n = cross(c0.a, c0.b);
    const float nl = length(n);
    return nl > 0.f ? n / nl : F3{0.f, 0.f, 0.f};
}
RDR_FN float corner_angle(const Corner &c) {
    const double x = (double)c.half_chord;
    const float as = (float)gm::atan2(x, sqrt((1.0 - x) * (1.0 + x)));
    return c.obtuse ? kPi - 2.0f * as : 2.0f * as;
}
// 1 / tan(angle) of a spread corner
RDR_FN float cotangent_of(float angle) {
    const float tangent = (float)(gm::sin((double)angle) / gm::cos((double)angle));
    return 1.0f / tangent;
}

// A face: its three corner records.  contrib[3 c ..] = the 'max' addend of corner c; cot[3 c ..] = w of corner c.
template <bool COT>
RDR_FN void face_forward(const float *vertices, const int *indices, int f, float *contrib, float *cot) {
    const size_t c0 = (size_t)3 * f;
    F3 p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = load3(vertices + (size_t)3 * indices[c0 + k]);
    F3 n{0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const F3 p1 = p[(k + 1) % 3], p2 = p[(k + 2) % 3];
        const Corner c = corner_of(p[k], p1, p2);
        if (k == 0) n = face_normal(c);
        F3 add{0.f, 0.f, 0.f}, w{0.f, 0.f, 0.f};
        if (c.live) {
            const float angle = corner_angle(c);
            add = n * ((float)gm::sin((double)angle) / c.e1e2);
            if (COT && c.spread) {
                w = (p2 - p1) * cotangent_of(angle);
            }
        }
        store3(contrib + 3 * (c0 + k), add);
        if (COT) store3(cot + 3 * (c0 + k), w);
    }
}

RDR_FN F3 unit_or_up(F3 s) {
    const float l = length(s);
    return l > 0.f ? s / l : F3{0.f, 0.f, 1.f};
}
// What a vertex does with its two sums (fp32, as saved): shared by the adjoint.
struct Pick { F3 normal; bool from_cotangent; bool flipped; };
RDR_FN Pick pick_cotangent(F3 sum_max, F3 sum_cot) {
    Pick p{};
    const F3 nmax = unit_or_up(sum_max);
    p.flipped = !(dot(sum_cot, nmax) > 0.f);
    const F3 s = p.flipped ? -sum_cot : sum_cot;
    const float l = length(s);
    p.from_cotangent = l > kCotangentMinLength;
    p.normal = p.from_cotangent ? s / l : nmax;
    return p;
}

// A vertex: gathers its row in the canonical order.  saved = [V, 3] 'max' sums, then for 'cotangent' [V, 3] cotangent sums.
template <bool COT>
RDR_FN void vertex_forward(const int *offsets, const int *corners, const float *contrib, const float *cot, int v, int num_vertices,
                           float *normals, float *saved) {
    D3 sm{0.0, 0.0, 0.0}, sc{0.0, 0.0, 0.0};
    for (int j = offsets[v]; j < offsets[v + 1]; ++j) {
        const int c = corners[j];
        const float *m = contrib + (size_t)3 * c;
        sm.x += (double)m[0]; sm.y += (double)m[1]; sm.z += (double)m[2];
        if (COT) {
            const int f = c / 3, k = c - 3 * f;
            const float *plus = cot + 3 * ((size_t)3 * f + (k + 2) % 3), *minus = cot + 3 * ((size_t)3 * f + (k + 1) % 3);
            sc.x += (double)plus[0]; sc.y += (double)plus[1]; sc.z += (double)plus[2];
            sc.x -= (double)minus[0]; sc.y -= (double)minus[1]; sc.z -= (double)minus[2];
        }
    }
    const F3 sum_max = narrow(sm);
    store3(saved + (size_t)3 * v, sum_max);
    if (!COT) {
        store3(normals + (size_t)3 * v, unit_or_up(sum_max));
    } else {
        const F3 sum_cot = narrow(sc);
        store3(saved + (size_t)3 * ((size_t)num_vertices + v), sum_cot);
        store3(normals + (size_t)3 * v, pick_cotangent(sum_max, sum_cot).normal);
    }
}

// ---- the adjoint, per item ---------------------------------------------------------------------------------------------------
// d(s / |s|)^T g
RDR_FN D3 unit_adjoint(D3 s, D3 g) {
    const double inv = 1.0 / sqrt(dot(s, s));
    const D3 n = s * inv;
    return (g - n * dot(n, g)) * inv;
}
// d_sum of vertex v: the adjoint of normalise / flip / fallback
struct SumGrad { D3 max, cot; };
template <bool COT>
RDR_FN SumGrad vertex_adjoint(const float *saved, const float *d_normals, int v, int num_vertices) {
    const D3 zero{0.0, 0.0, 0.0};
    SumGrad d{zero, zero};
    const F3 sum_max = load3(saved + (size_t)3 * v);
    const D3 g = widen(load3(d_normals + (size_t)3 * v));
    const bool max_live = length(sum_max) > 0.f;
    if (!COT) {
        if (max_live) d.max = unit_adjoint(widen(sum_max), g);
        return d;
    }
    const F3 sum_cot = load3(saved + (size_t)3 * ((size_t)num_vertices + v));
    const Pick p = pick_cotangent(sum_max, sum_cot);
    if (p.from_cotangent) {
        const double sign = p.flipped ? -1.0 : 1.0;
        d.cot = unit_adjoint(widen(sum_cot) * sign, g) * sign;
    } else if (max_live) {
        d.max = unit_adjoint(widen(sum_max), g);
    }
    return d;
}

// A spread corner i of a face, cot_i = (e1 . e2) / |e1 x e2|: adds to dp[0 .. 3) the position gradient of a loss whose
// derivative with respect to the vector (p[i+2] - p[i+1]) cot_i is h and whose derivative with respect to cot_i, the edge held,
// is u (h . (p[i+2] - p[i+1]), plus whatever else the caller hangs on cot_i: mesh_smooth.h).  Nothing where |e1 x e2| == 0.
RDR_FN void cotangent_corner_adjoint(const D3 *P, int i, D3 h, double u, D3 *dp) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    const D3 e1 = P[i1] - P[i], e2 = P[i2] - P[i], Mi = cross(e1, e2);
    const double S = sqrt(dot(Mi, Mi)), D = dot(e1, e2);
    if (!(S > 0.0)) return;
    const D3 through = h * (D / S);
    dp[i2] = dp[i2] + through;
    dp[i1] = dp[i1] - through;
    const double dD = u / S, dS = -u * D / (S * S);
    const D3 dM = Mi * (dS / S);
    const D3 de1 = e2 * dD + cross(e2, dM), de2 = e1 * dD + cross(dM, e1);
    dp[i1] = dp[i1] + de1;
    dp[i2] = dp[i2] + de2;
    dp[i] = dp[i] - (de1 + de2);
}

// A face: rec[3 c ..] = d loss / d position of the vertex at corner c through this face (all three corners' terms).
template <bool COT>
RDR_FN void face_adjoint(const float *vertices, const int *indices, const float *saved, const float *d_normals, int num_vertices,
                         int f, float *rec) {
    const size_t c0 = (size_t)3 * f;
    const D3 zero{0.0, 0.0, 0.0};
    F3 p[3];
    D3 P[3], gmax[3], gcot[3], dp[3] = {zero, zero, zero};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = indices[c0 + k];
        p[k] = load3(vertices + (size_t)3 * v);
        P[k] = widen(p[k]);
        const SumGrad d = vertex_adjoint<COT>(saved, d_normals, v, num_vertices);
        gmax[k] = d.max;
        gcot[k] = d.cot;
    }
    Corner corner[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) corner[k] = corner_of(p[k], p[(k + 1) % 3], p[(k + 2) % 3]);
    const F3 n = face_normal(corner[0]);
    const bool face_live = n.x != 0.f || n.y != 0.f || n.z != 0.f;
    if (face_live) {
        // sum over the live corners of g_k . M / (|e1|^2 |e2|^2)
        const D3 E1 = P[1] - P[0], E2 = P[2] - P[0], M = cross(E1, E2);
        D3 G = zero;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!corner[k].live) continue;
            const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const D3 e1 = P[k1] - P[k], e2 = P[k2] - P[k];
            const double q1 = dot(e1, e1), q2 = dot(e2, e2), q = q1 * q2, gM = dot(gmax[k], M);
            G = G + gmax[k] * (1.0 / q);
            const D3 de1 = e1 * (-2.0 * gM / (q * q1)), de2 = e2 * (-2.0 * gM / (q * q2));
            dp[k1] = dp[k1] + de1;
            dp[k2] = dp[k2] + de2;
            dp[k] = dp[k] - (de1 + de2);
        }
        const D3 dE1 = cross(E2, G), dE2 = cross(G, E1);
        dp[1] = dp[1] + dE1;
        dp[2] = dp[2] + dE2;
        dp[0] = dp[0] - (dE1 + dE2);
    }
    if (COT) {
        // corner i: (h . (p2 - p1)) (e1 . e2) / |e1 x e2|, h = d_cot[i + 1] - d_cot[i + 2]
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!corner[i].spread) continue;
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
            const D3 h = gcot[i1] - gcot[i2];
            cotangent_corner_adjoint(P, i, h, dot(h, P[i2] - P[i1]), dp);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) store3(rec + 3 * (c0 + k), narrow(dp[k]));
}

// A vertex: d_vertices[v] = the sum of its row's records in the canonical order
RDR_FN void vertex_gather(const int *offsets, const int *corners, const float *rec, int v, float *d_vertices) {
    D3 s{0.0, 0.0, 0.0};
    for (int j = offsets[v]; j < offsets[v + 1]; ++j) {
        const float *r = rec + (size_t)3 * corners[j];
        s.x += (double)r[0]; s.y += (double)r[1]; s.z += (double)r[2];
    }
    store3(d_vertices + (size_t)3 * v, narrow(s));
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// sorts row[0 .. n) ascending, in place
RDR_FN void sort_row(int *row, int n) {
    if (n <= kInsertionRow) {
        for (int i = 1; i < n; ++i) {
            const int key = row[i];
            int j = i - 1;
            for (; j >= 0 && row[j] > key; --j) row[j + 1] = row[j];
            row[j + 1] = key;
        }
        return;
    }
    auto sift = [&](int root, int end) {          // the heap is row[0 .. end)
        const int key = row[root];
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && row[child + 1] > row[child]) ++child;
            if (!(row[child] > key)) break;
            row[root] = row[child];
            root = child;
        }
        row[root] = key;
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int end = n - 1; end > 0; --end) {
        const int top = row[0];
        row[0] = row[end];
        row[end] = top;
        sift(0, end);
    }
}

struct Topology {
    int num_vertices = 0, num_triangles = 0;
    int gpu_index = -1;                                   // negative: host memory (the CPU harness)
    int *indices = nullptr, *offsets = nullptr, *corners = nullptr;
    ~Topology() { exec::dfree(indices); exec::dfree(offsets); exec::dfree(corners); }
    Topology() = default;
    Topology(const Topology &) = delete;
    Topology &operator=(const Topology &) = delete;
};

#if !defined(RDR_HOSTSIM)
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(256) vn_count_kernel(const int *__restrict__ indices, int num_corners, int num_vertices,
                                                       int *__restrict__ counts, int *__restrict__ bad) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)num_corners) return;
    const int v = indices[c];
    if ((unsigned)v >= (unsigned)num_vertices) atomicOr(bad, 1);
    else atomicAdd(counts + v, 1);
}
// offsets[0 .. V] = the exclusive scan of counts[0 .. V), by one workgroup: a lane sums a contiguous piece, the pieces' sums
// are scanned in LDS, and the lane writes its piece
__global__ void __launch_bounds__(kScanThreads) vn_scan_kernel(const int *__restrict__ counts, int num_vertices,
                                                               int *__restrict__ offsets) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x, per = (num_vertices + kScanThreads - 1) / kScanThreads;
    const long long first = (long long)t * per;
    const int lo = first < num_vertices ? (int)first : num_vertices, hi = first + per < num_vertices ? (int)(first + per) : num_vertices;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += counts[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int below = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += below;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int i = lo; i < hi; ++i) { offsets[i] = run; run += counts[i]; }
    if (t == kScanThreads - 1) offsets[num_vertices] = part[t];
}
// (only after validation: every index is in range; counts[v] goes back to 0)
__global__ void __launch_bounds__(256) vn_scatter_kernel(const int *__restrict__ indices, int num_corners, int num_vertices,
                                                         const int *__restrict__ offsets, int *__restrict__ counts,
                                                         int *__restrict__ corners) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)num_corners) return;
    const int v = indices[c];
    if ((unsigned)v >= (unsigned)num_vertices) return;
    const int slot = offsets[v] + atomicSub(counts + v, 1) - 1;
    if (slot >= offsets[v] && slot < offsets[v + 1]) corners[slot] = (int)c;
}
__global__ void __launch_bounds__(256) vn_sort_kernel(const int *__restrict__ offsets, int num_vertices, int *__restrict__ corners) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (size_t)num_vertices) return;
    sort_row(corners + offsets[v], offsets[v + 1] - offsets[v]);
}

template <bool COT>
__global__ void __launch_bounds__(256) vn_face_kernel(const float *__restrict__ vertices, const int *__restrict__ indices,
                                                      int num_triangles, float *__restrict__ contrib, float *__restrict__ cot) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)num_triangles) face_forward<COT>(vertices, indices, (int)f, contrib, cot);
}
template <bool COT>
__global__ void __launch_bounds__(256) vn_vertex_kernel(const int *__restrict__ offsets, const int *__restrict__ corners,
                                                        const float *__restrict__ contrib, const float *__restrict__ cot,
                                                        int num_vertices, float *__restrict__ normals, float *__restrict__ saved) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)num_vertices) vertex_forward<COT>(offsets, corners, contrib, cot, (int)v, num_vertices, normals, saved);
}
template <bool COT>
__global__ void __launch_bounds__(256) vn_face_adjoint_kernel(const float *__restrict__ vertices, const int *__restrict__ indices,
                                                              const float *__restrict__ saved, const float *__restrict__ d_normals,
                                                              int num_vertices, int num_triangles, float *__restrict__ rec) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)num_triangles) face_adjoint<COT>(vertices, indices, saved, d_normals, num_vertices, (int)f, rec);
}
__global__ void __launch_bounds__(256) vn_gather_kernel(const int *__restrict__ offsets, const int *__restrict__ corners,
                                                        const float *__restrict__ rec, int num_vertices,
                                                        float *__restrict__ d_vertices) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)num_vertices) vertex_gather(offsets, corners, rec, (int)v, d_vertices);
}
#endif

// rdr_mesh_topology_create.  `indices` is memory of the plan's place (device memory of gpu_index, or host memory for the
// harness); the plan keeps its own copy.  Synchronises (once, for the validation readback).
inline Topology *create_topology(const int *indices, int num_triangles, int num_vertices, int gpu_index) {
    const char *who = "rdr_mesh_topology_create: ";
    if (num_vertices < 1) throw std::runtime_error(std::string(who) + "num_vertices must be at least 1");
    if (num_triangles < 0) throw std::runtime_error(std::string(who) + "num_triangles must not be negative");
    if ((long long)num_triangles * 3 >= ((long long)1 << 31)) throw std::runtime_error(std::string(who) + "3 * num_triangles must be below 2^31");
    if (num_triangles > 0 && !indices) throw std::runtime_error(std::string(who) + "indices is required");
    const int num_corners = 3 * num_triangles;
    Topology *t = new Topology();
    try {
        t->num_vertices = num_vertices;
        t->num_triangles = num_triangles;
        t->gpu_index = gpu_index;
        t->indices = (int *)exec::dmalloc(sizeof(int) * (size_t)num_corners);
        t->offsets = (int *)exec::dmalloc(sizeof(int) * ((size_t)num_vertices + 1));
        t->corners = (int *)exec::dmalloc(sizeof(int) * (size_t)num_corners);
        auto out_of_range = [&]() {
            throw std::runtime_error(std::string(who) + "an index is outside [0, " + std::to_string(num_vertices) + ")");
        };
#if !defined(RDR_HOSTSIM)
        hipStream_t stream = exec::ctx().stream;
        // counts [V], then the validation flag
        int *counts = (int *)exec::dmalloc(sizeof(int) * ((size_t)num_vertices + 1));
        try {
            exec::zero(counts, sizeof(int) * ((size_t)num_vertices + 1));
            exec::copy_dev(t->indices, indices, sizeof(int) * (size_t)num_corners);
            if (num_corners > 0) {
                hipLaunchKernelGGL(vn_count_kernel, exec::grid_of(num_corners), dim3(256), 0, stream, t->indices, num_corners, num_vertices,
                                   counts, counts + num_vertices);
                exec::check(hipGetLastError(), "vn_count launch");
            }
            int bad = 0;
            exec::download(&bad, counts + num_vertices, sizeof(int));
            if (bad) out_of_range();
            hipLaunchKernelGGL(vn_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, counts, num_vertices, t->offsets);
            exec::check(hipGetLastError(), "vn_scan launch");
            if (num_corners > 0) {
                hipLaunchKernelGGL(vn_scatter_kernel, exec::grid_of(num_corners), dim3(256), 0, stream, t->indices, num_corners,
                                   num_vertices, t->offsets, counts, t->corners);
                exec::check(hipGetLastError(), "vn_scatter launch");
                hipLaunchKernelGGL(vn_sort_kernel, exec::grid_of(num_vertices), dim3(256), 0, stream, t->offsets, num_vertices, t->corners);
                exec::check(hipGetLastError(), "vn_sort launch");
            }
            exec::sync();                        // `counts` is released below
        } catch (...) {
            exec::device_sync();
            exec::dfree(counts);
            throw;
        }
        exec::dfree(counts);
#else
        for (int c = 0; c < num_corners; ++c) {
            if (indices[c] < 0 || indices[c] >= num_vertices) out_of_range();
            t->indices[c] = indices[c];
        }
        // counting sort by vertex; corners are visited in ascending id, so every row comes out ascending
        for (int v = 0; v <= num_vertices; ++v) t->offsets[v] = 0;
        for (int c = 0; c < num_corners; ++c) ++t->offsets[indices[c] + 1];
        for (int v = 0; v < num_vertices; ++v) t->offsets[v + 1] += t->offsets[v];
        std::vector<int> next(t->offsets, t->offsets + num_vertices);
        for (int c = 0; c < num_corners; ++c) t->corners[next[indices[c]]++] = c;
#endif
    } catch (...) {
        delete t;
        throw;
    }
    return t;
}

// rdr_mesh_topology_read (tests): offsets [V + 1] and corners [3 T] into HOST memory; synchronises
inline void read_topology(const Topology &t, int *offsets, int *corners) {
    if (!offsets || !corners) throw std::runtime_error("rdr_mesh_topology_read: offsets and corners are required");
    exec::download(offsets, t.offsets, sizeof(int) * ((size_t)t.num_vertices + 1));
    exec::download(corners, t.corners, sizeof(int) * (size_t)3 * t.num_triangles);
}

inline bool cotangent(int scheme, const char *who) {
    if (scheme != rdr_normal_weighting_max && scheme != rdr_normal_weighting_cotangent)
        throw std::runtime_error(std::string(who) + ": unknown weighting scheme " + std::to_string(scheme));
    return scheme == rdr_normal_weighting_cotangent;
}
// floats: the corner records of the forward pass / of the adjoint / what the forward pass saves for the adjoint
inline size_t forward_scratch_floats(const Topology &t, bool cot) { return (size_t)9 * t.num_triangles * (cot ? 2 : 1); }
inline size_t backward_scratch_floats(const Topology &t, bool) { return (size_t)9 * t.num_triangles; }
inline size_t saved_floats(const Topology &t, bool cot) { return (size_t)3 * t.num_vertices * (cot ? 2 : 1); }

template <bool COT>
inline void forward_impl(const Topology &t, const float *vertices, float *normals, float *saved, float *scratch) {
    float *contrib = scratch, *cot = COT ? scratch + (size_t)9 * t.num_triangles : nullptr;
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (t.num_triangles > 0) {
        hipLaunchKernelGGL(vn_face_kernel<COT>, exec::grid_of(t.num_triangles), dim3(256), 0, stream, vertices, t.indices, t.num_triangles,
                           contrib, cot);
        exec::check(hipGetLastError(), "vn_face launch");
    }
    hipLaunchKernelGGL(vn_vertex_kernel<COT>, exec::grid_of(t.num_vertices), dim3(256), 0, stream, t.offsets, t.corners, contrib, cot,
                       t.num_vertices, normals, saved);
    exec::check(hipGetLastError(), "vn_vertex launch");
#else
    for (int f = 0; f < t.num_triangles; ++f) face_forward<COT>(vertices, t.indices, f, contrib, cot);
    for (int v = 0; v < t.num_vertices; ++v) vertex_forward<COT>(t.offsets, t.corners, contrib, cot, v, t.num_vertices, normals, saved);
#endif
}

template <bool COT>
inline void backward_impl(const Topology &t, const float *vertices, const float *saved, const float *d_normals, float *d_vertices,
                          float *rec) {
#if !defined(RDR_HOSTSIM)
    hipStream_t stream = exec::ctx().stream;
    if (t.num_triangles > 0) {
        hipLaunchKernelGGL(vn_face_adjoint_kernel<COT>, exec::grid_of(t.num_triangles), dim3(256), 0, stream, vertices, t.indices, saved,
                           d_normals, t.num_vertices, t.num_triangles, rec);
        exec::check(hipGetLastError(), "vn_face_adjoint launch");
    }
    hipLaunchKernelGGL(vn_gather_kernel, exec::grid_of(t.num_vertices), dim3(256), 0, stream, t.offsets, t.corners, rec, t.num_vertices,
                       d_vertices);
    exec::check(hipGetLastError(), "vn_gather launch");
#else
    for (int f = 0; f < t.num_triangles; ++f) face_adjoint<COT>(vertices, t.indices, saved, d_normals, t.num_vertices, f, rec);
    for (int v = 0; v < t.num_vertices; ++v) vertex_gather(t.offsets, t.corners, rec, v, d_vertices);
#endif
}

// rdr_vertex_normal: writes every element of normals [V, 3] and of saved; stream-ordered, not synchronised
inline void forward(const Topology &t, int scheme, const float *vertices, float *normals, float *saved, float *scratch,
                    size_t scratch_count) {
    const bool cot = cotangent(scheme, "rdr_vertex_normal");
    if (!vertices || !normals || !saved) throw std::runtime_error("rdr_vertex_normal: vertices, normals and saved are required");
    need_scratch("rdr_vertex_normal", forward_scratch_floats(t, cot), scratch, scratch_count);
    if (cot) forward_impl<true>(t, vertices, normals, saved, scratch);
    else forward_impl<false>(t, vertices, normals, saved, scratch);
}

// rdr_vertex_normal_backward: writes every element of d_vertices [V, 3]; stream-ordered, not synchronised
inline void backward(const Topology &t, int scheme, const float *vertices, const float *saved, const float *d_normals,
                     float *d_vertices, float *scratch, size_t scratch_count) {
    const bool cot = cotangent(scheme, "rdr_vertex_normal_backward");
    if (!vertices || !saved || !d_normals || !d_vertices)
        throw std::runtime_error("rdr_vertex_normal_backward: vertices, saved, d_normals and d_vertices are required");
    need_scratch("rdr_vertex_normal_backward", backward_scratch_floats(t, cot), scratch, scratch_count);
    if (cot) backward_impl<true>(t, vertices, saved, d_normals, d_vertices, scratch);
    else backward_impl<false>(t, vertices, saved, d_normals, d_vertices, scratch);
}

} // namespace vnrm
} // namespace rdr
