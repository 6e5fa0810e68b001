// deferred_quad.h -- a rectangular area light in deferred shading and its adjoint (rdr_deferred_quad / _backward).
//
// The diffuse irradiance of a uniformly emitting polygon has a closed form: Lambert's contour integral over the edges of the
// polygon as seen from the texel, clipped to the texel's horizon.  So a G-buffer is lit by an area emitter exactly, without
// noise, and with gradients to the four corners.  Inputs per texel of the oversampled G-buffer: p, n and a of deferred.h's Texel
// (the alpha channel is not read).  Per quad, one row of sixteen floats: the corners q0..q3 in perimeter order [0..11], the
// radiance L[3] [12..14], [15] unused (its gradient is exactly 0); and a flag two_sided (the quad's entry of the descriptor's
// light_type: 0 one-sided, 1 two-sided).  The emitting side of a one-sided quad is that of cross(q1 - q0, q3 - q0).
//
// THE ORDER OF THE fp32 OPERATIONS (dot products are a[0] b[0] + a[1] b[1] + a[2] b[2], left to right;
//                                   u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)):
//   surface     nn = n.n; nothing unless 0 < nn < inf (background texels have n = 0) and p.p < inf.   nh = n / sqrtf(nn)
//   corners     r_i = q_i - p,  h_i = nh.r_i                                                            i = 0..3
//   contour     S = 0.  For edge i = 0..3, (A, B) = (r_i, r_{(i+1)%4}), (hA, hB) = (h_i, h_{(i+1)%4}):
//                   upA = hA > 0, upB = hB > 0;  neither: the edge adds nothing
//                   upA != upB:  x = A + (B - A) * (hA / (hA - hB));  the end that is not up is replaced by x;
//                                x is the EXIT point when upA, the ENTRY point when upB
//                   S += edge(A', B')
//               if some edge crossed:  S += edge(exit, entry)                      (the arc along the horizon)
//   edge(A, B)  c = B x A,  cc = c.c;  0 unless cc > 0;  s = sqrtf(cc);  (atan2f(s, A.B) * (c.nh)) / s
//   light       F = (two_sided ? |S| : fmaxf(S, 0)) / 2
//               rgb[k] += (L[k] * (a[k] / pi)) * F
// then the mean over each aa x aa block; the image has three channels (no alpha), like rdr_deferred_specular's.
// A quad that fills the hemisphere gives S = 2 pi and rgb = L a;  F / pi is the view factor of the heat-transfer tables.
// Every comparison is false for a NaN.  A NaN or an infinity in p fails p.p < inf: the definition would form inf - inf there,
// and the texel is gated instead, like a background texel.
// The normal is NORMALISED, as in the specular pass (deferred_specular.h); the point light of deferred.h uses it as stored.
// The quad is expected to be planar and convex: at most one exit and one entry.  For anything else the rule above still
// defines the result: the last exit and the last entry win.
// atan2f, sqrtf and the arithmetic are the device library's in BOTH builds of the library (this header is compiled in a unit the
// two share), as powf is in deferred.h.
//
// DERIVATIVES are those of the expression above as torch autograd takes them: the conditions (up*, cc > 0, the texel's gate) are
// constants; fmaxf(S, 0) passes HALF the gradient at S == 0 (deferred.h: step_half); |S| passes sign(S), 0 at 0; the crossing
// point x is differentiated through hA and hB (and so through nh and the corners); d atan2(s, d) = (d ds - s dd) / (s s + d d).
// A gated texel or edge adds exactly 0 to every gradient.  Gradients go to p, n, a, the twelve corner floats and L.  The only
// fp64 is the per-quad partial sums of the adjoint.
//
// SOFT SHADOWS (deferred_quad_shadow.h): the SHADOWED instantiations of the bodies and kernels below multiply F by a visibility
// factor per (quad, texel) that a shadow pass stored; the plain ones are untouched by it.
//
// The per-texel bodies are shared by the kernels at the end of this header (one lane per OUTPUT pixel) and by the plain loops of
// the CPU debugging harness.  They walk the four edges with constant indices, carrying S, the exit and entry points and the
// edges that made them: no per-lane array is indexed by a computed value.
#pragma once
#include "deferred.h"

namespace rdr {
namespace dfq {

using dfr::Texel; using dfr::View; using dfr::F4; using dfr::F2;
using dfr::dot3; using dfr::step_half; using dfr::finite_f; using dfr::load_texel; using dfr::texel_row; using dfr::kPi;

constexpr int kQuadFloats = 16;          // a row of the quad table: 64 bytes
constexpr int kRadiance = 12;            // [0..11] corners, [12..14] radiance, [15] unused
constexpr int kQuadGrads = 15;           // what the adjoint sums per quad

RDR_DEV_FN void cross3(const float *u, const float *v, float *c) {
    c[0] = u[1] * v[2] - u[2] * v[1]; c[1] = u[2] * v[0] - u[0] * v[2]; c[2] = u[0] * v[1] - u[1] * v[0];
}

// What the quads of a texel share.
struct Frame { float nh[3], len; };

RDR_DEV_FN bool frame_at(const Texel &t, Frame &f) {
    const float nn = dot3(t.n, t.n);
    if (!(nn > 0.f) || !finite_f(nn) || !finite_f(dot3(t.p, t.p))) return false;
    f.len = sqrtf(nn);
    for (int k = 0; k < 3; ++k) f.nh[k] = t.n[k] / f.len;
    return true;
}

enum { kBelow = 0, kWhole = 1, kExit = 2, kEntry = 3 };
// The edge A -> B against the horizon: kBelow adds nothing; kExit: B' = x; kEntry: A' = x.
RDR_DEV_FN int clip_edge(const float *A, const float *B, float hA, float hB, float *x) {
    const bool upA = hA > 0.f, upB = hB > 0.f;
    if (!upA && !upB) return kBelow;
    if (upA && upB) return kWhole;
    const float t = hA / (hA - hB);
    for (int k = 0; k < 3; ++k) x[k] = A[k] + (B[k] - A[k]) * t;
    return upA ? kExit : kEntry;
}

RDR_DEV_FN float edge_form(const float *A, const float *B, const float *nh) {
    float c[3];
    cross3(B, A, c);
    const float cc = dot3(c, c);
    if (!(cc > 0.f)) return 0.f;
    const float s = sqrtf(cc);
    return (atan2f(s, dot3(A, B)) * dot3(c, nh)) / s;
}

// dA, dB, dnh += dS * d edge(A, B) / d(A, B, nh)
RDR_DEV_FN void edge_adjoint(const float *A, const float *B, const float *nh, float dS, float *dA, float *dB, float *dnh) {
    float c[3];
    cross3(B, A, c);
    const float cc = dot3(c, c);
    if (!(cc > 0.f)) return;
    const float s = sqrtf(cc), d = dot3(A, B), g = dot3(c, nh), th = atan2f(s, d);
    const float q = cc + d * d;
    const float dth = (dS * g) / s, dg = (dS * th) / s;
    const float ds = dth * (d / q) - ((dS * th) * g) / cc;       // through atan2 and through 1 / s
    const float dd = -dth * (s / q);
    float dc[3], ax[3], xb[3];
    for (int k = 0; k < 3; ++k) {
        dc[k] = dg * nh[k] + (ds / s) * c[k];
        dnh[k] += dg * c[k];
    }
    cross3(A, dc, ax);                   // c = B x A
    cross3(dc, B, xb);
    for (int k = 0; k < 3; ++k) {
        dB[k] += ax[k] + dd * A[k];
        dA[k] += xb[k] + dd * B[k];
    }
}

// x = A + (B - A) * (hA / (hA - hB)), hA = nh.A, hB = nh.B:  dA, dB, dnh += what dx sends back
RDR_DEV_FN void crossing_adjoint(const float *A, const float *B, float hA, float hB, const float *nh, const float *dx, float *dA,
                                 float *dB, float *dnh) {
    const float den = hA - hB, t = hA / den;
    float dt = 0.f;
    for (int k = 0; k < 3; ++k) dt += dx[k] * (B[k] - A[k]);
    const float dhA = (dt * -hB) / (den * den), dhB = (dt * hA) / (den * den);
    for (int k = 0; k < 3; ++k) {
        dA[k] += (dx[k] - dx[k] * t) + dhA * nh[k];
        dB[k] += dx[k] * t + dhB * nh[k];
        dnh[k] += dhA * A[k] + dhB * B[k];
    }
}

// The contour so far: S, the exit and the entry point and the edges that made them (-1: none yet).
struct Walk { float S, ex[3], en[3]; int exit_edge, entry_edge; };

RDR_DEV_FN void walk_edge(int i, const float *A, const float *B, float hA, float hB, const float *nh, Walk &wk) {
    float x[3], a[3], b[3];
    const int kind = clip_edge(A, B, hA, hB, x);
    if (kind == kBelow) return;
    for (int k = 0; k < 3; ++k) {        // (selected by value: a pointer chosen by `kind` would put the points into scratch)
        const float xk = x[k], Ak = A[k], Bk = B[k];
        a[k] = kind == kEntry ? xk : Ak;
        b[k] = kind == kExit ? xk : Bk;
    }
    wk.S += edge_form(a, b, nh);
    const bool leaves = kind == kExit, enters = kind == kEntry;
    for (int k = 0; k < 3; ++k) {
        const float xk = x[k], exk = wk.ex[k], enk = wk.en[k];
        wk.ex[k] = leaves ? xk : exk;
        wk.en[k] = enters ? xk : enk;
    }
    const int was_exit = wk.exit_edge, was_entry = wk.entry_edge;
    wk.exit_edge = leaves ? i : was_exit;
    wk.entry_edge = enters ? i : was_entry;
}

// Edge i again, with dS pushed through it; dex / den: what the horizon arc sent to the exit / entry point.
RDR_DEV_FN void unwalk_edge(int i, const float *A, const float *B, float hA, float hB, const float *nh, const Walk &wk, float dS,
                            const float *dex, const float *den, float *dA, float *dB, float *dnh) {
    float x[3], a[3], b[3], da[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 0.f};
    const int kind = clip_edge(A, B, hA, hB, x);
    if (kind == kBelow) return;
    for (int k = 0; k < 3; ++k) {
        const float xk = x[k], Ak = A[k], Bk = B[k];
        a[k] = kind == kEntry ? xk : Ak;
        b[k] = kind == kExit ? xk : Bk;
    }
    edge_adjoint(a, b, nh, dS, da, db, dnh);
    if (kind == kWhole) {
        for (int k = 0; k < 3; ++k) { dA[k] += da[k]; dB[k] += db[k]; }
        return;
    }
    float dx[3];
    if (kind == kExit) {
        const bool last = wk.exit_edge == i;
        for (int k = 0; k < 3; ++k) { const float arc = db[k] + dex[k]; dA[k] += da[k]; dx[k] = last ? arc : db[k]; }
    } else {
        const bool last = wk.entry_edge == i;
        for (int k = 0; k < 3; ++k) { const float arc = da[k] + den[k]; dB[k] += db[k]; dx[k] = last ? arc : da[k]; }
    }
    crossing_adjoint(A, B, hA, hB, nh, dx, dA, dB, dnh);
}

// What quad `quad` (sixteen floats) adds to texel t with frame f.  !ADJOINT: rgb += its light.  ADJOINT, for the texel's upstream
// gradient w[3]: dt += the texel's gradient and, when PARAMS, part[15] += the quad's.  (The two passes of the adjoint kernel each
// use one half; the other is dead code there.)
// SHADOWED (here, in the three bodies below and in the kernels): V, the visibility factor of this (quad, texel) pair that the
// shadow pass stored (deferred_quad_shadow.h), multiplies F: F V stands where F stands, and dF is multiplied by V.  V is a
// constant of the adjoint.  The plain instantiation never looks at V and is the code it was before there were soft shadows.
template <bool ADJOINT, bool PARAMS, bool SHADOWED = false>
RDR_DEV_FN void quad_light(const float *quad, bool two_sided, const Texel &t, const Frame &f, const float *w, float *rgb, Texel &dt,
                           double *part, float V = 1.f) {
    float r0[3], r1[3], r2[3], r3[3];
    for (int k = 0; k < 3; ++k) {
        r0[k] = quad[k] - t.p[k]; r1[k] = quad[3 + k] - t.p[k]; r2[k] = quad[6 + k] - t.p[k]; r3[k] = quad[9 + k] - t.p[k];
    }
    const float h0 = dot3(f.nh, r0), h1 = dot3(f.nh, r1), h2 = dot3(f.nh, r2), h3 = dot3(f.nh, r3);
    Walk wk;
    wk.S = 0.f; wk.exit_edge = wk.entry_edge = -1;
    for (int k = 0; k < 3; ++k) wk.ex[k] = wk.en[k] = 0.f;
    walk_edge(0, r0, r1, h0, h1, f.nh, wk);
    walk_edge(1, r1, r2, h1, h2, f.nh, wk);
    walk_edge(2, r2, r3, h2, h3, f.nh, wk);
    walk_edge(3, r3, r0, h3, h0, f.nh, wk);
    const bool crossed = wk.exit_edge >= 0 || wk.entry_edge >= 0;
    if (crossed) wk.S += edge_form(wk.ex, wk.en, f.nh);
    const float S = wk.S;
    const float F0 = (two_sided ? fabsf(S) : fmaxf(S, 0.f)) / 2.f;
    const float F = SHADOWED ? F0 * V : F0;
    const float *L = quad + kRadiance;
    if (!ADJOINT) {
        for (int k = 0; k < 3; ++k) rgb[k] += (L[k] * (t.a[k] / kPi)) * F;
        return;
    }
    // ---- the adjoint ------------------------------------------------------------------------------------------------------
    float dF = 0.f;
    for (int k = 0; k < 3; ++k) {
        dF += w[k] * (L[k] * (t.a[k] / kPi));
        dt.a[k] += ((w[k] * L[k]) * F) / kPi;
        if (PARAMS) part[kRadiance + k] += (double)((w[k] * (t.a[k] / kPi)) * F);
    }
    if (SHADOWED) dF = dF * V;
    const float pass = two_sided ? (S > 0.f ? 1.f : (S < 0.f ? -1.f : 0.f)) : step_half(S);
    const float dS = (dF / 2.f) * pass;
    if (dS == 0.f) return;
    float d0[3] = {0.f, 0.f, 0.f}, d1[3] = {0.f, 0.f, 0.f}, d2[3] = {0.f, 0.f, 0.f}, d3[3] = {0.f, 0.f, 0.f};
    float dnh[3] = {0.f, 0.f, 0.f}, dex[3] = {0.f, 0.f, 0.f}, den[3] = {0.f, 0.f, 0.f};
    if (crossed) edge_adjoint(wk.ex, wk.en, f.nh, dS, dex, den, dnh);
    unwalk_edge(0, r0, r1, h0, h1, f.nh, wk, dS, dex, den, d0, d1, dnh);
    unwalk_edge(1, r1, r2, h1, h2, f.nh, wk, dS, dex, den, d1, d2, dnh);
    unwalk_edge(2, r2, r3, h2, h3, f.nh, wk, dS, dex, den, d2, d3, dnh);
    unwalk_edge(3, r3, r0, h3, h0, f.nh, wk, dS, dex, den, d3, d0, dnh);
    const float dnn = dot3(dnh, f.nh);
    for (int k = 0; k < 3; ++k) {
        dt.p[k] -= (d0[k] + d1[k]) + (d2[k] + d3[k]);
        dt.n[k] += (dnh[k] - dnn * f.nh[k]) / f.len;
        if (PARAMS) {
            part[k] += (double)d0[k]; part[3 + k] += (double)d1[k]; part[6 + k] += (double)d2[k]; part[9 + k] += (double)d3[k];
        }
    }
}

// Where the factor of pair `pair` of an image and texel (tx, ty) of pixel (x, y) stands among the image's factors.
RDR_DEV_FN size_t factor_at(const View &v, int pair, int y, int x, int ty, int tx) {
    const size_t hg = (size_t)v.height * v.aa, wg = (size_t)v.width * v.aa;
    return ((size_t)pair * hg + (size_t)y * v.aa + ty) * wg + (size_t)x * v.aa + tx;
}

// One OUTPUT pixel of image n: the light of the quads [lb, le) on its aa x aa texels, averaged, three floats.
// `factors` (SHADOWED): the image's first pair, [le - lb][height * aa][width * aa]; V is fetched before the edge walk and held as
// one scalar.
template <int C, bool SHADOWED = false>
RDR_DEV_FN void quad_pixel(const View &v, int n, int pix, int lb, int le, float *image, const float *factors = nullptr) {
    const int y = pix / v.width, x = pix - y * v.width;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            Frame f;
            if (!frame_at(t, f)) continue;
            float rgb[3] = {0.f, 0.f, 0.f};
            for (int l = lb; l < le; ++l) {
                const float V = SHADOWED ? factors[factor_at(v, l - lb, y, x, ty, tx)] : 1.f;
                quad_light<false, false, SHADOWED>(v.params + (size_t)l * kQuadFloats, v.type[l] != 0, t, f, nullptr, rgb, dt, nullptr, V);
            }
            for (int k = 0; k < 3; ++k) acc[k] += rgb[k];
        }
    }
    const float count = (float)(v.aa * v.aa);
    float *out = image + ((size_t)n * v.height * v.width + pix) * 3;
    for (int k = 0; k < 3; ++k) out[k] = acc[k] / count;
}

RDR_DEV_FN void load_upstream(const View &v, int n, int pix, const float *d_image, float *w) {
    const float *gi = d_image + ((size_t)n * v.height * v.width + pix) * 3;
    const float count = (float)(v.aa * v.aa);
    for (int k = 0; k < 3; ++k) w[k] = gi[k] / count;
}

// Adjoint, pass 1: the gradient of every texel of one output pixel (each texel belongs to exactly one pixel: plain stores).
// All nine channels are written; the alpha channel is 0.
template <int C, bool SHADOWED = false>
RDR_DEV_FN void quad_adjoint_texels(const View &v, int n, int pix, int lb, int le, const float *d_image, float *d_g,
                                    const float *factors = nullptr) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[3];
    load_upstream(v, n, pix, d_image, w);
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        float *drow = d_g + (row - v.g);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            Frame f;
            if (frame_at(t, f))
                for (int l = lb; l < le; ++l) {
                    const float V = SHADOWED ? factors[factor_at(v, l - lb, y, x, ty, tx)] : 1.f;
                    quad_light<true, false, SHADOWED>(v.params + (size_t)l * kQuadFloats, v.type[l] != 0, t, f, w, nullptr, dt, nullptr, V);
                }
            float *o = drow + tx * C;
            if (C == 10) {
                F2 *q = reinterpret_cast<F2 *>(o);
                q[0] = F2{dt.p[0], dt.p[1]}; q[1] = F2{dt.p[2], dt.n[0]}; q[2] = F2{dt.n[1], dt.n[2]};
                q[3] = F2{dt.a[0], dt.a[1]}; q[4] = F2{dt.a[2], 0.f};
            } else {
                for (int k = 0; k < 3; ++k) { o[k] = dt.p[k]; o[3 + k] = dt.n[k]; o[6 + k] = dt.a[k]; }
            }
        }
    }
}

// Adjoint, pass 2: what one output pixel adds to the fifteen gradients of quad l.
// (`factors`, SHADOWED: the factors of quad l's own pair, [height * aa][width * aa])
template <int C, bool SHADOWED = false>
RDR_DEV_FN void quad_adjoint_params(const View &v, int n, int pix, int l, const float *d_image, double *part,
                                    const float *factors = nullptr) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[3];
    load_upstream(v, n, pix, d_image, w);
    const float *quad = v.params + (size_t)l * kQuadFloats;
    const bool two_sided = v.type[l] != 0;
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            Frame f;
            if (!frame_at(t, f)) continue;
            const float V = SHADOWED ? factors[factor_at(v, 0, y, x, ty, tx)] : 1.f;
            quad_light<true, true, SHADOWED>(quad, two_sided, t, f, w, nullptr, dt, part, V);
        }
    }
}

// The factors of image n's first pair: pair_base[n] is the sum of the earlier images' range lengths.
RDR_DEV_FN const float *image_factors(const View &v, const float *factors, const int *pair_base, int n) {
    return factors + (size_t)pair_base[n] * ((size_t)v.height * v.aa * (size_t)v.width * v.aa);
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// grid = (blocks per image, N): the quad range of a block is uniform, so the table is read through scalar loads.
// SHADOWED: `factors` [pairs][height * aa][width * aa] and `pair_base` [N], the first pair of each image; the plain instantiations
// look at neither.
template <int C, bool SHADOWED>
__global__ void __launch_bounds__(256) deferred_quad_kernel(const float *__restrict__ g, const float *__restrict__ quads,
                                                            const int *__restrict__ type, const int *__restrict__ range, int height,
                                                            int width, int aa, float *__restrict__ image,
                                                            const float *__restrict__ factors, const int *__restrict__ pair_base) {
    const View v{g, quads, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    const float *fi = SHADOWED ? image_factors(v, factors, pair_base, n) : nullptr;
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += gridDim.x * 256)
        quad_pixel<C, SHADOWED>(v, n, pix, lb, le, image, fi);
}

// The two-pass shape of deferred_adjoint_kernel: a capped grid that strides over the pixels; pass 1 stores the texel gradients;
// pass 2 loops over the quads on the outside with fifteen fp64 partials per lane, summed across the wave, across the four waves
// through LDS, and the block writes ONE row of the slab: [quads of the image][15].  No atomics, a fixed order.
template <int C, bool SHADOWED>
__global__ void __launch_bounds__(256, 2) deferred_quad_adjoint_kernel(const float *__restrict__ g, const float *__restrict__ quads,
                                                                       const int *__restrict__ type, const int *__restrict__ range,
                                                                       int height, int width, int aa,
                                                                       const float *__restrict__ d_image, float *__restrict__ d_g,
                                                                       double *__restrict__ slab, int slab_stride,
                                                                       const float *__restrict__ factors,
                                                                       const int *__restrict__ pair_base) {
    const View v{g, quads, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    const float *fi = SHADOWED ? image_factors(v, factors, pair_base, n) : nullptr;
    for (int pix = first; pix < pixels; pix += step)
        quad_adjoint_texels<C, SHADOWED>(v, n, pix, lb, le, d_image, d_g, fi);
    __shared__ double wave_part[4][kQuadGrads];
    double *row = slab + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * slab_stride;
    for (int l = lb; l < le; ++l) {
        double part[kQuadGrads];
        for (int k = 0; k < kQuadGrads; ++k) part[k] = 0.0;
        for (int pix = first; pix < pixels; pix += step)
            quad_adjoint_params<C, SHADOWED>(v, n, pix, l, d_image, part, SHADOWED ? fi + factor_at(v, l - lb, 0, 0, 0, 0) : nullptr);
        for (int k = 0; k < kQuadGrads; ++k) part[k] = wave_sum(part[k]);           // every lane is active here
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < kQuadGrads; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
        __syncthreads();
        if (threadIdx.x < kQuadGrads) {
            const int k = threadIdx.x;
            row[(l - lb) * kQuadGrads + k] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
        }
        __syncthreads();
    }
}

// Block l folds quad l: the rows of the images that use it, in image order and block order.  Lane t takes rows t, t + 256, ...;
// then the lanes are summed as above.  Rounded to fp32 once; the unused sixteenth float of the row is written as 0.
__global__ void __launch_bounds__(256) deferred_quad_fold_kernel(const double *__restrict__ slab, int slab_stride,
                                                                 int blocks_per_image, const int *__restrict__ range, int num_images,
                                                                 float *__restrict__ d_quads) {
    const int l = blockIdx.x;
    double part[kQuadGrads];
    for (int k = 0; k < kQuadGrads; ++k) part[k] = 0.0;
    for (int n = 0; n < num_images; ++n) {
        const int lb = range[2 * n], le = range[2 * n + 1];
        if (l < lb || l >= le) continue;
        for (int b = threadIdx.x; b < blocks_per_image; b += 256) {
            const double *row = slab + (size_t)(n * blocks_per_image + b) * slab_stride + (l - lb) * kQuadGrads;
            for (int k = 0; k < kQuadGrads; ++k) part[k] += row[k];
        }
    }
    __shared__ double wave_part[4][kQuadGrads];
    for (int k = 0; k < kQuadGrads; ++k) part[k] = wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kQuadGrads; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < kQuadGrads) {
        const int k = threadIdx.x;
        d_quads[l * kQuadFloats + k] = (float)((wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]));
    } else if (threadIdx.x == kQuadGrads) {
        d_quads[l * kQuadFloats + kQuadGrads] = 0.f;
    }
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
// `factors` and `pair_base` (SHADOWED): see the kernels; in the harness pair_base is host memory
template <int C, bool SHADOWED = false>
inline void quad_impl(const rdr_deferred_desc &d, const View &v, float *image, const float *factors = nullptr,
                      const int *pair_base = nullptr) {
    const int pixels = d.height * d.width;
#if !defined(RDR_HOSTSIM)
    const dim3 grid((pixels + 255) / 256, d.num_images);
    hipLaunchKernelGGL((deferred_quad_kernel<C, SHADOWED>), grid, dim3(256), 0, exec::ctx().stream, v.g, v.params, v.type, v.range,
                       v.height, v.width, v.aa, image, factors, pair_base);
    exec::check(hipGetLastError(), "deferred_quad launch");
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            quad_pixel<C, SHADOWED>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], image,
                                    SHADOWED ? image_factors(v, factors, pair_base, n) : nullptr);
#endif
}

template <int C, bool SHADOWED = false>
inline void quad_adjoint_impl(const rdr_deferred_desc &d, const View &v, const float *d_image, float *d_g, float *d_quads,
                              const float *factors = nullptr, const int *pair_base = nullptr) {
    const int pixels = d.height * d.width;
#if !defined(RDR_HOSTSIM)
    int per_image = (pixels + 255) / 256;
    const int cap = dfr::kAdjointBlocks / d.num_images > 0 ? dfr::kAdjointBlocks / d.num_images : 1;
    if (per_image > cap) per_image = cap;
    int longest = 1;                     // (an all-empty table still gets a row per block: nothing is written to it)
    for (int n = 0; n < d.num_images; ++n) {
        const int len = d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
        if (len > longest) longest = len;
    }
    const int slab_stride = longest * kQuadGrads;
    Arena arena;
    double *slab = arena.get<double>((size_t)per_image * d.num_images * slab_stride);
    hipLaunchKernelGGL((deferred_quad_adjoint_kernel<C, SHADOWED>), dim3(per_image, d.num_images), dim3(256), 0, exec::ctx().stream,
                       v.g, v.params, v.type, v.range, v.height, v.width, v.aa, d_image, d_g, slab, slab_stride, factors, pair_base);
    exec::check(hipGetLastError(), "deferred_quad_adjoint launch");
    if (d.num_lights > 0) {
        hipLaunchKernelGGL(deferred_quad_fold_kernel, dim3(d.num_lights), dim3(256), 0, exec::ctx().stream, slab, slab_stride,
                           per_image, v.range, d.num_images, d_quads);
        exec::check(hipGetLastError(), "deferred_quad_fold launch");
    }
    exec::upload_flush();              // the stream is drained before the slab goes back to the pool
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            quad_adjoint_texels<C, SHADOWED>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], d_image, d_g,
                                             SHADOWED ? image_factors(v, factors, pair_base, n) : nullptr);
    for (int l = 0; l < d.num_lights; ++l) {
        double part[kQuadGrads] = {0};
        for (int n = 0; n < d.num_images; ++n) {
            if (l < v.range[2 * n] || l >= v.range[2 * n + 1]) continue;
            for (int pix = 0; pix < pixels; ++pix)
                quad_adjoint_params<C, SHADOWED>(v, n, pix, l, d_image, part,
                                                 SHADOWED ? image_factors(v, factors, pair_base, n) +
                                                            factor_at(v, l - v.range[2 * n], 0, 0, 0, 0) : nullptr);
        }
        for (int k = 0; k < kQuadGrads; ++k) d_quads[l * kQuadFloats + k] = (float)part[k];
        d_quads[l * kQuadFloats + kQuadGrads] = 0.f;
    }
#endif
}

// What both calls refuse before anything is launched.
inline void validate_quad(const rdr_deferred_desc &d, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (d.num_lights > 0 && d.light_type)
        for (int l = 0; l < d.num_lights; ++l)
            if (d.light_type[l] != 0 && d.light_type[l] != 1)
                fail("light_type of quad " + std::to_string(l) + " is " + std::to_string(d.light_type[l]) +
                     ": it must be 0 (one-sided) or 1 (two-sided)");
    dfr::validate(d, who);
    if (d.occluders || d.visibility || d.ao_occluders || d.ao_words || d.ao_rays != 0)
        fail("occluders, visibility, ao_occluders, ao_words and ao_rays must be zero: a quad light traces nothing");
}

template <class F>
inline void dispatch(bool alpha, const F &f) {
    if (alpha) f(std::integral_constant<int, 10>()); else f(std::integral_constant<int, 9>());
}

// rdr_deferred_quad: synchronised on return
inline void quad(const rdr_deferred_desc &d, const float *g, const float *quads, float *image) {
    const char *who = "rdr_deferred_quad";
    validate_quad(d, who);
    if (!g || !image || (d.num_lights > 0 && !quads)) throw std::runtime_error(std::string(who) + ": null tensor");
    if (d.alpha && ((uintptr_t)g & 7)) throw std::runtime_error(std::string(who) + ": with alpha the G-buffer must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, quads);
    dispatch(d.alpha != 0, [&](auto c) { quad_impl<decltype(c)::value>(d, v, image); });
    exec::upload_flush();
}

// rdr_deferred_quad_backward: synchronised on return.  Writes every element of d_g and d_quads.
inline void quad_backward(const rdr_deferred_desc &d, const float *g, const float *quads, const float *d_image, float *d_g,
                          float *d_quads) {
    const char *who = "rdr_deferred_quad_backward";
    validate_quad(d, who);
    if (!g || !d_image || !d_g || (d.num_lights > 0 && (!quads || !d_quads)))
        throw std::runtime_error(std::string(who) + ": null tensor");
    if (d.alpha && (((uintptr_t)g | (uintptr_t)d_g) & 7))
        throw std::runtime_error(std::string(who) + ": with alpha the G-buffers must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, quads);
    dispatch(d.alpha != 0, [&](auto c) { quad_adjoint_impl<decltype(c)::value>(d, v, d_image, d_g, d_quads); });
    exec::upload_flush();
}

} // namespace dfq
} // namespace rdr
