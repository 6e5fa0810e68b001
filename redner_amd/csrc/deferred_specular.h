// deferred_specular.h -- the specular half of deferred shading and its adjoint (rdr_deferred_specular / _backward).
//
// The lobe is the specular lobe of the path tracer's BSDF (csrc/bsdf.h; the reference's src/material.h:405-446: Blinn-Phong
// normal distribution, Smith shadowing by the rational fit, Schlick Fresnel), one-sided, lit by the point, spot and directional
// rows of deferred.h's light table.  Ambient rows and SH rows add no specular and their parameter gradients from here are exactly 0.
// Inputs per texel of the oversampled G-buffer: p and n of deferred.h's Texel (the albedo and alpha channels are not read), the
// material texel ks[3], rho, and the eye of the texel's image.
//
// THE ORDER OF THE fp32 OPERATIONS (dot products are a[0] b[0] + a[1] b[1] + a[2] b[2], left to right):
//   surface     nn = n.n; no specular unless 0 < nn < inf.   len = sqrtf(nn), nh = n / len
//               ev = eye - p, rv = sqrtf(ev.ev), v = ev / rv, cv = nh.v; no specular unless cv > 0
//               r = fmaxf(rho, 1e-3f), e = fmaxf(2 / r - 2, 0)
//   light       point        d = pos - p, r2 = d.d, rd = sqrtf(r2), l = d / rd, E_k = I_k / r2
//               spot         l likewise, s = -sdir / |sdir|, f = powf(fmaxf(l.s, 0), e_spot), E_k = I_k f
//               directional  l = -dir / |dir|, E_k = I_k
//   lobe        cl = nh.l; no specular unless cl > 1e-3f
//               hv = v + l, hl = sqrtf(hv.hv), m = hv / hl, cm = nh.m; no specular unless cm > 0
//               P = powf(cm, e), D = P (e + 2) / (2 pi)
//               G1(c): t = sqrtf(fmaxf(1 / (c c) - 1, 0)); t == 0: 1; a = 1 / (sqrtf(r) t); a >= 1.6: 1;
//                      else (3.535 a + (2.181 a) a) / ((1 + 2.276 a) + (2.577 a) a)
//               G = G1(cv) G1(cl),  B = (D G) / (4 cv)
//               x = m.l, q = fmaxf(1 - |x|, 0), q5 = ((q q) (q q)) q,  k_k = fmaxf(ks_k, 0),  F_k = k_k + (1 - k_k) q5
//               rgb[k] += (E_k F_k) B
// Every comparison is false for a NaN, so a texel on top of the eye or of a light is gated, not shaded.
//
// DERIVATIVES are those of the expression above as torch autograd takes them: every max(x, 0) and the roughness floor pass HALF
// the gradient at the tie (deferred.h: step_half); the conditions (cv > 0, cl > 1e-3, cm > 0, a >= 1.6, t == 0) and the
// visibility bits are constants.  d pow(cm, e) / d cm is formed as e P / cm (0 for e == 0), d / de as P logf(cm); the spot's
// pow follows deferred.h.  A gated texel or light adds exactly 0 to every gradient.  The only fp64 is the partial sums of the
// light parameters and of the eye.
//
// The per-texel bodies are shared by the kernels at the end of this header (one lane per OUTPUT pixel) and by the plain loops of
// the CPU debugging harness.
#pragma once
#include "deferred.h"

namespace rdr {
namespace dfs {

using dfr::Texel; using dfr::View; using dfr::F4; using dfr::F2;
using dfr::dot3; using dfr::step_half; using dfr::finite_f; using dfr::load_texel; using dfr::texel_row; using dfr::visibility_row;
using dfr::light_reaches; using dfr::kLightParams; using dfr::kIntensity; using dfr::kPosition; using dfr::kDirection;
using dfr::kExponent;

constexpr float kGrazing = 1e-3f, kRoughnessFloor = 1e-3f, kTwoPi = 6.28318530717958647692f;
constexpr int kEye = 3;                  // eye components; a slab row is [kEye][lights of the image][kLightParams]

// What the lights of a texel share.
struct Surface { float nh[3], len, v[3], rv, cv, r, e, ks[3], rho; };

RDR_DEV_FN bool surface_at(const Texel &t, const F4 &mat, const float *eye, Surface &s) {
    const float nn = dot3(t.n, t.n);
    if (!(nn > 0.f) || !finite_f(nn)) return false;
    s.len = sqrtf(nn);
    float ev[3];
    for (int k = 0; k < 3; ++k) { s.nh[k] = t.n[k] / s.len; ev[k] = eye[k] - t.p[k]; }
    s.rv = sqrtf(dot3(ev, ev));
    for (int k = 0; k < 3; ++k) s.v[k] = ev[k] / s.rv;
    s.cv = dot3(s.nh, s.v);
    if (!(s.cv > 0.f)) return false;
    s.ks[0] = mat.x; s.ks[1] = mat.y; s.ks[2] = mat.z; s.rho = mat.w;
    s.r = fmaxf(s.rho, kRoughnessFloor);
    s.e = fmaxf(2.f / s.r - 2.f, 0.f);
    return true;
}

// d max(rho, floor) / d rho
RDR_DEV_FN float floor_half(float rho) { return rho > kRoughnessFloor ? 1.f : (rho == kRoughnessFloor ? 0.5f : 0.f); }

// G1(c) at roughness r; when GRAD also its derivatives by c and by r (0 on the constant branches)
template <bool GRAD>
RDR_DEV_FN float smith_g1(float c, float r, float &dc, float &dr) {
    dc = dr = 0.f;
    const float t = sqrtf(fmaxf(1.f / (c * c) - 1.f, 0.f));
    if (t == 0.f) return 1.f;
    const float a = 1.f / (sqrtf(r) * t);
    if (a >= 1.6f) return 1.f;
    const float num = 3.535f * a + (2.181f * a) * a, den = (1.f + 2.276f * a) + (2.577f * a) * a;
    if (GRAD) {
        const float dg = ((3.535f + 4.362f * a) * den - num * (2.276f + 5.154f * a)) / (den * den);
        dc = dg * (a / ((t * t) * ((c * c) * c)));          // a = r^-1/2 (1 / c^2 - 1)^-1/2
        dr = dg * (-a / (2.f * r));
    }
    return num / den;
}

// What light (type, lp) adds to texel t with surface s.  !ADJOINT: rgb += the lobe.  ADJOINT, for the texel's upstream gradient
// w[3]: dt.p, dt.n, dmat[4] += the texel's gradient and, when PARAMS, part[10] += the light's and epart[3] += the eye's.  (The two
// passes of the adjoint kernel each use one half; the other is dead code there.)
template <bool ADJOINT, bool PARAMS>
RDR_DEV_FN void light_lobe(int type, const float *lp, const Texel &t, const Surface &s, const float *w, float *rgb, Texel &dt,
                           float *dmat, double *part, double *epart) {
    if (type == RDR_DL_AMBIENT || type >= RDR_DL_SH_R) return;
    const float *I = lp + kIntensity;
    float l[3], E[3], d[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
    float rd = 0.f, r2 = 0.f, nd = 0.f, ns = 0.f, sc0 = 0.f, sc = 0.f, f = 0.f;
    if (type == RDR_DL_DIRECTIONAL) {
        const float *Dr = lp + kDirection;
        nd = sqrtf(dot3(Dr, Dr));
        for (int k = 0; k < 3; ++k) { l[k] = -Dr[k] / nd; E[k] = I[k]; }
    } else {
        for (int k = 0; k < 3; ++k) d[k] = lp[kPosition + k] - t.p[k];
        r2 = dot3(d, d);
        rd = sqrtf(r2);
        for (int k = 0; k < 3; ++k) l[k] = d[k] / rd;
        if (type == RDR_DL_POINT) {
            for (int k = 0; k < 3; ++k) E[k] = I[k] / r2;
        } else {             // RDR_DL_SPOT (the table was validated)
            const float *Dr = lp + kDirection;
            ns = sqrtf(dot3(Dr, Dr));
            for (int k = 0; k < 3; ++k) sv[k] = -Dr[k] / ns;
            sc0 = dot3(l, sv);
            sc = fmaxf(sc0, 0.f);
            f = powf(sc, lp[kExponent]);
            for (int k = 0; k < 3; ++k) E[k] = I[k] * f;
        }
    }
    const float cl = dot3(s.nh, l);
    if (!(cl > kGrazing)) return;
    float hv[3], m[3];
    for (int k = 0; k < 3; ++k) hv[k] = s.v[k] + l[k];
    const float hl = sqrtf(dot3(hv, hv));
    for (int k = 0; k < 3; ++k) m[k] = hv[k] / hl;
    const float cm = dot3(s.nh, m);
    if (!(cm > 0.f)) return;
    const float P = powf(cm, s.e);
    const float D = P * (s.e + 2.f) / kTwoPi;
    float g1v_c, g1v_r, g1l_c, g1l_r;
    const float g1v = smith_g1<ADJOINT>(s.cv, s.r, g1v_c, g1v_r);
    const float g1l = smith_g1<ADJOINT>(cl, s.r, g1l_c, g1l_r);
    const float G = g1v * g1l;
    const float B = (D * G) / (4.f * s.cv);
    const float x = dot3(m, l);
    const float q0 = 1.f - fabsf(x), q = fmaxf(q0, 0.f);
    const float q4 = (q * q) * (q * q), q5 = q4 * q;
    float F[3];
    for (int k = 0; k < 3; ++k) {
        const float kk = fmaxf(s.ks[k], 0.f);
        F[k] = kk + (1.f - kk) * q5;
    }
    if (!ADJOINT) {
        for (int k = 0; k < 3; ++k) rgb[k] += (E[k] * F[k]) * B;
        return;
    }
    // ---- the adjoint ------------------------------------------------------------------------------------------------------
    float dE[3], dB = 0.f, dq5 = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float kk = fmaxf(s.ks[k], 0.f);
        const float dF = (w[k] * E[k]) * B;
        dE[k] = (w[k] * F[k]) * B;
        dB += w[k] * (E[k] * F[k]);
        dmat[k] += (dF * (1.f - q5)) * step_half(s.ks[k]);
        dq5 += dF * (1.f - kk);
    }
    // |x|: the sign of x (0 at 0); q = max(q0, 0): half at the tie
    const float dx = -((5.f * q4) * dq5 * step_half(q0)) * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
    const float inv = 1.f / (4.f * s.cv);
    const float dD = (dB * G) * inv, dG = (dB * D) * inv;
    float dcv = -(dB * B) / s.cv;
    const float dcm = s.e > 0.f ? (dD * (s.e + 2.f) / kTwoPi) * (s.e * P / cm) : 0.f;
    const float de = dD * (P / kTwoPi + (P * logf(cm)) * (s.e + 2.f) / kTwoPi);
    float dr = (de * step_half(2.f / s.r - 2.f)) * (-2.f / (s.r * s.r));
    dcv += (dG * g1l) * g1v_c;
    const float dcl = (dG * g1v) * g1l_c;
    dr += dG * (g1l * g1v_r + g1v * g1l_r);
    dmat[3] += dr * floor_half(s.rho);
    float dnh[3], dl[3], dv[3], dm[3];
    for (int k = 0; k < 3; ++k) {
        dnh[k] = (dcl * l[k] + dcv * s.v[k]) + dcm * m[k];
        dm[k] = dcm * s.nh[k] + dx * l[k];
        dl[k] = dcl * s.nh[k] + dx * m[k];
        dv[k] = dcv * s.nh[k];
    }
    const float dmm = dot3(dm, m);
    for (int k = 0; k < 3; ++k) {
        const float dhv = (dm[k] - dmm * m[k]) / hl;
        dl[k] += dhv;
        dv[k] += dhv;
    }
    const float dvv = dot3(dv, s.v), dnn = dot3(dnh, s.nh);
    for (int k = 0; k < 3; ++k) {
        const float dev = (dv[k] - dvv * s.v[k]) / s.rv;
        dt.p[k] -= dev;
        dt.n[k] += (dnh[k] - dnn * s.nh[k]) / s.len;
        if (PARAMS) epart[k] += (double)dev;
    }
    if (type == RDR_DL_DIRECTIONAL) {
        if (PARAMS) {
            const float dll = dot3(dl, l);
            for (int k = 0; k < 3; ++k) {
                part[kIntensity + k] += (double)dE[k];
                part[kDirection + k] += (double)(-(dl[k] - dll * l[k]) / nd);
            }
        }
        return;
    }
    if (type == RDR_DL_POINT) {
        const float dr2 = -((dE[0] * E[0] + dE[1] * E[1]) + dE[2] * E[2]) / r2;         // E_k = I_k / r2
        const float dll = dot3(dl, l);
        for (int k = 0; k < 3; ++k) {
            const float dd = (dl[k] - dll * l[k]) / rd + 2.f * d[k] * dr2;
            dt.p[k] -= dd;
            if (PARAMS) {
                part[kIntensity + k] += (double)(dE[k] / r2);
                part[kPosition + k] += (double)dd;
            }
        }
        return;
    }
    // RDR_DL_SPOT
    const float es = lp[kExponent];
    const float df = (dE[0] * I[0] + dE[1] * I[1]) + dE[2] * I[2];
    // e * sc^(e-1): 1 at sc == 0 for e == 1, 0 for e > 1; for e < 1 (inf) the gradient is defined as 0 (deferred.h)
    const float dsc = (sc == 0.f && es < 1.f) ? 0.f : df * es * powf(sc, es - 1.f);
    const float dsc0 = dsc * step_half(sc0);
    float ds[3];
    for (int k = 0; k < 3; ++k) { dl[k] += dsc0 * sv[k]; ds[k] = dsc0 * l[k]; }
    const float dll = dot3(dl, l);
    for (int k = 0; k < 3; ++k) {
        const float dd = (dl[k] - dll * l[k]) / rd;
        dt.p[k] -= dd;
        if (PARAMS) {
            part[kIntensity + k] += (double)(dE[k] * f);
            part[kPosition + k] += (double)dd;
        }
    }
    if (PARAMS) {
        const float dss = dot3(ds, sv);
        for (int k = 0; k < 3; ++k) part[kDirection + k] += (double)(-(ds[k] - dss * sv[k]) / ns);
        if (sc > 0.f) part[kExponent] += (double)(df * f * logf(sc));
    }
}

// the material texel that belongs to G-buffer texel `texel` (a pointer into v.g) of C channels
template <int C>
RDR_DEV_FN size_t material_offset(const View &v, const float *texel) { return (size_t)(texel - v.g) / C * 4; }

// One OUTPUT pixel of image n: the lobe of its aa x aa texels under the lights [lb, le), averaged, three floats.
// SHADOWED (here and in the two adjoint bodies): a light whose bit in the texel's word of `vis` is 0 is skipped.
template <int C, bool SHADOWED>
RDR_DEV_FN void specular_pixel(const View &v, const float *material, const float *eye, int n, int pix, int lb, int le, float *image,
                               const uint32_t *vis) {
    const int y = pix / v.width, x = pix - y * v.width;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        const F4 *mrow = reinterpret_cast<const F4 *>(material + material_offset<C>(v, row));
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            Surface s;
            if (!surface_at(t, mrow[tx], eye + 3 * n, s)) continue;
            float rgb[3] = {0.f, 0.f, 0.f};
            const uint32_t word = SHADOWED ? vrow[tx] : 0u;
            for (int l = lb; l < le; ++l) {
                if (SHADOWED && !light_reaches(word, l - lb)) continue;
                light_lobe<false, false>(v.type[l], v.params + (size_t)l * kLightParams, t, s, nullptr, rgb, dt, nullptr, nullptr,
                                         nullptr);
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
// d_g: p and n; the albedo and alpha channels are written as 0.  d_material: all four channels.
template <int C, bool SHADOWED>
RDR_DEV_FN void adjoint_pixel_texels(const View &v, const float *material, const float *eye, int n, int pix, int lb, int le,
                                     const float *d_image, float *d_g, float *d_material, const uint32_t *vis) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[3];
    load_upstream(v, n, pix, d_image, w);
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        const size_t moff = material_offset<C>(v, row);
        const F4 *mrow = reinterpret_cast<const F4 *>(material + moff);
        F4 *dmrow = reinterpret_cast<F4 *>(d_material + moff);
        float *drow = d_g + (row - v.g);
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha, dmat[4] = {0.f, 0.f, 0.f, 0.f};
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = 0.f;
            Surface s;
            if (surface_at(t, mrow[tx], eye + 3 * n, s)) {
                const uint32_t word = SHADOWED ? vrow[tx] : 0u;
                for (int l = lb; l < le; ++l) {
                    if (SHADOWED && !light_reaches(word, l - lb)) continue;
                    light_lobe<true, false>(v.type[l], v.params + (size_t)l * kLightParams, t, s, w, nullptr, dt, dmat, nullptr,
                                            nullptr);
                }
            }
            dmrow[tx] = F4{dmat[0], dmat[1], dmat[2], dmat[3]};
            float *o = drow + tx * C;
            if (C == 10) {
                F2 *q = reinterpret_cast<F2 *>(o);
                q[0] = F2{dt.p[0], dt.p[1]}; q[1] = F2{dt.p[2], dt.n[0]}; q[2] = F2{dt.n[1], dt.n[2]};
                q[3] = F2{0.f, 0.f}; q[4] = F2{0.f, 0.f};
            } else {
                for (int k = 0; k < 3; ++k) { o[k] = dt.p[k]; o[3 + k] = dt.n[k]; o[6 + k] = 0.f; }
            }
        }
    }
}

// Adjoint, pass 2: what one output pixel adds to the ten parameter gradients of light l and, through that light, to the eye.
template <int C, bool SHADOWED>
RDR_DEV_FN void adjoint_pixel_light(const View &v, const float *material, const float *eye, int n, int pix, int l, int lb,
                                    const float *d_image, double *part, double *epart, const uint32_t *vis) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[3];
    load_upstream(v, n, pix, d_image, w);
    const int type = v.type[l];
    const float *lp = v.params + (size_t)l * kLightParams;
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        const F4 *mrow = reinterpret_cast<const F4 *>(material + material_offset<C>(v, row));
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            if (SHADOWED && !light_reaches(vrow[tx], l - lb)) continue;
            Texel t, dt;
            float alpha, dmat[4] = {0.f, 0.f, 0.f, 0.f};
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = 0.f;
            Surface s;
            if (!surface_at(t, mrow[tx], eye + 3 * n, s)) continue;
            light_lobe<true, true>(type, lp, t, s, w, nullptr, dt, dmat, part, epart);
        }
    }
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// grid = (blocks per image, N): the light range and the eye of a block are uniform, so the table is read through scalar loads.
template <int C, bool SHADOWED>
__global__ void __launch_bounds__(256) deferred_specular_kernel(const float *__restrict__ g, const float *__restrict__ material,
                                                                const float *__restrict__ eye, const float *__restrict__ params,
                                                                const int *__restrict__ type, const int *__restrict__ range,
                                                                int height, int width, int aa, float *__restrict__ image,
                                                                const uint32_t *__restrict__ vis) {
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += gridDim.x * 256)
        specular_pixel<C, SHADOWED>(v, material, eye, n, pix, lb, le, image, vis);
}

// The two-pass shape of deferred_adjoint_kernel: a capped grid that strides over the pixels; pass 1 stores the texel gradients;
// pass 2 loops over the lights on the outside with ten fp64 partials of the light and three of the eye per lane, summed across
// the wave, across the four waves through LDS, and the block writes ONE row of the slab: [3 eye][lights of the image][10].  No
// atomics, a fixed order.
template <int C, bool SHADOWED>
__global__ void __launch_bounds__(256, 2) deferred_specular_adjoint_kernel(
    const float *__restrict__ g, const float *__restrict__ material, const float *__restrict__ eye, const float *__restrict__ params,
    const int *__restrict__ type, const int *__restrict__ range, int height, int width, int aa, const float *__restrict__ d_image,
    float *__restrict__ d_g, float *__restrict__ d_material, double *__restrict__ slab, int slab_stride,
    const uint32_t *__restrict__ vis) {
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int pix = first; pix < pixels; pix += step)
        adjoint_pixel_texels<C, SHADOWED>(v, material, eye, n, pix, lb, le, d_image, d_g, d_material, vis);
    __shared__ double wave_part[4][kLightParams];
    double *row = slab + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * slab_stride;
    double epart[kEye] = {0.0, 0.0, 0.0};
    for (int l = lb; l < le; ++l) {
        double part[kLightParams];
        for (int k = 0; k < kLightParams; ++k) part[k] = 0.0;
        for (int pix = first; pix < pixels; pix += step)
            adjoint_pixel_light<C, SHADOWED>(v, material, eye, n, pix, l, lb, d_image, part, epart, vis);
        for (int k = 0; k < kLightParams; ++k) part[k] = wave_sum(part[k]);         // every lane is active here
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < kLightParams; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
        __syncthreads();
        if (threadIdx.x < kLightParams) {
            const int k = threadIdx.x;
            row[kEye + (l - lb) * kLightParams + k] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
        }
        __syncthreads();
    }
    for (int k = 0; k < kEye; ++k) epart[k] = wave_sum(epart[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kEye; ++k) wave_part[threadIdx.x >> 6][k] = epart[k];
    __syncthreads();
    if (threadIdx.x < kEye) {
        const int k = threadIdx.x;
        row[k] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
    }
}

// Block b < L folds light b: the rows of the images that use it, in image order and block order.  Block L + n folds the eye of
// image n.  Lane t takes rows t, t + 256, ...; then the lanes are summed as above.  Rounded to fp32 once.
__global__ void __launch_bounds__(256) deferred_specular_fold_kernel(const double *__restrict__ slab, int slab_stride,
                                                                     int blocks_per_image, const int *__restrict__ range,
                                                                     int num_images, int num_lights, float *__restrict__ d_params,
                                                                     float *__restrict__ d_eye) {
    const bool is_eye = (int)blockIdx.x >= num_lights;
    const int l = blockIdx.x, image = (int)blockIdx.x - num_lights;
    const int count = is_eye ? kEye : kLightParams;
    double part[kLightParams];
    for (int k = 0; k < kLightParams; ++k) part[k] = 0.0;
    for (int n = is_eye ? image : 0; n < (is_eye ? image + 1 : num_images); ++n) {
        const int lb = range[2 * n], le = range[2 * n + 1];
        if (!is_eye && (l < lb || l >= le)) continue;
        const int offset = is_eye ? 0 : kEye + (l - lb) * kLightParams;
        for (int b = threadIdx.x; b < blocks_per_image; b += 256) {
            const double *row = slab + (size_t)(n * blocks_per_image + b) * slab_stride + offset;
            for (int k = 0; k < kLightParams; ++k)
                if (k < count) part[k] += row[k];
        }
    }
    __shared__ double wave_part[4][kLightParams];
    for (int k = 0; k < kLightParams; ++k) part[k] = wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kLightParams; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if ((int)threadIdx.x < count) {
        const int k = threadIdx.x;
        const float sum = (float)((wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]));
        if (is_eye) d_eye[image * kEye + k] = sum; else d_params[l * kLightParams + k] = sum;
    }
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
template <int C, bool SHADOWED>
inline void specular_impl(const rdr_deferred_desc &d, const View &v, const float *material, const float *eye, float *image) {
    const int pixels = d.height * d.width;
    const uint32_t *vis = d.visibility;
#if !defined(RDR_HOSTSIM)
    const dim3 grid((pixels + 255) / 256, d.num_images);
    hipLaunchKernelGGL((deferred_specular_kernel<C, SHADOWED>), grid, dim3(256), 0, exec::ctx().stream, v.g, material, eye, v.params,
                       v.type, v.range, v.height, v.width, v.aa, image, vis);
    exec::check(hipGetLastError(), "deferred_specular launch");
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            specular_pixel<C, SHADOWED>(v, material, eye, n, pix, v.range[2 * n], v.range[2 * n + 1], image, vis);
#endif
}

template <int C, bool SHADOWED>
inline void specular_adjoint_impl(const rdr_deferred_desc &d, const View &v, const float *material, const float *eye,
                                  const float *d_image, float *d_g, float *d_material, float *d_eye, float *d_params) {
    const int pixels = d.height * d.width;
    const uint32_t *vis = d.visibility;
#if !defined(RDR_HOSTSIM)
    int per_image = (pixels + 255) / 256;
    const int cap = dfr::kAdjointBlocks / d.num_images > 0 ? dfr::kAdjointBlocks / d.num_images : 1;
    if (per_image > cap) per_image = cap;
    int longest = 0;
    for (int n = 0; n < d.num_images; ++n) {
        const int len = d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
        if (len > longest) longest = len;
    }
    const int slab_stride = kEye + longest * kLightParams;
    Arena arena;
    double *slab = arena.get<double>((size_t)per_image * d.num_images * slab_stride);
    hipLaunchKernelGGL((deferred_specular_adjoint_kernel<C, SHADOWED>), dim3(per_image, d.num_images), dim3(256), 0,
                       exec::ctx().stream, v.g, material, eye, v.params, v.type, v.range, v.height, v.width, v.aa, d_image, d_g,
                       d_material, slab, slab_stride, vis);
    exec::check(hipGetLastError(), "deferred_specular_adjoint launch");
    hipLaunchKernelGGL(deferred_specular_fold_kernel, dim3(d.num_lights + d.num_images), dim3(256), 0, exec::ctx().stream, slab,
                       slab_stride, per_image, v.range, d.num_images, d.num_lights, d_params, d_eye);
    exec::check(hipGetLastError(), "deferred_specular_fold launch");
    exec::upload_flush();              // the stream is drained before the slab goes back to the pool
#else
    std::vector<double> eye_part((size_t)d.num_images * kEye, 0.0);
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            adjoint_pixel_texels<C, SHADOWED>(v, material, eye, n, pix, v.range[2 * n], v.range[2 * n + 1], d_image, d_g, d_material,
                                              vis);
    for (int l = 0; l < d.num_lights; ++l) {
        double part[kLightParams] = {0};
        for (int n = 0; n < d.num_images; ++n) {
            if (l < v.range[2 * n] || l >= v.range[2 * n + 1]) continue;
            for (int pix = 0; pix < pixels; ++pix)
                adjoint_pixel_light<C, SHADOWED>(v, material, eye, n, pix, l, v.range[2 * n], d_image, part,
                                                 eye_part.data() + (size_t)n * kEye, vis);
        }
        for (int k = 0; k < kLightParams; ++k) d_params[l * kLightParams + k] = (float)part[k];
    }
    for (size_t k = 0; k < eye_part.size(); ++k) d_eye[k] = (float)eye_part[k];
#endif
}

// What both calls refuse before anything is launched.
inline void validate_specular(const rdr_deferred_desc &d, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    dfr::validate(d, who);
    if (d.occluders || d.ao_occluders || d.ao_words || d.ao_rays != 0)
        fail("occluders, ao_occluders, ao_words and ao_rays must be zero: the lobe traces nothing (visibility words are read only)");
    if (d.visibility && ((uintptr_t)d.visibility & 3)) fail("the visibility buffer must be 4-byte aligned");
    if (!d.visibility) return;
    for (int n = 0; n < d.num_images; ++n) {
        const int len = d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
        if (len > 32)
            fail("image " + std::to_string(n) + " has " + std::to_string(len) + " lights, at most 32 fit its visibility word");
    }
}

template <class F>
inline void dispatch(bool alpha, bool shadowed, const F &f) {
    using std::integral_constant;
    auto by_mode = [&](auto c) {
        if (shadowed) f(c, integral_constant<bool, true>()); else f(c, integral_constant<bool, false>());
    };
    if (alpha) by_mode(integral_constant<int, 10>()); else by_mode(integral_constant<int, 9>());
}

// rdr_deferred_specular: synchronised on return
inline void specular(const rdr_deferred_desc &d, const float *g, const float *material, const float *eye, const float *params,
                     float *image) {
    const char *who = "rdr_deferred_specular";
    validate_specular(d, who);
    if (!g || !material || !eye || !image || (d.num_lights > 0 && !params)) throw std::runtime_error(std::string(who) + ": null tensor");
    if ((uintptr_t)material & 15) throw std::runtime_error(std::string(who) + ": the material buffer must be 16-byte aligned");
    if (d.alpha && ((uintptr_t)g & 7)) throw std::runtime_error(std::string(who) + ": with alpha the G-buffer must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, params);
    dispatch(d.alpha != 0, d.visibility != nullptr, [&](auto c, auto shadowed) {
        specular_impl<decltype(c)::value, decltype(shadowed)::value>(d, v, material, eye, image);
    });
    exec::upload_flush();
}

// rdr_deferred_specular_backward: synchronised on return.  Writes every element of d_g, d_material, d_eye and d_params.
inline void specular_backward(const rdr_deferred_desc &d, const float *g, const float *material, const float *eye,
                              const float *params, const float *d_image, float *d_g, float *d_material, float *d_eye,
                              float *d_params) {
    const char *who = "rdr_deferred_specular_backward";
    validate_specular(d, who);
    if (!g || !material || !eye || !d_image || !d_g || !d_material || !d_eye || (d.num_lights > 0 && (!params || !d_params)))
        throw std::runtime_error(std::string(who) + ": null tensor");
    if (((uintptr_t)material | (uintptr_t)d_material) & 15)
        throw std::runtime_error(std::string(who) + ": the material buffers must be 16-byte aligned");
    if (d.alpha && (((uintptr_t)g | (uintptr_t)d_g) & 7))
        throw std::runtime_error(std::string(who) + ": with alpha the G-buffers must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, params);
    dispatch(d.alpha != 0, d.visibility != nullptr, [&](auto c, auto shadowed) {
        specular_adjoint_impl<decltype(c)::value, decltype(shadowed)::value>(d, v, material, eye, d_image, d_g, d_material, d_eye,
                                                                             d_params);
    });
    exec::upload_flush();
}

} // namespace dfs
} // namespace rdr
