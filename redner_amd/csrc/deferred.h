// deferred.h -- deferred shading of a G-buffer and its adjoint (rdr_deferred_shade / rdr_deferred_shade_backward).
//
// The G-buffer is [N, H*aa, W*aa, C] fp32 with C = 9 (position 3, shading normal 3, diffuse reflectance 3) or 10 (+ alpha).
// Every texel is shaded by the lights of its image and the aa x aa texels of an output pixel are averaged: [N, H, W, 3 | 4].
// The meaning is that of pyredner/render_utils.py:8-102 (the four light classes) and :197-213 (sum over the lights, alpha
// appended unshaded, interpolate(mode='area')), derivatives as torch autograd takes them:
//   * max(x, 0) passes HALF the gradient at x == 0 exactly (torch.max of two tensors splits ties);
//   * pow(c, e): d/de = 0 at c == 0; d/dc = e * c^(e-1), which is 1 at c == 0 for e == 1 and 0 for e > 1.  For e < 1 the
//     reference yields inf * 0 = NaN behind the spot; here that gradient is 0.
//
// LIGHT TABLE: one `int type[L]` (rdr_deferred_light_type) and `float params[L][10]`:
//   [0..2] intensity (all types)   [3..5] position (point, spot)   [6..8] direction (directional; spot: spot_direction)
//   [9] spot exponent (spot)       -- entries a type does not use are ignored and their gradient is 0.
// Image n is lit by the lights [range[2n], range[2n+1]) of the table.
//
// SH ROWS (RDR_DL_SH_R / _G / _B; not in the reference, whose deferred lights are the four above): a row lights ONE colour
// channel c with an environment given by nine spherical-harmonic coefficients, [0..8] = k_i in the order i = l*l + l + m of
// rdr_sh_reconstruct (l = 0..2, m = -l..l); [9] is unused and its gradient is 0.  The Python SHLight is three consecutive rows.
// The basis and the directions are those of rdr_sh_reconstruct and of an environment map with identity env_to_world: the texel
// of the reconstructed map at (theta, phi) lies in world direction (sin phi sin theta, cos theta, -cos phi sin theta).  With the
// texel's shading normal n AS STORED (not normalised, like the other lights), x = -n.z, y = n.x, z = n.y:
//   Y0 =  0.28209479           Y1 = -0.48860251 y         Y2 =  0.48860251 z        Y3 = -0.48860251 x
//   Y4 = (1.09254843 x) y      Y5 = (-1.09254843 y) z     Y6 =  0.31539157 ((3 z) z - 1)
//   Y7 = (-1.09254843 x) z     Y8 =  0.54627422 (x x - y y)
//   E  = sum over ascending i, from 0.f, of (A_i k_i) Y_i,   A_i = pi (l = 0), 2 pi / 3 (l = 1), pi / 4 (l = 2): the irradiance
//   the row adds  max(E, 0) * (a_c / pi)  to channel c and nothing to the others.
// All in fp32 in exactly that order.  The clamp (an order-2 expansion rings negative) follows the rule above: at E == 0 exactly
// half the gradient passes, so all-zero coefficients -- where an optimisation starts -- receive a gradient.  Derivatives, for
// the texel's upstream gradient w:  d k_i = w_c (a_c / pi) step_half(E) (A_i Y_i);  d a_c = w_c max(E, 0) / pi;  d n through
// dY_i / d(x, y, z) and the permutation above;  d p = 0 exactly.  SH rows cast no shadow ray (like ambient rows), and their
// bits in a visibility word stay set.
//
// The per-texel bodies below are shared by the kernels (one lane per OUTPUT pixel, at the end of this header) and by the plain
// loops of the CPU debugging harness.  Arithmetic is fp32 in the order the reference's torch expressions evaluate; the only
// fp64 is the light-parameter partial sums of the adjoint.
#pragma once
#include "../../include/redner_amd.h"
#include "arena.h"
#include "scene.h"
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace rdr {
namespace dfr {

constexpr int kLightParams = 10;
constexpr int kIntensity = 0, kPosition = 3, kDirection = 6, kExponent = 9;
constexpr float kPi = 3.14159265358979323846f;

struct Texel { float p[3], n[3], a[3]; };
// 8- and 16-byte accesses: alpha texels (40 bytes) and alpha pixels (16 bytes); rdr_deferred_shade* check the alignment
struct alignas(8) F2 { float x, y; };
struct alignas(16) F4 { float x, y, z, w; };

// What a launch reads and writes.  `type` / `range` are DEVICE copies of the descriptor's host arrays.
struct View {
    const float *g;          // G-buffer
    const float *params;     // [L][10]
    const int *type;         // [L]
    const int *range;        // [N][2]
    int height, width, aa;   // OUTPUT size
};

RDR_DEV_FN float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// d max(x, 0) / dx as torch.max(x, zeros) has it
RDR_DEV_FN float step_half(float x) { return x > 0.f ? 1.f : (x == 0.f ? 0.5f : 0.f); }

template <int C>
RDR_DEV_FN void load_texel(const float *t, Texel &x, float &alpha) {
    if (C == 10) {           // 40-byte texels: 8-byte aligned
        const F2 *q = reinterpret_cast<const F2 *>(t);
        const F2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
        x.p[0] = a.x; x.p[1] = a.y; x.p[2] = b.x; x.n[0] = b.y; x.n[1] = c.x; x.n[2] = c.y;
        x.a[0] = d.x; x.a[1] = d.y; x.a[2] = e.x; alpha = e.y;
    } else {
        for (int k = 0; k < 3; ++k) { x.p[k] = t[k]; x.n[k] = t[3 + k]; x.a[k] = t[6 + k]; }
        alpha = 0.f;
    }
}

// ---- SH rows: the basis at a normal and the irradiance of a row, in the order the header comment states -----------------------
constexpr int kShCoeffs = 9;
constexpr float kShK0 = 0.282094791774f, kShK1 = 0.488602511903f, kShK2 = 1.092548430592f, kShK20 = 0.315391565253f,
                kShK22 = 0.546274215296f;
// the clamped-cosine factor A_i of coefficient i (a constant once the loops over i are unrolled)
RDR_DEV_FN float sh_lobe(int i) { return i == 0 ? kPi : (i < 4 ? 2.09439510239319549f : 0.78539816339744831f); }
RDR_DEV_FN void sh_basis(const float *n, float *Y) {
    const float x = -n[2], y = n[0], z = n[1];
    Y[0] = kShK0; Y[1] = -kShK1 * y; Y[2] = kShK1 * z; Y[3] = -kShK1 * x;
    Y[4] = (kShK2 * x) * y; Y[5] = (-kShK2 * y) * z; Y[6] = kShK20 * ((3.f * z) * z - 1.f);
    Y[7] = (-kShK2 * x) * z; Y[8] = kShK22 * (x * x - y * y);
}
RDR_DEV_FN float sh_irradiance(const float *k, const float *Y) {
    float E = 0.f;
    for (int i = 0; i < kShCoeffs; ++i) E += (sh_lobe(i) * k[i]) * Y[i];
    return E;
}
// max(E, 0) of an SH row with coefficients k at a texel with normal n
RDR_DEV_FN float sh_irradiance_at(const float *k, const float *n) {
    float Y[kShCoeffs];
    sh_basis(n, Y);
    return fmaxf(sh_irradiance(k, Y), 0.f);
}
// The adjoint of an SH row for a (the albedo) and w (the upstream gradient) of ITS channel: da, dn += the texel's gradient; when
// PARAMS, part[0..8] += the coefficients' instead.  The caller names the channel by a constant index (a branch per type): an
// index computed from the type puts the kernel's per-lane arrays into scratch memory.
template <bool PARAMS>
RDR_DEV_FN void sh_adjoint_row(const float *k, const float *n, float a, float w, float &da, float *dn, double *part) {
    float Y[kShCoeffs];
    sh_basis(n, Y);
    const float E0 = sh_irradiance(k, Y), E = fmaxf(E0, 0.f);
    const float dE = w * (a / kPi) * step_half(E0);
    if (PARAMS) {
        for (int i = 0; i < kShCoeffs; ++i) part[i] += (double)(dE * (sh_lobe(i) * Y[i]));
        return;
    }
    // dE / d(x, y, z) = sum_i (A_i k_i) dY_i / d(x, y, z), each sum in ascending i
    const float x = -n[2], y = n[0], z = n[1];
    float q[kShCoeffs];
    for (int i = 0; i < kShCoeffs; ++i) q[i] = sh_lobe(i) * k[i];
    const float gx = ((q[3] * -kShK1 + q[4] * (kShK2 * y)) + q[7] * (-kShK2 * z)) + q[8] * ((2.f * kShK22) * x);
    const float gy = ((q[1] * -kShK1 + q[4] * (kShK2 * x)) + q[5] * (-kShK2 * z)) + q[8] * ((-2.f * kShK22) * y);
    const float gz = ((q[2] * kShK1 + q[5] * (-kShK2 * y)) + q[6] * ((6.f * kShK20) * z)) + q[7] * (-kShK2 * x);
    da += w * E / kPi;
    dn[0] += dE * gy; dn[1] += dE * gz; dn[2] -= dE * gx;
}

// rgb += what light (type, lp) adds to texel t
RDR_DEV_FN void light_shade(int type, const float *lp, const Texel &t, float *rgb) {
    const float *I = lp + kIntensity;
    switch (type) {
    case RDR_DL_SH_R: case RDR_DL_SH_G: case RDR_DL_SH_B: {
        const float E = sh_irradiance_at(lp, t.n);       // once; the three channels differ in what follows only
        for (int k = 0; k < 3; ++k)
            if (k == type - RDR_DL_SH_R) rgb[k] += E * (t.a[k] / kPi);
        break;
    }
    case RDR_DL_AMBIENT:
        for (int k = 0; k < 3; ++k) rgb[k] += I[k] * t.a[k];
        break;
    case RDR_DL_POINT: {
        float d[3], l[3];
        for (int k = 0; k < 3; ++k) d[k] = lp[kPosition + k] - t.p[k];
        const float r2 = dot3(d, d), r = sqrtf(r2);
        for (int k = 0; k < 3; ++k) l[k] = d[k] / r;
        const float c = fmaxf(dot3(l, t.n), 0.f);
        for (int k = 0; k < 3; ++k) rgb[k] += I[k] * c * (t.a[k] / kPi) / r2;
        break;
    }
    case RDR_DL_DIRECTIONAL: {
        const float *D = lp + kDirection;
        const float nd = sqrtf(dot3(D, D));
        float l[3];
        for (int k = 0; k < 3; ++k) l[k] = -D[k] / nd;
        const float c = fmaxf(dot3(l, t.n), 0.f);
        for (int k = 0; k < 3; ++k) rgb[k] += I[k] * c * (t.a[k] / kPi);
        break;
    }
    default: {               // RDR_DL_SPOT (the table was validated)
        const float *D = lp + kDirection;
        float d[3], l[3], s[3];
        for (int k = 0; k < 3; ++k) d[k] = lp[kPosition + k] - t.p[k];
        const float nr = sqrtf(dot3(d, d)), ns = sqrtf(dot3(D, D));
        for (int k = 0; k < 3; ++k) { l[k] = d[k] / nr; s[k] = -D[k] / ns; }
        const float f = powf(fmaxf(dot3(l, s), 0.f), lp[kExponent]);
        const float c = fmaxf(dot3(l, t.n), 0.f);
        for (int k = 0; k < 3; ++k) rgb[k] += I[k] * f * c * (t.a[k] / kPi);
        break;
    }
    }
}

// ---- shadows: the ray a texel casts towards a light, and the texel's visibility word ------------------------------------------
// THE RULE (fp32; the operands are the ones light_shade forms, the offsets the path tracer's: lights.h shadow_ray_to, camera.h
// make_ray).  Origin p, tmin = 1e-3f and
//   point, spot   d = pos - p, r = sqrtf(d.d):   dir = d / r,       tmax = (1 - 1e-3f) * r
//   directional                                  dir = -D / |D|,    tmax = +inf
//   ambient, SH   no ray.
// A ray is cast only if dir.n > 0, for a spot also dir.s > 0, r > 0, and every float of the record is finite (tmax of a
// directional light: +inf by the rule above, nothing else).  Background texels (normal 0) therefore never cast, and a non-finite
// ray never reaches the traversal kernels.  A texel is lit by the light iff the any-hit query finds no triangle in (tmin, tmax);
// a texel that casts no ray counts as lit: light_shade decides (its cosine is <= 0 or NaN there).
constexpr float kShadowOffset = 1e-3f;
RDR_FN bool casts_no_ray(int type) { return type == RDR_DL_AMBIENT || type >= RDR_DL_SH_R; }
RDR_DEV_FN bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }
RDR_DEV_FN bool shadow_ray(int type, const float *lp, const Texel &t, rt::RayRec &rec) {
    if (casts_no_ray(type)) return false;
    float dir[3], tmax;
    if (type == RDR_DL_DIRECTIONAL) {
        const float *D = lp + kDirection;
        const float nd = sqrtf(dot3(D, D));
        for (int k = 0; k < 3; ++k) dir[k] = -D[k] / nd;
        tmax = INFINITY;
    } else {
        float d[3];
        for (int k = 0; k < 3; ++k) d[k] = lp[kPosition + k] - t.p[k];
        const float r = sqrtf(dot3(d, d));
        if (!(r > 0.f)) return false;
        for (int k = 0; k < 3; ++k) dir[k] = d[k] / r;
        tmax = (1.f - kShadowOffset) * r;
        if (!finite_f(tmax)) return false;
        if (type == RDR_DL_SPOT) {
            const float *D = lp + kDirection;
            const float ns = sqrtf(dot3(D, D));
            float s[3];
            for (int k = 0; k < 3; ++k) s[k] = -D[k] / ns;
            if (!(dot3(dir, s) > 0.f)) return false;
        }
    }
    if (!(dot3(dir, t.n) > 0.f)) return false;
    for (int k = 0; k < 3; ++k)
        if (!finite_f(t.p[k]) || !finite_f(dir[k])) return false;
    rec.ox = t.p[0]; rec.oy = t.p[1]; rec.oz = t.p[2]; rec.tmin = kShadowOffset;
    rec.dx = dir[0]; rec.dy = dir[1]; rec.dz = dir[2]; rec.tmax = tmax;
    return true;
}
// Bit b of a texel's word: light lb + b reaches the texel.  An image that is not shadowed may have more than 32 lights: those
// beyond the word are lit.
RDR_DEV_FN bool light_reaches(uint32_t word, int b) { return b >= 32 || ((word >> b) & 1u) != 0; }
RDR_FN uint32_t full_mask(int len) { return len >= 32 ? 0xffffffffu : ((1u << len) - 1u); }

// ---- ambient occlusion: the K hemisphere rays of a texel, its occlusion word and the factor on the sky rows --------------------
// THE RULE (fp32 unless said otherwise).  The SKY rows of the light table are the ambient row and the SH rows: the rows that cast
// no shadow ray.  With occlusion, a texel casts K any-hit rays (1 <= K <= 32) over the occluder scene; bit r of its word is set
// iff ray r found no triangle in (tmin, tmax) or the texel did not cast; bits at and above K are 0.  o = popcount(word) / K
// multiplies what the sky rows add to the texel; the other rows are untouched (shadows are their business).
//   which texels cast   nn = n.n (n[0] n[0] + n[1] n[1] + n[2] n[2], left to right) with 0 < nn < inf, every float of p finite,
//                       every float of nh = n / sqrtf(nn) finite and every float of the ray finite.  Background texels (normal 0),
//                       a normal whose nn underflows to 0 or overflows, a NaN anywhere: no ray, all K bits set, o = 1.
//   local directions    a table l[16][K][3] the HOST computes in fp64 and rounds once to fp32 (ao_directions below; no
//                       trigonometry runs in a kernel): for ray r of rotation j,  u1 = (r + 0.5) / K,  u2 = the base-2 radical
//                       inverse of r,  phi = 2 pi (u2 + (j + 0.5) / 16),  l = (sqrt(u1) cos phi, sqrt(u1) sin phi, sqrt(1 - u1)):
//                       cosine-distributed, l.z >= sqrt(0.5 / K) >= 0.125, so no ray is tangent.  The rotation of a texel is
//                       j = (x & 3) + 4 (y & 3), x and y its column and row in ITS image of the G-buffer (not in the chunk).
//                       The HALF step in phi keeps phi off 0, where sin phi is exactly 0: about an axis-aligned normal (a wall, a
//                       floor) such a ray has a direction component of exactly 0, and the conservative slab test (raytri.h:
//                       ray_box_once) accepts every box whose slab the origin lies outside of -- the ray walks most of the
//                       hierarchy.  With phi = 0 in the table (ray 0 of rotation 0), the any-hit launch of a 256^2 call on bunny_box
//                       (1 M rays, K = 4) took 26 ms; with the half step it takes 0.16 ms (profiles/deferred_ao.txt).
//   frame               the branch-free basis of Duff et al. about nh:  s = copysignf(1, nh.z),  a = -1 / (s + nh.z),
//                       b = (nh.x nh.y) a,  T = (1 + ((s nh.x) nh.x) a,  s b,  -(s nh.x)),  B = (b,  s + (nh.y nh.y) a,  -nh.y);
//                       defined at nh = (0, 0, -1).
//   ray                 dir[k] = (l.x T[k] + l.y B[k]) + l.z nh[k];  origin p,  tmin = 1e-3f (the shadow rays' offset),
//                       tmax = ao_radius (+inf allowed).
//   forward             a sky row's contribution is formed by light_shade into a zeroed c[3], then rgb[k] += o * c[k];
//                       o = (float)popcount(word) / (float)K.  Every other row accumulates as without occlusion, in the same order.
//   adjoint             light_adjoint of a sky row takes o * w[k] in place of the upstream gradient w[k], in both passes (the
//                       texel's gradient and the row's own); alpha is untouched.  o is a CONSTANT: nothing is differentiated
//                       through it, and the backward call reads the saved words and traces nothing.
// With o == 1 both forms give the bits of the call without occlusion (1 * c == c; 0 + c == c, -0 included: the sums start at +0).
constexpr int kAoRotations = 16, kAoMaxRays = 32;
// ray r (local direction l) of texel t: false where the texel does not cast
RDR_DEV_FN bool ao_ray(const Texel &t, const float *l, float tmax, rt::RayRec &rec) {
    const float nn = dot3(t.n, t.n);
    if (!(nn > 0.f) || !finite_f(nn)) return false;
    const float len = sqrtf(nn);
    float nh[3];
    for (int k = 0; k < 3; ++k) nh[k] = t.n[k] / len;
    const float s = copysignf(1.f, nh[2]);
    const float a = -1.f / (s + nh[2]);
    const float b = (nh[0] * nh[1]) * a;
    const float sx = s * nh[0];
    const float T[3] = {1.f + (sx * nh[0]) * a, s * b, -sx};
    const float B[3] = {b, s + (nh[1] * nh[1]) * a, -nh[1]};
    float dir[3];
    for (int k = 0; k < 3; ++k) dir[k] = (l[0] * T[k] + l[1] * B[k]) + l[2] * nh[k];
    for (int k = 0; k < 3; ++k)
        if (!finite_f(t.p[k]) || !finite_f(nh[k]) || !finite_f(dir[k])) return false;
    rec.ox = t.p[0]; rec.oy = t.p[1]; rec.oz = t.p[2]; rec.tmin = kShadowOffset;
    rec.dx = dir[0]; rec.dy = dir[1]; rec.dz = dir[2]; rec.tmax = tmax;
    return true;
}
// (Whether a texel casts does not depend on l: |l| = 1, and with a finite nh the frame is finite -- |s + nh.z| >= 1 -- so
// |dir[k]| <= 3.  The cast list is therefore made once for all K rays, with the table's first direction.)
RDR_DEV_FN float ao_factor(uint32_t word, int rays) { return (float)__builtin_popcount(word) / (float)rays; }
RDR_FN bool sky_row(int type) { return casts_no_ray(type); }

// Adjoint of light_shade for the texel's upstream gradient w[3]: adds the texel's gradient to dt and, when PARAMS, the ten
// parameter gradients to part.  (The two passes of the adjoint kernel each use one half; the other is dead code there.)
template <bool PARAMS>
RDR_DEV_FN void light_adjoint(int type, const float *lp, const Texel &t, const float *w, Texel &dt, double *part) {
    const float *I = lp + kIntensity;
    if (type == RDR_DL_AMBIENT) {
        for (int k = 0; k < 3; ++k) {
            dt.a[k] += w[k] * I[k];
            if (PARAMS) part[kIntensity + k] += (double)(w[k] * t.a[k]);
        }
        return;
    }
    if (type >= RDR_DL_SH_R) {
        if (type == RDR_DL_SH_R) sh_adjoint_row<PARAMS>(lp, t.n, t.a[0], w[0], dt.a[0], dt.n, part);
        else if (type == RDR_DL_SH_G) sh_adjoint_row<PARAMS>(lp, t.n, t.a[1], w[1], dt.a[1], dt.n, part);
        else sh_adjoint_row<PARAMS>(lp, t.n, t.a[2], w[2], dt.a[2], dt.n, part);
        return;
    }
    float S = 0.f;           // sum_k w_k I_k a_k / pi: what multiplies the geometric factor
    float wa[3];
    for (int k = 0; k < 3; ++k) { wa[k] = w[k] * (t.a[k] / kPi); S += wa[k] * I[k]; }
    if (type == RDR_DL_DIRECTIONAL) {
        const float *D = lp + kDirection;
        const float nd = sqrtf(dot3(D, D));
        float l[3];
        for (int k = 0; k < 3; ++k) l[k] = -D[k] / nd;
        const float c0 = dot3(l, t.n), c = fmaxf(c0, 0.f);
        const float dc0 = S * step_half(c0);
        for (int k = 0; k < 3; ++k) {
            dt.a[k] += w[k] * I[k] * c / kPi;
            dt.n[k] += dc0 * l[k];
        }
        if (PARAMS) {
            float dl[3];
            for (int k = 0; k < 3; ++k) dl[k] = dc0 * t.n[k];
            const float dll = dot3(dl, l);
            for (int k = 0; k < 3; ++k) {
                part[kIntensity + k] += (double)(wa[k] * c);
                part[kDirection + k] += (double)(-(dl[k] - dll * l[k]) / nd);
            }
        }
        return;
    }
    float d[3], l[3], dl[3];
    for (int k = 0; k < 3; ++k) d[k] = lp[kPosition + k] - t.p[k];
    const float r2 = dot3(d, d), r = sqrtf(r2);
    for (int k = 0; k < 3; ++k) l[k] = d[k] / r;
    const float c0 = dot3(l, t.n), c = fmaxf(c0, 0.f);
    if (type == RDR_DL_POINT) {
        const float dc0 = S / r2 * step_half(c0);
        const float dr2 = -S * c / (r2 * r2);
        for (int k = 0; k < 3; ++k) {
            dt.a[k] += w[k] * I[k] * c / kPi / r2;
            dt.n[k] += dc0 * l[k];
            dl[k] = dc0 * t.n[k];
        }
        const float dll = dot3(dl, l);
        for (int k = 0; k < 3; ++k) {
            const float dd = (dl[k] - dll * l[k]) / r + 2.f * d[k] * dr2;
            dt.p[k] -= dd;
            if (PARAMS) {
                part[kIntensity + k] += (double)(wa[k] * c / r2);
                part[kPosition + k] += (double)dd;
            }
        }
        return;
    }
    // RDR_DL_SPOT
    const float *D = lp + kDirection;
    const float e = lp[kExponent];
    const float ns = sqrtf(dot3(D, D));
    float s[3];
    for (int k = 0; k < 3; ++k) s[k] = -D[k] / ns;
    const float sc0 = dot3(l, s), sc = fmaxf(sc0, 0.f);
    const float f = powf(sc, e);
    const float df = S * c, dc0 = S * f * step_half(c0);
    // e * sc^(e-1): 1 at sc == 0 for e == 1 (0^0), 0 for e > 1; for e < 1 (inf) the gradient is defined as 0
    const float dsc = (sc == 0.f && e < 1.f) ? 0.f : df * e * powf(sc, e - 1.f);
    const float dsc0 = dsc * step_half(sc0);
    for (int k = 0; k < 3; ++k) {
        dt.a[k] += w[k] * I[k] * f * c / kPi;
        dt.n[k] += dc0 * l[k];
        dl[k] = dsc0 * s[k] + dc0 * t.n[k];
    }
    const float dll = dot3(dl, l);
    float ds[3];
    for (int k = 0; k < 3; ++k) {
        const float dd = (dl[k] - dll * l[k]) / r;
        dt.p[k] -= dd;
        ds[k] = dsc0 * l[k];
        if (PARAMS) {
            part[kIntensity + k] += (double)(wa[k] * f * c);
            part[kPosition + k] += (double)dd;
        }
    }
    if (PARAMS) {
        const float dss = dot3(ds, s);
        for (int k = 0; k < 3; ++k) part[kDirection + k] += (double)(-(ds[k] - dss * s[k]) / ns);
        if (sc > 0.f) part[kExponent] += (double)(df * f * logf(sc));
    }
}

template <int C>
RDR_DEV_FN const float *texel_row(const View &v, int n, int y, int x, int ty) {
    const size_t hg = (size_t)v.height * v.aa, wg = (size_t)v.width * v.aa;
    return v.g + (((size_t)n * hg + (size_t)y * v.aa + ty) * wg + (size_t)x * v.aa) * C;
}
// ... and the visibility words of the same texels (one word per texel, whatever C is)
RDR_DEV_FN const uint32_t *visibility_row(const View &v, const uint32_t *vis, int n, int y, int x, int ty) {
    const size_t hg = (size_t)v.height * v.aa, wg = (size_t)v.width * v.aa;
    return vis + ((size_t)n * hg + (size_t)y * v.aa + ty) * wg + (size_t)x * v.aa;
}

// One OUTPUT pixel of image n: shade its aa x aa texels by the lights [lb, le), average, write 3 | 4 floats.
// SHADOWED (here and in the two adjoint bodies): a light whose bit in the texel's word of `vis` is 0 is skipped; the plain
// instantiation never looks at `vis` and is the code it was before there were shadows.
// OCCLUDED (likewise): the sky rows are scaled by the factor of the texel's word of `ao` (K = ao_rays), by the rule above; the
// instantiations without it never look at `ao`.
struct Occlusion { const uint32_t *words; int rays; };
template <int C, bool SHADOWED = false, bool OCCLUDED = false>
RDR_DEV_FN void shade_pixel(const View &v, int n, int pix, int lb, int le, float *image, const uint32_t *vis = nullptr,
                            Occlusion ao = Occlusion{nullptr, 0}) {
    const int y = pix / v.width, x = pix - y * v.width;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        const uint32_t *arow = OCCLUDED ? visibility_row(v, ao.words, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            float rgb[3] = {0.f, 0.f, 0.f};
            const uint32_t word = SHADOWED ? vrow[tx] : 0u;
            const float o = OCCLUDED ? ao_factor(arow[tx], ao.rays) : 1.f;
            for (int l = lb; l < le; ++l) {
                if (SHADOWED && !light_reaches(word, l - lb)) continue;
                const int type = v.type[l];
                if (OCCLUDED && sky_row(type)) {
                    float c[3] = {0.f, 0.f, 0.f};
                    light_shade(type, v.params + (size_t)l * kLightParams, t, c);
                    for (int k = 0; k < 3; ++k) rgb[k] += o * c[k];
                    continue;
                }
                light_shade(type, v.params + (size_t)l * kLightParams, t, rgb);
            }
            for (int k = 0; k < 3; ++k) acc[k] += rgb[k];
            acc[3] += alpha;
        }
    }
    const float count = (float)(v.aa * v.aa);
    constexpr int CO = C - 6;
    float *out = image + ((size_t)n * v.height * v.width + pix) * CO;
    if (CO == 4) {
        *reinterpret_cast<F4 *>(out) = F4{acc[0] / count, acc[1] / count, acc[2] / count, acc[3] / count};
    } else {
        for (int k = 0; k < 3; ++k) out[k] = acc[k] / count;
    }
}

template <int C>
RDR_DEV_FN void load_upstream(const View &v, int n, int pix, const float *d_image, float *w) {
    constexpr int CO = C - 6;
    const float *gi = d_image + ((size_t)n * v.height * v.width + pix) * CO;
    const float count = (float)(v.aa * v.aa);
    if (CO == 4) {
        const F4 q = *reinterpret_cast<const F4 *>(gi);
        w[0] = q.x / count; w[1] = q.y / count; w[2] = q.z / count; w[3] = q.w / count;
    } else {
        for (int k = 0; k < 3; ++k) w[k] = gi[k] / count;
        w[3] = 0.f;
    }
}

// Adjoint, pass 1: the gradient of every texel of one output pixel (each texel belongs to exactly one pixel: plain stores).
template <int C, bool SHADOWED = false, bool OCCLUDED = false>
RDR_DEV_FN void adjoint_pixel_texels(const View &v, int n, int pix, int lb, int le, const float *d_image, float *d_g,
                                     const uint32_t *vis = nullptr, Occlusion ao = Occlusion{nullptr, 0}) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[4];
    load_upstream<C>(v, n, pix, d_image, w);
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        float *drow = d_g + (row - v.g);
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        const uint32_t *arow = OCCLUDED ? visibility_row(v, ao.words, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            const uint32_t word = SHADOWED ? vrow[tx] : 0u;
            float wo[3] = {0.f, 0.f, 0.f};       // o * w, the upstream gradient of the sky rows
            if (OCCLUDED) {
                const float o = ao_factor(arow[tx], ao.rays);
                for (int k = 0; k < 3; ++k) wo[k] = o * w[k];
            }
            for (int l = lb; l < le; ++l) {
                if (SHADOWED && !light_reaches(word, l - lb)) continue;
                const int type = v.type[l];
                if (OCCLUDED) {                  // (values, not a pointer, are selected: the arrays stay in registers)
                    const bool sky = sky_row(type);
                    const float wl[3] = {sky ? wo[0] : w[0], sky ? wo[1] : w[1], sky ? wo[2] : w[2]};
                    light_adjoint<false>(type, v.params + (size_t)l * kLightParams, t, wl, dt, nullptr);
                    continue;
                }
                light_adjoint<false>(type, v.params + (size_t)l * kLightParams, t, w, dt, nullptr);
            }
            float *o = drow + tx * C;
            if (C == 10) {
                F2 *q = reinterpret_cast<F2 *>(o);
                q[0] = F2{dt.p[0], dt.p[1]}; q[1] = F2{dt.p[2], dt.n[0]}; q[2] = F2{dt.n[1], dt.n[2]};
                q[3] = F2{dt.a[0], dt.a[1]}; q[4] = F2{dt.a[2], w[3]};
            } else {
                for (int k = 0; k < 3; ++k) { o[k] = dt.p[k]; o[3 + k] = dt.n[k]; o[6 + k] = dt.a[k]; }
            }
        }
    }
}

// Adjoint, pass 2: what one output pixel adds to the ten parameter gradients of light l.
template <int C, bool SHADOWED = false, bool OCCLUDED = false>
RDR_DEV_FN void adjoint_pixel_light(const View &v, int n, int pix, int l, const float *d_image, double *part,
                                    const uint32_t *vis = nullptr, int lb = 0, Occlusion ao = Occlusion{nullptr, 0}) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[4];
    load_upstream<C>(v, n, pix, d_image, w);
    const int type = v.type[l];
    const float *lp = v.params + (size_t)l * kLightParams;
    const bool scaled = OCCLUDED && sky_row(type);       // (uniform: one light per trip of the kernel's outer loop)
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        const uint32_t *vrow = SHADOWED ? visibility_row(v, vis, n, y, x, ty) : nullptr;
        const uint32_t *arow = OCCLUDED ? visibility_row(v, ao.words, n, y, x, ty) : nullptr;
        for (int tx = 0; tx < v.aa; ++tx) {
            if (SHADOWED && !light_reaches(vrow[tx], l - lb)) continue;
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            if (OCCLUDED) {                      // (one call site: 1 * w is w exactly for the rows that are not scaled)
                const float o = scaled ? ao_factor(arow[tx], ao.rays) : 1.f;
                const float wo[3] = {o * w[0], o * w[1], o * w[2]};
                light_adjoint<true>(type, lp, t, wo, dt, part);
                continue;
            }
            light_adjoint<true>(type, lp, t, w, dt, part);
        }
    }
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// grid = (blocks per image, N): the light range of a block is uniform, so the table is read through scalar loads.
template <int C, bool SHADOWED, bool OCCLUDED>
__global__ void __launch_bounds__(256) deferred_shade_kernel(const float *__restrict__ g, const float *__restrict__ params,
                                                             const int *__restrict__ type, const int *__restrict__ range, int height,
                                                             int width, int aa, float *__restrict__ image,
                                                             const uint32_t *__restrict__ vis, const uint32_t *__restrict__ ao,
                                                             int ao_rays) {
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += gridDim.x * 256)
        shade_pixel<C, SHADOWED, OCCLUDED>(v, n, pix, lb, le, image, vis, Occlusion{ao, ao_rays});
}

// The grid is capped (kAdjointBlocks) and strides over the pixels.  Pass 1 writes the texel gradients.  Pass 2 loops over the
// lights on the OUTSIDE: ten fp64 partials per lane are live at a time whatever L is (the block's part of the G-buffer is read
// again per light; a variant that kept it in the L1 / L2 was no faster, profiles/deferred_shade.txt); they are summed across
// the wave (DPP), across the four waves through LDS, and the block writes
// ONE row of the slab [blocks][slab_stride]: no atomics, and a fixed summation order (deferred_fold_kernel).
constexpr int kAdjointBlocks = 2048;
template <int C, bool SHADOWED, bool OCCLUDED>
__global__ void __launch_bounds__(256, 4) deferred_adjoint_kernel(const float *__restrict__ g, const float *__restrict__ params,
                                                               const int *__restrict__ type, const int *__restrict__ range, int height,
                                                               int width, int aa, const float *__restrict__ d_image,
                                                               float *__restrict__ d_g, double *__restrict__ slab, int slab_stride,
                                                               const uint32_t *__restrict__ vis, const uint32_t *__restrict__ ao,
                                                               int ao_rays) {
    // (the tables as `restrict` arguments: the stores of pass 1 cannot alias them, so their loads stay scalar)
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int pix = first; pix < pixels; pix += step)
        adjoint_pixel_texels<C, SHADOWED, OCCLUDED>(v, n, pix, lb, le, d_image, d_g, vis, Occlusion{ao, ao_rays});
    __shared__ double wave_part[4][kLightParams];
    double *row = slab + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * slab_stride;
    for (int l = lb; l < le; ++l) {
        double part[kLightParams];
        for (int k = 0; k < kLightParams; ++k) part[k] = 0.0;
        for (int pix = first; pix < pixels; pix += step)
            adjoint_pixel_light<C, SHADOWED, OCCLUDED>(v, n, pix, l, d_image, part, vis, lb, Occlusion{ao, ao_rays});
        for (int k = 0; k < kLightParams; ++k) part[k] = wave_sum(part[k]);         // every lane is active here
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < kLightParams; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
        __syncthreads();
        if (threadIdx.x < kLightParams) {
            const int k = threadIdx.x;
            row[(l - lb) * kLightParams + k] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
        }
        __syncthreads();
    }
}

// One block per light: the rows of the images that use it, in image order and block order; lane t takes rows t, t + 256, ...
// of each image, then the lanes are summed as above.  Rounded to fp32 once.
__global__ void __launch_bounds__(256) deferred_fold_kernel(const double *__restrict__ slab, int slab_stride, int blocks_per_image,
                                                            const int *__restrict__ range, int num_images, float *__restrict__ d_params) {
    const int l = blockIdx.x;
    double part[kLightParams];
    for (int k = 0; k < kLightParams; ++k) part[k] = 0.0;
    for (int n = 0; n < num_images; ++n) {
        const int lb = range[2 * n], le = range[2 * n + 1];
        if (l < lb || l >= le) continue;
        for (int b = threadIdx.x; b < blocks_per_image; b += 256) {
            const double *row = slab + (size_t)(n * blocks_per_image + b) * slab_stride + (l - lb) * kLightParams;
            for (int k = 0; k < kLightParams; ++k) part[k] += row[k];
        }
    }
    __shared__ double wave_part[4][kLightParams];
    for (int k = 0; k < kLightParams; ++k) part[k] = wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kLightParams; ++k) wave_part[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < kLightParams) {
        const int k = threadIdx.x;
        d_params[l * kLightParams + k] = (float)((wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]));
    }
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------------------
inline void validate(const rdr_deferred_desc &d, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (d.num_images <= 0 || d.height <= 0 || d.width <= 0) fail("num_images, height and width must be positive");
    if (d.num_images > 65535) fail("at most 65535 images per call");
    if (d.aa_samples <= 0) fail("aa_samples must be positive");
    if (d.alpha != 0 && d.alpha != 1) fail("alpha must be 0 or 1");
    if (d.num_lights < 0) fail("num_lights must not be negative");
    if ((long long)d.height * d.aa_samples * (long long)d.width * d.aa_samples > (long long)200000000)
        fail("G-buffer of more than 2e8 texels per image");
    if (d.num_lights > 0 && !d.light_type) fail("light_type is required");
    if (!d.image_light_range) fail("image_light_range is required");
    for (int l = 0; l < d.num_lights; ++l)
        if (d.light_type[l] < RDR_DL_AMBIENT || d.light_type[l] > RDR_DL_SH_B)
            fail("unknown light type " + std::to_string(d.light_type[l]) + " at index " + std::to_string(l));
    for (int n = 0; n < d.num_images; ++n) {
        const int lb = d.image_light_range[2 * n], le = d.image_light_range[2 * n + 1];
        if (lb < 0 || le < lb || le > d.num_lights)
            fail("light range [" + std::to_string(lb) + ", " + std::to_string(le) + ") of image " + std::to_string(n) +
                 " is outside the table of " + std::to_string(d.num_lights) + " lights");
    }
}

// `type` and `range` in memory the launch can read (one block: [L types][2 N range entries]), back in the pool when the call
// ends (arena.h: shade / shade_backward end with upload_flush)
struct Tables {
    Arena arena;
    int *dev = nullptr;
    Tables(const rdr_deferred_desc &d) {
        std::vector<int> h((size_t)d.num_lights + 2 * (size_t)d.num_images);
        for (int l = 0; l < d.num_lights; ++l) h[l] = d.light_type[l];
        for (int i = 0; i < 2 * d.num_images; ++i) h[d.num_lights + i] = d.image_light_range[i];
        dev = arena.put(h.data(), h.size());
    }
};

inline View make_view(const rdr_deferred_desc &d, const Tables &t, const float *g, const float *params) {
    return View{g, params, t.dev, t.dev + d.num_lights, d.height, d.width, d.aa_samples};
}

// ---- shadows: the visibility words of a call (stages on exec::launch: kernels on the GPU, plain loops in the harness) ---------
// One pass per (shadowed image, ray-casting light, chunk of at most kShadowChunk texels), all on the call's stream:
//   compact_dev   the texels of the chunk that cast a ray by the rule -> list; the count stays on the device
//   ShadowRays    one lane per listed texel: the 32-byte record as two 16-byte stores
//   exec::trace   any-hit over the occluder scene's hierarchy, trimmed by the device's count
//   ShadowMark    one lane per listed texel: a hit clears the light's bit.  Within a pass a word has one owner, and passes are
//                 ordered by the stream: a plain read-modify-write.
// The host reads no count back, and the scratch (list 4 + rays 32 + hits 8 bytes per texel of a chunk) does not grow with the
// number of lights.
constexpr int kShadowChunk = 1 << 22;
// RDR_DEFERRED_SHADOW_CHUNK: a smaller chunk (tests: a pass split into several chunks gives the same words)
inline int shadow_chunk() {
    const char *e = std::getenv("RDR_DEFERRED_SHADOW_CHUNK");
    const long v = e ? std::atol(e) : 0;
    return v > 0 && v < kShadowChunk ? (int)v : kShadowChunk;
}

struct FillWords {
    uint32_t *words; uint32_t value;
    RDR_DEV_FN void operator()(int i) const { words[i] = value; }
};
// `texels`: the first texel of the chunk; `lp`: the light's ten parameters (uniform: scalar loads)
template <int C>
struct CastsShadowRay {
    const float *texels; int type; const float *lp;
    RDR_DEV_FN bool operator()(int i) const {
        Texel t;
        float alpha;
        load_texel<C>(texels + (size_t)i * C, t, alpha);
        rt::RayRec rec;
        return shadow_ray(type, lp, t, rec);
    }
};
template <int C>
struct ShadowRays {
    const float *texels; int type; const float *lp; const int *list; rt::RayRec *queue;
    RDR_DEV_FN void operator()(int slot) const {
        Texel t;
        float alpha;
        load_texel<C>(texels + (size_t)list[slot] * C, t, alpha);
        rt::RayRec rec;
        if (!shadow_ray(type, lp, t, rec)) {         // (the list holds only texels that cast; a moot ray all the same)
            rec.ox = rec.oy = rec.oz = rec.tmin = rec.dx = rec.dy = rec.dz = 0.f;
            rec.tmax = -1.f;
        }
        F4 *out = reinterpret_cast<F4 *>(queue + slot);
        out[0] = F4{rec.ox, rec.oy, rec.oz, rec.tmin};
        out[1] = F4{rec.dx, rec.dy, rec.dz, rec.tmax};
    }
};
struct ShadowMark {
    const int *list; const rt::HitRec *hits; uint32_t *words; uint32_t bit;
    RDR_DEV_FN void operator()(int slot) const {
        if (hits[slot].shape >= 0) words[list[slot]] &= ~bit;
    }
};

template <int C>
inline void cast_shadows(const rdr_deferred_desc &d, const View &v, uint32_t *vis, Arena &arena) {
    const size_t texels = (size_t)d.height * d.aa_samples * (size_t)d.width * d.aa_samples;       // validate: at most 2e8
    const int chunk = texels < (size_t)shadow_chunk() ? (int)texels : shadow_chunk();
    int *list = nullptr;
    rt::RayRec *queue = nullptr;
    rt::HitRec *hits = nullptr;
    for (int n = 0; n < d.num_images; ++n) {
        const int lb = d.image_light_range[2 * n], le = d.image_light_range[2 * n + 1];
        uint32_t *words = vis + (size_t)n * texels;
        exec::launch((int)texels, FillWords{words, full_mask(le - lb)});
        if (!d.occluders[n]) continue;
        const Scene &scene = *reinterpret_cast<const Scene *>(d.occluders[n]);
        for (int l = lb; l < le; ++l) {
            const int type = d.light_type[l];
            if (casts_no_ray(type)) continue;
            if (!list) {
                list = arena.get<int>((size_t)chunk);
                queue = arena.get<rt::RayRec>((size_t)chunk);
                hits = arena.get<rt::HitRec>((size_t)chunk);
            }
            const float *lp = v.params + (size_t)l * kLightParams;
            for (size_t base = 0; base < texels; base += (size_t)chunk) {
                const int count = texels - base < (size_t)chunk ? (int)(texels - base) : chunk;
                const float *first = v.g + ((size_t)n * texels + base) * C;
                const exec::Count live = exec::compact_dev(nullptr, exec::Count(count), list, CastsShadowRay<C>{first, type, lp});
                exec::launch(live, ShadowRays<C>{first, type, lp, list, queue});
                exec::trace(scene.bvh, queue, hits, live, true);
                exec::launch(live, ShadowMark{list, hits, words + base, 1u << (l - lb)});
            }
        }
    }
}

// ---- ambient occlusion: the occlusion words of a call ----------------------------------------------------------------------------
// ONE pass per (occluded image, chunk of texels), whatever K is -- all K rays of a chunk's texels go into one queue, so the
// launches of a call do not grow with K (small frames are launch-bound: profiles/deferred_shadows.txt).  A chunk holds
// shadow_chunk() / K texels, so the scratch (list 4 bytes per texel, rays 32 + hits 8 bytes per ray) is bounded by the chunk:
//   compact_dev         the texels of the chunk that cast (ao_ray) -> list, once for all K rays; `live` stays on the device
//   exec::scaled_count  one lane: K * live, the device count of the queue
//   AoRays              one lane per ray; the queue is RAY-MAJOR, slot r * live + i is ray r of listed texel i, so neighbouring
//                       slots hold the same local direction (up to the rotation) of neighbouring texels
//   exec::trace         any-hit, trimmed by the device's count
//   AoMark              one lane per listed texel: reads its K hits and stores the whole word -- no read-modify-write
// The host reads no count back.
template <int C>
struct CastsAoRays {
    const float *texels; const float *dirs;
    RDR_DEV_FN bool operator()(int i) const {
        Texel t;
        float alpha;
        load_texel<C>(texels + (size_t)i * C, t, alpha);
        rt::RayRec rec;
        return ao_ray(t, dirs, 1.f, rec);
    }
};
// `first_texel`: the chunk's first texel, counted within its image (the rotation goes by the texel's place in the image);
// `wg`: texels per row of the image; `dirs`: the table [16][K][3]
template <int C>
struct AoRays {
    const float *texels; const int *list; const int *live; int live_upper; const float *dirs; int rays; float tmax;
    unsigned first_texel, wg; rt::RayRec *queue;
    RDR_DEV_FN void operator()(int slot) const {
        const int c = *live, count = c < live_upper ? c : live_upper;      // (slot < rays * count: count > 0)
        const int r = slot / count, i = slot - r * count;
        const int item = list[i];
        Texel t;
        float alpha;
        load_texel<C>(texels + (size_t)item * C, t, alpha);
        const unsigned at = first_texel + (unsigned)item, y = at / wg, x = at - y * wg;
        const int j = (int)((x & 3u) + 4u * (y & 3u));
        rt::RayRec rec;
        if (!ao_ray(t, dirs + ((size_t)j * rays + r) * 3, tmax, rec)) {    // (the list holds only texels that cast; a moot ray all the same)
            rec.ox = rec.oy = rec.oz = rec.tmin = rec.dx = rec.dy = rec.dz = 0.f;
            rec.tmax = -1.f;
        }
        F4 *out = reinterpret_cast<F4 *>(queue + slot);
        out[0] = F4{rec.ox, rec.oy, rec.oz, rec.tmin};
        out[1] = F4{rec.dx, rec.dy, rec.dz, rec.tmax};
    }
};
struct AoMark {
    const int *list; const int *live; int live_upper; const rt::HitRec *hits; uint32_t *words; int rays;
    RDR_DEV_FN void operator()(int i) const {
        const int c = *live, count = c < live_upper ? c : live_upper;
        uint32_t word = 0u;
        for (int r = 0; r < rays; ++r)
            if (hits[(size_t)r * count + i].shape < 0) word |= 1u << r;
        words[list[i]] = word;
    }
};
// The local directions by the rule above: fp64 on the host, rounded once
inline std::vector<float> ao_directions(int rays) {
    std::vector<float> table((size_t)kAoRotations * rays * 3);
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < kAoRotations; ++j)
        for (int r = 0; r < rays; ++r) {
            double u2 = 0.0, digit = 0.5;
            for (unsigned b = (unsigned)r; b; b >>= 1, digit *= 0.5)
                if (b & 1u) u2 += digit;
            const double u1 = (r + 0.5) / rays, phi = two_pi * (u2 + (j + 0.5) / 16.0);
            float *l = table.data() + ((size_t)j * rays + r) * 3;
            l[0] = (float)(std::sqrt(u1) * std::cos(phi));
            l[1] = (float)(std::sqrt(u1) * std::sin(phi));
            l[2] = (float)std::sqrt(1.0 - u1);
        }
    return table;
}

template <int C>
inline void cast_occlusion(const rdr_deferred_desc &d, const View &v, Arena &arena) {
    const size_t texels = (size_t)d.height * d.aa_samples * (size_t)d.width * d.aa_samples;       // validate: at most 2e8
    const int rays = d.ao_rays;
    const int per_chunk = shadow_chunk() / rays > 0 ? shadow_chunk() / rays : 1;
    const int chunk = texels < (size_t)per_chunk ? (int)texels : per_chunk;
    const unsigned wg = (unsigned)d.width * (unsigned)d.aa_samples;
    int *list = nullptr;
    rt::RayRec *queue = nullptr;
    rt::HitRec *hits = nullptr;
    const float *dirs = nullptr;
    for (int n = 0; n < d.num_images; ++n) {
        uint32_t *words = d.ao_words + (size_t)n * texels;
        exec::launch((int)texels, FillWords{words, full_mask(rays)});
        if (!d.ao_occluders[n]) continue;
        const Scene &scene = *reinterpret_cast<const Scene *>(d.ao_occluders[n]);
        if (!list) {
            const std::vector<float> table = ao_directions(rays);
            dirs = arena.put(table.data(), table.size());
            list = arena.get<int>((size_t)chunk);
            queue = arena.get<rt::RayRec>((size_t)chunk * rays);
            hits = arena.get<rt::HitRec>((size_t)chunk * rays);
        }
        for (size_t base = 0; base < texels; base += (size_t)chunk) {
            const int count = texels - base < (size_t)chunk ? (int)(texels - base) : chunk;
            const float *first = v.g + ((size_t)n * texels + base) * C;
            const exec::Count live = exec::compact_dev(nullptr, exec::Count(count), list, CastsAoRays<C>{first, dirs});
            const exec::Count all = exec::scaled_count(live, rays);
            exec::launch(all, AoRays<C>{first, list, live.dev, live.upper, dirs, rays, d.ao_radius, (unsigned)base, wg, queue});
            exec::trace(scene.bvh, queue, hits, all, true);
            exec::launch(live, AoMark{list, live.dev, live.upper, hits, words + base, rays});
        }
    }
}

template <int C, bool SHADOWED, bool OCCLUDED>
inline void shade_impl(const rdr_deferred_desc &d, const View &v, float *image, const uint32_t *vis, Occlusion ao) {
    const int pixels = d.height * d.width;
#if !defined(RDR_HOSTSIM)
    const dim3 grid((pixels + 255) / 256, d.num_images);
    hipLaunchKernelGGL((deferred_shade_kernel<C, SHADOWED, OCCLUDED>), grid, dim3(256), 0, exec::ctx().stream, v.g, v.params, v.type,
                       v.range, v.height, v.width, v.aa, image, vis, ao.words, ao.rays);
    exec::check(hipGetLastError(), "deferred_shade launch");
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            shade_pixel<C, SHADOWED, OCCLUDED>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], image, vis, ao);
#endif
}

template <int C, bool SHADOWED, bool OCCLUDED>
inline void adjoint_impl(const rdr_deferred_desc &d, const View &v, const float *d_image, float *d_g, float *d_params,
                         const uint32_t *vis, Occlusion ao) {
    const int pixels = d.height * d.width;
#if !defined(RDR_HOSTSIM)
    int per_image = (pixels + 255) / 256;
    const int cap = kAdjointBlocks / d.num_images > 0 ? kAdjointBlocks / d.num_images : 1;
    if (per_image > cap) per_image = cap;
    int longest = 0;
    for (int n = 0; n < d.num_images; ++n) {
        const int len = d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
        if (len > longest) longest = len;
    }
    const int slab_stride = longest * kLightParams;
    Arena arena;
    double *slab = arena.get<double>((size_t)per_image * d.num_images * (slab_stride > 0 ? slab_stride : 1));
    hipLaunchKernelGGL((deferred_adjoint_kernel<C, SHADOWED, OCCLUDED>), dim3(per_image, d.num_images), dim3(256), 0,
                       exec::ctx().stream, v.g, v.params, v.type, v.range, v.height, v.width, v.aa, d_image, d_g, slab, slab_stride, vis,
                       ao.words, ao.rays);
    exec::check(hipGetLastError(), "deferred_shade_adjoint launch");
    if (d.num_lights > 0) {
        hipLaunchKernelGGL(deferred_fold_kernel, dim3(d.num_lights), dim3(256), 0, exec::ctx().stream, slab, slab_stride, per_image,
                           v.range, d.num_images, d_params);
        exec::check(hipGetLastError(), "deferred_fold launch");
    }
    exec::upload_flush();              // the stream is drained before the slab goes back to the pool
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix)
            adjoint_pixel_texels<C, SHADOWED, OCCLUDED>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], d_image, d_g, vis, ao);
    for (int l = 0; l < d.num_lights; ++l) {
        double part[kLightParams] = {0};
        for (int n = 0; n < d.num_images; ++n) {
            if (l < v.range[2 * n] || l >= v.range[2 * n + 1]) continue;
            for (int pix = 0; pix < pixels; ++pix)
                adjoint_pixel_light<C, SHADOWED, OCCLUDED>(v, n, pix, l, d_image, part, vis, v.range[2 * n], ao);
        }
        for (int k = 0; k < kLightParams; ++k) d_params[l * kLightParams + k] = (float)part[k];
    }
#endif
}

// What the two shadow fields of the description ask for, checked before anything is launched.  `forward`: the words are written
// (occluders and visibility come together); backward: the words are read and no scene is looked at.
inline void validate_shadows(const rdr_deferred_desc &d, bool forward, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (forward && d.occluders && !d.visibility) fail("occluders need a visibility buffer");
    if (forward && !d.occluders && d.visibility) fail("a visibility buffer needs occluders");
    if (d.visibility && ((uintptr_t)d.visibility & 3)) fail("the visibility buffer must be 4-byte aligned");
    if (!forward || !d.occluders) return;
    for (int n = 0; n < d.num_images; ++n) {
        if (!d.occluders[n]) continue;
        const int len = d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
        if (len > 32)
            fail("shadowed image " + std::to_string(n) + " has " + std::to_string(len) + " lights, at most 32 fit its visibility word");
#if !defined(RDR_HOSTSIM)
        const int at = reinterpret_cast<const Scene *>(d.occluders[n])->gpu_index;
        if (at != d.gpu_index)
            fail("the occluder scene of image " + std::to_string(n) + " lives on device " + std::to_string(at) +
                 ", the call runs on device " + std::to_string(d.gpu_index));
#endif
    }
}

// ... and the four occlusion fields, likewise.  The limit of 32 lights is the visibility word's: an occluded image may have more.
inline void validate_occlusion(const rdr_deferred_desc &d, bool forward, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (!d.ao_occluders && !d.ao_words) return;
    if (d.ao_rays < 1 || d.ao_rays > kAoMaxRays) fail("ao_rays must be 1 .. 32, got " + std::to_string(d.ao_rays));
    if (forward && d.ao_occluders && !d.ao_words) fail("ao_occluders need an ao_words buffer");
    if (forward && !d.ao_occluders && d.ao_words) fail("an ao_words buffer needs ao_occluders");
    if (d.ao_words && ((uintptr_t)d.ao_words & 3)) fail("the ao_words buffer must be 4-byte aligned");
    if (!forward) return;
    if (!(d.ao_radius > 0.f)) fail("ao_radius must be positive (+inf: unbounded), got " + std::to_string(d.ao_radius));
#if !defined(RDR_HOSTSIM)
    for (int n = 0; n < d.num_images; ++n) {
        if (!d.ao_occluders[n]) continue;
        const int at = reinterpret_cast<const Scene *>(d.ao_occluders[n])->gpu_index;
        if (at != d.gpu_index)
            fail("the ao occluder scene of image " + std::to_string(n) + " lives on device " + std::to_string(at) +
                 ", the call runs on device " + std::to_string(d.gpu_index));
    }
#endif
}

// The instantiation a call asks for: F is called with (C, SHADOWED, OCCLUDED) as integral constants
template <class F>
inline void dispatch(bool alpha, bool shadowed, bool occluded, const F &f) {
    using std::integral_constant;
    auto by_mode = [&](auto c) {
        if (shadowed && occluded) f(c, integral_constant<bool, true>(), integral_constant<bool, true>());
        else if (shadowed) f(c, integral_constant<bool, true>(), integral_constant<bool, false>());
        else if (occluded) f(c, integral_constant<bool, false>(), integral_constant<bool, true>());
        else f(c, integral_constant<bool, false>(), integral_constant<bool, false>());
    };
    if (alpha) by_mode(integral_constant<int, 10>()); else by_mode(integral_constant<int, 9>());
}

// rdr_deferred_shade: synchronised on return
inline void shade(const rdr_deferred_desc &d, const float *g, const float *params, float *image) {
    validate(d, "rdr_deferred_shade");
    if (!g || !image || (d.num_lights > 0 && !params)) throw std::runtime_error("rdr_deferred_shade: null tensor");
    if (d.alpha && (((uintptr_t)g & 7) || ((uintptr_t)image & 15)))
        throw std::runtime_error("rdr_deferred_shade: with alpha the G-buffer must be 8-byte and the image 16-byte aligned");
    validate_shadows(d, true, "rdr_deferred_shade");
    validate_occlusion(d, true, "rdr_deferred_shade");
    Tables tables(d);
    const View v = make_view(d, tables, g, params);
    Arena scratch;                         // (empty without shadows and occlusion) back in the pool after the upload_flush below
    const Occlusion ao{d.ao_words, d.ao_rays};
    dispatch(d.alpha != 0, d.occluders != nullptr, d.ao_occluders != nullptr, [&](auto c, auto shadowed, auto occluded) {
        constexpr int C = decltype(c)::value;
        if (shadowed) cast_shadows<C>(d, v, d.visibility, scratch);
        if (occluded) cast_occlusion<C>(d, v, scratch);
        shade_impl<C, decltype(shadowed)::value, decltype(occluded)::value>(d, v, image, d.visibility, ao);
    });
    exec::upload_flush();
}

// rdr_deferred_shade_backward: synchronised on return.  Visibility is a constant of the adjoint: a light whose bit is 0 adds
// nothing to the texel's gradient nor to its own.
inline void shade_backward(const rdr_deferred_desc &d, const float *g, const float *params, const float *d_image, float *d_g,
                           float *d_params) {
    validate(d, "rdr_deferred_shade_backward");
    if (!g || !d_image || !d_g || (d.num_lights > 0 && (!params || !d_params)))
        throw std::runtime_error("rdr_deferred_shade_backward: null tensor");
    if (d.alpha && ((((uintptr_t)g | (uintptr_t)d_g) & 7) || ((uintptr_t)d_image & 15)))
        throw std::runtime_error("rdr_deferred_shade_backward: with alpha the G-buffers must be 8-byte and the image gradient 16-byte aligned");
    validate_shadows(d, false, "rdr_deferred_shade_backward");
    validate_occlusion(d, false, "rdr_deferred_shade_backward");
    Tables tables(d);
    const View v = make_view(d, tables, g, params);
    const Occlusion ao{d.ao_words, d.ao_rays};      // the saved words: occlusion, like visibility, is a constant of the adjoint
    dispatch(d.alpha != 0, d.visibility != nullptr, d.ao_words != nullptr, [&](auto c, auto shadowed, auto occluded) {
        adjoint_impl<decltype(c)::value, decltype(shadowed)::value, decltype(occluded)::value>(d, v, d_image, d_g, d_params,
                                                                                                 d.visibility, ao);
    });
    exec::upload_flush();
}

} // namespace dfr
} // namespace rdr
