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
// The per-texel bodies below are shared by the kernels (one lane per OUTPUT pixel, at the end of this header) and by the plain
// loops of the CPU debugging harness.  Arithmetic is fp32 in the order the reference's torch expressions evaluate; the only
// fp64 is the light-parameter partial sums of the adjoint.
#pragma once
#include "../../include/redner_amd.h"
#include "arena.h"
#include <cmath>
#include <stdexcept>
#include <string>
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

// rgb += what light (type, lp) adds to texel t
RDR_DEV_FN void light_shade(int type, const float *lp, const Texel &t, float *rgb) {
    const float *I = lp + kIntensity;
    switch (type) {
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

// One OUTPUT pixel of image n: shade its aa x aa texels by the lights [lb, le), average, write 3 | 4 floats.
template <int C>
RDR_DEV_FN void shade_pixel(const View &v, int n, int pix, int lb, int le, float *image) {
    const int y = pix / v.width, x = pix - y * v.width;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            float rgb[3] = {0.f, 0.f, 0.f};
            for (int l = lb; l < le; ++l) light_shade(v.type[l], v.params + (size_t)l * kLightParams, t, rgb);
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
template <int C>
RDR_DEV_FN void adjoint_pixel_texels(const View &v, int n, int pix, int lb, int le, const float *d_image, float *d_g) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[4];
    load_upstream<C>(v, n, pix, d_image, w);
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        float *drow = d_g + (row - v.g);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            for (int l = lb; l < le; ++l)
                light_adjoint<false>(v.type[l], v.params + (size_t)l * kLightParams, t, w, dt, nullptr);
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
template <int C>
RDR_DEV_FN void adjoint_pixel_light(const View &v, int n, int pix, int l, const float *d_image, double *part) {
    const int y = pix / v.width, x = pix - y * v.width;
    float w[4];
    load_upstream<C>(v, n, pix, d_image, w);
    const int type = v.type[l];
    const float *lp = v.params + (size_t)l * kLightParams;
    for (int ty = 0; ty < v.aa; ++ty) {
        const float *row = texel_row<C>(v, n, y, x, ty);
        for (int tx = 0; tx < v.aa; ++tx) {
            Texel t, dt;
            float alpha;
            load_texel<C>(row + tx * C, t, alpha);
            for (int k = 0; k < 3; ++k) dt.p[k] = dt.n[k] = dt.a[k] = 0.f;
            light_adjoint<true>(type, lp, t, w, dt, part);
        }
    }
}

#if !defined(RDR_HOSTSIM)
// ---- gfx950 kernels --------------------------------------------------------------------------------------------------------
// grid = (blocks per image, N): the light range of a block is uniform, so the table is read through scalar loads.
template <int C>
__global__ void __launch_bounds__(256) deferred_shade_kernel(const float *__restrict__ g, const float *__restrict__ params,
                                                             const int *__restrict__ type, const int *__restrict__ range, int height,
                                                             int width, int aa, float *__restrict__ image) {
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += gridDim.x * 256) shade_pixel<C>(v, n, pix, lb, le, image);
}

// The grid is capped (kAdjointBlocks) and strides over the pixels.  Pass 1 writes the texel gradients.  Pass 2 loops over the
// lights on the OUTSIDE: ten fp64 partials per lane are live at a time whatever L is (the block's part of the G-buffer is read
// again per light; a variant that kept it in the L1 / L2 was no faster, profiles/deferred_shade.txt); they are summed across
// the wave (DPP), across the four waves through LDS, and the block writes
// ONE row of the slab [blocks][slab_stride]: no atomics, and a fixed summation order (deferred_fold_kernel).
constexpr int kAdjointBlocks = 2048;
template <int C>
__global__ void __launch_bounds__(256, 4) deferred_adjoint_kernel(const float *__restrict__ g, const float *__restrict__ params,
                                                               const int *__restrict__ type, const int *__restrict__ range, int height,
                                                               int width, int aa, const float *__restrict__ d_image,
                                                               float *__restrict__ d_g, double *__restrict__ slab, int slab_stride) {
    // (the tables as `restrict` arguments: the stores of pass 1 cannot alias them, so their loads stay scalar)
    const View v{g, params, type, range, height, width, aa};
    const int n = blockIdx.y, pixels = v.height * v.width;
    const int lb = v.range[2 * n], le = v.range[2 * n + 1];
    const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int pix = first; pix < pixels; pix += step) adjoint_pixel_texels<C>(v, n, pix, lb, le, d_image, d_g);
    __shared__ double wave_part[4][kLightParams];
    double *row = slab + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * slab_stride;
    for (int l = lb; l < le; ++l) {
        double part[kLightParams];
        for (int k = 0; k < kLightParams; ++k) part[k] = 0.0;
        for (int pix = first; pix < pixels; pix += step) adjoint_pixel_light<C>(v, n, pix, l, d_image, part);
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
        if (d.light_type[l] < RDR_DL_AMBIENT || d.light_type[l] > RDR_DL_SPOT)
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

template <int C>
inline void shade_impl(const rdr_deferred_desc &d, const View &v, float *image) {
    const int pixels = d.height * d.width;
#if !defined(RDR_HOSTSIM)
    const dim3 grid((pixels + 255) / 256, d.num_images);
    hipLaunchKernelGGL(deferred_shade_kernel<C>, grid, dim3(256), 0, exec::ctx().stream, v.g, v.params, v.type, v.range,
                       v.height, v.width, v.aa, image);
    exec::check(hipGetLastError(), "deferred_shade launch");
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix) shade_pixel<C>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], image);
#endif
}

template <int C>
inline void adjoint_impl(const rdr_deferred_desc &d, const View &v, const float *d_image, float *d_g, float *d_params) {
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
    hipLaunchKernelGGL(deferred_adjoint_kernel<C>, dim3(per_image, d.num_images), dim3(256), 0, exec::ctx().stream, v.g, v.params,
                       v.type, v.range, v.height, v.width, v.aa, d_image, d_g, slab, slab_stride);
    exec::check(hipGetLastError(), "deferred_shade_adjoint launch");
    if (d.num_lights > 0) {
        hipLaunchKernelGGL(deferred_fold_kernel, dim3(d.num_lights), dim3(256), 0, exec::ctx().stream, slab, slab_stride, per_image,
                           v.range, d.num_images, d_params);
        exec::check(hipGetLastError(), "deferred_fold launch");
    }
    exec::upload_flush();              // the stream is drained before the slab goes back to the pool
#else
    for (int n = 0; n < d.num_images; ++n)
        for (int pix = 0; pix < pixels; ++pix) adjoint_pixel_texels<C>(v, n, pix, v.range[2 * n], v.range[2 * n + 1], d_image, d_g);
    for (int l = 0; l < d.num_lights; ++l) {
        double part[kLightParams] = {0};
        for (int n = 0; n < d.num_images; ++n) {
            if (l < v.range[2 * n] || l >= v.range[2 * n + 1]) continue;
            for (int pix = 0; pix < pixels; ++pix) adjoint_pixel_light<C>(v, n, pix, l, d_image, part);
        }
        for (int k = 0; k < kLightParams; ++k) d_params[l * kLightParams + k] = (float)part[k];
    }
#endif
}

// rdr_deferred_shade: synchronised on return
inline void shade(const rdr_deferred_desc &d, const float *g, const float *params, float *image) {
    validate(d, "rdr_deferred_shade");
    if (!g || !image || (d.num_lights > 0 && !params)) throw std::runtime_error("rdr_deferred_shade: null tensor");
    if (d.alpha && (((uintptr_t)g & 7) || ((uintptr_t)image & 15)))
        throw std::runtime_error("rdr_deferred_shade: with alpha the G-buffer must be 8-byte and the image 16-byte aligned");
    Tables tables(d);
    const View v = make_view(d, tables, g, params);
    if (d.alpha) shade_impl<10>(d, v, image); else shade_impl<9>(d, v, image);
    exec::upload_flush();
}

// rdr_deferred_shade_backward: synchronised on return
inline void shade_backward(const rdr_deferred_desc &d, const float *g, const float *params, const float *d_image, float *d_g,
                           float *d_params) {
    validate(d, "rdr_deferred_shade_backward");
    if (!g || !d_image || !d_g || (d.num_lights > 0 && (!params || !d_params)))
        throw std::runtime_error("rdr_deferred_shade_backward: null tensor");
    if (d.alpha && ((((uintptr_t)g | (uintptr_t)d_g) & 7) || ((uintptr_t)d_image & 15)))
        throw std::runtime_error("rdr_deferred_shade_backward: with alpha the G-buffers must be 8-byte and the image gradient 16-byte aligned");
    Tables tables(d);
    const View v = make_view(d, tables, g, params);
    if (d.alpha) adjoint_impl<10>(d, v, d_image, d_g, d_params); else adjoint_impl<9>(d, v, d_image, d_g, d_params);
    exec::upload_flush();
}

} // namespace dfr
} // namespace rdr
