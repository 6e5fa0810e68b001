// deferred_quad_shadow.h -- soft shadows for the quad lights of deferred_quad.h (rdr_deferred_quad_shadowed / _backward).
//
// The exact irradiance F of a quad is multiplied by V = sum_k w_k vis_k / sum_k w_k, K <= 32 fixed stratified points of the quad
// tested by any-hit rays and weighted by the unshadowed integrand: the ratio estimator of Heitz et al. 2018.  THE RULE -- the
// sample table, the point and its area element, the weight, which samples count, the ray, the word and the factor, in the order
// of the fp32 operations -- is stated once, in deferred_quad_shadow_abi.h; quad_sample below is that rule and the only place it
// is written down in code: the predicate of the compaction, the ray generator and the mark all call it.
//
// The pass (stages on exec::launch: kernels on the GPU, plain loops in the CPU debugging harness), after ONE launch that fills
// every word of the call with full_mask(K) and every factor with 1: one pass per (image with an occluder, quad, chunk), a chunk
// holding shadow_chunk() / K texels (RDR_DEFERRED_SHADOW_CHUNK is honoured), all on the call's stream:
//   compact_dev         the texels of the chunk with at least one counting sample -> list; `live` stays on the device
//   exec::scaled_count  one lane: K * live, the device count of the queue
//   QuadRays            one lane per ray; the queue is RAY-MAJOR, slot k * live + i is ray k of listed texel i, so neighbouring
//                       slots hold the same stratum of neighbouring texels.  A sample that does not count writes a moot ray
//                       (tmax = -1).  Two 16-byte stores per record.
//   exec::trace         any-hit over the occluder scene's hierarchy, trimmed by the device's count
//   QuadMark            one lane per listed texel: reads its K hits, recomputes the K weights and stores the whole word and the
//                       factor -- nothing is read, modified and written back.
// The host reads no count back, and the scratch (list 4 bytes per texel, rays 32 + hits 8 bytes per ray of a chunk) does not grow
// with the number of quads.
#pragma once
#include "deferred_quad.h"

namespace rdr {
namespace dfq {

constexpr int kQuadRotations = 16, kQuadMaxRays = 32;

// Sample (u, v) = uv[0], uv[1] of `quad` seen from texel t with frame f: whether it counts, and then its weight and its ray.
RDR_DEV_FN bool quad_sample(const float *quad, bool two_sided, const Texel &t, const Frame &f, const float *uv, float &w,
                            rt::RayRec &rec) {
    const float u = uv[0], v = uv[1], uv2 = u * v;
    float ag[3], bg[3], s[3], d[3], J[3];
    for (int k = 0; k < 3; ++k) {
        const float a = quad[3 + k] - quad[k], b = quad[9 + k] - quad[k], g = (quad[6 + k] - quad[3 + k]) - b;
        s[k] = ((quad[k] + u * a) + v * b) + uv2 * g;
        ag[k] = a + v * g;
        bg[k] = b + u * g;
        d[k] = s[k] - t.p[k];
    }
    cross3(ag, bg, J);
    const float r2 = dot3(d, d), cs = dot3(d, f.nh), dj = dot3(d, J);
    const float ce = two_sided ? fabsf(dj) : -dj;
    if (!(r2 > 0.f) || !(cs > 0.f) || !(ce > 0.f)) return false;
    w = (cs * ce) / (r2 * r2);
    if (!(w > 0.f) || !finite_f(w)) return false;
    const float r = sqrtf(r2), tmax = (1.f - dfr::kShadowOffset) * r;
    float dir[3];
    for (int k = 0; k < 3; ++k) dir[k] = d[k] / r;
    if (!finite_f(tmax)) return false;
    for (int k = 0; k < 3; ++k)
        if (!finite_f(t.p[k]) || !finite_f(dir[k])) return false;
    rec.ox = t.p[0]; rec.oy = t.p[1]; rec.oz = t.p[2]; rec.tmin = dfr::kShadowOffset;
    rec.dx = dir[0]; rec.dy = dir[1]; rec.dz = dir[2]; rec.tmax = tmax;
    return true;
}

// The rotation of texel `at` of its image (`wg` texels per row): the texel's place in the image, not in the chunk
RDR_DEV_FN int quad_rotation(unsigned at, unsigned wg) {
    const unsigned y = at / wg, x = at - y * wg;
    return (int)((x & 3u) + 4u * (y & 3u));
}

// What the stages of a pass share.  `texels`: the chunk's first texel; `first_texel`: its index within its image; `quad`: the
// quad's sixteen floats (uniform: scalar loads); `uv`: the table [16][K][2]
struct QuadPass {
    const float *texels, *quad, *uv;
    int two_sided, rays;
    unsigned first_texel, wg;
};
template <int C>
RDR_DEV_FN bool pass_texel(const QuadPass &q, int item, Texel &t, Frame &f, const float *&uv) {
    float alpha;
    load_texel<C>(q.texels + (size_t)item * C, t, alpha);
    uv = q.uv + (size_t)quad_rotation(q.first_texel + (unsigned)item, q.wg) * q.rays * 2;
    return frame_at(t, f);
}

struct FillPairs {
    uint32_t *words; float *factors; uint32_t mask;
    RDR_DEV_FN void operator()(int i) const { words[i] = mask; factors[i] = 1.f; }
};
template <int C>
struct CastsQuadRays {
    QuadPass q;
    RDR_DEV_FN bool operator()(int i) const {
        Texel t;
        Frame f;
        const float *uv;
        if (!pass_texel<C>(q, i, t, f, uv)) return false;
        for (int k = 0; k < q.rays; ++k) {
            float w;
            rt::RayRec rec;
            if (quad_sample(q.quad, q.two_sided != 0, t, f, uv + 2 * k, w, rec)) return true;
        }
        return false;
    }
};
template <int C>
struct QuadRays {
    QuadPass q; const int *list; const int *live; int live_upper; rt::RayRec *queue;
    RDR_DEV_FN void operator()(int slot) const {
        const int c = *live, count = c < live_upper ? c : live_upper;      // (slot < rays * count: count > 0)
        const int k = slot / count, i = slot - k * count;
        Texel t;
        Frame f;
        const float *uv;
        float w;
        rt::RayRec rec;
        if (!pass_texel<C>(q, list[i], t, f, uv) || !quad_sample(q.quad, q.two_sided != 0, t, f, uv + 2 * k, w, rec)) {
            rec.ox = rec.oy = rec.oz = rec.tmin = rec.dx = rec.dy = rec.dz = 0.f;
            rec.tmax = -1.f;
        }
        F4 *out = reinterpret_cast<F4 *>(queue + slot);
        out[0] = F4{rec.ox, rec.oy, rec.oz, rec.tmin};
        out[1] = F4{rec.dx, rec.dy, rec.dz, rec.tmax};
    }
};
// `words` and `factors`: those of the chunk's first texel in the pass's pair
template <int C>
struct QuadMark {
    QuadPass q; const int *list; const int *live; int live_upper; const rt::HitRec *hits; uint32_t *words; float *factors;
    RDR_DEV_FN void operator()(int i) const {
        const int c = *live, count = c < live_upper ? c : live_upper;
        const int item = list[i];
        Texel t;
        Frame f;
        const float *uv;
        const bool framed = pass_texel<C>(q, item, t, f, uv);
        uint32_t word = 0u;
        float num = 0.f, den = 0.f;
        for (int k = 0; k < q.rays; ++k) {
            float w;
            rt::RayRec rec;
            const bool counts = framed && quad_sample(q.quad, q.two_sided != 0, t, f, uv + 2 * k, w, rec);
            const bool clear = !counts || hits[(size_t)k * count + i].shape < 0;
            if (clear) word |= 1u << k;
            if (counts) {
                den += w;
                if (clear) num += w;
            }
        }
        words[item] = word;
        factors[item] = (den > 0.f && finite_f(den)) ? num / den : 1.f;
    }
};

// The sample table by the rule: fp64 on the host, rounded once
inline std::vector<float> quad_samples(int rays) {
    std::vector<float> table((size_t)kQuadRotations * rays * 2);
    int pow2 = 1;
    while (pow2 < rays) pow2 *= 2;
    for (int j = 0; j < kQuadRotations; ++j)
        for (int k = 0; k < rays; ++k) {
            double inverse = 0.0, digit = 0.5;
            for (unsigned b = (unsigned)k; b; b >>= 1, digit *= 0.5)
                if (b & 1u) inverse += digit;
            float *uv = table.data() + ((size_t)j * rays + k) * 2;
            uv[0] = (float)((k + ((j & 3) + 0.5) / 4.0) / rays);
            uv[1] = (float)(inverse + ((j >> 2) + 0.5) / (4.0 * pow2));
        }
    return table;
}

// The first pair of every image: the sum of the earlier images' range lengths; -> the number of pairs
inline long long pair_bases(const rdr_deferred_desc &d, std::vector<int> *bases) {
    long long pairs = 0;
    for (int n = 0; n < d.num_images; ++n) {
        if (bases) bases->push_back((int)pairs);
        pairs += d.image_light_range[2 * n + 1] - d.image_light_range[2 * n];
    }
    return pairs;
}

template <int C>
inline void cast_quad_shadows(const rdr_deferred_desc &d, const View &v, int rays, float *factors, Arena &arena) {
    const size_t texels = (size_t)d.height * d.aa_samples * (size_t)d.width * d.aa_samples;
    const long long pairs = pair_bases(d, nullptr);                                   // validate: pairs * texels fits an int
    uint32_t *words = reinterpret_cast<uint32_t *>(d.visibility);
    const long long total = pairs * (long long)texels, slice = 1ll << 30;                // (a launch rounds its lanes up to a block)
    for (long long at = 0; at < total; at += slice)
        exec::launch((int)(total - at < slice ? total - at : slice), FillPairs{words + at, factors + at, dfr::full_mask(rays)});
    const int per_chunk = dfr::shadow_chunk() / rays > 0 ? dfr::shadow_chunk() / rays : 1;
    const int chunk = texels < (size_t)per_chunk ? (int)texels : per_chunk;
    const unsigned wg = (unsigned)d.width * (unsigned)d.aa_samples;
    int *list = nullptr;
    rt::RayRec *queue = nullptr;
    rt::HitRec *hits = nullptr;
    const float *uv = nullptr;
    size_t pair = 0;
    for (int n = 0; n < d.num_images; ++n) {
        const int lb = d.image_light_range[2 * n], le = d.image_light_range[2 * n + 1];
        if (!d.occluders[n]) { pair += (size_t)(le - lb); continue; }
        const Scene &scene = *reinterpret_cast<const Scene *>(d.occluders[n]);
        for (int l = lb; l < le; ++l, ++pair) {
            if (!list) {
                const std::vector<float> table = quad_samples(rays);
                uv = arena.put(table.data(), table.size());
                list = arena.get<int>((size_t)chunk);
                queue = arena.get<rt::RayRec>((size_t)chunk * rays);
                hits = arena.get<rt::HitRec>((size_t)chunk * rays);
            }
            for (size_t base = 0; base < texels; base += (size_t)chunk) {
                const int count = texels - base < (size_t)chunk ? (int)(texels - base) : chunk;
                const QuadPass q{v.g + ((size_t)n * texels + base) * C, v.params + (size_t)l * kQuadFloats, uv, d.light_type[l], rays,
                                 (unsigned)base, wg};
                const exec::Count live = exec::compact_dev(nullptr, exec::Count(count), list, CastsQuadRays<C>{q});
                const exec::Count all = exec::scaled_count(live, rays);
                exec::launch(all, QuadRays<C>{q, list, live.dev, live.upper, queue});
                exec::trace(scene.bvh, queue, hits, all, true);
                exec::launch(live, QuadMark<C>{q, list, live.dev, live.upper, hits, words + pair * texels + base,
                                               factors + pair * texels + base});
            }
        }
    }
}

// What the two calls refuse before anything is launched.
inline void validate_quad_shadowed(const rdr_deferred_desc &d, bool forward, int rays, const char *who) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
    if (d.num_lights > 0 && d.light_type)
        for (int l = 0; l < d.num_lights; ++l)
            if (d.light_type[l] != 0 && d.light_type[l] != 1)
                fail("light_type of quad " + std::to_string(l) + " is " + std::to_string(d.light_type[l]) +
                     ": it must be 0 (one-sided) or 1 (two-sided)");
    dfr::validate(d, who);
    if (d.ao_occluders || d.ao_words || d.ao_rays != 0)
        fail("ao_occluders, ao_words and ao_rays must be zero: quad lights are not dimmed by ambient occlusion");
    const long long texels = (long long)d.height * d.aa_samples * (long long)d.width * d.aa_samples;
    const long long pairs = pair_bases(d, nullptr);
    if (pairs * texels > (long long)2147483647)
        fail(std::to_string(pairs) + " (image, quad) pairs of " + std::to_string(texels) +
             " texels: the words and factors cannot be indexed (at most 2^31 - 1 of each)");
    if (!forward) {
        if (d.occluders || d.visibility)
            fail("occluders and visibility must be zero: the backward call traces nothing and reads the saved factors");
        return;
    }
    if (rays < 1 || rays > kQuadMaxRays) fail("shadow_rays must be 1 .. 32, got " + std::to_string(rays));
    if (!d.occluders) fail("occluders are required (single entries may be NULL: that image is not shadowed)");
    if (!d.visibility) fail("a visibility buffer is required: the words are written to it");
    if ((uintptr_t)d.visibility & 3) fail("the visibility buffer must be 4-byte aligned");
#if !defined(RDR_HOSTSIM)
    for (int n = 0; n < d.num_images; ++n) {
        if (!d.occluders[n]) continue;
        const int at = reinterpret_cast<const Scene *>(d.occluders[n])->gpu_index;
        if (at != d.gpu_index)
            fail("the occluder scene of image " + std::to_string(n) + " lives on device " + std::to_string(at) +
                 ", the call runs on device " + std::to_string(d.gpu_index));
    }
#endif
}

// ... and the first pair of every image where the launch can read it
inline const int *put_pair_bases(const rdr_deferred_desc &d, Arena &arena) {
    std::vector<int> bases;
    pair_bases(d, &bases);
    return arena.put(bases.data(), bases.size());
}

// rdr_deferred_quad_shadowed: synchronised on return.  Writes every word, every factor and every element of image.
inline void quad_shadowed(const rdr_deferred_desc &d, const float *g, const float *quads, int rays, float *factors, float *image) {
    const char *who = "rdr_deferred_quad_shadowed";
    validate_quad_shadowed(d, true, rays, who);
    if (!g || !image || !factors || (d.num_lights > 0 && !quads)) throw std::runtime_error(std::string(who) + ": null tensor");
    if ((uintptr_t)factors & 3) throw std::runtime_error(std::string(who) + ": factors must be 4-byte aligned");
    if (d.alpha && ((uintptr_t)g & 7)) throw std::runtime_error(std::string(who) + ": with alpha the G-buffer must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, quads);
    Arena scratch;                         // back in the pool after the upload_flush below
    const int *bases = put_pair_bases(d, scratch);
    dispatch(d.alpha != 0, [&](auto c) {
        constexpr int C = decltype(c)::value;
        cast_quad_shadows<C>(d, v, rays, factors, scratch);
        quad_impl<C, true>(d, v, image, factors, bases);
    });
    exec::upload_flush();
}

// rdr_deferred_quad_shadowed_backward: synchronised on return.  Writes every element of d_g and d_quads; the factors are read
// and held constant.
inline void quad_shadowed_backward(const rdr_deferred_desc &d, const float *g, const float *quads, const float *factors,
                                   const float *d_image, float *d_g, float *d_quads) {
    const char *who = "rdr_deferred_quad_shadowed_backward";
    validate_quad_shadowed(d, false, 0, who);
    if (!g || !factors || !d_image || !d_g || (d.num_lights > 0 && (!quads || !d_quads)))
        throw std::runtime_error(std::string(who) + ": null tensor");
    if (d.alpha && (((uintptr_t)g | (uintptr_t)d_g) & 7))
        throw std::runtime_error(std::string(who) + ": with alpha the G-buffers must be 8-byte aligned");
    dfr::Tables tables(d);
    const View v = dfr::make_view(d, tables, g, quads);
    Arena scratch;
    const int *bases = put_pair_bases(d, scratch);
    dispatch(d.alpha != 0, [&](auto c) { quad_adjoint_impl<decltype(c)::value, true>(d, v, d_image, d_g, d_quads, factors, bases); });
    exec::upload_flush();
}

} // namespace dfq
} // namespace rdr
