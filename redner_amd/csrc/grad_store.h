// grad_store.h -- the fp64 gradient accumulators of the host driver (render.cpp).
// Included by render.cpp alone: exec::choose_replicas / set_replicas belong to the translation unit that instantiates the
// stage kernels (hip/exec.h).
#pragma once
#include "arena.h"
#include "scene.h"
#include "stages_bwd.h"
#include <algorithm>
#include <stdexcept>
#include <vector>

namespace rdr {

// ---- gradient accumulators ------------------------------------------------------------------------
// fp64 mirrors of every tensor in the caller's DScene; folded into the fp32 tensors by flush().
struct GradStore {
    Arena arena;               // (arena.h) back in the pool when the call ends: the next render() of the same shape allocates nothing
    GScene g;
    std::vector<GShape> h_shapes;
    std::vector<GMaterial> h_materials;

    // The accumulators live in ONE allocation in two tiers (exec.h: ReplicaLayout), each a block of `stride` doubles that
    // is replicated `replicas` times (replica r at base + r * stride); rdr::accum() picks the replica from the wave id,
    // which spreads the atomics on hot addresses (camera, lights, constant albedos, wall corners) over many cache lines /
    // memory channels.  Tensors of at most kSmallTensor elements go to the small tier (256 replicas) while it has room;
    // the rest -- image textures, big meshes -- to the large tier, which gets the replicas that fit exec::replica_budget():
    // 256 MiB, up to 1 GiB for a job whose length pays for zeroing and summing that much.
    // (One tier for everything gave the camera of a scene with 60 MB of texture gradients 4 replicas: every stage that adds
    // to it or to the walls ran 2-3.5 x longer than with 256, profiles/r3_notes.md.)  flush() sums the replicas in fixed order.
    static constexpr size_t kSmallTensor = 16384, kSmallTierMax = 65536;      // doubles (one replica of the small tier: <= 512 KiB)
    struct Tier { double *base = nullptr; size_t stride = 0, cursor = 0; int replicas = 1; };
    Tier tier[2];                  // 0 = small tensors, 1 = large
    struct Pair { double *acc; float *out; size_t count; int tier; };
    std::vector<Pair> pairs;
    bool counting = true;

    double *place(size_t count, int &t) {
        const size_t padded = (count + 3) & ~(size_t)3;
        t = (count <= kSmallTensor && tier[0].cursor + padded <= kSmallTierMax) ? 0 : 1;
        const size_t at = tier[t].cursor;
        tier[t].cursor += padded;
        return counting ? reinterpret_cast<double *>(8) : tier[t].base + at;       // placeholder in pass 1
    }
    double *mirror(float *out, size_t count) {
        if (!out || count == 0) return nullptr;
        int t;
        double *acc = place(count, t);
        if (!counting) pairs.push_back(Pair{acc, out, count, t});
        return acc;
    }
    GTex mirror_tex(const TexD &t, const rdr_dtexture_desc &d) {
        GTex g;
        for (int i = 0; i < kMaxMip; ++i) g.texels[i] = nullptr;
        g.uv_scale = nullptr;
        if (t.num_levels == 0 || d.num_levels == 0) return g;
        bool constant = t.width[0] <= 0 && t.height[0] <= 0;
        for (int i = 0; i < t.num_levels && i < d.num_levels; ++i) {
            size_t count = constant ? (size_t)t.channels : (size_t)t.width[i] * t.height[i] * t.channels;
            g.texels[i] = mirror(d.texels[i], count);
        }
        g.uv_scale = mirror(d.uv_scale, 2);
        return g;
    }

    GradStore(const Scene &scene, const rdr_dscene_desc &ds, size_t job_samples) {
        counting = true;
        layout(scene, ds);                                   // pass 1: size of one replica of each tier
        for (Tier &t : tier) t.stride = (t.cursor + 31) & ~(size_t)31;
        tier[0].replicas = tier[0].stride ? exec::choose_replicas(tier[0].stride * sizeof(double), 256 * kSmallTierMax * sizeof(double)) : 1;
        tier[1].replicas = tier[1].stride ? exec::choose_replicas(tier[1].stride * sizeof(double), exec::replica_budget(job_samples)) : 1;
        const size_t small_total = tier[0].stride * tier[0].replicas, total = small_total + tier[1].stride * tier[1].replicas;
        double *block = arena.get<double>(total);
        exec::zero(block, sizeof(double) * total);
        tier[0].base = block; tier[1].base = block + small_total;
        exec::set_replicas(ReplicaLayout{block + tier[0].stride, tier[0].stride, tier[1].stride,
                                         (unsigned)(tier[0].replicas - 1), (unsigned)(tier[1].replicas - 1)});
        counting = false; pairs.clear();
        for (Tier &t : tier) t.cursor = 0;
        layout(scene, ds);                                   // pass 2: real pointers
        // accum_triple / accum_block pick the replica from the FIRST address of a group (exec.h: replica_of) and add the
        // others at the same offset: a tensor must lie in one tier as a whole (place() puts it there; checked, not assumed)
        for (const Pair &p : pairs) {
            const Tier &t = tier[p.tier];
            if (p.acc < t.base || p.acc + p.count > t.base + t.stride)
                throw std::runtime_error("render: gradient accumulator straddles a replica tier (GradStore::layout)");
        }
        accumulators_laid_out(tier[0].base, tier[0].stride);           // (a hook of the accumulator backend: nothing on the device)
    }
    void layout(const Scene &scene, const rdr_dscene_desc &ds) {
        if (ds.num_shapes != (int)scene.shapes.size() || ds.num_materials != (int)scene.materials.size() ||
            ds.num_area_lights != (int)scene.lights.size())
            throw std::runtime_error("render: DScene does not match the Scene (shape/material/light counts)");
        h_shapes.resize(scene.shapes.size());
        for (size_t i = 0; i < scene.shapes.size(); ++i) {
            const ShapeD &sh = scene.shapes[i];
            const rdr_dshape_desc &d = ds.shapes[i];
            h_shapes[i].vertices = mirror(d.vertices, (size_t)3 * sh.num_vertices);
            if (!h_shapes[i].vertices) throw std::runtime_error("render: DShape.vertices is required");
            h_shapes[i].uvs = sh.uvs ? mirror(d.uvs, (size_t)2 * (sh.num_uv_vertices > 0 ? sh.num_uv_vertices : sh.num_vertices)) : nullptr;
            h_shapes[i].normals = sh.normals ? mirror(d.normals, (size_t)3 * (sh.num_normal_vertices > 0 ? sh.num_normal_vertices : sh.num_vertices)) : nullptr;
            h_shapes[i].colors = sh.colors ? mirror(d.colors, (size_t)3 * sh.num_vertices) : nullptr;
        }
        h_materials.resize(scene.materials.size());
        for (size_t i = 0; i < scene.materials.size(); ++i) {
            const MaterialD &m = scene.materials[i];
            const rdr_dmaterial_desc &d = ds.materials[i];
            h_materials[i].diffuse = mirror_tex(m.diffuse, d.diffuse_reflectance);
            h_materials[i].specular = mirror_tex(m.specular, d.specular_reflectance);
            h_materials[i].roughness = mirror_tex(m.roughness, d.roughness);
            h_materials[i].generic = mirror_tex(m.generic, d.generic_texture);
            h_materials[i].normal_map = mirror_tex(m.normal_map, d.normal_map);
        }
        if (!counting) {
            g.shapes = arena.get<GShape>(h_shapes.size());
            exec::upload(g.shapes, h_shapes.data(), sizeof(GShape) * h_shapes.size());
            g.materials = arena.get<GMaterial>(h_materials.size());
            exec::upload(g.materials, h_materials.data(), sizeof(GMaterial) * h_materials.size());
        }
        // light intensities: one contiguous fp64 block, scattered back per light
        g.light_intensity = nullptr;
        if (!scene.lights.empty()) {
            int light_tier = 0;
            g.light_intensity = place(3 * scene.lights.size(), light_tier);
            if (!counting)
                for (size_t l = 0; l < scene.lights.size(); ++l)
                    if (ds.area_lights[l].intensity) pairs.push_back(Pair{g.light_intensity + 3 * l, ds.area_lights[l].intensity, 3, light_tier});
        }
        const rdr_dcamera_desc &dc = ds.camera;
        g.cam.position = mirror(dc.position, 3); g.cam.look = mirror(dc.look, 3); g.cam.up = mirror(dc.up, 3);
        g.cam.cam_to_world = mirror(dc.cam_to_world, 16); g.cam.world_to_cam = mirror(dc.world_to_cam, 16);
        g.cam.intrinsic_mat_inv = mirror(dc.intrinsic_mat_inv, 9); g.cam.intrinsic_mat = mirror(dc.intrinsic_mat, 9);
        g.cam.distortion = mirror(dc.distortion_params, 8);
        g.envmap = nullptr;
        if (scene.d.envmap && ds.envmap) {
            GEnvmap h_envmap;
            h_envmap.values = mirror_tex(scene.h_envmap.values, ds.envmap->values);
            h_envmap.world_to_env = mirror(ds.envmap->world_to_env, 16);
            if (!counting) {
                g.envmap = arena.get<GEnvmap>(1);
                exec::upload(g.envmap, &h_envmap, sizeof(GEnvmap));
            }
        }
    }
    void flush() {
        for (const Pair &p : pairs)
            if (p.tier == 0) accumulator_before_fold(tier[0].base, p.acc, p.count);
        accumulators_folded();
        // one launch per tier for all its tensors, unless two mirrors feed overlapping output ranges (a tensor shared by two
        // DScene entries): those must add one after the other
        std::vector<Pair> by_out(pairs);
        std::sort(by_out.begin(), by_out.end(), [](const Pair &a, const Pair &b) { return a.out < b.out; });
        bool aliased = false;
        for (size_t i = 1; i < by_out.size(); ++i) aliased = aliased || by_out[i - 1].out + by_out[i - 1].count > by_out[i].out;
        for (int t = 0; t < 2; ++t) {
            const Tier &tr = tier[t];
            std::vector<FlushSegment> seg;
            for (const Pair &p : pairs) if (p.tier == t) seg.push_back(FlushSegment{(size_t)(p.acc - tr.base), p.count, p.out});
            if (seg.empty()) continue;
            std::sort(seg.begin(), seg.end(), [](const FlushSegment &a, const FlushSegment &b) { return a.begin < b.begin; });
            if (tr.stride > (size_t)0x7fffffff) throw std::runtime_error("render: gradient block too large");
            FlushSegment *d_seg = arena.get<FlushSegment>(seg.size());
            exec::upload(d_seg, seg.data(), sizeof(FlushSegment) * seg.size());
            if (!aliased) exec::launch((int)tr.stride, FlushGrad{tr.base, tr.stride, tr.replicas, d_seg, (int)seg.size()});
            else for (size_t i = 0; i < seg.size(); ++i)
                exec::launch((int)(seg[i].begin + seg[i].count), FlushGrad{tr.base, tr.stride, tr.replicas, d_seg + i, 1});
        }
        exec::set_replicas(ReplicaLayout{nullptr, 0, 0, 0, 0});
    }
};

} // namespace rdr
