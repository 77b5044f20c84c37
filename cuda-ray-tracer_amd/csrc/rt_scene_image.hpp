// rt_scene_image.hpp -- the whole scene image of a context, formed on the host from an rt_scene_desc: the blob (rt_scene_dev.h:
// [DevObject x n_obj][UsEntry x n_us][GqEntry x n_gq][LinEntry x n_lin][uint32 x n_cub][MatEntry x n_obj]), the two light tables, and every
// word of FrameArgs that describes them.  rt_create uploads the result (rt_capi.cpp); the test tools call the same function
// (tests/tools/scene_pack_lab.cpp), so the class-table order, the offsets and their 16-byte rounding have one copy.
//
// Host only and free of HIP calls: it compiles with a plain C++ compiler.  The records come from rt_scene_pack.hpp, whose rule holds
// here too: every translation unit that includes this is built with -ffp-contract=off.
#ifndef RT_SCENE_IMAGE_HPP
#define RT_SCENE_IMAGE_HPP

#include <algorithm>
#include <cstring>
#include <vector>

#include "mi355rt.h"
#include "rt_scene_pack.hpp"

namespace rtp {

struct SceneImage {
    std::vector<unsigned char> blob; // FrameArgs::scene_bytes of them
    std::vector<DevLight> lights;
    std::vector<LightK> lightk;      // the same lights as the lean path reads them
    std::vector<double> cub_coefs;   // the 20 coefficients of the first RT_CUB_AT_MAX degree-3 objects (FrameArgs::cub_rec is formed from them every frame)
    uint32_t n_cullable = 0;         // objects with a bounding radius
    std::vector<UsEntry> bounds;     // RT_FLAG_STREAM_CULL contexts: the bound of every 64-entry chunk of the ordered unit-sphere table (stream_cull_image)
    std::vector<UsEntry> groups;     // RT_FLAG_STREAM_CULL_GROUPS contexts: the bound of every 64 consecutive chunk bounds (stream_group_image)
    bool lean_ok = false;            // the scene and the flags qualify for the wave-per-block instantiation (FrameArgs::lean)
};

// Fills fa's scene words: n_obj, n_lights, n_us .. n_cub, off_us .. off_mat, scene_bytes, stage_bytes, has_mirror, cull, all_cullable, lights_plain,
// pt_mask.  `flags` are rt_config's.  `fill` is the byte every record starts out as before its pack function writes it (the blob's rounding
// gaps keep it): 0 in the product; the test tools poison with it, since a pack function has to write every byte of its record itself.
inline SceneImage scene_image(const rt_scene_desc &sd, uint32_t flags, FrameArgs &fa, unsigned char fill = 0)
{
    SceneImage im;
    fa.n_obj = sd.n_objects;
    fa.n_lights = sd.n_lights;
    fa.has_mirror = 0;
    for (uint32_t i = 0; i < sd.n_objects; i++)
        if (is_mirror(sd.reflection[i])) fa.has_mirror = 1;
    std::vector<DevObject> objs(sd.n_objects);
    if (!objs.empty()) std::memset(objs.data(), fill, sizeof(DevObject) * objs.size());
    bool albedos_finite = true;
    for (uint32_t i = 0; i < sd.n_objects; i++) { // (rt_scene_pack.hpp: class word, bounding sphere)
        pack_object(objs[i], sd.coefs + (size_t) i * RT_NCOEF, sd.albedo + 3 * (size_t) i, sd.reflection[i]);
        if (cullable(objs[i])) im.n_cullable++;
        albedos_finite = albedos_finite && albedo_finite(objs[i].albedo);
    }
    // culling costs one bounding-volume decision per (object, light, 64-hit chunk); worth it from a handful
    // of bounded objects upwards
    fa.cull = (!(flags & RT_FLAG_NOCULL) && im.n_cullable >= 4) ? 1u : 0u;
    fa.all_cullable = (fa.cull && im.n_cullable == sd.n_objects) ? 1u : 0u;

    // per-class tables behind the object array (rt_scene_dev.h): first their sizes and offsets, then the entries in scene order
    fa.n_us = fa.n_gq = fa.n_lin = fa.n_cub = 0;
    for (const DevObject &o : objs) {
        const uint32_t t = table_of(o.cls);
        (t == 0u ? fa.n_us : t == 1u ? fa.n_gq : t == 2u ? fa.n_lin : fa.n_cub)++;
    }
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t) 15; };
    size_t off = up16(sizeof(DevObject) * objs.size());
    fa.off_us = (uint32_t) off; off = up16(off + sizeof(UsEntry) * fa.n_us);
    fa.off_gq = (uint32_t) off; off = up16(off + sizeof(GqEntry) * fa.n_gq);
    fa.off_lin = (uint32_t) off; off = up16(off + sizeof(LinEntry) * fa.n_lin);
    fa.off_cub = (uint32_t) off; off = up16(off + sizeof(uint32_t) * fa.n_cub);
    fa.off_mat = (uint32_t) off; off = up16(off + sizeof(MatEntry) * objs.size());
    fa.scene_bytes = (uint32_t) (off ? off : 16);
    fa.stage_bytes = fa.scene_bytes - fa.off_us;
    im.blob.assign(fa.scene_bytes, fill);
    unsigned char *b = im.blob.data();
    if (!objs.empty()) std::memcpy(b, objs.data(), sizeof(DevObject) * objs.size());
    UsEntry *t_us = reinterpret_cast<UsEntry *>(b + fa.off_us);
    GqEntry *t_gq = reinterpret_cast<GqEntry *>(b + fa.off_gq);
    LinEntry *t_lin = reinterpret_cast<LinEntry *>(b + fa.off_lin);
    uint32_t *t_cub = reinterpret_cast<uint32_t *>(b + fa.off_cub);
    MatEntry *t_mat = reinterpret_cast<MatEntry *>(b + fa.off_mat);
    for (uint32_t i = 0, n_cub = 0; i < sd.n_objects; i++) {
        const DevObject &o = objs[i];
        switch (table_of(o.cls)) {
        case 0u: pack_us(*t_us++, o, i); break; // (with the own-sphere window of the lean path)
        case 1u: pack_gq(*t_gq++, o, i); break;
        case 2u: pack_lin(*t_lin++, o, i); break;
        default:
            if (n_cub++ < RT_CUB_AT_MAX) im.cub_coefs.insert(im.cub_coefs.end(), o.c, o.c + RT_NCOEF);
            *t_cub++ = i;
        }
        pack_mat(t_mat[i], o);
    }
    im.lights.resize(sd.n_lights);
    im.lightk.resize(sd.n_lights);
    if (sd.n_lights) {
        std::memset(im.lights.data(), fill, sizeof(DevLight) * sd.n_lights);
        std::memset(im.lightk.data(), fill, sizeof(LightK) * sd.n_lights);
    }
    fa.lights_plain = 1u;
    for (uint32_t i = 0; i < sd.n_lights; i++) {
        const bool term_finite = pack_light(im.lights[i], sd.light_p + 3 * (size_t) i, sd.light_color + 3 * (size_t) i, sd.light_is_spherical[i], albedos_finite);
        pack_lightk(im.lightk[i], im.lights[i], term_finite);
        if (!im.lights[i].spherical && (im.lightk[i].flags & 6u) != 6u) fa.lights_plain = 0u;
    }

    // the wave-per-block instantiation: unit spheres only, every one with a bounding radius, no mirror (sparse frames take the other one)
    im.lean_ok = !(flags & (RT_FLAG_SIMPLE | RT_FLAG_NOLEAN)) && fa.all_cullable && fa.n_us == sd.n_objects && !fa.has_mirror && fa.n_gq == 0 && fa.n_lin == 0 &&
                 fa.n_cub == 0;
    if (sd.n_lights > 64u) im.lean_ok = false; // (its point-light pass keeps one bit per light and lane)
    fa.pt_mask[0] = fa.pt_mask[1] = 0u;
    for (uint32_t i = 0; i < sd.n_lights && i < 64u; i++)
        if (sd.light_is_spherical[i]) fa.pt_mask[i >> 5] |= 1u << (i & 31u);
    return im;
}

// RT_FLAG_STREAM_CULL, for a context whose decision is true: put the blob's unit-sphere table into the context's
// spatial order and form the chunk bounds (one UsEntry per 64 entries of the ordered table, pack_chunk_bound).  Nothing else in the blob
// moves; an entry keeps its bytes, `orig` included.
//
// The order (slot_orig == nullptr, rt_create): the spheres with a bounding radius first, by the Morton key of their centres, ties by
// object index; the others behind them in index order.  Key (rt_scene_pack.hpp, stream_cull_key: one copy for the host and the device): per axis
// q = (uint64) ((c - lo) / (hi - lo) * 2097151.0) (21 bits; 0 where hi == lo), lo / hi = the box of the bounded spheres' centres; bit 3 b + 2 of the
// key is bit b of q_x, 3 b + 1 that of q_y, 3 b that of q_z.  No result depends on it: it only decides which spheres share a chunk.
// slot_orig != nullptr (the tests, for a context that has seen rt_set_scene): slot s takes the entry of object slot_orig[s] -- the order
// is the context's, chosen at rt_create, and rt_set_scene keeps it.  (rt_reorder_scene, rt_reorder_scene.hip, chooses it anew on the device by the rule
// above -- the same key function, stream_cull_key -- and then the device holds what this function packs with slot_orig == nullptr.)
inline std::vector<UsEntry> stream_cull_image(SceneImage &im, const FrameArgs &fa, unsigned char fill = 0, const uint32_t *slot_orig = nullptr)
{
    const uint32_t n = fa.n_us;
    UsEntry *t_us = reinterpret_cast<UsEntry *>(im.blob.data() + fa.off_us);
    const std::vector<UsEntry> old(t_us, t_us + n);
    std::vector<uint32_t> order(n); // slot -> index into `old`
    if (slot_orig) {
        std::vector<uint32_t> where(fa.n_obj, 0u);
        for (uint32_t j = 0; j < n; j++) where[old[j].orig] = j;
        for (uint32_t s = 0; s < n; s++) order[s] = where[slot_orig[s]];
    } else {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (const UsEntry &e : old) {
            if (!(e.r < INFINITY)) continue;
            const double c[3] = {-0.5 * e.kx, -0.5 * e.ky, -0.5 * e.kz};
            for (int k = 0; k < 3; k++) {
                lo[k] = c[k] < lo[k] ? c[k] : lo[k];
                hi[k] = c[k] > hi[k] ? c[k] : hi[k];
            }
        }
        std::vector<uint64_t> key(n);
        for (uint32_t j = 0; j < n; j++) key[j] = stream_cull_key(old[j], lo, hi); // (unbounded: ~0, behind every bounded sphere)
        for (uint32_t j = 0; j < n; j++) order[j] = j;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : old[a].orig < old[b].orig; });
    }
    for (uint32_t s = 0; s < n; s++) t_us[s] = old[order[s]];
    const uint32_t n_chunks = (n + 63u) / 64u;
    std::vector<UsEntry> bounds(n_chunks);
    if (n_chunks) std::memset(bounds.data(), fill, sizeof(UsEntry) * n_chunks);
    for (uint32_t c = 0; c < n_chunks; c++) pack_chunk_bound(bounds[c], t_us + 64u * c, (n - 64u * c < 64u) ? n - 64u * c : 64u, c);
    return bounds;
}

// The group bounds of an RT_FLAG_STREAM_CULL_GROUPS context: one bound per 64 consecutive chunk bounds, formed by the function that
// forms the chunk bounds themselves -- pack_chunk_bound's proof asks of its members a centre -k / 2, an r and an inv_r, which a chunk bound has --, orig =
// the group's index.  A group with an unbounded chunk (r = +inf) is unbounded.  bounds: stream_cull_image's result, or the chunk bounds a device holds;
// fill: as in scene_image.  rt_group_bounds.hip forms the same bytes on the device.
inline std::vector<UsEntry> stream_group_image(const std::vector<UsEntry> &bounds, unsigned char fill = 0)
{
    const uint32_t n = (uint32_t) bounds.size(), n_groups = (n + 63u) / 64u;
    std::vector<UsEntry> groups(n_groups);
    if (n_groups) std::memset(groups.data(), fill, sizeof(UsEntry) * n_groups);
    for (uint32_t g = 0; g < n_groups; g++) pack_chunk_bound(groups[g], bounds.data() + 64u * g, (n - 64u * g < 64u) ? n - 64u * g : 64u, g);
    return groups;
}

} // namespace rtp

#endif
