// rt_scene_image.hpp -- the whole scene image of a context, formed on the host from an rt_scene_desc: the blob (rt_scene_dev.h:
// [DevObject x n_obj][UsEntry x n_us][GqEntry x n_gq][LinEntry x n_lin][uint32 x n_cub][MatEntry x n_obj]), the two light tables, and every
// word of FrameArgs that describes them.  rt_create uploads the result (rt_capi.cpp); the test tools call the same function
// (tests/tools/scene_pack_lab.cpp), so the class-table order, the offsets and their 16-byte rounding have one copy.
//
// Host only and free of HIP calls: it compiles with a plain C++ compiler.  The records come from rt_scene_pack.hpp, whose rule holds
// here too: every translation unit that includes this is built with -ffp-contract=off.
#ifndef RT_SCENE_IMAGE_HPP
#define RT_SCENE_IMAGE_HPP

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

} // namespace rtp

#endif
