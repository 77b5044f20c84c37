// scene_pack_lab.cpp -- csrc/rt_scene_pack.hpp compiled for the host, called the way create_impl (csrc/rt_capi.cpp) calls it; the other
// side of the comparison is scene_pack_parent.cpp.  Driver: tests/tools/scene_pack_lab.py.
#include <cstring>
#include <vector>

#include "rt_scene_pack.hpp"
#include "scene_pack_lab.h"

extern "C" uint64_t lab_pack_bytes(uint32_t n_objects, uint32_t n_lights)
{
    return sizeof(LabHeader) + sizeof(LabObject) * (uint64_t) n_objects + sizeof(LabLight) * (uint64_t) n_lights;
}

extern "C" void lab_pack_header(const LabDesc *sd, unsigned char *out)
{
    LabHeader hdr{};
    for (uint32_t i = 0; i < sd->n_objects; i++)
        if (rtp::is_mirror(sd->reflection[i])) hdr.has_mirror = 1;
    std::vector<DevObject> objs(sd->n_objects);
    bool albedos_finite = true;
    if (!objs.empty()) std::memset(objs.data(), 0xA5, sizeof(DevObject) * objs.size()); // (poison: the pack functions must fill every byte of their records themselves)
    for (uint32_t i = 0; i < sd->n_objects; i++) {
        rtp::pack_object(objs[i], sd->coefs + (size_t) i * 20, sd->albedo + 3 * (size_t) i, sd->reflection[i]);
        if (rtp::cullable(objs[i])) hdr.n_cullable++;
        albedos_finite = albedos_finite && rtp::albedo_finite(objs[i].albedo);
    }
    for (uint32_t i = 0; i < sd->n_objects; i++) {
        const DevObject &o = objs[i];
        LabObject rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.obj = o;
        rec.table = rtp::table_of(o.cls);
        if (rec.table == 0) {
            std::memset(&rec.us, 0xA5, sizeof(rec.us));
            rtp::pack_us(rec.us, o, i);
        } else if (rec.table == 1) {
            std::memset(&rec.gq, 0xA5, sizeof(rec.gq));
            rtp::pack_gq(rec.gq, o, i);
        } else if (rec.table == 2) {
            std::memset(&rec.lin, 0xA5, sizeof(rec.lin));
            rtp::pack_lin(rec.lin, o, i);
        }
        std::memset(&rec.mat, 0xA5, sizeof(rec.mat));
        rtp::pack_mat(rec.mat, o);
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * i, &rec, sizeof(rec));
    }
    hdr.lights_plain = 1u;
    for (uint32_t i = 0; i < sd->n_lights; i++) {
        LabLight rec;
        std::memset(&rec, 0, sizeof(rec));
        std::memset(&rec.light, 0xA5, sizeof(rec.light));
        std::memset(&rec.k, 0xA5, sizeof(rec.k));
        const bool term_finite = rtp::pack_light(rec.light, sd->light_p + 3 * (size_t) i, sd->light_color + 3 * (size_t) i, sd->light_is_spherical[i], albedos_finite);
        rtp::pack_lightk(rec.k, rec.light, term_finite);
        if (!rec.light.spherical && (rec.k.flags & 6u) != 6u) hdr.lights_plain = 0u;
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * sd->n_objects + sizeof(LabLight) * i, &rec, sizeof(rec));
    }
    std::memcpy(out, &hdr, sizeof(hdr));
}
