// scene_pack_lab.cpp -- the scene image rt_create uploads, formed by the library's own host function (csrc/rt_scene_image.hpp over
// csrc/rt_scene_pack.hpp) and read back record by record through the offsets it returns; the other side of the comparison is
// scene_pack_parent.cpp.  Driver: tests/tools/scene_pack_lab.py.
#include <cstring>

#include "rt_scene_image.hpp"
#include "scene_pack_lab.h"

extern "C" uint64_t lab_pack_bytes(uint32_t n_objects, uint32_t n_lights)
{
    return sizeof(LabHeader) + sizeof(LabObject) * (uint64_t) n_objects + sizeof(LabLight) * (uint64_t) n_lights;
}

extern "C" void lab_pack_header(const LabDesc *sd, unsigned char *out)
{
    FrameArgs fa{};
    const rtp::SceneImage im = rtp::scene_image(lab_desc(sd), 0u, fa, 0xA5); // (poison: the pack functions must fill every byte of their records themselves)
    const LabHeader hdr = {fa.has_mirror, im.n_cullable, fa.lights_plain, 0u};
    const unsigned char *b = im.blob.data();
    uint32_t seen[4] = {0, 0, 0, 0}; // objects of each table so far: an object's entry is the next one of its table
    for (uint32_t i = 0; i < sd->n_objects; i++) {
        LabObject rec;
        std::memset(&rec, 0, sizeof(rec));
        std::memcpy(&rec.obj, b + sizeof(DevObject) * i, sizeof(DevObject));
        rec.table = rtp::table_of(rec.obj.cls);
        const uint32_t j = seen[rec.table]++;
        if (rec.table == 0) std::memcpy(&rec.us, b + fa.off_us + sizeof(UsEntry) * j, sizeof(UsEntry));
        if (rec.table == 1) std::memcpy(&rec.gq, b + fa.off_gq + sizeof(GqEntry) * j, sizeof(GqEntry));
        if (rec.table == 2) std::memcpy(&rec.lin, b + fa.off_lin + sizeof(LinEntry) * j, sizeof(LinEntry));
        std::memcpy(&rec.mat, b + fa.off_mat + sizeof(MatEntry) * i, sizeof(MatEntry));
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * i, &rec, sizeof(rec));
    }
    for (uint32_t i = 0; i < sd->n_lights; i++) {
        LabLight rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.light = im.lights[i];
        rec.k = im.lightk[i];
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * sd->n_objects + sizeof(LabLight) * i, &rec, sizeof(rec));
    }
    std::memcpy(out, &hdr, sizeof(hdr));
}
