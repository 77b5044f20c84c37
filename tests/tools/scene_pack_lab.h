// scene_pack_lab.h -- what both sides of tests/tools/scene_pack_lab.py write: the derived data of a scene, record by record.
//   [LabHeader][LabObject x n_objects][LabLight x n_lights]
// An object's record holds its DevObject, the entry of the ONE class table it belongs to (the others stay zero) and its MatEntry.
#ifndef SCENE_PACK_LAB_H
#define SCENE_PACK_LAB_H

#include <stdint.h>

#include "mi355rt.h"
#include "rt_scene_dev.h"

struct LabDesc { // the arrays of rt_scene_desc
    uint32_t n_objects, n_lights;
    const double *coefs;
    const float *reflection, *albedo;
    const uint8_t *light_is_spherical;
    const double *light_p;
    const float *light_color;
};

inline rt_scene_desc lab_desc(const LabDesc *sd) // ... as the rt_scene_desc the library's own host code takes
{
    rt_scene_desc d{};
    d.n_objects = sd->n_objects; d.n_lights = sd->n_lights;
    d.coefs = sd->coefs; d.reflection = sd->reflection; d.albedo = sd->albedo;
    d.light_is_spherical = sd->light_is_spherical; d.light_p = sd->light_p; d.light_color = sd->light_color;
    return d;
}

struct alignas(16) LabHeader {
    uint32_t has_mirror, n_cullable, lights_plain, pad;
};

struct alignas(16) LabObject {
    DevObject obj;
    UsEntry us;
    GqEntry gq;
    LinEntry lin;
    MatEntry mat;
    uint32_t table, pad[3]; // 0 us, 1 gq, 2 lin, 3 degree 3
};
static_assert(sizeof(LabObject) == 224 + 64 + 96 + 48 + 16 + 16, "LabObject layout");

struct alignas(16) LabLight {
    DevLight light;
    LightK k;
};
static_assert(sizeof(LabLight) == 144 + 128 + 48, "LabLight layout (LightK is 64-byte aligned)");

#endif
