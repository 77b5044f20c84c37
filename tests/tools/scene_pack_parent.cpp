// scene_pack_parent.cpp -- the yardstick of tests/tools/scene_pack_lab.py: the derived scene data exactly as rt_create formed it INLINE
// (create_impl in csrc/rt_capi.cpp) before the derivations moved into csrc/rt_scene_pack.hpp -- the statements, their order, std::memset
// + std::memcpy, std::isfinite and std::nextafterf kept as they stood there.  It must not include rt_scene_pack.hpp: it is what that
// header is held to, byte for byte.  Output layout: scene_pack_lab.h.
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_scene_dev.h"
#include "scene_pack_lab.h"

static uint32_t classify(const double *c)
{
    uint32_t cls = 0;
    for (int i = K_X3; i <= K_XYZ; i++)
        if (c[i] != 0.0) cls |= RT_CLS_CUBIC;
    if (cls & RT_CLS_CUBIC) return RT_CLS_CUBIC; // dense path handles everything
    if (c[K_X2] != 0.0 || c[K_Y2] != 0.0 || c[K_Z2] != 0.0) cls |= RT_CLS_SQUARE;
    if (c[K_XY] != 0.0 || c[K_XZ] != 0.0 || c[K_YZ] != 0.0) cls |= RT_CLS_CROSS;
    if (!(cls & RT_CLS_CROSS) && c[K_X2] == 1.0 && c[K_Y2] == 1.0 && c[K_Z2] == 1.0) cls |= RT_CLS_UNITSQ;
    return cls;
}

extern "C" void lab_pack_parent(const LabDesc *sd, unsigned char *out)
{
    LabHeader hdr{};
    for (uint32_t i = 0; i < sd->n_objects; i++)
        if ((double) sd->reflection[i] > 1e-7) hdr.has_mirror = 1; // EPS of the reflection loop, src/update-cpu.cpp:101
    std::vector<DevObject> objs(sd->n_objects);
    for (uint32_t i = 0; i < sd->n_objects; i++) {
        DevObject &o = objs[i];
        std::memset(&o, 0, sizeof(o));
        std::memcpy(o.c, sd->coefs + (size_t) i * 20, sizeof(double) * 20);
        o.albedo[0] = sd->albedo[3 * i + 0];
        o.albedo[1] = sd->albedo[3 * i + 1];
        o.albedo[2] = sd->albedo[3 * i + 2];
        o.refl = sd->reflection[i];
        o.cls = classify(o.c);
        // bounding sphere of a sphere: centre -k/2, r^2 = |centre|^2 - c (src/surface.cpp:4-15 inverted)
        o.bs_radius = INFINITY;
        if (o.cls & RT_CLS_UNITSQ) {
            const double cx = -0.5 * o.c[K_X], cy = -0.5 * o.c[K_Y], cz = -0.5 * o.c[K_Z];
            const double r2 = cx * cx + cy * cy + cz * cz - o.c[K_C];
            if (r2 > 0.0 && std::isfinite(r2)) {
                o.bs_center[0] = cx;
                o.bs_center[1] = cy;
                o.bs_center[2] = cz;
                o.bs_radius = std::sqrt(r2);
                hdr.n_cullable++;
            }
        }
    }
    for (uint32_t i = 0; i < sd->n_objects; i++) {
        const DevObject &o = objs[i];
        LabObject rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.obj = o;
        if (o.cls & RT_CLS_CUBIC) {
            rec.table = 3;
        } else if (o.cls & RT_CLS_UNITSQ) {
            UsEntry e{};
            e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
            e.r = o.bs_radius;
            e.inv_r = (o.bs_radius < INFINITY) ? 1.0 / o.bs_radius : 0.0;
            e.orig = i;
            e.own_lo = INFINITY;
            e.own_hi = 0.0f;
            if (o.bs_radius < INFINITY && o.bs_radius > 0.0) {
                const double r = o.bs_radius, S = 2.0 * (std::fabs(o.bs_center[0]) + std::fabs(o.bs_center[1]) + std::fabs(o.bs_center[2])) + 3.0 * r + 3.0;
                const double lo = 1e-10 * (r * r + 1.0) + 1e-20 * S * S, hi = (r + 1.0) * (r + 1.0);
                float flo = (float) lo, fhi = (float) hi;
                if (!((double) flo > lo)) flo = std::nextafterf(flo, INFINITY);
                if (!((double) fhi < hi)) fhi = std::nextafterf(fhi, -INFINITY);
                if (std::isfinite(lo) && std::isfinite(hi) && (double) flo > lo && (double) fhi < hi && flo < fhi) {
                    e.own_lo = flo;
                    e.own_hi = fhi;
                }
            }
            rec.table = 0;
            rec.us = e;
        } else if (o.cls & (RT_CLS_SQUARE | RT_CLS_CROSS)) {
            GqEntry e{};
            e.x2 = o.c[K_X2]; e.y2 = o.c[K_Y2]; e.z2 = o.c[K_Z2];
            e.xy = o.c[K_XY]; e.xz = o.c[K_XZ]; e.yz = o.c[K_YZ];
            e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
            e.orig = i;
            rec.table = 1;
            rec.gq = e;
        } else {
            LinEntry e{};
            e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
            e.orig = i;
            rec.table = 2;
            rec.lin = e;
        }
        MatEntry m{};
        m.albedo[0] = objs[i].albedo[0];
        m.albedo[1] = objs[i].albedo[1];
        m.albedo[2] = objs[i].albedo[2];
        m.refl = objs[i].refl;
        rec.mat = m;
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * i, &rec, sizeof(rec));
    }
    std::vector<DevLight> lights(sd->n_lights);
    std::vector<char> term_finite(sd->n_lights, 0); // this light's colour and every albedo are finite: a factor max(0, n.l) = 0 makes its term exactly +0
    for (uint32_t i = 0; i < sd->n_lights; i++) {
        DevLight &l = lights[i];
        std::memset(&l, 0, sizeof(l));
        for (int k = 0; k < 3; k++) {
            l.p[k] = sd->light_p[3 * i + k];
            l.color[k] = sd->light_color[3 * i + k];
        }
        l.spherical = sd->light_is_spherical[i] ? 1u : 0u;
        for (int k = 0; k < 3; k++) l.sdir[k] = (double) (float) l.p[k];
        l.dxx = l.sdir[0] * l.sdir[0];
        l.dyy = l.sdir[1] * l.sdir[1];
        l.dzz = l.sdir[2] * l.sdir[2];
        l.dxy = l.sdir[0] * l.sdir[1];
        l.dxz = l.sdir[0] * l.sdir[2];
        l.dyz = l.sdir[1] * l.sdir[2];
        l.u2 = (l.dxx + l.dyy) + l.dzz;
        l.inv_uu = l.u2 > 0.0 ? 1.0 / l.u2 : 0.0;
        l.len_u = 1.001 * std::sqrt(l.u2);
        bool finite = std::isfinite(l.color[0]) && std::isfinite(l.color[1]) && std::isfinite(l.color[2]);
        for (uint32_t k = 0; k < sd->n_objects * 3u && finite; k++) finite = std::isfinite(sd->albedo[k]);
        l.backface_exact = (!l.spherical && finite) ? 1u : 0u;
        term_finite[i] = finite ? 1 : 0;
    }
    hdr.lights_plain = 1u;
    for (uint32_t i = 0; i < sd->n_lights; i++) {
        const DevLight &l = lights[i];
        LightK k;
        std::memset(&k, 0, sizeof(k));
        for (int c = 0; c < 3; c++) { k.p[c] = l.p[c]; k.sdir[c] = l.sdir[c]; k.color[c] = l.color[c]; }
        k.u2 = l.u2; k.inv_uu = l.inv_uu; k.len_u = l.len_u;
        k.four_u2 = 4.0 * l.u2;
        k.s_yz = std::fabs(l.sdir[1]) + std::fabs(l.sdir[2]);
        k.s_xz = std::fabs(l.sdir[0]) + std::fabs(l.sdir[2]);
        k.s_xy = std::fabs(l.sdir[0]) + std::fabs(l.sdir[1]);
        k.flags = (l.spherical ? 1u : 0u) | (l.backface_exact ? 2u : 0u) | (std::fabs(l.u2) > 1e-7 ? 4u : 0u) | // EPS of include/surface_impl.h:16,138
                  ((l.spherical && term_finite[i]) ? 8u : 0u);
        if (!l.spherical && (k.flags & 6u) != 6u) hdr.lights_plain = 0u;
        LabLight rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.light = l;
        rec.k = k;
        std::memcpy(out + sizeof(LabHeader) + sizeof(LabObject) * sd->n_objects + sizeof(LabLight) * i, &rec, sizeof(rec));
    }
    std::memcpy(out, &hdr, sizeof(hdr));
}
