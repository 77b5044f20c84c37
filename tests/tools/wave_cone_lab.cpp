// wave_cone_lab.cpp -- host lab behind the wave cone of ray_list_cull_kernel (csrc/rt_wave_cone.hpp, csrc/rt_stream_cull_adaptive.hip;
// DESIGN.md section 26; test infrastructure: it links the oracle).  The kernel's own header is compiled for the host, as cull_lab.cpp
// compiles rt_wavefront_math.hpp, and the lanes' parts of the cone are called through it; the wave's reductions between them (the
// butterfly sum, the maximum, the first candidate, the minimum) are restated here in the kernel's order.
//   * lab_sample_rays: the oracle's direction and primary hit (the reference's nearest-hit loop) of every listed ray;
//   * lab_wave_cones:  the cone of every wave of 64 lanes, and how many used lanes violate dot3(axis, d) >= cos_t;
//   * lab_cone_verdicts: sphere_in_cone about bounds for a wave's cone.
// Built and driven by tests/tools/stream_cull_adaptive_scenes.py.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rt_wave_cone.hpp"
#include "rt_wavefront_math.hpp"
#include "../../oracle/rt_oracle.h"

using namespace rtm;

// n rays: pixel (xy[2 i], xy[2 i + 1]) of the scene's grid, or x < 0: a lane without a ray.  dirs [n][3], owner [n] (-1: no hit or no ray).
extern "C" void lab_sample_rays(const orc_scene *sc, const double *cam, uint64_t n, const int32_t *xy, double *dirs, int32_t *owner)
{
    const double origin[3] = {cam[12], cam[13], cam[14]};
    for (uint64_t i = 0; i < n; i++) {
        owner[i] = -1;
        dirs[3 * i] = dirs[3 * i + 1] = 0.0;
        dirs[3 * i + 2] = 1.0;
        if (xy[2 * i] < 0) continue;
        orc_primary_dir(sc, cam, xy[2 * i], xy[2 * i + 1], dirs + 3 * i);
        double best_t = INFINITY;
        for (uint32_t k = 0; k < sc->n_objects; k++) {
            const double t = orc_intersect_ray(sc->objects[k].c, origin, dirs + 3 * i);
            if (t >= EPS && t < MAX_T && t < best_t) {
                best_t = t;
                owner[i] = (int32_t) k;
            }
        }
    }
}

// n waves of 64 lanes: dirs [n][64][3], use [n][64].  axis [n][3], cos_t [n], pick [n] (the axis lane; -1: no lane in use, no cone),
// bad [n] (used lanes with !(dot3(axis, d) >= cos_t), evaluated as the kernel evaluates it).
extern "C" void lab_wave_cones(uint64_t n, const double *dirs, const uint8_t *use, double *axis, double *cos_t, int32_t *pick, int32_t *bad)
{
    for (uint64_t w = 0; w < n; w++) {
        const double *dw = dirs + w * 64 * 3;
        const uint8_t *uw = use + w * 64;
        D3 d[64], s[64];
        bool any = false;
        for (int l = 0; l < 64; l++) {
            d[l] = D3{dw[3 * l], dw[3 * l + 1], dw[3 * l + 2]};
            s[l] = wc_term(d[l], uw[l] != 0);
            any = any || uw[l] != 0;
        }
        pick[w] = -1;
        bad[w] = 0;
        axis[3 * w] = axis[3 * w + 1] = axis[3 * w + 2] = cos_t[w] = 0.0;
        if (!any) continue;
        for (int off = 32; off > 0; off >>= 1) { // the kernel's butterfly: every lane adds its partner's value
            D3 t[64];
            for (int l = 0; l < 64; l++) t[l] = D3{s[l].x + s[l ^ off].x, s[l].y + s[l ^ off].y, s[l].z + s[l ^ off].z};
            memcpy(s, t, sizeof(s));
        }
        double score[64], top = -INFINITY;
        for (int l = 0; l < 64; l++) {
            score[l] = wc_score(s[l], d[l], uw[l] != 0);
            top = score[l] > top ? score[l] : top;
        }
        int p = -1, first = -1;
        for (int l = 63; l >= 0; l--) {
            if (wc_is_pick(score[l], top, uw[l] != 0)) p = l;
            if (uw[l]) first = l;
        }
        if (p < 0) p = first;
        pick[w] = p;
        double c = INFINITY;
        for (int l = 0; l < 64; l++) {
            const double v = wc_cos(d[p], d[l], uw[l] != 0);
            c = v < c ? v : c;
        }
        for (int l = 0; l < 64; l++)
            if (uw[l] && !(dot3(d[p], d[l]) >= c)) bad[w]++;
        axis[3 * w] = d[p].x; axis[3 * w + 1] = d[p].y; axis[3 * w + 2] = d[p].z;
        cos_t[w] = c;
    }
}

// sphere_in_cone about n bounds (64-byte UsEntry records) for one cone
extern "C" void lab_cone_verdicts(uint64_t n, const UsEntry *bounds, const double *org, const double *axis, double cos_t, int32_t *verdict)
{
    const D3 o{org[0], org[1], org[2]}, a{axis[0], axis[1], axis[2]};
    for (uint64_t i = 0; i < n; i++) verdict[i] = sphere_in_cone(bounds[i].kx, bounds[i].ky, bounds[i].kz, bounds[i].r, bounds[i].inv_r, o, a, cos_t) ? 1 : 0;
}
