// rt_stream_shade.hpp -- the reference's render_pixel (src/update-cpu.cpp:82-119) for one ray per lane, once: the loop that
// the three shade_rays kernels (through their one body, rt_ray_kernels.hpp: rk_shade_rays), the three streamed frame kernels
// (rt_stream.hip, rt_stream_cull.hip, rt_stream_cull_bounce.hip) and the two streamed ray-list kernels (rt_stream_adaptive.hip,
// rt_stream_cull_adaptive.hip) all run.  It is the image's definition: nearest hit, normal_vector in full, every light in index order
// with its occlusion query from sp + SHADOW_BIAS * sn, surface_color, the clamp, the reflection loop with its blends.  No facing-away
// skip and no own-sphere rule.  A kernel states only what it does differently, as a policy:
//   nearest<HAS_GQ, HAS_CUBIC>(k, lane, o, d, use, best_t, best)                the nearest-hit query of segment k (what k == 0 means is the policy's)
//   segment(hit, sp) -> Policy::Segment                                         once per segment that has a hit: what the light loop shares
//   occluded<HAS_GQ, HAS_CUBIC>(seg, lane, lt, so, sd, use, max_t, blocked)     the occlusion query towards one light
//   first_hit(best, best_t, sp, sn)                                             behind the hit point of segment 0 (the shade_rays kernels' record: RkShade)
// The wave-level rules are the callers' and the policies' alike: all 64 lanes call; `use` is a predicate; no lane leaves before the
// wave's last ballot, readlane or staged chunk; nothing is workgroup-wide (no barrier: the waves of a workgroup run different numbers
// of bounces and chunks); no hook puts divergent control flow around a staging call.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_SHADE_HPP
#define RT_STREAM_SHADE_HPP

#include <hip/hip_runtime.h>

#include "rt_stream.hpp" // sq_query, for SqShade alone: shade_loop itself needs nothing of the streamed loops, only rt_rayquery.hpp's types and
                         // rt_shade.hpp's arithmetic (so the files that stage all tables read rt_stream.hpp without using it)

namespace RT_SYM(rtk) {

// The bounce loop for the ray (o, d) of every lane in `use`: iteration k traces the k-th segment of every lane that is still bouncing
// (all such lanes have bounced exactly k times, so the reference's `cur_reflections` is the wave-uniform k).  a: FrameArgs or
// ShadeRaysArgs (bg, n_lights, max_refl); scene: the blob, the DevObject records first.  Returns the colour; bg for a lane not in use.
template <bool HAS_GQ, bool HAS_CUBIC, typename Args, typename Policy>
__device__ __forceinline__ F3 shade_loop(const Args &a, const unsigned char *scene, const DevLight *lights, uint32_t lane, Policy &pol, D3 o, D3 d,
                                         bool use)
{
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const F3 bg{a.bg[0], a.bg[1], a.bg[2]};
    F3 res = bg; // a first-segment miss is the background colour
    float cur_ratio = 1.0f;
    bool bouncing = use;
    for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++) {
        // get_color_and_object, src/update-cpu.cpp:45-80: the nearest hit ...
        double best_t = INFINITY;
        int best = -1;
        pol.template nearest<HAS_GQ, HAS_CUBIC>(k, lane, o, d, bouncing, best_t, best);
        const bool hit = bouncing && best >= 0;
        const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
        D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
        if (hit) {
            sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
            sn = normal_vector(bo->c, sp); // all twenty coefficients; FP64, never flipped
        }
        if (k == 0u) pol.first_hit(best, best_t, sp, sn);
        // ... every light in index order (wave-uniform: scalar loads), shadow_ray from sp + SHADOW_BIAS * sn.  The shadow ray is a ray
        // the kernel formed: sp can lie beyond the tables' proven range and sn can be NaN, so the query decides anew whether the tables
        // are proven for it.
        const D3 so{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
        F3 acc{0.0f, 0.0f, 0.0f};
        if (__ballot(hit) != 0ull) {
            const F3 albedo{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
            const typename Policy::Segment seg = pol.segment(hit, sp);
            for (uint32_t l = 0; l < a.n_lights; l++) {
                const DevLight *lt = &lights[l];
                const bool spherical = lt->spherical != 0;
                double max_t;
                const D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
                int blocked = 0;
                pol.template occluded<HAS_GQ, HAS_CUBIC>(seg, lane, *lt, so, sd, hit, max_t, blocked);
                if (hit && blocked == 0) {
                    const F3 c = surface_color(lt->p, lt->color, spherical, sp, sn, albedo);
                    acc.x += c.x;
                    acc.y += c.y;
                    acc.z += c.z;
                }
            }
        }
        if (bouncing) {
            if (!hit) {
                if (k != 0u) RT_SYM(rtk)::blend(res, cur_ratio, bg); // a bounce that leaves the scene picks up the background
                bouncing = false;
            } else {
                // glm::min(vec3(1.0f), acc)
                const F3 oc{(acc.x < 1.0f) ? acc.x : 1.0f, (acc.y < 1.0f) ? acc.y : 1.0f, (acc.z < 1.0f) ? acc.z : 1.0f};
                if (k == 0u) res = oc;
                else RT_SYM(rtk)::blend(res, cur_ratio, oc);
                // the reflection loop, src/update-cpu.cpp:96-117
                const float refl = bo->refl;
                if (!((double) refl > EPS)) {
                    bouncing = false;
                } else {
                    cur_ratio *= refl;
                    if (k == a.max_refl) {
                        RT_SYM(rtk)::blend(res, cur_ratio, bg);
                        bouncing = false;
                    } else {
                        d = reflect_ray(d, sn); // of the direction as it is
                        o = so;
                    }
                }
            }
        }
    }
    return res;
}

// what a policy without a per-segment state hands the light loop
struct ShadeNoSegment {};

// The policy over sq_query: every query a full sweep of the streamed tables.  cone (wave-uniform): the wave's lanes are the pixels of
// one 8 x 8 block and the context culls, so segment 0 may use the block's cone; false: never a cone.
struct SqShade {
    using Segment = ShadeNoSegment;
    const RayQueryArgs &qa;
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave
    bool cone;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t k, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, k == 0u && cone, MAX_T, best_t, best);
    }
    __device__ __forceinline__ Segment segment(bool, const D3 &) const { return Segment{}; }
    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void occluded(const Segment &, uint32_t lane, const DevLight &, const D3 &so, const D3 &sd, bool use, double max_t, int &blocked) const
    {
        double unused_t = INFINITY;
        sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, use, false, max_t, unused_t, blocked);
    }
    __device__ __forceinline__ void first_hit(int, double, const D3 &, const D3 &) const {}
};

} // namespace RT_SYM(rtk)

#endif
