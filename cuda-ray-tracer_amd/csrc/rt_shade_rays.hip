// rt_shade_rays.hip -- the reference's colour for caller-supplied rays (include/mi355rt.h, rt_shade_rays).
//
// render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d of a ray the caller hands in, the direction used exactly as
// given: nearest hit, every light's shadow test and surface_color, the clamp, then the reflection loop with its blends.  Compiled
// twice like rt_rays.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The object loops are the ray
// queries' (rt_rayquery.hpp): the class tables where they are proven for the ray in hand -- decided anew for every shadow ray and every
// bounce, whose origins and directions the kernel forms itself -- and the dense expansion elsewhere.  None of the render kernels' work
// removal is used (facing-away skip, own-sphere rule, bounding-volume culling): their proofs lean on a pixel grid's rays, finite
// lights and colours, and a normalised direction.
// The kernel reads the scene blob, the lights and the caller's rays and writes the caller's pixels / records: no camera tables, tile
// words, launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_rayquery.hpp" // RayQueryArgs, the class tables in LDS, rq_tables / rq_plain, the ray and record layouts

namespace RT_SYM(rtk) {

// One object loop for the ray (o, d) of every lane in `use`: through the tables where rq_tables_proven says so, the plain path for
// the other lanes.  OCCLUSION: best = 1 once something blocks before t_max.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__device__ __forceinline__ void shade_query(const RayQueryArgs &qa, const RqTables &S, const DevObject *__restrict__ gobj, const D3 &o, const D3 &d, bool use, double t_max,
                                            double &best_t, int &best)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, use && proven, t_max, best_t, best);
    if (__ballot(use && !proven) != 0ull) rq_plain<OCCLUSION>(qa, gobj, o, d, use && !proven, t_max, best_t, best);
}

// 256-thread workgroups, one ray per lane, the grid-stride loop of ray_query_kernel; the class tables go to LDS once per workgroup.
// Per ray one bounce loop for the whole wave: iteration k traces the k-th segment of every lane that is still bouncing (all such
// lanes have bounced exactly k times, so the reference's `cur_reflections` is the wave-uniform k).  out_rec != NULL: the rt_hit of
// segment 0, as rt_trace_rays writes it.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_kernel(const ShadeRaysArgs sa, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                                         const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba, RqRecord *__restrict__ out_rec)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const RayQueryArgs &qa = sa.qa;
    const uint32_t tid = threadIdx.x;
    const RqTables S = rq_stage_tables(qa, scene, smem);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const F3 bg{sa.bg[0], sa.bg[1], sa.bg[2]};

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (wave-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
        if (live) {
            const double2 *w = reinterpret_cast<const double2 *>(rays + i); // three 16-byte loads
            const double2 w0 = w[0], w1 = w[1], w2 = w[2];
            o = D3{w0.x, w0.y, w1.x};
            d = D3{w1.y, w2.x, w2.y};
        }
        F3 res = bg; // a first-segment miss is the background colour
        float cur_ratio = 1.0f;
        bool bouncing = live;
        for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++) {
            // get_color_and_object, src/update-cpu.cpp:45-80: the nearest hit ...
            double best_t = INFINITY;
            int best = -1;
            shade_query<HAS_GQ, HAS_CUBIC, false>(qa, S, gobj, o, d, bouncing, MAX_T, best_t, best);
            const bool hit = bouncing && best >= 0;
            const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
            D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
            if (hit) {
                sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                sn = normal_vector(bo->c, sp); // all twenty coefficients, as rt_rays.hip; FP64, never flipped
            }
            if (k == 0u && out_rec && live) rq_store_record(out_rec + i, best, best_t, sp, sn);
            // ... every light in index order (wave-uniform: scalar loads), shadow_ray from sp + SHADOW_BIAS * sn.  The shadow ray is a ray
            // the kernel formed: sp can lie beyond the tables' proven range and sn can be NaN, so shade_query decides again.
            const D3 so{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
            F3 acc{0.0f, 0.0f, 0.0f};
            if (__ballot(hit) != 0ull) {
                const F3 albedo{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
                for (uint32_t l = 0; l < sa.n_lights; l++) {
                    const DevLight *lt = &lights[l];
                    const bool spherical = lt->spherical != 0;
                    double max_t;
                    const D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
                    double unused_t = INFINITY;
                    int blocked = 0;
                    shade_query<HAS_GQ, HAS_CUBIC, true>(qa, S, gobj, so, sd, hit, max_t, unused_t, blocked);
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
                        if (k == sa.max_refl) {
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
        if (live) out_rgba[i] = float4{res.x, res.y, res.z, 1.0f}; // one 16-byte store
    }
}

} // namespace RT_SYM(rtk)

// rays = n rt_ray, rgba = n x 4 float32, hits = n rt_hit or NULL, all in device memory and 16-byte aligned; lights = the context's
// DevLight array; at most max_grid workgroups.  The scene must fit the LDS limit (rt_rays_lds_bytes).
extern "C" hipError_t RT_SYM(rt_launch_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba, void *hits,
                                                    uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    ShadeRaysArgs sa;
    sa.qa = rq_args(fa, n);
    sa.n_lights = fa->n_lights;
    sa.max_refl = fa->max_refl;
    sa.bg[0] = fa->bg[0]; sa.bg[1] = fa->bg[1]; sa.bg[2] = fa->bg[2];
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    const dim3 g(need < max_grid ? need : (max_grid ? max_grid : 1u)), block(256);
    const size_t lds = sa.qa.tab_bytes;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    float4 *px = reinterpret_cast<float4 *>(rgba);
    RqRecord *rec = reinterpret_cast<RqRecord *>(hits);
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((shade_rays_kernel<true, true>), g, block, lds, stream, sa, s, lt, r, px, rec);
        else hipLaunchKernelGGL((shade_rays_kernel<false, true>), g, block, lds, stream, sa, s, lt, r, px, rec);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((shade_rays_kernel<true, false>), g, block, lds, stream, sa, s, lt, r, px, rec);
        else hipLaunchKernelGGL((shade_rays_kernel<false, false>), g, block, lds, stream, sa, s, lt, r, px, rec);
    }
    return hipGetLastError();
}
