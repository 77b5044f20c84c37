// rt_stream_cull_rays.hip -- the streamed ray queries with whole chunks of the unit-sphere table culled per ray: rt_trace_rays,
// rt_occluded_rays, rt_shade_rays, rt_trace_paths (and rt_pick_paths and the _host forms through them) of a context whose
// RT_FLAG_STREAM_CULL_RAYS decision is true (include/mi355rt.h, "Culled ray queries").
//
// Every kernel here is the twin of a kernel of rt_stream_queries.hip -- body, launch bounds, grid, loads and stores -- and differs from it in
// one thing: a query is sc_query_ray (rt_stream_cull_rays.hpp: sc_query_bounce's loop for the nearest hit and for occlusion) instead of
// sq_query's full sweep of the unit-sphere table.  Every lane asks rtm::ray_reaches about its own ray and each
// chunk bound, the wave stages a chunk only if some lane in use reaches it, and sweeps it for those lanes alone.  No dropped object's root
// could have been accepted and the acceptance rule does not depend on the order, so every output is the twin's bit for bit.
// The ray loader and the grid are rt_stream_queries.hip's, restated: that file stays as it is.
// Compiled twice like rt_stream_queries.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot or staged chunk: a lane without
// work stays with `use = false`.  Every kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS.  The work words (rt_debug_stream_cull_rays) are kept
// per wave in scalars behind a wave-uniform test and added with one vector atomic per word at the wave's end.
#include <hip/hip_runtime.h>
#include "rt_launch.h"              // the launchers below, as the host sees them
#include "rt_stream_cull_rays.hpp"  // sc_query_ray and ScRayShade

namespace RT_SYM(rtk) {

// one caller-supplied ray per lane: three 16-byte loads (lanes without a ray keep zeroes)
__device__ __forceinline__ void scr_load_ray(const RqRay *__restrict__ rays, uint64_t i, bool live, D3 &o, D3 &d)
{
    o = D3{0.0, 0.0, 0.0};
    d = D3{0.0, 0.0, 0.0};
    if (live) {
        const double2 *w = reinterpret_cast<const double2 *>(rays + i);
        const double2 w0 = w[0], w1 = w[1], w2 = w[2];
        o = D3{w0.x, w0.y, w1.x};
        d = D3{w1.y, w2.x, w2.y};
    }
}

// ---- closest hit and occlusion (ray_query_stream_kernel) ---------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_cull_kernel(const RayQueryArgs qa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                             const RqRay *__restrict__ rays, const double *__restrict__ t_max, RqRecord *__restrict__ out_rec,
                                                             int32_t *__restrict__ out_blocked)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const bool count = ca.stats != nullptr;
    ScBounceStats bs{false, {0u, 0u, 0u, 0u, 0u}};

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (workgroup-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        scr_load_ray(rays, i, live, o, d);
        double tm = MAX_T;
        if (OCCLUSION && t_max && live) tm = t_max[i];
        double best_t = INFINITY;
        int best = OCCLUSION ? 0 : -1;
        bs.on = count && __ballot(live) != 0ull; // (wave-uniform) a wave without a ray asks nothing and counts nothing
        sc_query_ray<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, ca, scene, slice, lane, o, d, live, tm, best_t, best, bs);
        if (OCCLUSION) {
            if (live) out_blocked[i] = best;
        } else if (live) {
            D3 p{0.0, 0.0, 0.0}, nv{0.0, 0.0, 0.0};
            if (best >= 0) {
                p = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                nv = normal_vector(gobj[best].c, p); // in full for every class, as ray_query_kernel
            }
            rq_store_record(out_rec + i, best, best_t, p, nv);
        }
    }
    if (count) sc_flush(bs.w, ca.stats, lane);
}

// ---- colour (shade_rays_stream_kernel) -----------------------------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_cull_kernel(const ShadeRaysArgs sa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                              const DevLight *__restrict__ lights, const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba,
                                                              RqRecord *__restrict__ out_rec)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const RayQueryArgs &qa = sa.qa;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES;
    ScBounceStats bs{ca.stats != nullptr, {0u, 0u, 0u, 0u, 0u}};

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (workgroup-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        scr_load_ray(rays, i, live, o, d);
        ScRayShade pol{qa, ca, scene, slice, bs, out_rec, i, live};
        const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(sa, scene, lights, lane, pol, o, d, live); // (queries only while a lane is in use)
        if (live) out_rgba[i] = float4{res.x, res.y, res.z, 1.0f}; // one 16-byte store
    }
    if (bs.on) sc_flush(bs.w, ca.stats, lane);
}

// ---- paths (path_query_stream_kernel) ------------------------------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void path_query_cull_kernel(const PathArgs pa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                              const RqRay *__restrict__ rays, RqRecord *__restrict__ out_seg, RqRecord *__restrict__ out_last,
                                                              PathEnd *__restrict__ out_end)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const RayQueryArgs &qa = pa.qa;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES;
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    ScBounceStats bs{ca.stats != nullptr, {0u, 0u, 0u, 0u, 0u}};

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (workgroup-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        scr_load_ray(rays, i, live, o, d);
        float cur_ratio = 1.0f;
        uint32_t segments = 0u, end = PATH_MISS;
        int last = -1; // the last hit: what out_last receives
        double last_t = INFINITY;
        D3 last_p{0.0, 0.0, 0.0}, last_n{0.0, 0.0, 0.0};
        bool bouncing = live;
        uint32_t k = 0;
        for (; __ballot(bouncing) != 0ull; k++) {
            // the nearest hit of segment k: every lane its own ray, the first segment included
            double best_t = INFINITY;
            int best = -1;
            sc_query_ray<HAS_GQ, HAS_CUBIC, false>(qa, ca, scene, slice, lane, o, d, bouncing, MAX_T, best_t, best, bs);
            const bool hit = bouncing && best >= 0;
            const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
            D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
            if (hit) {
                sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                sn = normal_vector(bo->c, sp);
            }
            if (k < pa.max_segments && live) rq_store_record(out_seg + ((uint64_t) k * qa.n + i), hit ? best : -1, best_t, sp, sn);
            if (bouncing) {
                if (!hit) {
                    end = (k == 0u) ? PATH_MISS : PATH_ESCAPED;
                    bouncing = false;
                } else {
                    segments = k + 1u;
                    last = best;
                    last_t = best_t;
                    last_p = sp;
                    last_n = sn;
                    // path_query_stream_kernel's bounce step (the reference's reflections, src/update-cpu.cpp:96-117)
                    const float refl = bo->refl;
                    if (!((double) refl > EPS)) {
                        end = PATH_SURFACE;
                        bouncing = false;
                    } else {
                        cur_ratio *= refl;
                        if (k == pa.max_refl) {
                            end = PATH_CAP;
                            bouncing = false;
                        } else {
                            d = reflect_ray(d, sn); // of the direction as it is
                            o = D3{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
                        }
                    }
                }
            }
        }
        if (live) {
            const D3 zero{0.0, 0.0, 0.0};
            for (; k < pa.max_segments; k++) rq_store_record(out_seg + ((uint64_t) k * qa.n + i), -1, INFINITY, zero, zero); // planes no lane of the wave reached
            if (out_last) rq_store_record(out_last + i, last, last_t, last_p, last_n);
            out_end[i] = PathEnd{segments, end, cur_ratio, last}; // one 16-byte store
        }
    }
    if (bs.on) sc_flush(bs.w, ca.stats, lane);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
static inline dim3 scr_ray_grid(uint32_t n, uint32_t max_grid)
{
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    return dim3(need < max_grid ? need : (max_grid ? max_grid : 1u));
}

// the chunk bounds as the kernels take them; false: they do not belong to this scene's table
static inline bool scr_cull_args(const FrameArgs *fa, const void *bounds, uint32_t n_chunks, unsigned long long *stats, StreamCullArgs &ca)
{
    if (n_chunks != (fa->n_us + SQ_CHUNK - 1u) / SQ_CHUNK || (n_chunks && !bounds)) return false;
    ca = StreamCullArgs{reinterpret_cast<const UsEntry *>(bounds), stats, n_chunks, 0u};
    return true;
}

// launch kernel<HAS_GQ, HAS_CUBIC, extra...> for the scene's classes (rt_rayquery.hpp: rq_for_classes)
#define SCR_LAUNCH(fa, kernel, extra, g, stream, ...) \
    rq_for_classes(fa, [&](auto gq, auto cub) { hipLaunchKernelGGL((kernel<decltype(gq)::value, decltype(cub)::value extra>), g, dim3(256), 0, stream, __VA_ARGS__); })
#define SCR_COMMA ,

} // namespace RT_SYM(rtk)

// The streamed launchers' arguments (rt_stream_queries.hip), and: the chunk bounds ([n_chunks] UsEntry, n_chunks = ceil(n_us / 64)) and the
// work words to add to (8, the kernels write the first five; or NULL).  A launch is the same number of graph nodes as its twin's.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid,
                                                                const void *bounds, uint32_t n_chunks, unsigned long long *stats, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!scr_cull_args(fa, bounds, n_chunks, stats, ca)) return hipErrorInvalidValue;
    const RayQueryArgs qa = rq_args(fa, n);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    SCR_LAUNCH(fa, ray_query_cull_kernel, SCR_COMMA false, scr_ray_grid(n, max_grid), stream, qa, ca, s, r, (const double *) nullptr, reinterpret_cast<RqRecord *>(out),
               (int32_t *) nullptr);
    return hipGetLastError();
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                                   uint32_t max_grid, const void *bounds, uint32_t n_chunks, unsigned long long *stats,
                                                                   hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!scr_cull_args(fa, bounds, n_chunks, stats, ca)) return hipErrorInvalidValue;
    const RayQueryArgs qa = rq_args(fa, n);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    SCR_LAUNCH(fa, ray_query_cull_kernel, SCR_COMMA true, scr_ray_grid(n, max_grid), stream, qa, ca, s, r, t_max, (RqRecord *) nullptr, out);
    return hipGetLastError();
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba,
                                                                void *hits, uint32_t max_grid, const void *bounds, uint32_t n_chunks, unsigned long long *stats,
                                                                hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!scr_cull_args(fa, bounds, n_chunks, stats, ca)) return hipErrorInvalidValue;
    ShadeRaysArgs sa;
    sa.qa = rq_args(fa, n);
    sa.n_lights = fa->n_lights;
    sa.max_refl = fa->max_refl;
    sa.bg[0] = fa->bg[0]; sa.bg[1] = fa->bg[1]; sa.bg[2] = fa->bg[2];
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    SCR_LAUNCH(fa, shade_rays_cull_kernel, , scr_ray_grid(n, max_grid), stream, sa, ca, s, lt, r, reinterpret_cast<float4 *>(rgba), reinterpret_cast<RqRecord *>(hits));
    return hipGetLastError();
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_trace_paths)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments,
                                                                 void *last, void *ends, uint32_t max_grid, const void *bounds, uint32_t n_chunks,
                                                                 unsigned long long *stats, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!scr_cull_args(fa, bounds, n_chunks, stats, ca)) return hipErrorInvalidValue;
    PathArgs pa;
    pa.qa = rq_args(fa, n);
    pa.max_refl = fa->max_refl;
    pa.max_segments = max_segments;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    SCR_LAUNCH(fa, path_query_cull_kernel, , scr_ray_grid(n, max_grid), stream, pa, ca, s, r, reinterpret_cast<RqRecord *>(segments), reinterpret_cast<RqRecord *>(last),
               reinterpret_cast<PathEnd *>(ends));
    return hipGetLastError();
}
