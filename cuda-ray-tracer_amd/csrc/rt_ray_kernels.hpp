// rt_ray_kernels.hpp -- the kernels for caller-supplied rays, once: what rt_trace_rays / rt_occluded_rays, rt_shade_rays and
// rt_trace_paths do with a ray is the same whichever way the context reads the class tables.  The nine kernels
// -- staged (rt_rays.hip, rt_shade_rays.hip, rt_paths.hip), streamed (rt_stream_queries.hip), culled (rt_stream_cull_rays.hip) -- take
// their LDS, build a query object and call one of the three bodies here (but path_query_stream_kernel, which keeps rk_path_query's text:
// see there).  A query object offers one call,
//   query<HAS_GQ, HAS_CUBIC, OCCLUSION>(lane, o, d, use, t_max, best_t, best)
// the object loop for the ray (o, d) of every lane in `use` (OCCLUSION: best = 1 once something blocks before t_max), and nothing else:
//   RqStaged    rt_rayquery.hpp          all class tables in the workgroup's LDS (rq_tables), the plain path elsewhere
//   SqQuery     rt_stream.hpp            sq_query without a cone: the tables through the wave's slice
//   ScRayQuery  rt_stream_cull_rays.hpp  sc_query_ray, and the wave's work words
// The wave-level rules are rt_stream_shade.hpp's: all 64 lanes call; `use` is a predicate; no lane leaves before the wave's last
// ballot, readlane or staged chunk; nothing here is workgroup-wide.  LDS and whatever fills it are the kernels' business.
// The bodies' pointer parameters carry no restrict: the kernels' own parameters do, and with it on both the compiler orders the colour
// kernels' code differently ("Shapes").
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_RAY_KERNELS_HPP
#define RT_RAY_KERNELS_HPP

#include <hip/hip_runtime.h>

#include "rt_stream_shade.hpp" // shade_loop; RayQueryArgs, the ray and record layouts (rt_rayquery.hpp)

namespace RT_SYM(rtk) {

// one caller-supplied ray per lane: three 16-byte loads (lanes without a ray keep zeroes)
__device__ __forceinline__ void rk_load_ray(const RqRay *__restrict__ rays, uint64_t i, bool live, D3 &o, D3 &d)
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

// ---- closest hit and occlusion ---------------------------------------------------------------------------------------------------------------
// 256-thread workgroups, one ray per lane, a grid-stride loop over the rays (the grid is bounded by the launcher; the trip count is
// workgroup-uniform).  Closest hit: one rt_hit per ray.  OCCLUSION: one int32 per ray (t_max == NULL: MAX_T for every ray).
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION, typename Query>
__device__ __forceinline__ void rk_ray_query(const RayQueryArgs &qa, const unsigned char *scene, const RqRay *rays,
                                             const double *t_max, RqRecord *out_rec, int32_t *out_blocked, Query &q)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) {
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        rk_load_ray(rays, i, live, o, d);
        double tm = MAX_T;
        if (OCCLUSION && t_max && live) tm = t_max[i];
        double best_t = INFINITY;
        int best = OCCLUSION ? 0 : -1;
        q.template query<HAS_GQ, HAS_CUBIC, OCCLUSION>(lane, o, d, live, tm, best_t, best);
        if (OCCLUSION) {
            if (live) out_blocked[i] = best;
        } else if (live) {
            D3 p{0.0, 0.0, 0.0}, nv{0.0, 0.0, 0.0};
            if (best >= 0) {
                p = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                // normal_vector in full for every class (per-lane index: a gather from global memory, per hit): the three-coefficient form
                // of a sphere differs in the sign of a zero component when the hit point has a negative-zero coordinate, which a caller's
                // origin can have
                nv = normal_vector(gobj[best].c, p);
            }
            rq_store_record(out_rec + i, best, best_t, p, nv);
        }
    }
}

// ---- paths ---------------------------------------------------------------------------------------------------------------------------------
// The grid-stride loop of rk_ray_query.  Per ray one bounce loop for the whole wave: iteration k traces segment k of every lane that is
// still bouncing, and every lane with a ray -- done or not -- stores its record of plane k while k < max_segments (a lane that is done
// stores the miss record), so the wave's stores of one iteration are consecutive 48-byte records: out_seg is segment-major, record
// k * n + i.  max_segments only limits what is stored; the path is followed to its end.  out_last (may be NULL): the hit of the last
// segment.  out_end: one record per ray.
template <bool HAS_GQ, bool HAS_CUBIC, typename Query>
__device__ __forceinline__ void rk_path_query(const PathArgs &pa, const unsigned char *scene, const RqRay *rays, RqRecord *out_seg,
                                              RqRecord *out_last, PathEnd *out_end, Query &q)
{
    const RayQueryArgs &qa = pa.qa;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) {
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        rk_load_ray(rays, i, live, o, d);
        float cur_ratio = 1.0f;
        uint32_t segments = 0u, end = PATH_MISS;
        int last = -1; // the last hit: what out_last receives
        double last_t = INFINITY;
        D3 last_p{0.0, 0.0, 0.0}, last_n{0.0, 0.0, 0.0};
        bool bouncing = live;
        uint32_t k = 0;
        for (; __ballot(bouncing) != 0ull; k++) {
            // the nearest hit of segment k (src/update-cpu.cpp:50-56).  From the first bounce on the ray is one the kernel formed: sp can lie
            // beyond the tables' proven range and sn can be NaN, so the query decides for every segment
            double best_t = INFINITY;
            int best = -1;
            q.template query<HAS_GQ, HAS_CUBIC, false>(lane, o, d, bouncing, MAX_T, best_t, best);
            const bool hit = bouncing && best >= 0;
            const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
            D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
            if (hit) {
                sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                sn = normal_vector(bo->c, sp); // all twenty coefficients, as rk_ray_query; FP64, never flipped
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
                    // the reflection loop, src/update-cpu.cpp:96-117
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
}

// ---- colour ----------------------------------------------------------------------------------------------------------------------------------
// The shading policy (rt_stream_shade.hpp) of a wave of unrelated caller-supplied rays: every nearest hit and every shadow ray is the
// query's; segment 0 stores the rt_hit of the lane's ray, as rk_ray_query writes it (out_rec == NULL: nothing).
template <typename Query>
struct RkShade {
    using Segment = ShadeNoSegment;
    Query &q;
    RqRecord *out_rec;
    uint64_t i;
    bool live;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        q.template query<HAS_GQ, HAS_CUBIC, false>(lane, o, d, use, MAX_T, best_t, best);
    }
    __device__ __forceinline__ Segment segment(bool, const D3 &) const { return Segment{}; }
    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void occluded(const Segment &, uint32_t lane, const DevLight &, const D3 &so, const D3 &sd, bool use, double max_t, int &blocked) const
    {
        double unused_t = INFINITY;
        q.template query<HAS_GQ, HAS_CUBIC, true>(lane, so, sd, use, max_t, unused_t, blocked);
    }
    __device__ __forceinline__ void first_hit(int best, double best_t, const D3 &sp, const D3 &sn) const
    {
        if (out_rec && live) rq_store_record(out_rec + i, best, best_t, sp, sn);
    }
};

// The grid-stride loop of rk_ray_query around the shared shading loop: iteration k of shade_loop traces the k-th segment of every lane
// that is still bouncing.  out_rec != NULL: the rt_hit of segment 0.
template <bool HAS_GQ, bool HAS_CUBIC, typename Query>
__device__ __forceinline__ void rk_shade_rays(const ShadeRaysArgs &sa, const unsigned char *scene, const DevLight *lights,
                                              const RqRay *rays, float4 *out_rgba, RqRecord *out_rec, Query &q)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < sa.qa.n; first += stride) {
        const uint64_t i = first + tid;
        const bool live = i < sa.qa.n;
        D3 o, d;
        rk_load_ray(rays, i, live, o, d);
        RkShade<Query> pol{q, out_rec, i, live};
        const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(sa, scene, lights, lane, pol, o, d, live);
        if (live) out_rgba[i] = float4{res.x, res.y, res.z, 1.0f}; // one 16-byte store
    }
}

// ---- what the twelve launchers share -----------------------------------------------------------------------------------------------------------
// one workgroup per 256 rays, at most max_grid of them
static inline dim3 rk_ray_grid(uint64_t n, uint32_t max_grid)
{
    const uint64_t need = (n + 255u) / 256u;
    return dim3((uint32_t) (need < max_grid ? need : (max_grid ? max_grid : 1u)));
}

static inline ShadeRaysArgs rk_shade_args(const FrameArgs *fa, uint32_t n)
{
    ShadeRaysArgs sa;
    sa.qa = rq_args(fa, n);
    sa.n_lights = fa->n_lights;
    sa.max_refl = fa->max_refl;
    sa.bg[0] = fa->bg[0]; sa.bg[1] = fa->bg[1]; sa.bg[2] = fa->bg[2];
    return sa;
}

static inline PathArgs rk_path_args(const FrameArgs *fa, uint32_t n, uint32_t max_segments)
{
    PathArgs pa;
    pa.qa = rq_args(fa, n);
    pa.max_refl = fa->max_refl;
    pa.max_segments = max_segments;
    return pa;
}

} // namespace RT_SYM(rtk)

#endif
