// rt_rays.hip -- ray queries for gfx950: closest hit and occlusion of caller-supplied rays (include/mi355rt.h, rt_trace_rays /
// rt_occluded_rays).
//
// What does THIS ray hit: the reference's nearest-hit loop (src/update-cpu.cpp:50-56) and its shadow loop (src/update-cpu.cpp:66-72) for
// rays the caller hands in, origin and direction per ray, the direction used exactly as given.  Compiled twice like rt_gbuffer.hip
// (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The arithmetic and the exact work removal come from
// the headers the render kernels use (rt_math.hpp, rt_wavefront_math.hpp); nothing of the render kernels' schedule applies: the rays
// of a wave are unrelated, so there is no cone, no chunk, no record per light.
// The kernel reads the scene blob and the caller's rays and writes the caller's records / flags: no camera tables, tile words,
// launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_rayquery.hpp" // RayQueryArgs, the class tables in LDS, rq_tables / rq_plain, the ray and record layouts

namespace RT_SYM(rtk) {

// 256-thread workgroups, one ray per lane, a grid-stride loop over the rays (the grid is bounded by the launcher); the class tables go
// to LDS once per workgroup.  Closest hit: one rt_hit per ray.  OCCLUSION: one int32 per ray (t_max == NULL: MAX_T for every ray).
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_kernel(const RayQueryArgs qa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                        const double *__restrict__ t_max, RqRecord *__restrict__ out_rec, int32_t *__restrict__ out_blocked)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x;
    const RqTables S = rq_stage_tables(qa, scene, smem);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (wave-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
        double tm = MAX_T;
        if (live) {
            const double2 *w = reinterpret_cast<const double2 *>(rays + i); // three 16-byte loads
            const double2 w0 = w[0], w1 = w[1], w2 = w[2];
            o = D3{w0.x, w0.y, w1.x};
            d = D3{w1.y, w2.x, w2.y};
            if (OCCLUSION && t_max) tm = t_max[i];
        }
        const bool proven = rq_tables_proven(o, d);
        Mono m;
        mono_set_o<NEED_CROSS>(m, o);
        mono_set_d<NEED_CROSS>(m, d);
        mono_set_od<NEED_CROSS>(m);
        double best_t = INFINITY;
        int best = OCCLUSION ? 0 : -1;
        rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, live && proven, tm, best_t, best);
        if (__ballot(live && !proven) != 0ull) rq_plain<OCCLUSION>(qa, gobj, o, d, live && !proven, tm, best_t, best);
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

template <bool OCCLUSION>
static hipError_t launch(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, n);
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    const dim3 g(need < max_grid ? need : (max_grid ? max_grid : 1u)), block(256);
    const size_t lds = qa.tab_bytes;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    RqRecord *rec = OCCLUSION ? nullptr : reinterpret_cast<RqRecord *>(out);
    int32_t *blk = OCCLUSION ? reinterpret_cast<int32_t *>(out) : nullptr;
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((ray_query_kernel<true, true, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
        else hipLaunchKernelGGL((ray_query_kernel<false, true, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((ray_query_kernel<true, false, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
        else hipLaunchKernelGGL((ray_query_kernel<false, false, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
    }
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// LDS bytes of one ray_query_kernel workgroup for this scene (the entry points refuse scenes beyond the device's limit)
extern "C" size_t RT_SYM(rt_rays_lds_bytes)(const FrameArgs *fa) { return (size_t) (fa->off_mat - fa->off_us); }

// rays = n rt_ray, out = n rt_hit, both in device memory and 16-byte aligned; at most max_grid workgroups
extern "C" hipError_t RT_SYM(rt_launch_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<false>(fa, scene, rays, nullptr, n, out, max_grid, stream);
}

// t_max = n doubles or NULL (MAX_T for every ray), out = n int32
extern "C" hipError_t RT_SYM(rt_launch_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                       uint32_t max_grid, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<true>(fa, scene, rays, t_max, n, out, max_grid, stream);
}
