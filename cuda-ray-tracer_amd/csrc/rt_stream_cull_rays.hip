// rt_stream_cull_rays.hip -- the streamed ray queries with whole chunks of the unit-sphere table culled per ray: rt_trace_rays,
// rt_occluded_rays, rt_shade_rays, rt_trace_paths (and rt_pick_paths and the _host forms through them) of a context whose
// RT_FLAG_STREAM_CULL_RAYS decision is true (include/mi355rt.h, "Culled ray queries").
//
// Every kernel here is the twin of a kernel of rt_stream_queries.hip and runs the very body that one runs (rt_ray_kernels.hpp; DESIGN.md
// section 30) -- launch bounds, grid, loads and stores with it -- over another query object: a query is sc_query_ray
// (rt_stream_cull_rays.hpp: sc_query_bounce's loop for the nearest hit and for occlusion) instead of
// sq_query's full sweep of the unit-sphere table.  Every lane asks rtm::ray_reaches about its own ray and each
// chunk bound, the wave stages a chunk only if some lane in use reaches it, and sweeps it for those lanes alone.  No dropped object's root
// could have been accepted and the acceptance rule does not depend on the order, so every output is the twin's bit for bit.
// Compiled twice like rt_stream_queries.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot or staged chunk: a lane without
// work stays with `use = false`.  Every kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS.  The work words (rt_debug_stream_cull_rays) are kept
// per wave in scalars behind a wave-uniform test and added with one vector atomic per word at the wave's end.
#include <hip/hip_runtime.h>
#include "rt_launch.h"              // the launchers below, as the host sees them
#include "rt_ray_kernels.hpp"       // the kernels' bodies
#include "rt_stream_cull_rays.hpp"  // sc_query_ray and ScRayQuery

namespace RT_SYM(rtk) {

// (the slice: this wave's quarter of the workgroup's LDS, never another's)
// ---- closest hit and occlusion (ray_query_stream_kernel) ---------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_cull_kernel(const RayQueryArgs qa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                             const RqRay *__restrict__ rays, const double *__restrict__ t_max, RqRecord *__restrict__ out_rec,
                                                             int32_t *__restrict__ out_blocked)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    ScRayQuery q{qa, ca, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, {false, {0u, 0u, 0u, 0u, 0u}}};
    rk_ray_query<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, rays, t_max, out_rec, out_blocked, q);
    if (ca.stats) sc_flush(q.bs.w, ca.stats, threadIdx.x & 63u);
}

// ---- colour (shade_rays_stream_kernel) -----------------------------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_cull_kernel(const ShadeRaysArgs sa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                              const DevLight *__restrict__ lights, const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba,
                                                              RqRecord *__restrict__ out_rec)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    ScRayQuery q{sa.qa, ca, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, {false, {0u, 0u, 0u, 0u, 0u}}};
    rk_shade_rays<HAS_GQ, HAS_CUBIC>(sa, scene, lights, rays, out_rgba, out_rec, q);
    if (ca.stats) sc_flush(q.bs.w, ca.stats, threadIdx.x & 63u);
}

// ---- paths (path_query_stream_kernel) ------------------------------------------------------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void path_query_cull_kernel(const PathArgs pa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                              const RqRay *__restrict__ rays, RqRecord *__restrict__ out_seg, RqRecord *__restrict__ out_last,
                                                              PathEnd *__restrict__ out_end)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    ScRayQuery q{pa.qa, ca, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, {false, {0u, 0u, 0u, 0u, 0u}}};
    rk_path_query<HAS_GQ, HAS_CUBIC>(pa, scene, rays, out_seg, out_last, out_end, q);
    if (ca.stats) sc_flush(q.bs.w, ca.stats, threadIdx.x & 63u);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
template <bool OCCLUSION>
static hipError_t scr_launch_rays(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, void *out, uint32_t max_grid,
                                  const ChunkTables *chunks, hipStream_t stream)
{
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    const RayQueryArgs qa = rq_args(fa, n);
    RK_LAUNCH(fa, (ray_query_cull_kernel<GQ, CUB, OCCLUSION>), rk_ray_grid(n, max_grid), 0, stream, qa, ca, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), t_max, OCCLUSION ? nullptr : reinterpret_cast<RqRecord *>(out), OCCLUSION ? reinterpret_cast<int32_t *>(out) : nullptr);
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// The streamed launchers' arguments (rt_stream_queries.hip), read: chunks = the context's chunk bounds and the work words to add to (8, the
// kernels write the first five; or NULL).  A launch is the same number of graph nodes as its twin's.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid,
                                                                const ChunkTables *chunks, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::scr_launch_rays<false>(fa, scene, rays, nullptr, n, out, max_grid, chunks, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                                   uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::scr_launch_rays<true>(fa, scene, rays, t_max, n, out, max_grid, chunks, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba,
                                                                void *hits, uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    const ShadeRaysArgs sa = rk_shade_args(fa, n);
    RK_LAUNCH(fa, (shade_rays_cull_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), 0, stream, sa, ca, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const DevLight *>(lights), reinterpret_cast<const RqRay *>(rays), reinterpret_cast<float4 *>(rgba), reinterpret_cast<RqRecord *>(hits));
    return hipGetLastError();
}

extern "C" hipError_t RT_SYM(rt_launch_stream_cull_trace_paths)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments,
                                                                 void *last, void *ends, uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    const PathArgs pa = rk_path_args(fa, n, max_segments);
    RK_LAUNCH(fa, (path_query_cull_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), 0, stream, pa, ca, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), reinterpret_cast<RqRecord *>(segments), reinterpret_cast<RqRecord *>(last), reinterpret_cast<PathEnd *>(ends));
    return hipGetLastError();
}
