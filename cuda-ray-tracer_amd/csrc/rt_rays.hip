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
// The kernel's body is rk_ray_query (rt_ray_kernels.hpp), which the streamed and the culled twin run too; this
// file says where the tables are: all of them in the workgroup's LDS (RqStaged, rt_rayquery.hpp).
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_ray_kernels.hpp" // the kernel's body (rk_ray_query); RayQueryArgs, the class tables in LDS and RqStaged (rt_rayquery.hpp)

namespace RT_SYM(rtk) {

// rk_ray_query over all class tables in LDS: they go there once per workgroup
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_kernel(const RayQueryArgs qa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                        const double *__restrict__ t_max, RqRecord *__restrict__ out_rec, int32_t *__restrict__ out_blocked)
{
    extern __shared__ __align__(16) unsigned char smem[];
    RqStaged q{qa, rq_stage_tables(qa, scene, smem), reinterpret_cast<const DevObject *>(scene)};
    rk_ray_query<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, rays, t_max, out_rec, out_blocked, q);
}

template <bool OCCLUSION>
static hipError_t launch(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, n);
    RK_LAUNCH(fa, (ray_query_kernel<GQ, CUB, OCCLUSION>), rk_ray_grid(n, max_grid), qa.tab_bytes, stream, qa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), t_max, OCCLUSION ? nullptr : reinterpret_cast<RqRecord *>(out), OCCLUSION ? reinterpret_cast<int32_t *>(out) : nullptr);
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// LDS bytes of one ray_query_kernel workgroup for this scene (the entry points refuse scenes beyond the device's limit)
extern "C" size_t RT_SYM(rt_rays_lds_bytes)(const FrameArgs *fa) { return (size_t) (fa->off_mat - fa->off_us); }

// rays = n rt_ray, out = n rt_hit, both in device memory and 16-byte aligned; at most max_grid workgroups
extern "C" hipError_t RT_SYM(rt_launch_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid,
                                                    const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<false>(fa, scene, rays, nullptr, n, out, max_grid, stream);
}

// t_max = n doubles or NULL (MAX_T for every ray), out = n int32
extern "C" hipError_t RT_SYM(rt_launch_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                       uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<true>(fa, scene, rays, t_max, n, out, max_grid, stream);
}
