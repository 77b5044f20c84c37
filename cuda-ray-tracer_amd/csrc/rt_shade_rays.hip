// rt_shade_rays.hip -- the reference's colour for caller-supplied rays (include/mi355rt.h, rt_shade_rays).
//
// render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d of a ray the caller hands in, the direction used exactly as
// given: nearest hit, every light's shadow test and surface_color, the clamp, then the reflection loop with its blends -- the shading
// loop this kernel shares with the streamed kernels (rt_stream_shade.hpp: shade_loop), under the policy RkShade over the query object
// RqStaged (rt_ray_kernels.hpp: rk_shade_rays, the body the streamed and the culled twin run too).  Compiled
// twice like rt_rays.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The object loops are the ray
// queries' (rt_rayquery.hpp): the class tables where they are proven for the ray in hand -- decided anew for every shadow ray and every
// bounce, whose origins and directions the kernel forms itself -- and the dense expansion elsewhere.  None of the render kernels' work
// removal is used (facing-away skip, own-sphere rule, bounding-volume culling): their proofs lean on a pixel grid's rays, finite
// lights and colours, and a normalised direction.
// The kernel reads the scene blob, the lights and the caller's rays and writes the caller's pixels / records: no camera tables, tile
// words, launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_ray_kernels.hpp" // the kernel's body (rk_shade_rays) around the shading loop; RayQueryArgs, the class tables in LDS and RqStaged (rt_rayquery.hpp)

namespace RT_SYM(rtk) {

// rk_shade_rays over all class tables in LDS: they go there once per workgroup
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_kernel(const ShadeRaysArgs sa, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                                         const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba, RqRecord *__restrict__ out_rec)
{
    extern __shared__ __align__(16) unsigned char smem[];
    RqStaged q{sa.qa, rq_stage_tables(sa.qa, scene, smem), reinterpret_cast<const DevObject *>(scene)};
    rk_shade_rays<HAS_GQ, HAS_CUBIC>(sa, scene, lights, rays, out_rgba, out_rec, q);
}

} // namespace RT_SYM(rtk)

// rays = n rt_ray, rgba = n x 4 float32, hits = n rt_hit or NULL, all in device memory and 16-byte aligned; lights = the context's
// DevLight array; at most max_grid workgroups.  The scene must fit the LDS limit (rt_rays_lds_bytes).
extern "C" hipError_t RT_SYM(rt_launch_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba, void *hits,
                                                    uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    const ShadeRaysArgs sa = rk_shade_args(fa, n);
    RK_LAUNCH(fa, (shade_rays_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), sa.qa.tab_bytes, stream, sa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const DevLight *>(lights), reinterpret_cast<const RqRay *>(rays), reinterpret_cast<float4 *>(rgba), reinterpret_cast<RqRecord *>(hits));
    return hipGetLastError();
}
