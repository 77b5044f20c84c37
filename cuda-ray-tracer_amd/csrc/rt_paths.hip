// rt_paths.hip -- the hits along a ray's mirror bounces, and the context's own primary rays as explicit rays (include/mi355rt.h,
// rt_trace_paths / rt_primary_rays / rt_pick_paths).
//
// A path is the geometry of the reference's render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d of a ray the
// caller hands in, minus everything that concerns colour: nearest hit, normal_vector, the reflection-ratio test, reflect_ray and the
// bias step, until a hit is no mirror, a bounce leaves the scene or the scene's max_reflections is reached.  It is shade_rays_kernel
// (rt_shade_rays.hip) without its light loops, and it writes down what it met.  Compiled twice like rt_rays.hip (-DRT_VARIANT=strict
// -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The object loops are the ray queries' (rt_rayquery.hpp): the class
// tables where they are proven for the ray in hand -- decided anew for every bounce, whose origin and direction the kernel forms itself
// -- and the dense expansion elsewhere.
// The path kernel reads the scene blob and the caller's rays; the primary-ray kernel reads the camera-plane tables.  Neither touches
// tile words, launch-order generations, census, counters or frame tag -- both are invisible to rt_render.
// The path kernel's body is rk_path_query (rt_ray_kernels.hpp), which the streamed and the culled twin run too;
// this file says where the tables are: all of them in the workgroup's LDS (RqStaged, rt_rayquery.hpp).
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_ray_kernels.hpp" // the path kernel's body (rk_path_query); RayQueryArgs, the class tables in LDS and RqStaged (rt_rayquery.hpp)

namespace RT_SYM(rtk) {

// rk_path_query over all class tables in LDS: they go there once per workgroup
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void path_query_kernel(const PathArgs pa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                         RqRecord *__restrict__ out_seg, RqRecord *__restrict__ out_last, PathEnd *__restrict__ out_end)
{
    extern __shared__ __align__(16) unsigned char smem[];
    RqStaged q{pa.qa, rq_stage_tables(pa.qa, scene, smem), reinterpret_cast<const DevObject *>(scene)};
    rk_path_query<HAS_GQ, HAS_CUBIC>(pa, scene, rays, out_seg, out_last, out_end, q);
}

// The context's own primary rays as rt_ray records: o = the frame's ray origin, d = primary_dir_tab of the pixel on the context's
// camera-plane tables -- the very function and tables of the render, G-buffer and pick kernels.  xy == NULL: the pixels of the rectangle
// x0 .. x0 + w - 1, y0 .. (GLOBAL rows), row-major from row y0; else n pixels by GLOBAL coordinates xy[2 * i], xy[2 * i + 1].
__global__ __launch_bounds__(256) void primary_rays_kernel(const FrameArgs fa, const double *__restrict__ camx, const double *__restrict__ camy,
                                                           const uint32_t *__restrict__ xy, uint32_t x0, uint32_t y0, uint32_t w, uint64_t n, RqRay *__restrict__ out)
{
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        uint32_t col, row; // (validated by the host: col < width, row < height)
        if (xy) {
            col = xy[2u * i];
            row = xy[2u * i + 1u];
        } else {
            col = x0 + (uint32_t) (i % w);
            row = y0 + (uint32_t) (i / w);
        }
        const D3 dir = primary_dir_tab(fa, camx[col], camy[row]);
        double2 *dst = reinterpret_cast<double2 *>(out + i); // three 16-byte stores
        dst[0] = double2{fa.origin[0], fa.origin[1]};
        dst[1] = double2{fa.origin[2], dir.x};
        dst[2] = double2{dir.y, dir.z};
    }
}

} // namespace RT_SYM(rtk)

// rays = n rt_ray, segments = [max_segments][n] rt_hit (NULL iff max_segments == 0), last = n rt_hit or NULL, ends = n rt_path_end, all
// in device memory and 16-byte aligned; at most max_grid workgroups.  The scene must fit the LDS limit (rt_rays_lds_bytes).
extern "C" hipError_t RT_SYM(rt_launch_trace_paths)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments,
                                                     void *last, void *ends, uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    const PathArgs pa = rk_path_args(fa, n, max_segments);
    RK_LAUNCH(fa, (path_query_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), pa.qa.tab_bytes, stream, pa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), reinterpret_cast<RqRecord *>(segments), reinterpret_cast<RqRecord *>(last), reinterpret_cast<PathEnd *>(ends));
    return hipGetLastError();
}

// fa = the frame arguments with this call's camera and origin (rtf::frame_origin).  xy == NULL: rect = x0, y0, x1, y1 (inclusive, inside
// the image, validated by the caller) -> (y1 - y0 + 1) * (x1 - x0 + 1) rt_ray; else n_list pixels -> n_list rt_ray.  out in device
// memory, 16-byte aligned; at most max_grid workgroups.
extern "C" hipError_t RT_SYM(rt_launch_primary_rays)(const FrameArgs *fa, const double *camx, const double *camy, const uint32_t *rect, const uint32_t *xy,
                                                      uint32_t n_list, void *out, uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    const uint32_t w = xy ? 1u : rect[2] - rect[0] + 1u;
    const uint64_t n = xy ? (uint64_t) n_list : (uint64_t) w * (rect[3] - rect[1] + 1u);
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(primary_rays_kernel, rk_ray_grid(n, max_grid), dim3(256), 0, stream, *fa, camx, camy, xy, xy ? 0u : rect[0], xy ? 0u : rect[1], w, n, reinterpret_cast<RqRay *>(out));
    return hipGetLastError();
}
