// rt_gbuffer.hip -- the primary-hit G-buffer (object, depth, normal planes) and pixel picking for gfx950 (include/mi355rt.h,
// rt_render_gbuffer / rt_pick), and the same rays reduced per object (rt_object_extents; section 18; at the end).
//
// What is under a pixel: the nearest hit of its primary ray -- phase A of the wavefront kernel (rt_wavefront.hip) without anything
// behind it.  Compiled twice like rt_adaptive.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// The arithmetic and the exact work removal come from the headers the render kernels use (rt_math.hpp, rt_wavefront_math.hpp).
// The pass reads the scene blob and the camera-plane tables (both constant after rt_create) and writes the caller's planes: no tile
// words, launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
// The kernels' bodies are pk_gbuffer and pk_extents (rt_pixel_kernels.hpp), which the streamed twins run too;
// this file says where the tables are: all of them in the workgroup's LDS, with the host's degree-3 records behind them (RqPixels,
// rt_rayquery.hpp).
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_pixel_kernels.hpp" // the kernels' bodies; RqPixels, its staging and the launch ladder (rt_rayquery.hpp); the extent record (rt_extents.hpp)

namespace RT_SYM(rtk) {

// pk_gbuffer over all class tables in LDS: they go there once per workgroup in both launch modes
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void gbuffer_kernel(const FrameArgs fa, const unsigned char *__restrict__ scene, const double *__restrict__ camx,
                                                      const double *__restrict__ camy, int32_t *__restrict__ out_object, double *__restrict__ out_t,
                                                      float4 *__restrict__ out_normal, const uint32_t *__restrict__ xy, uint32_t n_query,
                                                      RqRecord *__restrict__ out_rec)
{
    extern __shared__ __align__(16) unsigned char smem[];
    RqPixels q = rq_stage_pixels<HAS_CUBIC>(fa, scene, smem);
    pk_gbuffer<HAS_GQ, HAS_CUBIC>(fa, scene, camx, camy, out_object, out_t, out_normal, xy, n_query, out_rec, q);
}

} // namespace RT_SYM(rtk)

// LDS bytes of one gbuffer_kernel workgroup for this scene (rt_render_gbuffer refuses scenes beyond the device's limit)
extern "C" size_t RT_SYM(rt_gbuffer_lds_bytes)(const FrameArgs *fa) { return (size_t) (fa->off_mat - fa->off_us) + (fa->n_cub ? RT_SYM(rtk)::RQ_PRIM_BYTES : 0u); }

namespace RT_SYM(rtk) {
static hipError_t launch(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, uint32_t grid, int32_t *out_object, double *out_t, float *out_normal,
                         const uint32_t *xy, uint32_t n, void *rec, hipStream_t stream)
{
    RK_LAUNCH(fa, (gbuffer_kernel<GQ, CUB>), dim3(grid), RT_SYM(rt_gbuffer_lds_bytes)(fa), stream, *fa, reinterpret_cast<const unsigned char *>(scene), camx, camy, out_object,
              out_t, reinterpret_cast<float4 *>(out_normal), xy, n, reinterpret_cast<RqRecord *>(rec));
    return hipGetLastError();
}
} // namespace RT_SYM(rtk)

// planes = [local_rows][width] each; any of them may be NULL
extern "C" hipError_t RT_SYM(rt_launch_gbuffer)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t,
                                                 float *out_normal, const ChunkTables *, hipStream_t stream)
{
    if (fa->n_tiles == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch(fa, scene, camx, camy, fa->n_tiles, out_object, out_t, out_normal, nullptr, 0u, nullptr, stream);
}

// xy = n coordinate pairs and out = n records (16-byte aligned), both in device memory: the planes' kernel in its picking mode
extern "C" hipError_t RT_SYM(rt_launch_pick)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *xy, uint32_t n, void *out,
                                              const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch(fa, scene, camx, camy, (n + 255u) / 256u, nullptr, nullptr, nullptr, xy, n, out, stream);
}

// ---- object extents (include/mi355rt.h, "Object extents") ------------------------------------------------------
namespace RT_SYM(rtk) {

EXT_INIT_KERNEL(extents_init_kernel)

// pk_extents over all class tables in LDS.  ea.lds_acc: one record per object in LDS behind the tables, into which the waves merge
// (ext_reduce_wave) and which the workgroup adds to `out` once, at its end; otherwise every wave updates `out` itself.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void extents_kernel(const FrameArgs fa, const ExtArgs ea, const unsigned char *__restrict__ scene, const double *__restrict__ camx,
                                                      const double *__restrict__ camy, ExtRecord *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ExtRecord *acc = ea.lds_acc ? reinterpret_cast<ExtRecord *>(smem + (fa.off_mat - fa.off_us) + (HAS_CUBIC ? RQ_PRIM_BYTES : 0u)) : nullptr;
    RqPixels q = rq_stage_pixels<HAS_CUBIC>(fa, scene, smem);
    if (acc) { // (behind the staging, with a barrier of their own: in front of it the kernel was up to 4 % slower)
        for (uint32_t i = threadIdx.x; i < fa.n_obj; i += 256u) acc[i] = ext_identity();
        __syncthreads();
    }
    pk_extents<HAS_GQ, HAS_CUBIC>(fa, ea, camx, camy, out, acc, q);
    if (acc) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < fa.n_obj; i += 256u) {
            const ExtRecord a = acc[i];
            if (a.pixels) ext_merge<__HIP_MEMORY_SCOPE_AGENT>(out + i, a.pixels, a.x_min, a.y_min, a.x_max, a.y_max, a.t_min, a.t_max);
        }
    }
}

} // namespace RT_SYM(rtk)

// Do the LDS accumulators (40 bytes per object) fit behind `table_bytes` of class tables in the 160 KiB a workgroup may take?  Otherwise
// the waves update the output records themselves.
extern "C" int RT_SYM(rt_extents_lds_accumulators)(size_t table_bytes, uint32_t n_obj)
{
    return table_bytes + sizeof(RT_SYM(rtk)::ExtRecord) * (size_t) n_obj <= 160u * 1024u;
}

// LDS bytes of one extents_kernel workgroup for this scene
extern "C" size_t RT_SYM(rt_extents_lds_bytes)(const FrameArgs *fa)
{
    const size_t tables = RT_SYM(rt_gbuffer_lds_bytes)(fa);
    return tables + (RT_SYM(rt_extents_lds_accumulators)(tables, fa->n_obj) ? sizeof(RT_SYM(rtk)::ExtRecord) * (size_t) fa->n_obj : 0u);
}

// rect = x0, y0, x1, y1 (inclusive, inside the image, GLOBAL rows); out = n_obj records in device memory.  Two nodes on `stream`: the
// identities, then -- when this rank owns a row of the rectangle -- the kernel, at most max_grid workgroups.
extern "C" hipError_t RT_SYM(rt_launch_object_extents)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *rect, void *out,
                                                        uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_obj == 0u) return hipSuccess;
    ExtRecord *rec = reinterpret_cast<ExtRecord *>(out);
    hipLaunchKernelGGL(extents_init_kernel, dim3((fa->n_obj + 255u) / 256u), dim3(256), 0, stream, rec, fa->n_obj);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ExtArgs ea;
    if (!ext_args(fa, rect, ea)) return hipSuccess; // no row of the rectangle is this rank's: the identities stand
    ea.lds_acc = RT_SYM(rt_extents_lds_accumulators)(RT_SYM(rt_gbuffer_lds_bytes)(fa), fa->n_obj) ? 1u : 0u;
    const dim3 g(ea.n_tiles < max_grid ? ea.n_tiles : (max_grid ? max_grid : 1u));
    RK_LAUNCH(fa, (extents_kernel<GQ, CUB>), g, RT_SYM(rt_extents_lds_bytes)(fa), stream, *fa, ea, reinterpret_cast<const unsigned char *>(scene), camx, camy, rec);
    return hipGetLastError();
}
