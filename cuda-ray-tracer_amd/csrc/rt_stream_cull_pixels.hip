// rt_stream_cull_pixels.hip -- the streamed pixel queries with whole chunks of the unit-sphere table culled by the block's cone:
// rt_render_gbuffer, rt_pick and rt_object_extents (and the _host and multi-GPU forms through them) of a context whose
// RT_FLAG_STREAM_CULL_PIXELS decision is true (include/mi355rt.h, "Culled pixel queries").
//
// Each kernel here is the twin of a kernel of rt_stream_queries.hip and runs the very body that one runs (rt_pixel_kernels.hpp; DESIGN.md
// section 32) -- launch bounds, grid, loads and stores with it -- over another query object: ScPixels (rt_stream_cull_pixels.hpp) asks
// sphere_in_cone about the chunk bounds before it stages a chunk, where SqPixels stages them all.  The spheres tested are the same and
// the acceptance rule does not depend on the order, so every output is the twin's bit for bit.
// Compiled twice like rt_stream_queries.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk.  Every
// kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS.  The work words (rt_debug_stream_cull_pixels) are kept per wave in scalars behind a
// wave-uniform test and added with one vector atomic per word at the wave's end.
#include <hip/hip_runtime.h>
#include "rt_launch.h"                // the launchers below, as the host sees them
#include "rt_pixel_kernels.hpp"       // the kernels' bodies; the extent record (rt_extents.hpp)
#include "rt_stream_cull_pixels.hpp"  // ScPixels

namespace RT_SYM(rtk) {

// (the slice: this wave's quarter of the workgroup's LDS, never another's)
// ---- the G-buffer and picking (gbuffer_stream_kernel): one kernel, two launch modes ------------------------------------------------------
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void gbuffer_cull_kernel(const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                           const double *__restrict__ camx, const double *__restrict__ camy, int32_t *__restrict__ out_object,
                                                           double *__restrict__ out_t, float4 *__restrict__ out_normal, const uint32_t *__restrict__ xy, uint32_t n_query,
                                                           RqRecord *__restrict__ out_rec)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    ScPixelStats ps{{0u, 0u, 0u, 0u}};
    ScPixels q{fa, qa, ca, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, ps};
    pk_gbuffer<HAS_GQ, HAS_CUBIC>(fa, scene, camx, camy, out_object, out_t, out_normal, xy, n_query, out_rec, q);
    if (ca.stats) sc_flush(ps.w, ca.stats, threadIdx.x & 63u);
}

// ---- object extents (extents_stream_kernel) ----------------------------------------------------------------------------------------------
// The identities of the n output records, one per thread: the one line that rt_extents.hpp's init kernel holds, under a name of this
// file's own (the two files that define that kernel through its macro are counted by tests/test_stream_shade_host.py).
__global__ __launch_bounds__(256) void ext_identities_cull_kernel(ExtRecord *__restrict__ out, uint32_t n_records)
{
    if (blockIdx.x * 256u + threadIdx.x < n_records) out[blockIdx.x * 256u + threadIdx.x] = ext_identity();
}

template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void extents_cull_kernel(const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, const ExtArgs ea,
                                                           const unsigned char *__restrict__ scene, const double *__restrict__ camx, const double *__restrict__ camy,
                                                           ExtRecord *__restrict__ out)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    ScPixelStats ps{{0u, 0u, 0u, 0u}};
    ScPixels q{fa, qa, ca, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, ps};
    pk_extents<HAS_GQ, HAS_CUBIC>(fa, ea, camx, camy, out, nullptr, q);
    if (ca.stats) sc_flush(ps.w, ca.stats, threadIdx.x & 63u);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
// (sc_cull_args, and: a context that does not cull has no cone)
static hipError_t scp_launch_pixels(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, uint32_t grid, int32_t *out_object, double *out_t,
                                    float *out_normal, const uint32_t *xy, uint32_t n, void *rec, const ChunkTables *chunks, hipStream_t stream)
{
    StreamCullArgs ca;
    if (fa->cull == 0u || !sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    const RayQueryArgs qa = rq_args(fa, 0u);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    float4 *nrm = reinterpret_cast<float4 *>(out_normal);
    RqRecord *r = reinterpret_cast<RqRecord *>(rec);
    RK_LAUNCH(fa, (gbuffer_cull_kernel<GQ, CUB>), dim3(grid), 0, stream, *fa, qa, ca, s, camx, camy, out_object, out_t, nrm, xy, n, r);
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// The streamed launchers' arguments (rt_stream_queries.hip), read: chunks = the context's chunk bounds and the work words to add to (8, the
// kernels write the first four; or NULL).  A launch is the same number of graph nodes as its twin's.
extern "C" hipError_t RT_SYM(rt_launch_pixel_cull_gbuffer)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t,
                                                            float *out_normal, const ChunkTables *chunks, hipStream_t stream)
{
    if (fa->n_tiles == 0u) return hipSuccess;
    return RT_SYM(rtk)::scp_launch_pixels(fa, scene, camx, camy, fa->n_tiles, out_object, out_t, out_normal, nullptr, 0u, nullptr, chunks, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_pixel_cull_pick)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *xy, uint32_t n, void *out,
                                                         const ChunkTables *chunks, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::scp_launch_pixels(fa, scene, camx, camy, (n + 255u) / 256u, nullptr, nullptr, nullptr, xy, n, out, chunks, stream);
}

// Two nodes on `stream`, as rt_launch_stream_object_extents: the identities, then -- when this rank owns a row of the rectangle -- the kernel.
extern "C" hipError_t RT_SYM(rt_launch_pixel_cull_object_extents)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *rect,
                                                                   void *out, uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_obj == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (fa->cull == 0u || !sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    ExtRecord *rec = reinterpret_cast<ExtRecord *>(out);
    hipLaunchKernelGGL(ext_identities_cull_kernel, dim3((fa->n_obj + 255u) / 256u), dim3(256), 0, stream, rec, fa->n_obj);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ExtArgs ea;
    if (!ext_args(fa, rect, ea)) return hipSuccess; // no row of the rectangle is this rank's: the identities stand
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(ea.n_tiles < max_grid ? ea.n_tiles : (max_grid ? max_grid : 1u));
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    RK_LAUNCH(fa, (extents_cull_kernel<GQ, CUB>), g, 0, stream, *fa, qa, ca, ea, s, camx, camy, rec);
    return hipGetLastError();
}
