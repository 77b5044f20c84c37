// rt_stream_cull.hip -- the streamed frame kernel with whole chunks of the unit-sphere table culled: rt_render of a context whose
// RT_FLAG_STREAM_CULL decision is true (include/mi355rt.h, "Culled streamed frames").
//
// stream_frame_kernel's launch shape (rt_stream_shell.hpp) and its shading loop (rt_stream_shade.hpp: shade_loop), under another policy
// (rt_stream_cull.hpp: ScShade).  What differs is which 64-entry chunks of the unit-sphere table a query stages: the primary rays of
// a block only those whose bound reaches into the block's cone, the shadow rays of a segment
// towards one light only those whose bound is relevant for the ball around the wave's hit points -- and of a staged chunk's entries
// only the relevant ones are swept.  Not culled: a segment with a non-finite hit point, a directional light with |d|^2 <= EPS (the
// reference's linear branch is not geometry), the other class tables, and the nearest-hit queries of bounce rays (segments >= 1).
// The frame is stream_frame_kernel's: the same arithmetic per tested object, and no dropped object's root could have been accepted.
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file.  The work words (rt_debug_stream_cull) are kept per wave in scalars behind a
// wave-uniform test and added with one vector atomic per word at the wave's end.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include "rt_stream_cull.hpp"  // the culled unit-sphere loops over rt_stream.hpp, and their shading policy
#include "rt_stream_shell.hpp" // a lane's pixel and the frame store

namespace RT_SYM(rtk) {

// stream_frame_kernel's shape: one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels;
// lanes outside the image trace a clamped pixel's whole path and store nothing.  ca: the chunk bounds and the work words.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void stream_cull_frame_kernel(const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, const unsigned char *__restrict__ scene,
                                                                const DevLight *__restrict__ lights, const double *__restrict__ camx, const double *__restrict__ camy,
                                                           void *__restrict__ fb)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    ScStats st{ca.stats != nullptr, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    const SfPixel p = sf_pixel(fa, wave, lane);
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    ScShade pol{qa, ca, scene, slice, st};
    const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, o, primary_dir_tab(fa, camx[p.col], camy[p.row]), true);
    if (st.on) sc_flush(st.w, ca.stats, lane);
    sf_store(fa, fb, p, res);
}

} // namespace RT_SYM(rtk)

// rt_launch_stream's arguments, and the context's chunks (rt_launch.h: ChunkTables).
extern "C" hipError_t RT_SYM(rt_launch_stream_cull)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
                                                    const ChunkTables *chunks, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_tiles == 0u) return hipSuccess;
    const RayQueryArgs qa = rq_args(fa, 0u);
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    const dim3 g(fa->n_tiles), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    rq_for_classes(fa, [&](auto gq, auto cub) {
        hipLaunchKernelGGL((stream_cull_frame_kernel<decltype(gq)::value, decltype(cub)::value>), g, block, 0, stream, *fa, qa, ca, s, lt, camx, camy, fb);
    });
    return hipGetLastError();
}
