// rt_stream.hip -- the streamed frame kernel: rt_render for scenes of any size (include/mi355rt.h, "Streamed frames").
//
// The frame of rt_render by the arithmetic of rt_shade_rays on the rays of rt_primary_rays: one ray per pixel from the frame's origin
// along primary_dir_tab, then the shading loop every kernel of this family runs (rt_stream_shade.hpp: shade_loop).  What differs from
// shade_rays_kernel is where the object loops read the class tables: not from a copy of all of them in LDS, which bounds the scene's
// size, but from the scene blob in global memory through a wave-private LDS slice, 64 entries at a time (rt_stream.hpp).  The only work
// removal is the cone culling of primary rays, one lane per sphere as in rt_gbuffer.hip (the policy SqShade with its cone on).
// Compiled twice like rt_shade_rays.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file: the four waves of a workgroup run different numbers of bounces and chunks.
// The kernel reads the scene blob, the lights and the camera-plane tables and writes the frame: no tile words, launch-order
// generations, census, counters or frame tag -- a frame depends on nothing an earlier frame left.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include "rt_stream_shell.hpp" // a lane's pixel and the frame store; the shading loop and SqShade (rt_stream_shade.hpp) over rt_stream.hpp

namespace RT_SYM(rtk) {

// The frames' launch shape (rt_stream_shell.hpp: sf_pixel).  Per wave one bounce loop: iteration k traces the k-th segment of every
// lane that is still bouncing.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void stream_frame_kernel(const FrameArgs fa, const RayQueryArgs qa, const unsigned char *__restrict__ scene,
                                                           const DevLight *__restrict__ lights, const double *__restrict__ camx, const double *__restrict__ camy,
                                                           void *__restrict__ fb)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    const SfPixel p = sf_pixel(fa, wave, lane);
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    SqShade pol{qa, scene, slice, fa.cull != 0u};
    const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, o, primary_dir_tab(fa, camx[p.col], camy[p.row]), true);
    sf_store(fa, fb, p, res);
}

} // namespace RT_SYM(rtk)

// fb = this rank's rows, [local_rows][width] pixels of fa's format; lights = the context's DevLight array; camx / camy = the context's
// camera-plane tables.  Any scene size: the kernel's LDS is 24 KiB whatever the tables hold.
extern "C" hipError_t RT_SYM(rt_launch_stream)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
                                               hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_tiles == 0u) return hipSuccess;
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(fa->n_tiles), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    rq_for_classes(fa, [&](auto gq, auto cub) {
        hipLaunchKernelGGL((stream_frame_kernel<decltype(gq)::value, decltype(cub)::value>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, fb);
    });
    return hipGetLastError();
}
