// rt_stream_adaptive.hip -- the streamed ray-list kernel: adaptive supersampling for scenes of any size (include/mi355rt.h,
// RT_FLAG_STREAM_ADAPTIVE).
//
// The twin of ray_list_kernel (rt_adaptive.hip): the same items, the same lane layout, the same resolve -- one lane per sample ray, a
// wave per 64 / K^2 listed pixels, the resolve's pairwise tree across the lanes, the exact 1 / K^2, the render kernels' RGBA8 store; K = 1
// traces the centre rays of the halo rows.  What differs is how a ray is shaded: not render_ray_culled over a copy of every object
// record in the workgroup's LDS, which bounds the scene's size, but the shading loop of stream_frame_kernel (rt_stream_shade.hpp:
// shade_loop) -- rt_shade_rays' arithmetic, the object loops of sq_query over the class tables in the scene blob, through a wave-private
// LDS slice, 64 entries at a time (rt_stream.hpp).  A sample's colour is therefore the pixel of a RT_FLAG_STREAM | RT_FLAG_SSAAk frame, bit for bit.
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk: a
// lane without a ray stays with `use = false`.  The kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS whatever the tables hold.
// Not culled: a wave's rays are not an 8 x 8 block, so there is no block cone (the policy SqShade with its cone off), and shadow and bounce
// rays test every object, as in every streamed kernel.  No counters.
#include <hip/hip_runtime.h>
#include "rt_launch.h"   // the launcher below, as the host sees it
#include "rt_stream_shell.hpp" // the items, the resolve and the launch ladder (rt_ray_list.hpp); the shading loop and SqShade (rt_stream_shade.hpp) over rt_stream.hpp

namespace RT_SYM(rtk) {

// ray_list_kernel's items (rt_adaptive.hip).  One lane = one sample ray; a wave = 64 / K^2 items.  Lane bits: i = sub-column (the low
// ones), j = sub-row (the next ones).  The waves take items by a grid-stride loop over the device-side count, so the grid size never
// depends on the frame; the loop's trip count is wave-uniform and nothing in it is workgroup-wide.
// The items and what is stored for them: rt_ray_list.hpp (sl_item, sl_resolve_store).
// Lanes past the list's end, and lanes of an off-image halo row, stay in the wave with use = false and skip only the store.
template <int K, bool RGBA8, bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void ray_list_stream_kernel(const FrameArgs fa, const RayQueryArgs qa, const unsigned char *__restrict__ scene,
                                                              const DevLight *__restrict__ lights, const double *__restrict__ camx, const double *__restrict__ camy,
                                                              const uint32_t *__restrict__ list, const uint32_t *__restrict__ count_ptr, uint32_t n_items,
                                                              void *__restrict__ out)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    constexpr uint32_t LANES = (uint32_t) (K * K), PPW = 64u / LANES; // lanes per item, items per wave
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    const uint32_t sub = lane % LANES, i = sub % (uint32_t) K, j = sub / (uint32_t) K;
    const uint32_t n = count_ptr ? *count_ptr : n_items; // (launch-uniform)
    const D3 origin{fa.origin[0], fa.origin[1], fa.origin[2]};
    for (uint32_t base = (blockIdx.x * 4u + wave) * PPW; base < n; base += gridDim.x * 4u * PPW) { // wave-uniform
        const SlItem it = sl_item<K>(fa, camx, camy, list, base + lane / LANES, n, i, j);
        SqShade pol{qa, scene, slice, false}; // never a cone
        const F3 c = shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, origin, it.dir, it.use);
        sl_resolve_store<K, RGBA8>(fa, out, it, sub, c);
    }
}

template <int K, bool RGBA8>
static hipError_t sa_launch(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, const uint32_t *list,
                            const uint32_t *count_ptr, uint32_t n_items, uint32_t grid, void *out, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(grid), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    rq_for_classes(fa, [&](auto gq, auto cub) {
        hipLaunchKernelGGL((ray_list_stream_kernel<K, RGBA8, decltype(gq)::value, decltype(cub)::value>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, list, count_ptr,
                           n_items, out);
    });
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// rt_launch_ray_list's arguments without the counters (the streamed passes book none): k = 2 / 4: the sample rays of the listed
// pixels (count_ptr = the device-side list length) into `out` (rgba8: uchar4, else float4); k = 1: the halo rows' centre rays, n_items
// = 2 * bands * width slots, into `out` = [2 * bands][width] float4.  scene = the blob, lights = the context's DevLight array.  `grid`
// workgroups of 256 lanes, fixed per context.  One graph node.
extern "C" hipError_t RT_SYM(rt_launch_stream_ray_list)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy,
                                                         const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out,
                                                         int rgba8, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (grid == 0u) return hipSuccess;
    return sl_for_shapes(k, rgba8, [&](auto kk, auto r8) {
        return sa_launch<decltype(kk)::value, decltype(r8)::value>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream);
    });
}
