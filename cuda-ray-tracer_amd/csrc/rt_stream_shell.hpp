// rt_stream_shell.hpp -- what the streamed kernels do around the shading loop (rt_stream_shade.hpp), once per launch shape:
//   frames (stream_frame_kernel, stream_cull_frame_kernel, stream_cull_bounce_frame_kernel): a lane's pixel and the frame store;
//   ray lists (ray_list_stream_kernel, ray_list_cull_kernel): the items, the resolve and the store of rt_ray_list.hpp, included here --
//   one text for these two and for ray_list_kernel (rt_adaptive.hip), which takes that header alone.
// Per lane only (sl_resolve_store's shuffles, rt_ray_list.hpp, read every lane of the wave).  Nothing is workgroup-wide.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_SHELL_HPP
#define RT_STREAM_SHELL_HPP

#include <hip/hip_runtime.h>

#include "rt_ray_list.hpp" // SlItem, sl_item, sl_resolve_store, sl_for_shapes
#include "rt_stream_shade.hpp"

namespace RT_SYM(rtk) {

// ---- frames: one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels (gbuffer_kernel's shape) ----
struct SfPixel {
    uint32_t x, lr;   // column and local row; stored only when `inside`
    uint32_t col, row; // camera-table indices: the pixel's, or those of the clamped pixel a lane outside the image traces
    bool inside;
};

// Lanes outside the image trace a clamped pixel's whole path, so that the block's corner lanes always span its cone, and store nothing.
__device__ __forceinline__ SfPixel sf_pixel(const FrameArgs &fa, uint32_t wave, uint32_t lane)
{
    const uint32_t tile_x = blockIdx.x % fa.tiles_x, tile_y = blockIdx.x / fa.tiles_x;
    SfPixel p;
    p.x = tile_x * 16u + (wave & 1u) * 8u + (lane & 7u);
    p.lr = tile_y * 16u + (wave >> 1) * 8u + (lane >> 3);
    p.inside = p.x < fa.width && p.lr < fa.local_rows;
    p.col = p.x < fa.width ? p.x : fa.width - 1u;
    p.row = global_row(fa, p.lr < fa.local_rows ? p.lr : fa.local_rows - 1u);
    return p;
}

// (behind the wave's last wave-wide operation)
__device__ __forceinline__ void sf_store(const FrameArgs &fa, void *__restrict__ fb, const SfPixel &p, const F3 &res)
{
    if (!p.inside) return;
    const size_t pix = (size_t) p.lr * fa.width + p.x;
    if (fa.rgba8) { // launch-uniform; the wire format of the render kernels: iround(c * 255), alpha 255
        uchar4 px;
        px.x = (unsigned char) (int) (res.x * 255.0f + 0.5f);
        px.y = (unsigned char) (int) (res.y * 255.0f + 0.5f);
        px.z = (unsigned char) (int) (res.z * 255.0f + 0.5f);
        px.w = 255;
        reinterpret_cast<uchar4 *>(fb)[pix] = px;
    } else {
        reinterpret_cast<float4 *>(fb)[pix] = make_float4(res.x, res.y, res.z, 1.0f);
    }
}

} // namespace RT_SYM(rtk)

#endif
