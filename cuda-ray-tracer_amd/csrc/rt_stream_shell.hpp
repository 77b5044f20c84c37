// rt_stream_shell.hpp -- what the streamed kernels do around the shading loop (rt_stream_shade.hpp), once per launch shape:
//   frames (stream_frame_kernel, stream_cull_frame_kernel, stream_cull_bounce_frame_kernel): a lane's pixel and the frame store;
//   ray lists (ray_list_stream_kernel, ray_list_cull_kernel): ray_list_kernel's items (rt_adaptive.hip) and its resolve and store.
// Per lane only, except for sl_resolve_store's shuffles, which read every lane of the wave.  Nothing is workgroup-wide.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_SHELL_HPP
#define RT_STREAM_SHELL_HPP

#include <hip/hip_runtime.h>

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

// ---- ray lists: one lane = one sample ray, a wave = 64 / K^2 items; lane bits: i = sub-column (the low ones), j = sub-row (the next ones) ----
struct SlItem {
    uint32_t x, lr; // where the item's pixel is stored: column and local row (K = 1: halo slot)
    D3 dir;
    bool use;       // false: past the list's end, or an off-image halo row -- the lane stays in the wave and skips only the store
};

//   K = 2 / 4: item q is list[q] = (local row << 16) | x; sample (i, j) is the ray of sample (K x + i, K y + j) of the K-times finer
//              frame (camx / camy: its camera-plane tables).
//   K = 1:     halo rows.  Item q = pixel x of halo slot h = q / width: band b = h / 2 of this rank, side 0 = the global row just below
//              the band, 1 = just above it (nothing when that row lies outside the image); camx / camy: the output frame's tables.
//              A wave may straddle two slots: every lane decides for itself.
template <int K>
__device__ __forceinline__ SlItem sl_item(const FrameArgs &fa, const double *__restrict__ camx, const double *__restrict__ camy, const uint32_t *__restrict__ list, uint32_t q,
                                          uint32_t n, uint32_t i, uint32_t j)
{
    SlItem it{0u, 0u, D3{0.0, 0.0, 1.0}, q < n};
    if (K == 1) {
        if (it.use) {
            const uint32_t h = q / fa.width, b = h >> 1;
            it.x = q - h * fa.width;
            it.lr = h; // (halo slot)
            const uint32_t start = b * fa.band_rows, rows = min(fa.band_rows, fa.local_rows - start);
            const int64_t g0 = ((int64_t) b * fa.world + fa.rank) * fa.band_rows;
            const int64_t gy = (h & 1u) ? g0 + rows : g0 - 1;
            it.use = gy >= 0 && gy < (int64_t) fa.height;
            if (it.use) it.dir = primary_dir_tab(fa, camx[it.x], camy[(uint32_t) gy]);
        }
    } else {
        if (it.use) {
            const uint32_t v = list[q];
            it.lr = v >> 16;
            it.x = v & 0xFFFFu;
            const uint32_t y = global_row(fa, it.lr);
            it.dir = primary_dir_tab(fa, camx[(size_t) K * it.x + i], camy[(size_t) K * y + j]);
        }
    }
    return it;
}

// K = 1: RGBA32F into halo[h][x].  K = 2 / 4: the lanes reduce with the resolve's pairwise tree, multiply by the exact 1 / K^2 and lane
// `sub == 0` stores one pixel of the output, RGBA8 quantised as the render kernels do.  Behind the wave's last staged chunk; the shuffles
// read every lane, and a pixel's lanes are all in use or all not.
template <int K, bool RGBA8>
__device__ __forceinline__ void sl_resolve_store(const FrameArgs &fa, void *__restrict__ out, const SlItem &it, uint32_t sub, F3 c)
{
    if (K == 1) {
        if (it.use) reinterpret_cast<float4 *>(out)[(size_t) it.lr * fa.width + it.x] = make_float4(c.x, c.y, c.z, 1.0f);
    } else {
        // (s0 + s1) [+ (s2 + s3)] over i, then the same over j: lanes i ^ 1, i ^ 2, then j's bits
        c = xor_add(c, 1);
        if (K == 4) c = xor_add(c, 2);
        c = xor_add(c, K);
        if (K == 4) c = xor_add(c, 2 * K);
        if (it.use && sub == 0u) {
            constexpr float inv = 1.0f / (float) (K * K); // exact
            const float vx = __fmul_rn(c.x, inv), vy = __fmul_rn(c.y, inv), vz = __fmul_rn(c.z, inv);
            const size_t at = (size_t) it.lr * fa.width + it.x;
            if (RGBA8) reinterpret_cast<uchar4 *>(out)[at] = quantise(vx, vy, vz);
            else reinterpret_cast<float4 *>(out)[at] = make_float4(vx, vy, vz, 1.0f);
        }
    }
}

} // namespace RT_SYM(rtk)

#endif
