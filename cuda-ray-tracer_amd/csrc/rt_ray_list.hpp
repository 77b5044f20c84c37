// rt_ray_list.hpp -- what the three ray-list kernels (ray_list_kernel, rt_adaptive.hip; ray_list_stream_kernel, rt_stream_adaptive.hip;
// ray_list_cull_kernel, rt_stream_cull_adaptive.hip) do around the shading of a ray, once: the items, the resolve and its store, and the
// launch ladder over (k, rgba8).  How a ray is shaded is each kernel's own.
// Per lane only, except for sl_resolve_store's shuffles, which read every lane of the wave.  Nothing is workgroup-wide.
// Needs rt_shade.hpp alone (quantise, xor_add).  Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast);
// everything lives in that variant's namespace.
#ifndef RT_RAY_LIST_HPP
#define RT_RAY_LIST_HPP

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt_shade.hpp"

namespace RT_SYM(rtk) {

// The launch ladder over a ray list's shape: calls launch(k, rgba8) once, with std::integral_constant<int, K> and std::true_type /
// std::false_type -- inside, decltype(k)::value and decltype(rgba8)::value are the kernel's <K, RGBA8> -- and returns what it returns.
// The halo rows (k = 1) are RGBA32F whatever the context's format; any other k is hipErrorInvalidValue.
template <typename Launch>
static inline hipError_t sl_for_shapes(uint32_t k, int rgba8, Launch &&launch)
{
    if (k == 1u) return launch(std::integral_constant<int, 1>{}, std::false_type{});
    if (k == 2u) return rgba8 ? launch(std::integral_constant<int, 2>{}, std::true_type{}) : launch(std::integral_constant<int, 2>{}, std::false_type{});
    if (k == 4u) return rgba8 ? launch(std::integral_constant<int, 4>{}, std::true_type{}) : launch(std::integral_constant<int, 4>{}, std::false_type{});
    return hipErrorInvalidValue;
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
// `sub == 0` stores one pixel of the output, RGBA8 quantised as the render kernels do.  Behind the wave's last wave-wide operation of the
// shading; the shuffles read every lane, and a pixel's lanes are all in use or all not.
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
