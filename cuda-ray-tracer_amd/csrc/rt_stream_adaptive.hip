// rt_stream_adaptive.hip -- the streamed ray-list kernel: adaptive supersampling for scenes of any size (include/mi355rt.h,
// RT_FLAG_STREAM_ADAPTIVE).
//
// The twin of ray_list_kernel (rt_adaptive.hip): the same items, the same lane layout, the same resolve -- one lane per sample ray, a
// wave per 64 / K^2 listed pixels, the resolve's pairwise tree across the lanes, the exact 1 / K^2, the render kernels' RGBA8 store; K = 1
// traces the centre rays of the halo rows.  What differs is how a ray is shaded: not render_ray_culled over a copy of every object
// record in the workgroup's LDS, which bounds the scene's size, but the body of stream_frame_kernel (rt_stream.hip) -- rt_shade_rays'
// arithmetic, the object loops of sq_query over the class tables in the scene blob, through a wave-private LDS slice, 64 entries at a
// time (rt_stream.hpp).  A sample's colour is therefore the pixel of a RT_FLAG_STREAM | RT_FLAG_SSAAk frame, bit for bit.
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk: a
// lane without a ray stays with `use = false`.  The kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS whatever the tables hold.
// Not culled: a wave's rays are not an 8 x 8 block, so there is no block cone (sq_query with block_cone = false), and shadow and bounce
// rays test every object, as in every streamed kernel.  No counters.
#include <hip/hip_runtime.h>
#include "rt_launch.h"   // the launcher below, as the host sees it
#include "rt_stream.hpp" // the streamed object loops; RayQueryArgs and the plain path (rt_rayquery.hpp)

namespace RT_SYM(rtk) {

// the RGBA8 store of the render kernels, (unsigned char)(int)(v * 255.0f + 0.5f), with both operations rounded separately in every
// build (rt_adaptive.hip's quantise: a second copy, so that no existing kernel object changes)
__device__ __forceinline__ uchar4 sa_quantise(float x, float y, float z)
{
    uchar4 px;
    px.x = (unsigned char) (int) __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
    px.y = (unsigned char) (int) __fadd_rn(__fmul_rn(y, 255.0f), 0.5f);
    px.z = (unsigned char) (int) __fadd_rn(__fmul_rn(z, 255.0f), 0.5f);
    px.w = 255;
    return px;
}

// pairwise float32 sum over the lanes `m` apart (the resolve's tree, one level; rt_adaptive.hip's xor_add)
__device__ __forceinline__ F3 sa_xor_add(const F3 &v, int m)
{
    return F3{__fadd_rn(v.x, __shfl_xor(v.x, m)), __fadd_rn(v.y, __shfl_xor(v.y, m)), __fadd_rn(v.z, __shfl_xor(v.z, m))};
}

// stream_frame_kernel's bounce loop for the ray (o, d) of every lane in `use`; all 64 lanes call.  Iteration k traces the k-th segment
// of every lane that is still bouncing.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ F3 sa_shade(const FrameArgs &fa, const RayQueryArgs &qa, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                       unsigned char *slice, uint32_t lane, D3 o, D3 d, bool use)
{
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const F3 bg{fa.bg[0], fa.bg[1], fa.bg[2]};
    F3 res = bg; // a first-segment miss is the background colour
    float cur_ratio = 1.0f;
    bool bouncing = use;
    for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++) {
        // get_color_and_object, src/update-cpu.cpp:45-80: the nearest hit ...
        double best_t = INFINITY;
        int best = -1;
        sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, bouncing, false, MAX_T, best_t, best);
        const bool hit = bouncing && best >= 0;
        const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
        D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
        if (hit) {
            sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
            sn = normal_vector(bo->c, sp); // all twenty coefficients; FP64, never flipped
        }
        // ... every light in index order (wave-uniform: scalar loads), shadow_ray from sp + SHADOW_BIAS * sn
        const D3 so{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
        F3 acc{0.0f, 0.0f, 0.0f};
        if (__ballot(hit) != 0ull) {
            const F3 albedo{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
            for (uint32_t l = 0; l < fa.n_lights; l++) {
                const DevLight *lt = &lights[l];
                const bool spherical = lt->spherical != 0;
                double max_t;
                const D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
                double unused_t = INFINITY;
                int blocked = 0;
                sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, hit, false, max_t, unused_t, blocked);
                if (hit && blocked == 0) {
                    const F3 c = surface_color(lt->p, lt->color, spherical, sp, sn, albedo);
                    acc.x += c.x;
                    acc.y += c.y;
                    acc.z += c.z;
                }
            }
        }
        if (bouncing) {
            if (!hit) {
                if (k != 0u) RT_SYM(rtk)::blend(res, cur_ratio, bg); // a bounce that leaves the scene picks up the background
                bouncing = false;
            } else {
                // glm::min(vec3(1.0f), acc)
                const F3 oc{(acc.x < 1.0f) ? acc.x : 1.0f, (acc.y < 1.0f) ? acc.y : 1.0f, (acc.z < 1.0f) ? acc.z : 1.0f};
                if (k == 0u) res = oc;
                else RT_SYM(rtk)::blend(res, cur_ratio, oc);
                // the reflection loop, src/update-cpu.cpp:96-117
                const float refl = bo->refl;
                if (!((double) refl > EPS)) {
                    bouncing = false;
                } else {
                    cur_ratio *= refl;
                    if (k == fa.max_refl) {
                        RT_SYM(rtk)::blend(res, cur_ratio, bg);
                        bouncing = false;
                    } else {
                        d = reflect_ray(d, sn); // of the direction as it is
                        o = so;
                    }
                }
            }
        }
    }
    return res;
}

// ray_list_kernel's items (rt_adaptive.hip).  One lane = one sample ray; a wave = 64 / K^2 items.  Lane bits: i = sub-column (the low
// ones), j = sub-row (the next ones).  The waves take items by a grid-stride loop over the device-side count, so the grid size never
// depends on the frame; the loop's trip count is wave-uniform and nothing in it is workgroup-wide.
//   K = 2 / 4: item q is list[q] = (local row << 16) | x; sample (i, j) is the ray of sample (K x + i, K y + j) of the K-times finer
//              frame (camx / camy: its camera-plane tables); the lanes reduce with the resolve's tree, multiply by 1/K^2 and store one
//              pixel of the output.
//   K = 1:     halo rows.  Item q = pixel x of halo slot h = q / width: band b = h / 2 of this rank, side 0 = the global row just below
//              the band, 1 = just above it (nothing when that row lies outside the image); camx / camy: the output frame's tables.
//              Stores RGBA32F into halo[h][x].  A wave may straddle two slots: every lane decides for itself.
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
        const uint32_t q = base + lane / LANES;
        bool use = q < n;
        uint32_t x = 0, lr = 0;
        D3 dir{0.0, 0.0, 1.0};
        if (K == 1) {
            if (use) {
                const uint32_t h = q / fa.width, b = h >> 1;
                x = q - h * fa.width;
                lr = h; // (halo slot)
                const uint32_t start = b * fa.band_rows, rows = min(fa.band_rows, fa.local_rows - start);
                const int64_t g0 = ((int64_t) b * fa.world + fa.rank) * fa.band_rows;
                const int64_t gy = (h & 1u) ? g0 + rows : g0 - 1;
                use = gy >= 0 && gy < (int64_t) fa.height;
                if (use) dir = primary_dir_tab(fa, camx[x], camy[(uint32_t) gy]);
            }
        } else {
            if (use) {
                const uint32_t v = list[q];
                lr = v >> 16;
                x = v & 0xFFFFu;
                const uint32_t y = global_row(fa, lr);
                dir = primary_dir_tab(fa, camx[(size_t) K * x + i], camy[(size_t) K * y + j]);
            }
        }
        F3 c = sa_shade<HAS_GQ, HAS_CUBIC>(fa, qa, scene, lights, slice, lane, origin, dir, use);
        // (behind the wave's last staged chunk; the shuffles below read every lane, and a pixel's lanes are all in use or all not)
        if (K == 1) {
            if (use) reinterpret_cast<float4 *>(out)[(size_t) lr * fa.width + x] = make_float4(c.x, c.y, c.z, 1.0f);
        } else {
            // (s0 + s1) [+ (s2 + s3)] over i, then the same over j: lanes i ^ 1, i ^ 2, then j's bits
            c = sa_xor_add(c, 1);
            if (K == 4) c = sa_xor_add(c, 2);
            c = sa_xor_add(c, K);
            if (K == 4) c = sa_xor_add(c, 2 * K);
            if (use && sub == 0u) {
                constexpr float inv = 1.0f / (float) (K * K); // exact
                const float vx = __fmul_rn(c.x, inv), vy = __fmul_rn(c.y, inv), vz = __fmul_rn(c.z, inv);
                const size_t at = (size_t) lr * fa.width + x;
                if (RGBA8) reinterpret_cast<uchar4 *>(out)[at] = sa_quantise(vx, vy, vz);
                else reinterpret_cast<float4 *>(out)[at] = make_float4(vx, vy, vz, 1.0f);
            }
        }
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
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((ray_list_stream_kernel<K, RGBA8, true, true>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, list, count_ptr, n_items, out);
        else hipLaunchKernelGGL((ray_list_stream_kernel<K, RGBA8, false, true>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, list, count_ptr, n_items, out);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((ray_list_stream_kernel<K, RGBA8, true, false>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, list, count_ptr, n_items, out);
        else hipLaunchKernelGGL((ray_list_stream_kernel<K, RGBA8, false, false>), g, block, 0, stream, *fa, qa, s, lt, camx, camy, list, count_ptr, n_items, out);
    }
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
    if (k == 1u) return sa_launch<1, false>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream);
    if (k == 2u) return rgba8 ? sa_launch<2, true>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream)
                              : sa_launch<2, false>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream);
    if (k == 4u) return rgba8 ? sa_launch<4, true>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream)
                              : sa_launch<4, false>(fa, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream);
    return hipErrorInvalidValue;
}
