// rt_stream_cull_adaptive.hip -- the streamed ray-list kernel with whole chunks of the unit-sphere table culled: the halo and refine
// passes of an adaptive frame on a context whose stream-cull-adaptive decision is true (include/mi355rt.h, rt_get_stream_cull_adaptive;
// DESIGN.md section 26).
//
// The twin of ray_list_stream_kernel (rt_stream_adaptive.hip): the same items, lane layout, grid-stride loop, resolve tree, exact 1 / K^2
// and RGBA8 store.  What differs is which 64-entry chunks of the unit-sphere table a query stages (rt_stream_cull.hpp):
//   * segment 0, nearest hit: the sample (or halo centre) rays of a wave all leave the frame's origin, so they have a cone -- not a block's
//     (the lanes are 64 / K^2 listed pixels, anywhere in the classifier's append order), but the wave's own: rt_wave_cone.hpp.  Lane j
//     asks sphere_in_cone about chunk bound g * 64 + j, only the surviving chunks are staged, and inside a staged chunk the per-entry cone
//     test and sc_sweep run, as in sc_query_primary.  A wave with an unproven lane, or with no lane in use, takes sq_query;
//   * shadow rays: sc_hit_ball once per segment and sc_query_shadow per light, under stream_cull_frame_kernel's conditions;
//   * bounce rays (nearest hit of segments >= 1): sq_query, a full sweep, as in the frame kernel.
// The colours are ray_list_stream_kernel's: the same arithmetic per tested object, and no dropped object's root could have been accepted.
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk: a
// lane without a ray stays with `use = false`.  The kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS whatever the tables hold.
// The work words (rt_debug_stream_cull_adaptive) are kept per wave in scalars behind a wave-uniform test and added with one vector atomic
// per word at the wave's end, behind the grid-stride loop.
#include <hip/hip_runtime.h>
#include "rt_launch.h"          // the launcher below, as the host sees it
#include "rt_stream_cull.hpp"   // the culled unit-sphere loops over rt_stream.hpp
#include "rt_wave_cone.hpp"     // the lanes' parts of the wave cone

namespace RT_SYM(rtk) {

// the RGBA8 store of the render kernels (rt_stream_adaptive.hip's sa_quantise: a third copy, so that no existing kernel object changes)
__device__ __forceinline__ uchar4 sca_quantise(float x, float y, float z)
{
    uchar4 px;
    px.x = (unsigned char) (int) __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
    px.y = (unsigned char) (int) __fadd_rn(__fmul_rn(y, 255.0f), 0.5f);
    px.z = (unsigned char) (int) __fadd_rn(__fmul_rn(z, 255.0f), 0.5f);
    px.w = 255;
    return px;
}

// pairwise float32 sum over the lanes `m` apart (the resolve's tree, one level; rt_adaptive.hip's xor_add)
__device__ __forceinline__ F3 sca_xor_add(const F3 &v, int m)
{
    return F3{__fadd_rn(v.x, __shfl_xor(v.x, m)), __fadd_rn(v.y, __shfl_xor(v.y, m)), __fadd_rn(v.z, __shfl_xor(v.z, m))};
}

// The cone of the wave's used directions (rt_wave_cone.hpp); at least one lane is in use.  Everything it returns is wave-uniform and
// read back through readlane, so the axis and the opening live in scalar registers.
__device__ __forceinline__ SqCone sca_wave_cone(const D3 &d, bool use)
{
    D3 s = wc_term(d, use);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { // (a + b == b + a: every lane ends with the same bits)
        s.x += __shfl_xor(s.x, off, 64);
        s.y += __shfl_xor(s.y, off, 64);
        s.z += __shfl_xor(s.z, off, 64);
    }
    const double score = wc_score(s, d, use);
    unsigned long long pick = __ballot(wc_is_pick(score, sc_wave_max(score), use));
    if (pick == 0ull) pick = __ballot(use);
    const int l = __builtin_ctzll(pick);
    SqCone c;
    c.on = true;
    c.axis = D3{sq_readlane(d.x, l), sq_readlane(d.y, l), sq_readlane(d.z, l)};
    c.cos_t = sq_readlane(sc_wave_min(wc_cos(c.axis, d, use)), 0);
    return c;
}

// sc_query_primary for a wave whose lanes are not a block: sq_query for the rays (o, d) of the lanes in `use`, all from one origin
// (nearest hit, segment 0).  nocone: word [7], the queries that ran without a cone.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void sca_query_primary(const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane,
                                                  const D3 &o, const D3 &d, bool use, double &best_t, int &best, ScStats &st, uint32_t &nocone)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    if (__ballot(use && !proven) != 0ull || __ballot(use) == 0ull) { // (wave-uniform) no cone: nothing to cull with
        sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, false, MAX_T, best_t, best);
        if (st.on) nocone += 1u;
        return;
    }
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    const SqCone cone = sca_wave_cone(d, use);
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const bool quad = fabs(m.u2) > EPS;
    const double four_t2 = 4.0 * m.u2;
    for (uint32_t g = 0; g < ca.n_chunks; g += SQ_CHUNK) {
        const ScBound bd = sc_load_bound(ca, g, lane);
        unsigned long long chunks = __ballot(g + lane < ca.n_chunks && sphere_in_cone(bd.kx, bd.ky, bd.kz, bd.r, bd.inv_r, m.o, cone.axis, cone.cos_t));
        if (st.on) {
            st.w[0] += (ca.n_chunks - g < SQ_CHUNK) ? ca.n_chunks - g : SQ_CHUNK;
            st.w[1] += (uint32_t) __popcll(chunks);
        }
        while (chunks) { // wave-uniform: the chunks that reach into the wave's cone
            const uint32_t base = (g + (uint32_t) __builtin_ctzll(chunks)) * SQ_CHUNK;
            chunks &= chunks - 1;
            const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
            const UsEntry mine = sq_stage_chunk(g_us, base, end, lane, slice);
            const bool rel = base + lane < end && sphere_in_cone(mine.kx, mine.ky, mine.kz, mine.r, mine.inv_r, m.o, cone.axis, cone.cos_t);
            sc_sweep<false>(s_us, __ballot(rel), m, quad, four_t2, use, MAX_T, best_t, best);
        }
    }
    RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
    rest.n_us = 0u;
    sq_tables<HAS_GQ, HAS_CUBIC, false>(rest, scene, slice, lane, m, use, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, MAX_T, best_t, best);
}

// stream_cull_frame_kernel's bounce loop for the ray (o, d) of every lane in `use`, all from the frame's origin; all 64 lanes call.
// Iteration k traces the k-th segment of every lane that is still bouncing.  (sa_shade's loop a third time: a shared one would change
// the existing kernel objects.)
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ F3 sca_shade(const FrameArgs &fa, const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene,
                                        const DevLight *__restrict__ lights, unsigned char *slice, uint32_t lane, D3 o, D3 d, bool use, ScStats &st, uint32_t &nocone)
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
        if (k == 0u) sca_query_primary<HAS_GQ, HAS_CUBIC>(qa, ca, scene, slice, lane, o, d, bouncing, best_t, best, st, nocone);
        else sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, bouncing, false, MAX_T, best_t, best); // bounce rays: a full sweep
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
            Ball ball;
            const bool cull_seg = sc_hit_ball(hit, sp, ball); // once per segment; false: a non-finite hit point, test everything
            // (every lane holds the same ball: read it back through lane 0, so that it lives in scalar registers across the light loop)
            ball = Ball{sq_readlane(ball.cx, 0), sq_readlane(ball.cy, 0), sq_readlane(ball.cz, 0), sq_readlane(ball.R, 0)};
            for (uint32_t l = 0; l < fa.n_lights; l++) {
                const DevLight *lt = &lights[l];
                const bool spherical = lt->spherical != 0;
                double max_t;
                const D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
                double unused_t = INFINITY;
                int blocked = 0;
                if (cull_seg && (spherical || fabs(lt->u2) > EPS)) { // (wave-uniform)
                    if (spherical) sc_query_shadow<HAS_GQ, HAS_CUBIC, true>(qa, ca, scene, slice, lane, so, sd, hit, ball, *lt, max_t, blocked, st);
                    else sc_query_shadow<HAS_GQ, HAS_CUBIC, false>(qa, ca, scene, slice, lane, so, sd, hit, ball, *lt, max_t, blocked, st);
                } else {
                    sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, hit, false, max_t, unused_t, blocked);
                    if (st.on) st.w[6] += 1u;
                }
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

// ray_list_stream_kernel's items (rt_stream_adaptive.hip).  ca: the chunk bounds and the work words.  One lane = one sample ray; a wave
// = 64 / K^2 items.  Lane bits: i = sub-column (the low ones), j = sub-row (the next ones).  The waves take items by a grid-stride loop over the device-side count, so the grid size never
// depends on the frame; the loop's trip count is wave-uniform and nothing in it is workgroup-wide.
//   K = 2 / 4: item q is list[q] = (local row << 16) | x; sample (i, j) is the ray of sample (K x + i, K y + j) of the K-times finer
//              frame (camx / camy: its camera-plane tables); the lanes reduce with the resolve's tree, multiply by 1/K^2 and store one
//              pixel of the output.
//   K = 1:     halo rows.  Item q = pixel x of halo slot h = q / width: band b = h / 2 of this rank, side 0 = the global row just below
//              the band, 1 = just above it (nothing when that row lies outside the image); camx / camy: the output frame's tables.
//              Stores RGBA32F into halo[h][x].  A wave may straddle two slots: every lane decides for itself.
// Lanes past the list's end, and lanes of an off-image halo row, stay in the wave with use = false and skip only the store.
// STATS: the work words are counted (a template parameter: counting costs some twenty registers).  Two waves per SIMD are asked of the
// compiler, because the host sizes the grid for two resident workgroups per CU; an instantiation that cannot have them spills, and the
// build refuses spills.
template <int K, bool RGBA8, bool HAS_GQ, bool HAS_CUBIC, bool STATS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ray_list_cull_kernel(
    const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
    const double *__restrict__ camx, const double *__restrict__ camy, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count_ptr, uint32_t n_items,
    void *__restrict__ out)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    constexpr uint32_t LANES = (uint32_t) (K * K), PPW = 64u / LANES; // lanes per item, items per wave
    // (the wave's index through readfirstlane: the compiler then knows that the grid-stride loop, and the work words it carries, are wave-uniform)
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    const uint32_t sub = lane % LANES, i = sub % (uint32_t) K, j = sub / (uint32_t) K;
    const uint32_t n = count_ptr ? *count_ptr : n_items; // (launch-uniform)
    const D3 origin{fa.origin[0], fa.origin[1], fa.origin[2]};
    ScStats st{STATS, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    uint32_t nocone = 0u; // word [7]
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
        F3 c = sca_shade<HAS_GQ, HAS_CUBIC>(fa, qa, ca, scene, lights, slice, lane, origin, dir, use, st, nocone);
        // (behind the wave's last staged chunk; the shuffles below read every lane, and a pixel's lanes are all in use or all not)
        if (K == 1) {
            if (use) reinterpret_cast<float4 *>(out)[(size_t) lr * fa.width + x] = make_float4(c.x, c.y, c.z, 1.0f);
        } else {
            // (s0 + s1) [+ (s2 + s3)] over i, then the same over j: lanes i ^ 1, i ^ 2, then j's bits
            c = sca_xor_add(c, 1);
            if (K == 4) c = sca_xor_add(c, 2);
            c = sca_xor_add(c, K);
            if (K == 4) c = sca_xor_add(c, 2 * K);
            if (use && sub == 0u) {
                constexpr float inv = 1.0f / (float) (K * K); // exact
                const float vx = __fmul_rn(c.x, inv), vy = __fmul_rn(c.y, inv), vz = __fmul_rn(c.z, inv);
                const size_t at = (size_t) lr * fa.width + x;
                if (RGBA8) reinterpret_cast<uchar4 *>(out)[at] = sca_quantise(vx, vy, vz);
                else reinterpret_cast<float4 *>(out)[at] = make_float4(vx, vy, vz, 1.0f);
            }
        }
    }
    if (st.on && lane < 8u) { // one vector atomic per word and wave, behind the grid-stride loop
        uint32_t mine = lane == 7u ? nocone : 0u;
#pragma unroll
        for (uint32_t w = 0; w < 7u; w++) mine = lane == w ? st.w[w] : mine;
        if (mine) atomicAdd(ca.stats + lane, (unsigned long long) mine);
    }
}

template <int K, bool RGBA8, bool STATS>
static hipError_t sca_launch(const FrameArgs *fa, const StreamCullArgs &ca, const void *scene, const void *lights, const double *camx, const double *camy,
                             const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t grid, void *out, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(grid), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
#define SCA_KERNEL(GQ, CUB) hipLaunchKernelGGL((ray_list_cull_kernel<K, RGBA8, GQ, CUB, STATS>), g, block, 0, stream, *fa, qa, ca, s, lt, camx, camy, list, count_ptr, n_items, out)
    if (fa->n_cub) {
        if (fa->n_gq) {
            // (the counting instantiation for both classes does not fit two waves per SIMD and is not compiled: rt_create keeps no work words there)
            if constexpr (STATS) return hipErrorInvalidValue;
            else SCA_KERNEL(true, true);
        } else {
            SCA_KERNEL(false, true);
        }
    } else {
        if (fa->n_gq) SCA_KERNEL(true, false);
        else SCA_KERNEL(false, false);
    }
#undef SCA_KERNEL
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// rt_launch_stream_ray_list's arguments, and: bounds = the context's chunk-bound table, [n_chunks] UsEntry for the ceil(n_us / 64) chunks
// of the blob's (ordered) unit-sphere table; stats = 8 work words to add to (rt_debug_stream_cull_adaptive), or NULL.  One graph node.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_ray_list)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy,
                                                              const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out,
                                                              int rgba8, const void *bounds, uint32_t n_chunks, unsigned long long *stats, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (grid == 0u) return hipSuccess;
    if (n_chunks != (fa->n_us + SQ_CHUNK - 1u) / SQ_CHUNK || (n_chunks && !bounds)) return hipErrorInvalidValue;
    const StreamCullArgs ca{reinterpret_cast<const UsEntry *>(bounds), stats, n_chunks, 0u};
#define SCA_LAUNCH(K, RGBA8) \
    (stats ? sca_launch<K, RGBA8, true>(fa, ca, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream) \
           : sca_launch<K, RGBA8, false>(fa, ca, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream))
    if (k == 1u) return SCA_LAUNCH(1, false);
    if (k == 2u) return rgba8 ? SCA_LAUNCH(2, true) : SCA_LAUNCH(2, false);
    if (k == 4u) return rgba8 ? SCA_LAUNCH(4, true) : SCA_LAUNCH(4, false);
#undef SCA_LAUNCH
    return hipErrorInvalidValue;
}
