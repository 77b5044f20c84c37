// rt_stream_cull_adaptive.hip -- the streamed ray-list kernel with whole chunks of the unit-sphere table culled: the halo and refine
// passes of an adaptive frame on a context whose stream-cull-adaptive decision is true (include/mi355rt.h, rt_get_stream_cull_adaptive;
// DESIGN.md section 26).
//
// The twin of ray_list_stream_kernel (rt_stream_adaptive.hip): the same items, lane layout, grid-stride loop, resolve tree, exact 1 / K^2
// and RGBA8 store (rt_ray_list.hpp), the same shading loop (rt_stream_shade.hpp: shade_loop).  What differs is the loop's policy
// (ScaShade below, over rt_stream_cull.hpp's ScShade), that is, which 64-entry chunks of the unit-sphere table a query stages:
//   * segment 0, nearest hit: the sample (or halo centre) rays of a wave all leave the frame's origin, so they have a cone -- not a block's
//     (the lanes are 64 / K^2 listed pixels, anywhere in the classifier's append order), but the wave's own: rt_wave_cone.hpp.  Lane j
//     asks sphere_in_cone about chunk bound g * 64 + j, only the surviving chunks are staged, and inside a staged chunk the per-entry cone
//     test and sc_sweep run, as in sc_query_primary.  A wave with an unproven lane, or with no lane in use, takes sq_query;
//   * shadow rays: wave_hit_ball (rt_wave_ball.hpp) once per segment and sc_query_shadow per light, under stream_cull_frame_kernel's conditions;
//   * bounce rays (nearest hit of segments >= 1): sq_query, a full sweep, as in the frame kernel.
// The colours are ray_list_stream_kernel's: the same arithmetic per tested object, and no dropped object's root could have been accepted.
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk: a
// lane without a ray stays with `use = false`.  The kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS whatever the tables hold.
// The work words (rt_debug_stream_cull_adaptive) are kept per wave in scalars behind a wave-uniform test and added with one vector atomic
// per word at the wave's end, behind the grid-stride loop.
#include <hip/hip_runtime.h>
#include "rt_launch.h"          // the launcher below, as the host sees it
#include "rt_stream_cull.hpp"   // the culled unit-sphere loops over rt_stream.hpp, and their shading policy
#include "rt_stream_shell.hpp"  // the items, the resolve and the launch ladder (rt_ray_list.hpp)
#include "rt_wave_cone.hpp"     // the lanes' parts of the wave cone

namespace RT_SYM(rtk) {

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
    unsigned long long pick = __ballot(wc_is_pick(score, wave_max<false>(score), use));
    if (pick == 0ull) pick = __ballot(use);
    const int l = __builtin_ctzll(pick);
    SqCone c;
    c.on = true;
    c.axis = D3{sq_readlane(d.x, l), sq_readlane(d.y, l), sq_readlane(d.z, l)};
    c.cos_t = sq_readlane(wave_min<false>(wc_cos(c.axis, d, use)), 0);
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

// ScShade for a wave whose lanes are not a block: segment 0 by the wave's own cone; the ball of a segment read back through lane 0.
// nocone: word [7].
struct ScaShade : ScShade {
    uint32_t &nocone;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t k, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        if (k == 0u) sca_query_primary<HAS_GQ, HAS_CUBIC>(qa, ca, scene, slice, lane, o, d, use, best_t, best, st, nocone);
        else sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, false, MAX_T, best_t, best); // bounce rays: a full sweep
    }
    __device__ __forceinline__ Segment segment(bool hit, const D3 &sp) const
    {
        Segment seg = ScShade::segment(hit, sp);
        // (every lane holds the same ball: read it back through lane 0, so that it lives in scalar registers across the light loop)
        seg.ball = Ball{sq_readlane(seg.ball.cx, 0), sq_readlane(seg.ball.cy, 0), sq_readlane(seg.ball.cz, 0), sq_readlane(seg.ball.R, 0)};
        return seg;
    }
};

// ray_list_stream_kernel's items (rt_stream_adaptive.hip).  ca: the chunk bounds and the work words.  One lane = one sample ray; a wave
// = 64 / K^2 items.  The waves take items by a grid-stride loop over the device-side count, so the grid size never depends on the frame;
// the loop's trip count is wave-uniform and nothing in it is workgroup-wide.  The items and what is stored for them: rt_ray_list.hpp
// (sl_item, sl_resolve_store).
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
        const SlItem it = sl_item<K>(fa, camx, camy, list, base + lane / LANES, n, i, j);
        ScaShade pol{{qa, ca, scene, slice, st}, nocone};
        const F3 c = shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, origin, it.dir, it.use);
        sl_resolve_store<K, RGBA8>(fa, out, it, sub, c);
    }
    if (st.on) sc_flush(st.w, ca.stats, lane, lane == 7u ? nocone : 0u); // behind the grid-stride loop
}

template <int K, bool RGBA8, bool STATS>
static hipError_t sca_launch(const FrameArgs *fa, const StreamCullArgs &ca, const void *scene, const void *lights, const double *camx, const double *camy,
                             const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t grid, void *out, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(grid), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    hipError_t refused = hipSuccess;
    rq_for_classes(fa, [&](auto gq, auto cub) {
        // (the counting instantiation for both classes does not fit two waves per SIMD and is not compiled: rt_create keeps no work words there)
        if constexpr (STATS && decltype(gq)::value && decltype(cub)::value) refused = hipErrorInvalidValue;
        else
            hipLaunchKernelGGL((ray_list_cull_kernel<K, RGBA8, decltype(gq)::value, decltype(cub)::value, STATS>), g, block, 0, stream, *fa, qa, ca, s, lt, camx, camy, list,
                               count_ptr, n_items, out);
    });
    if (refused != hipSuccess) return refused;
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// rt_launch_stream_ray_list's arguments, and the context's chunks (rt_launch.h: ChunkTables; the work words are rt_debug_stream_cull_adaptive's).
// One graph node.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_ray_list)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy,
                                                              const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out,
                                                              int rgba8, const ChunkTables *chunks, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (grid == 0u) return hipSuccess;
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca)) return hipErrorInvalidValue;
    return sl_for_shapes(k, rgba8, [&](auto kk, auto r8) {
        constexpr int K = decltype(kk)::value;
        constexpr bool RGBA8 = decltype(r8)::value;
        return ca.stats ? sca_launch<K, RGBA8, true>(fa, ca, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream)
                     : sca_launch<K, RGBA8, false>(fa, ca, scene, lights, camx, camy, list, count_ptr, n_items, grid, out, stream);
    });
}
