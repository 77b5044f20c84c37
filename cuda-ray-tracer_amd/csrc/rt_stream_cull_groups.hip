// rt_stream_cull_groups.hip -- the culled streamed frame kernel under a second level of bounds: rt_render of a context whose
// RT_FLAG_STREAM_CULL_GROUPS decision is true (include/mi355rt.h, "Grouped chunk bounds").
//
// stream_cull_frame_kernel's launch shape (rt_stream_shell.hpp) and the shared shading loop (rt_stream_shade.hpp: shade_loop) under the
// policy SgShade (rt_stream_cull_groups.hpp): every culled query asks its own predicate about the GROUP bounds first -- one bound per 64
// chunk bounds, formed by the function that forms the chunk bounds -- and runs a trip of the twin's chunk loop only for the groups that
// pass.  BOUNCE: the nearest hit of a bounce ray is culled per ray as in stream_cull_bounce_frame_kernel, group by group; otherwise bounce
// rays keep sq_query's full sweep.  The frame is stream_frame_kernel's: the chunks staged, their order and the place of the occlusion
// early-out are those of the kernel without the group level.  The twins' work words (rt_debug_stream_cull, rt_debug_stream_cull_bounce)
// count what this kernel asks and stages; the group verdicts have six words of their own (rt_debug_stream_groups).
// Compiled twice like rt_stream_cull.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file.  The work words are kept per wave in scalars and added with one vector atomic per
// word at the wave's end.  Whether a launch counts is a template argument here (STATS), not the twins' run-time test: with the 18 words
// of three families behind a run-time test the strict kernels take 241 .. 256 VGPRs and those for general quadrics plus degree 3 lose
// their second wave per SIMD; the kernels that do not count take 198 .. 235 (DESIGN.md section 37 has the table).  ONE instantiation
// per build is not built: the kernel that counts AND culls bounce rays for a scene with both general quadrics and degree-3 objects does
// not fit two waves per SIMD (the rule of every streamed frame kernel).  The launcher refuses that combination, and rt_create's decision
// is false for the contexts that would need it (such a scene, a true bounce decision and MI355RT_STREAM_CULL_STATS=1).
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include "rt_stream_cull_groups.hpp" // the grouped queries over rt_stream_cull.hpp's and rt_stream_cull_bounce.hpp's loops, and their shading policy
#include "rt_stream_shell.hpp"       // a lane's pixel and the frame store

namespace RT_SYM(rtk) {

// stream_frame_kernel's shape: one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels;
// lanes outside the image trace a clamped pixel's whole path and store nothing.  ca: the chunk bounds and the frame's work words; ga: the
// group bounds and the group words; bstats: the bounce work words (BOUNCE only; NULL exactly where ca.stats is).
template <bool HAS_GQ, bool HAS_CUBIC, bool BOUNCE, bool STATS>
__global__ __launch_bounds__(256) void stream_cull_groups_frame_kernel(const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, const StreamGroupArgs ga,
                                                                       unsigned long long *bstats, const unsigned char *__restrict__ scene,
                                                                       const DevLight *__restrict__ lights, const double *__restrict__ camx,
                                                                       const double *__restrict__ camy, void *__restrict__ fb)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    ScStats st{STATS, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    ScBounceStats bs{STATS, {0u, 0u, 0u, 0u, 0u}};
    SgStats gs{{0u, 0u, 0u, 0u, 0u, 0u}};
    const SfPixel p = sf_pixel(fa, wave, lane);
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    SgShade<BOUNCE> pol{qa, ca, ga, scene, slice, st, bs, gs};
    const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, o, primary_dir_tab(fa, camx[p.col], camy[p.row]), true);
    if (STATS) {
        sc_flush(st.w, ca.stats, lane);
        if (BOUNCE) sc_flush(bs.w, bstats, lane);
        sc_flush(gs.w, ga.stats, lane);
    }
    sf_store(fa, fb, p, res);
}

} // namespace RT_SYM(rtk)

// rt_launch_stream_cull_bounce's arguments, and: groups = the context's group bounds with their 8 work words (rt_launch.h: GroupTables; the
// words NULL exactly where chunks->stats is NULL); bounce != 0: the bounce rays are culled per ray as well (bounce_stats as the twin takes
// them), 0: they keep the full sweep and bounce_stats must be NULL.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_groups)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
                                                           const ChunkTables *chunks, const GroupTables *groups, unsigned long long *bounce_stats, int bounce,
                                                           hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_tiles == 0u) return hipSuccess;
    const RayQueryArgs qa = rq_args(fa, 0u);
    StreamCullArgs ca;
    StreamGroupArgs ga;
    if (!sg_group_args(fa, chunks, groups, ca, ga)) return hipErrorInvalidValue;
    if (bounce ? (ca.stats == nullptr) != (bounce_stats == nullptr) : bounce_stats != nullptr) return hipErrorInvalidValue;
    const dim3 g(fa->n_tiles), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    bool built = true;
    rq_for_classes(fa, [&](auto gq, auto cub) {
        constexpr bool GQ = decltype(gq)::value, CUB = decltype(cub)::value;
        auto go = [&](auto bnc, auto cnt) {
            constexpr bool BNC = decltype(bnc)::value, CNT = decltype(cnt)::value;
            if constexpr (GQ && CUB && BNC && CNT) built = false; // (not built: see the head of this file; rt_create's decision is false where it would be needed)
            else hipLaunchKernelGGL((stream_cull_groups_frame_kernel<GQ, CUB, BNC, CNT>), g, block, 0, stream, *fa, qa, ca, ga, bounce_stats, s, lt, camx, camy, fb);
        };
        if (bounce) ca.stats ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
        else ca.stats ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
    });
    return built ? hipGetLastError() : hipErrorInvalidValue;
}
