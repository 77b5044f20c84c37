// rt_stream_cull_groups.hpp -- the culled unit-sphere loops of the streamed frame kernel under a second level of bounds
// (RT_FLAG_STREAM_CULL_GROUPS; include/mi355rt.h).  rt_stream_cull.hpp asks one verdict per chunk bound, 64 bounds
// per trip of its loops, and rt_stream_cull_bounce.hpp one per chunk, lane and bounce ray; at 100 000 spheres that is 1 563 verdicts per
// query about bounds that are almost all nowhere near the query.  Here a GROUP is 64 consecutive chunks -- exactly one trip `g = 64 G` of
// those loops -- and its bound is rtp::pack_chunk_bound over the group's chunk bounds (rt_scene_pack.hpp: the proof there never uses that
// the members are scene spheres, so "group skipped" implies "every chunk bound skipped" implies "every sphere skipped").  A query asks
// its own predicate about the group bounds first and runs the trip of rt_stream_cull.hpp's loop only for the groups that pass:
//   primary, shadow   lane j loads group bound 64 B + j and asks sphere_in_cone / sphere_relevant with the query's own cone / ball and light;
//                     one ballot is the wave-uniform mask of the groups to enter, held in scalars: the group bound is dead before the first
//                     chunk bound is loaded.  The groups are entered in ascending order, and inside one the trip's text is the twin's, so
//                     the chunks staged, their order and the place of the occlusion early-out are the twin's.
//   bounce            lane = ray, as in sc_query_bounce: the group bound is read at a wave-uniform address, every lane asks ray_reaches
//                     about its own ray, one ballot decides: no lane in use reaches the group -> its 64 chunks are skipped, else the twin's
//                     per-chunk body runs with `use` unchanged.
// Nothing of the bounds goes to LDS, there is no workgroup barrier, and no lane leaves before the wave's last ballot.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_CULL_GROUPS_HPP
#define RT_STREAM_CULL_GROUPS_HPP

#include <hip/hip_runtime.h>

#include "rt_stream_cull_bounce.hpp" // sc_query_bounce's pieces over rt_stream_cull.hpp's loops, bounds and sweep

namespace RT_SYM(rtk) {

constexpr uint32_t SG_FANOUT = 64u; // chunks per group: one trip of the twin's loops, one lane per chunk bound
static_assert(SG_FANOUT == SQ_CHUNK, "a group is one trip of rt_stream_cull.hpp's loops: lane j = chunk 64 G + j");

// what the groups kernel gets beside stream_cull_frame_kernel's arguments: the group table travels in a record of its own
struct StreamGroupArgs {
    const UsEntry *groups;     // [n_groups], group G = chunks 64 G .. of the chunk bounds
    unsigned long long *stats; // 8 words (rt_debug_stream_groups), or NULL: nothing is counted
    uint32_t n_groups;
    uint32_t pad;
};

// (host) a context's chunks and groups (rt_launch.h) as the kernels take them; false: the chunk bounds do not belong to this scene's
// unit-sphere table (sc_cull_args' rule), or the group table is not one bound per 64 of those chunks.  The one rule the groups launcher refuses by.
static inline bool sg_group_args(const FrameArgs *fa, const ChunkTables *ct, const GroupTables *gt, StreamCullArgs &ca, StreamGroupArgs &ga)
{
    if (!sc_cull_args(fa, ct, ca)) return false;
    if (gt->n_groups != (ca.n_chunks + SG_FANOUT - 1u) / SG_FANOUT || (gt->n_groups && !gt->groups)) return false;
    if ((gt->stats == nullptr) != (ca.stats == nullptr)) return false; // (both or neither: one `on` per wave)
    ga = StreamGroupArgs{reinterpret_cast<const UsEntry *>(gt->groups), gt->stats, gt->n_groups, 0u};
    return true;
}

// a wave's group work words (rt_debug_stream_groups); wave-uniform, touched only behind a wave-uniform `if (on)` (ScStats::on)
struct SgStats {
    uint32_t w[6];
};

// lane j's bound of the block of 64 groups that starts at group b (zeroes beyond the table's end: never asked about)
__device__ __forceinline__ ScBound sg_load_group(const StreamGroupArgs &ga, uint32_t b, uint32_t lane)
{
    ScBound gb{0.0, 0.0, 0.0, 0.0, 0.0};
    if (b + lane < ga.n_groups) {
        const UsEntry *src = ga.groups + b + lane;
        gb = ScBound{src->kx, src->ky, src->kz, src->r, src->inv_r};
    }
    return gb;
}

// sc_query_primary with the trips of its chunk loop chosen by the group bounds: lane j asks sphere_in_cone about group bound 64 B + j, and
// only the groups that reach into the block's cone run the twin's trip g = 64 G.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void sg_query_primary(const RayQueryArgs &qa, const StreamCullArgs &ca, const StreamGroupArgs &ga, const unsigned char *__restrict__ scene,
                                                 unsigned char *slice, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best, ScStats &st, SgStats &gs)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    if (__ballot(use && !proven) != 0ull) { // (wave-uniform) no cone: nothing to cull with
        sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, false, MAX_T, best_t, best);
        return;
    }
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    const SqCone cone = sq_block_cone(d);
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const bool quad = fabs(m.u2) > EPS;
    const double four_t2 = 4.0 * m.u2;
    const bool usep = use && proven;
    for (uint32_t b = 0; b < ga.n_groups; b += SG_FANOUT) {
        const ScBound gb = sg_load_group(ga, b, lane);
        unsigned long long groups = __ballot(b + lane < ga.n_groups && sphere_in_cone(gb.kx, gb.ky, gb.kz, gb.r, gb.inv_r, m.o, cone.axis, cone.cos_t));
        if (st.on) {
            gs.w[0] += (ga.n_groups - b < SG_FANOUT) ? ga.n_groups - b : SG_FANOUT;
            gs.w[1] += (uint32_t) __popcll(groups);
        }
        while (groups) { // wave-uniform: the groups that reach into the block's cone, in ascending order
            const uint32_t g = (b + (uint32_t) __builtin_ctzll(groups)) * SG_FANOUT; // the group's first chunk: the twin's trip g
            groups &= groups - 1;
            const ScBound bd = sc_load_bound(ca, g, lane);
            unsigned long long chunks = __ballot(g + lane < ca.n_chunks && sphere_in_cone(bd.kx, bd.ky, bd.kz, bd.r, bd.inv_r, m.o, cone.axis, cone.cos_t));
            if (st.on) {
                st.w[0] += (ca.n_chunks - g < SQ_CHUNK) ? ca.n_chunks - g : SQ_CHUNK;
                st.w[1] += (uint32_t) __popcll(chunks);
            }
            while (chunks) { // wave-uniform: the chunks that reach into the block's cone
                const uint32_t base = (g + (uint32_t) __builtin_ctzll(chunks)) * SQ_CHUNK;
                chunks &= chunks - 1;
                const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
                const UsEntry mine = sq_stage_chunk(g_us, base, end, lane, slice);
                const bool rel = base + lane < end && sphere_in_cone(mine.kx, mine.ky, mine.kz, mine.r, mine.inv_r, m.o, cone.axis, cone.cos_t);
                sc_sweep<false>(s_us, __ballot(rel), m, quad, four_t2, usep, MAX_T, best_t, best);
            }
        }
    }
    RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
    rest.n_us = 0u;
    sq_tables<HAS_GQ, HAS_CUBIC, false>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, MAX_T, best_t, best);
}

// sc_query_shadow likewise: lane j asks sphere_relevant about group bound 64 B + j with the segment's ball and the light; the occlusion
// early-out stays behind every chunk and ends the group loops as it ends the twin's.
template <bool HAS_GQ, bool HAS_CUBIC, bool SPHERICAL>
__device__ __forceinline__ void sg_query_shadow(const RayQueryArgs &qa, const StreamCullArgs &ca, const StreamGroupArgs &ga, const unsigned char *__restrict__ scene,
                                                unsigned char *slice, uint32_t lane, const D3 &o, const D3 &d, bool use, const Ball &ball, const DevLight &lt, double t_max,
                                                int &best, ScStats &st, SgStats &gs)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    const unsigned long long plain = __ballot(use && !proven);
    const bool usep = use && proven;
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const bool quad = fabs(m.u2) > EPS;
    const double four_t2 = 4.0 * m.u2;
    double unused_t = INFINITY;
    bool decided = __ballot(usep && best == 0) == 0ull; // (wave-uniform)
    for (uint32_t b = 0; !decided && b < ga.n_groups; b += SG_FANOUT) {
        const ScBound gb = sg_load_group(ga, b, lane);
        unsigned long long groups = __ballot(b + lane < ga.n_groups && sphere_relevant<SPHERICAL>(sc_entry(gb), ball, lt));
        if (st.on) {
            gs.w[2] += (ga.n_groups - b < SG_FANOUT) ? ga.n_groups - b : SG_FANOUT;
            gs.w[3] += (uint32_t) __popcll(groups);
        }
        while (groups && !decided) {
            const uint32_t g = (b + (uint32_t) __builtin_ctzll(groups)) * SG_FANOUT; // the group's first chunk: the twin's trip g
            groups &= groups - 1;
            const ScBound bd = sc_load_bound(ca, g, lane);
            unsigned long long chunks = __ballot(g + lane < ca.n_chunks && sphere_relevant<SPHERICAL>(sc_entry(bd), ball, lt));
            if (st.on) {
                st.w[2] += (ca.n_chunks - g < SQ_CHUNK) ? ca.n_chunks - g : SQ_CHUNK;
                st.w[3] += (uint32_t) __popcll(chunks);
            }
            while (chunks && !decided) {
                const uint32_t base = (g + (uint32_t) __builtin_ctzll(chunks)) * SQ_CHUNK;
                chunks &= chunks - 1;
                const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
                const UsEntry mine = sq_stage_chunk(g_us, base, end, lane, slice);
                const unsigned long long it = __ballot(base + lane < end && sphere_relevant<SPHERICAL>(mine, ball, lt));
                if (st.on) {
                    st.w[4] += end - base;
                    st.w[5] += (uint32_t) __popcll(it);
                }
                sc_sweep<true>(s_us, it, m, quad, four_t2, usep, t_max, unused_t, best);
                decided = __ballot(usep && best == 0) == 0ull;
            }
            if (st.on && chunks) st.w[3] -= (uint32_t) __popcll(chunks); // (left unstaged by the early-out)
        }
        if (st.on && groups) gs.w[3] -= (uint32_t) __popcll(groups); // (left unentered by the early-out)
    }
    if (!decided) {
        RayQueryArgs rest = qa;
        rest.n_us = 0u;
        sq_tables<HAS_GQ, HAS_CUBIC, true>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, t_max, unused_t, best);
    }
    if (plain != 0ull) rq_plain<true>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, t_max, unused_t, best);
}

// sc_query_bounce with its chunk loop cut into groups: the bound of group G is read at a wave-uniform address, every lane asks ray_reaches
// about its own ray, and the 64 chunks of a group that no lane in use reaches are passed over.  An entered group runs the twin's body per
// chunk, `use` as the twin narrows it.  The twin's words count what this loop asks and stages: [0] and [2] the chunk verdicts of the
// entered groups, [1] and [3] as ever (a chunk of a skipped group is reached by no lane).
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void sg_query_bounce(const RayQueryArgs &qa, const StreamCullArgs &ca, const StreamGroupArgs &ga, const unsigned char *__restrict__ scene,
                                                unsigned char *slice, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best, bool on,
                                                ScBounceStats &bs, SgStats &gs)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    const unsigned long long plain = __ballot(use && !proven);
    const bool usep = use && proven;
    const RayBound rb = ray_bound(o, d);
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const bool quad = fabs(m.u2) > EPS;
    const double four_t2 = 4.0 * m.u2;
    uint32_t cullable = 0u;
    if (on) {
        cullable = (uint32_t) __popcll(__ballot(usep && rb.cull));
        bs.w[4] += cullable == 0u ? 1u : 0u;
        gs.w[4] += ga.n_groups;
    }
    for (uint32_t G = 0; G < ga.n_groups; G++) {
        const UsEntry *gsrc = ga.groups + G; // (wave-uniform)
        const bool greach = usep && ray_reaches(sc_entry(ScBound{gsrc->kx, gsrc->ky, gsrc->kz, gsrc->r, gsrc->inv_r}), rb);
        if (__ballot(greach) == 0ull) continue; // (wave-uniform) no lane in use can meet a member of any of the group's chunks
        const uint32_t first = G * SG_FANOUT, last = (first + SG_FANOUT < ca.n_chunks) ? first + SG_FANOUT : ca.n_chunks;
        if (on) {
            gs.w[5] += 1u;
            bs.w[0] += last - first;
            bs.w[2] += cullable * (last - first);
        }
        for (uint32_t c = first; c < last; c++) {
            const UsEntry *src = ca.bounds + c; // (wave-uniform)
            const bool reach = usep && ray_reaches(sc_entry(ScBound{src->kx, src->ky, src->kz, src->r, src->inv_r}), rb);
            const unsigned long long lanes = __ballot(reach);
            if (on) {
                bs.w[1] += lanes != 0ull ? 1u : 0u;
                bs.w[3] += (uint32_t) __popcll(__ballot(reach && rb.cull));
            }
            if (lanes == 0ull) continue; // (wave-uniform) no lane in use can meet a member
            const uint32_t base = c * SQ_CHUNK;
            const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
            (void) sq_stage_chunk(g_us, base, end, lane, slice);
            const unsigned long long it = end - base < SQ_CHUNK ? (1ull << (end - base)) - 1ull : ~0ull;
            sc_sweep<false>(s_us, it, m, quad, four_t2, reach, MAX_T, best_t, best);
        }
    }
    RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
    rest.n_us = 0u;
    sq_tables<HAS_GQ, HAS_CUBIC, false>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, MAX_T, best_t, best);
    if (plain != 0ull) rq_plain<false>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, MAX_T, best_t, best);
}

// The shading policy (rt_stream_shade.hpp) of a wave whose lanes are the pixels of one 8 x 8 block: ScShade with every culled query
// asked about the group bounds first.  BOUNCE: the nearest hit of segments >= 1 is sg_query_bounce (the context's bounce decision);
// false: sq_query's full sweep, as in ScShade.
template <bool BOUNCE>
struct SgShade {
    using Segment = ScSegment;
    const RayQueryArgs qa; // (by value, as in ScShade)
    const StreamCullArgs ca;
    const StreamGroupArgs ga;
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave
    ScStats &st;
    ScBounceStats &bs;
    SgStats &gs;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t k, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        if (k == 0u) sg_query_primary<HAS_GQ, HAS_CUBIC>(qa, ca, ga, scene, slice, lane, o, d, use, best_t, best, st, gs); // (fa.cull != 0: the context's decision)
        else if (BOUNCE) sg_query_bounce<HAS_GQ, HAS_CUBIC>(qa, ca, ga, scene, slice, lane, o, d, use, best_t, best, st.on, bs, gs);
        else sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, false, MAX_T, best_t, best); // bounce rays: a full sweep
    }
    __device__ __forceinline__ Segment segment(bool hit, const D3 &sp) const
    {
        Segment seg;
        seg.cull = wave_hit_ball(hit, sp, seg.ball);
        return seg;
    }
    // Not culled for: a directional light with |d|^2 <= EPS (the reference's linear branch is not geometry).
    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void occluded(const Segment &seg, uint32_t lane, const DevLight &lt, const D3 &so, const D3 &sd, bool use, double max_t, int &blocked) const
    {
        const bool spherical = lt.spherical != 0;
        if (seg.cull && (spherical || fabs(lt.u2) > EPS)) { // (wave-uniform)
            if (spherical) sg_query_shadow<HAS_GQ, HAS_CUBIC, true>(qa, ca, ga, scene, slice, lane, so, sd, use, seg.ball, lt, max_t, blocked, st, gs);
            else sg_query_shadow<HAS_GQ, HAS_CUBIC, false>(qa, ca, ga, scene, slice, lane, so, sd, use, seg.ball, lt, max_t, blocked, st, gs);
        } else {
            double unused_t = INFINITY;
            sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, use, false, max_t, unused_t, blocked);
            if (st.on) st.w[6] += 1u;
        }
    }
    __device__ __forceinline__ void first_hit(int, double, const D3 &, const D3 &) const {}
};

} // namespace RT_SYM(rtk)

#endif
