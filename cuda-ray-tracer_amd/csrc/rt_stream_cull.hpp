// rt_stream_cull.hpp -- the unit-sphere loops of the streamed frame kernel with whole chunks culled (RT_FLAG_STREAM_CULL; include/mi355rt.h,
// DESIGN.md section 25).  rt_stream.hpp's sq_tables stages every 64-entry chunk of the unit-sphere table; here a chunk is staged only if
// its BOUND -- one UsEntry per chunk, formed by rtp::pack_chunk_bound from the chunk's members -- passes the predicate that the members
// would be asked next: sphere_in_cone for the primary rays of an 8 x 8 block, sphere_relevant for the shadow rays of the wave's hits
// towards one light.  A staged chunk runs sq_tables' body; the other class tables (general quadrics, planes, degree 3) go through
// sq_tables itself, untouched.  A "skip" for a bound implies a "skip" for every member (rt_scene_pack.hpp, pack_chunk_bound), and a
// skipped member's root could not have been accepted, so every query returns what sq_query returns.
// The bounds and the ball are wave-uniform: lane j reads bound g * 64 + j with vector loads, nothing of them goes to LDS.  Nothing here
// is workgroup-wide: no barrier, the LDS idiom is sq_stage_chunk's.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_CULL_HPP
#define RT_STREAM_CULL_HPP

#include <hip/hip_runtime.h>

#include "rt_wave_ball.hpp"    // the ball around the wave's hit points (wave_hit_ball), wave_min and wave_max
#include "rt_stream_shade.hpp" // the shading loop whose policy ends this file; sq_query and the staging idiom (rt_stream.hpp)

namespace RT_SYM(rtk) {

// what the culling kernel gets beside stream_frame_kernel's arguments
struct StreamCullArgs {
    const UsEntry *bounds;      // [n_chunks], chunk c = entries 64 c .. of the unit-sphere table
    unsigned long long *stats;  // 8 words (rt_debug_stream_cull), or NULL: nothing is counted
    uint32_t n_chunks;
    uint32_t pad;
};

// (host) a context's chunks (rt_launch.h) as the kernels take them; false: the bounds do not belong to this scene's unit-sphere table.  The one
// rule every culled launcher refuses by.
static inline bool sc_cull_args(const FrameArgs *fa, const ChunkTables *chunks, StreamCullArgs &ca)
{
    if (chunks->n_chunks != (fa->n_us + SQ_CHUNK - 1u) / SQ_CHUNK || (chunks->n_chunks && !chunks->bounds)) return false;
    ca = StreamCullArgs{reinterpret_cast<const UsEntry *>(chunks->bounds), chunks->stats, chunks->n_chunks, 0u};
    return true;
}

// a wave's work words (rt_debug_stream_cull); wave-uniform, touched only behind a wave-uniform `if (on)`
struct ScStats {
    bool on;
    uint32_t w[7];
};

// a wave's work words w[0 .. N) added to dst[0 .. N) at the wave's end: one vector atomic per word, lane i adds word i (`mine`: what a
// lane beyond N adds to its own word, if anything)
template <uint32_t N>
__device__ __forceinline__ void sc_flush(const uint32_t (&w)[N], unsigned long long *dst, uint32_t lane, uint32_t mine = 0u)
{
#pragma unroll
    for (uint32_t i = 0; i < N; i++) mine = lane == i ? w[i] : mine;
    if (mine) atomicAdd(dst + lane, (unsigned long long) mine);
}

struct ScBound { // what the predicates read of a bound
    double kx, ky, kz, r, inv_r;
};
// lane j's bound of the group of 64 chunks that starts at chunk g (zeroes beyond the table's end: never asked about).  (Loading group 0
// once per wave instead of once per query was tried: ten more registers, no difference in any measured case.)
__device__ __forceinline__ ScBound sc_load_bound(const StreamCullArgs &ca, uint32_t g, uint32_t lane)
{
    ScBound b{0.0, 0.0, 0.0, 0.0, 0.0};
    if (g + lane < ca.n_chunks) {
        const UsEntry *src = ca.bounds + g + lane;
        b = ScBound{src->kx, src->ky, src->kz, src->r, src->inv_r};
    }
    return b;
}
__device__ __forceinline__ UsEntry sc_entry(const ScBound &b) // ... as the entry sphere_relevant takes
{
    UsEntry e{};
    e.kx = b.kx; e.ky = b.ky; e.kz = b.kz; e.r = b.r; e.inv_r = b.inv_r;
    return e;
}

// sq_tables' sweep of one staged chunk: the entries in `it` (wave-uniform) against the lanes' rays, roots where they are needed
template <bool OCCLUSION>
__device__ __forceinline__ void sc_sweep(const UsEntry *s_us, unsigned long long it, const Mono &m, bool quad, double four_t2, bool use, double t_max, double &best_t,
                                         int &best)
{
    unsigned long long cand = 0;
    while (it) {
        const int b = __builtin_ctzll(it);
        it &= it - 1;
        const UsEntry e = s_us[b];
        const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
        cand |= need ? (1ull << b) : 0ull;
    }
    if (!use) cand = 0;
    while (cand && !(OCCLUSION && best != 0)) {
        const int b = __builtin_ctzll(cand);
        cand &= cand - 1;
        const UsEntry e = s_us[b];
        rq_take<OCCLUSION>(solve_quadlin(m.u2, us_t1(e, m), us_t0(e, m)), (int) e.orig, t_max, best_t, best);
    }
}

// sq_query for the primary rays of a block (nearest hit, segment 0).  While the block's cone is on, lane j asks sphere_in_cone about chunk
// bound g * 64 + j and only the surviving chunks are staged; inside a staged chunk the per-sphere cone body of sq_tables runs unchanged.
// Without a cone (a lane outside the tables' proof) this is sq_query.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void sc_query_primary(const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane,
                                                 const D3 &o, const D3 &d, bool use, double &best_t, int &best, ScStats &st)
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
    for (uint32_t g = 0; g < ca.n_chunks; g += SQ_CHUNK) {
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
    RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
    rest.n_us = 0u;
    sq_tables<HAS_GQ, HAS_CUBIC, false>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, MAX_T, best_t, best);
}

// sq_query for the shadow rays (o, d) of the wave's hits towards light lt (occlusion), all of which start within ball.R of the ball's
// centre.  Level 1: lane = chunk, sphere_relevant about the chunk's bound; level 2: lane = entry of a staged chunk, sphere_relevant about
// the entry itself; only the survivors are swept.  The occlusion early-out stays behind every chunk.  Lanes whose ray is outside the
// tables' proof go through rq_plain over all objects, as in sq_query.  The caller has decided that this light may be culled for.
template <bool HAS_GQ, bool HAS_CUBIC, bool SPHERICAL>
__device__ __forceinline__ void sc_query_shadow(const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane,
                                                const D3 &o, const D3 &d, bool use, const Ball &ball, const DevLight &lt, double t_max, int &best, ScStats &st)
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
    for (uint32_t g = 0; !decided && g < ca.n_chunks; g += SQ_CHUNK) {
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
    if (!decided) {
        RayQueryArgs rest = qa;
        rest.n_us = 0u;
        sq_tables<HAS_GQ, HAS_CUBIC, true>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, t_max, unused_t, best);
    }
    if (plain != 0ull) rq_plain<true>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, t_max, unused_t, best);
}

// The shading policy (rt_stream_shade.hpp) of a wave whose lanes are the pixels of one 8 x 8 block: segment 0 culled by the block's cone,
// the shadow rays of a segment by the ball around the wave's hit points, bounce rays (the nearest hit of segments >= 1) swept in full.
struct ScSegment {
    Ball ball;
    bool cull; // false: a non-finite hit point, test everything in this segment
};
struct ScShade {
    using Segment = ScSegment;
    const RayQueryArgs qa; // (qa and ca by value: held by reference, the bounce sweeps of stream_cull_frame_kernel came out 4.7 % slower on a
    const StreamCullArgs ca; // mirrored field -- profiles/stream_shared_loop.txt)
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave
    ScStats &st;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t k, uint32_t lane, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        if (k == 0u) sc_query_primary<HAS_GQ, HAS_CUBIC>(qa, ca, scene, slice, lane, o, d, use, best_t, best, st); // (fa.cull != 0: the context's decision)
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
            if (spherical) sc_query_shadow<HAS_GQ, HAS_CUBIC, true>(qa, ca, scene, slice, lane, so, sd, use, seg.ball, lt, max_t, blocked, st);
            else sc_query_shadow<HAS_GQ, HAS_CUBIC, false>(qa, ca, scene, slice, lane, so, sd, use, seg.ball, lt, max_t, blocked, st);
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
