// rt_stream_cull_pixels.hpp -- the streamed pixel queries (the G-buffer, picking, object extents) with whole chunks of the unit-sphere table
// culled by the cone of the wave's 8 x 8 block (RT_FLAG_STREAM_CULL_PIXELS; include/mi355rt.h).  SqPixels
// (rt_stream.hpp) stages every 64-entry chunk and asks sphere_in_cone about each entry; here lane j asks it about the BOUND of chunk
// g + j first (rt_stream_cull.hpp: sc_load_bound), one ballot says which chunks are staged, and a staged chunk runs the per-entry step
// of sc_query_primary: sq_stage_chunk, sphere_in_cone per entry, sc_sweep over the survivors.  The other class tables go through
// sq_tables in SqPixels' own form -- rays from the frame's origin, the host's degree-3 records from the kernel's arguments -- which is
// NOT the form sc_query_primary passes: its degree-3 answers are another kernel's.
// Why the result is SqPixels': a "skip" for a bound implies a "skip" for every member by the same predicate (rt_scene_pack.hpp,
// pack_chunk_bound), and sq_tables' per-entry cone skips exactly those members already; so the spheres tested are SqPixels' spheres, and
// the acceptance rule (nearest, lowest index on a tie) does not depend on their order.
// The monomials are the caller's (pk_gbuffer / pk_extents formed them, as for the twins): nothing here rebuilds them.  The pixel family
// has no plain path.  Picking (block == false) runs the same loop under the cone that culls nothing: every chunk is staged, so a picked
// pixel is the planes' entry by construction, in the FMA-contracted build too; picks gain nothing and pay the verdicts.
// The chunk loop is this file's own.  One function for it and sc_query_primary was built twice and changed the frame kernels' objects
// both times, so rt_stream_cull.hpp is untouched ("The loop").
// The bounds are read with vector loads, lane = chunk; nothing of them goes to LDS, there is no workgroup barrier, and no lane leaves
// before the wave's last ballot or staged chunk.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_CULL_PIXELS_HPP
#define RT_STREAM_CULL_PIXELS_HPP

#include <hip/hip_runtime.h>

#include "rt_stream_cull.hpp" // StreamCullArgs, sc_load_bound, sc_sweep, sc_flush; sq_tables, sq_stage_chunk and SqCone behind it

namespace RT_SYM(rtk) {

// a wave's work words (rt_debug_stream_cull_pixels): [0] chunk decisions, [1] chunks staged, [2] entries asked inside staged chunks,
// [3] entries swept; wave-uniform, touched only behind a wave-uniform test
struct ScPixelStats {
    uint32_t w[4];
};

// The query object of the pixel kernels (rt_pixel_kernels.hpp) of a wave that streams the tables and culls the unit-sphere chunks by
// its block's cone.  The words count a call only if some lane is live (wave-uniform): a wave of a pick's last workgroup that holds no
// pixel counts nothing.  The kernel adds them up at its end (sc_flush).
struct ScPixels {
    const FrameArgs &fa; // (fa, qa, ca: the kernel's own arguments)
    const RayQueryArgs &qa;
    const StreamCullArgs &ca;
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave
    ScPixelStats &ps;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t lane, const Mono &m, bool live, bool block, double &best_t, int &best) const
    {
        best = -1;
        best_t = INFINITY;
        const SqCone cone = sq_pixel_cone(fa.cull != 0u, block, m.d); // (on: the launcher refuses a context that does not cull)
        const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
        const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
        const bool quad = fabs(m.u2) > EPS;
        const double four_t2 = 4.0 * m.u2;
        const bool count = ca.stats != nullptr && __ballot(live) != 0ull; // (wave-uniform)
        for (uint32_t g = 0; g < ca.n_chunks; g += SQ_CHUNK) {
            const ScBound bd = sc_load_bound(ca, g, lane);
            unsigned long long chunks = __ballot(g + lane < ca.n_chunks && sphere_in_cone(bd.kx, bd.ky, bd.kz, bd.r, bd.inv_r, m.o, cone.axis, cone.cos_t));
            if (count) {
                ps.w[0] += (ca.n_chunks - g < SQ_CHUNK) ? ca.n_chunks - g : SQ_CHUNK;
                ps.w[1] += (uint32_t) __popcll(chunks);
            }
            while (chunks) { // wave-uniform: the chunks that reach into the block's cone
                const uint32_t base = (g + (uint32_t) __builtin_ctzll(chunks)) * SQ_CHUNK;
                chunks &= chunks - 1;
                const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
                const UsEntry mine = sq_stage_chunk(g_us, base, end, lane, slice);
                const unsigned long long it = __ballot(base + lane < end && sphere_in_cone(mine.kx, mine.ky, mine.kz, mine.r, mine.inv_r, m.o, cone.axis, cone.cos_t));
                if (count) {
                    ps.w[2] += end - base;
                    ps.w[3] += (uint32_t) __popcll(it);
                }
                sc_sweep<false>(s_us, it, m, quad, four_t2, live, MAX_T, best_t, best);
            }
        }
        RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops, in SqPixels' form
        rest.n_us = 0u;
        sq_tables<HAS_GQ, HAS_CUBIC, false, true>(rest, scene, slice, lane, m, live, cone, MAX_T, best_t, best, &fa);
    }
};

} // namespace RT_SYM(rtk)

#endif
