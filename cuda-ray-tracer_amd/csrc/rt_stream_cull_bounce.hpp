// rt_stream_cull_bounce.hpp -- the nearest-hit query of the bounce rays of a culled streamed frame with whole chunks of the unit-sphere
// table culled per ray (RT_FLAG_STREAM_CULL_BOUNCE; include/mi355rt.h).  rt_stream_cull.hpp culls for rays that
// share something -- the origin of a block's primary rays, the light of a segment's shadow rays; bounce rays share nothing, so every lane
// asks about its OWN ray: rtm::ray_reaches (rt_ray_bound.hpp), which is sphere_relevant<false> for the half-line from the ray's origin.
// Loop shape: lane = ray.  The bound of chunk c is read at a wave-uniform address, every lane forms its own verdict, one ballot says
// whether any lane in use reaches the bound; only then the chunk is staged (sq_stage_chunk) and swept (sc_sweep) with `use` narrowed to the
// lanes that reach it.  (Lane = chunk with the rays broadcast by readlane was not built: by an instruction count it needs 64 x 9
// readlanes per group of bounds and still owes every lane its own mask of chunks; here the ballot IS that mask.)  A lane that does
// not reach a bound has no acceptable root in the chunk, so masking it changes no result.  The order of staging does not matter: the
// acceptance rule is rtm::accept's (nearest, lowest `orig` on a tie).
// Nothing of the bounds goes to LDS, there is no workgroup barrier, and no lane leaves before the wave's last ballot.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_CULL_BOUNCE_HPP
#define RT_STREAM_CULL_BOUNCE_HPP

#include <hip/hip_runtime.h>

#include "rt_stream_cull.hpp" // (first: rt_shade.hpp has to be read before rt_wavefront_math.hpp, as rt_rayquery.hpp arranges)
#include "rt_ray_bound.hpp"

namespace RT_SYM(rtk) {

static_assert(RB_PLAIN_ABOVE == RQ_PLAIN_ABOVE, "ray_bound culls only for rays the class tables are proven for");

// a wave's bounce work words (rt_debug_stream_cull_bounce); wave-uniform, touched only behind a wave-uniform `if (on)`
struct ScBounceStats {
    bool on;
    uint32_t w[5];
};

// sq_query for the bounce rays (o, d) of the lanes in `use` (nearest hit): origins and directions differ per lane.  Lanes whose ray is
// outside the tables' proof go through rq_plain over all objects, as in sc_query_shadow.  The other class tables go through sq_tables.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void sc_query_bounce(const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane,
                                                const D3 &o, const D3 &d, bool use, double &best_t, int &best, ScBounceStats &bs)
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
    if (bs.on) {
        const uint32_t cullable = (uint32_t) __popcll(__ballot(usep && rb.cull));
        bs.w[0] += ca.n_chunks;
        bs.w[2] += cullable * ca.n_chunks;
        bs.w[4] += cullable == 0u ? 1u : 0u;
    }
    for (uint32_t c = 0; c < ca.n_chunks; c++) {
        const UsEntry *src = ca.bounds + c; // (wave-uniform)
        const bool reach = usep && ray_reaches(sc_entry(ScBound{src->kx, src->ky, src->kz, src->r, src->inv_r}), rb);
        const unsigned long long lanes = __ballot(reach);
        if (bs.on) {
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
    RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
    rest.n_us = 0u;
    sq_tables<HAS_GQ, HAS_CUBIC, false>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, MAX_T, best_t, best);
    if (plain != 0ull) rq_plain<false>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, MAX_T, best_t, best);
}

} // namespace RT_SYM(rtk)

#endif
