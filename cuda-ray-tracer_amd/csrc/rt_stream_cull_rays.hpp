// rt_stream_cull_rays.hpp -- the streamed queries of caller-supplied rays with whole chunks of the unit-sphere table culled per ray
// (RT_FLAG_STREAM_CULL_RAYS; include/mi355rt.h).  A caller's rays share nothing, like the bounce rays of a frame: the
// loop is sc_query_bounce's (rt_stream_cull_bounce.hpp) -- lane = ray, the bound of chunk c read at a wave-uniform address, one verdict
// per lane (rtm::ray_reaches, rt_ray_bound.hpp), one ballot, the chunk staged only if some lane in use reaches it and swept (sc_sweep) for
// those lanes alone -- as one template for both kinds of query, with sc_query_shadow's wave-uniform early-out for occlusion.
// Why sc_query_bounce itself is not called for the nearest hit ("The contracted build"): it forms the ray's bound
// from the very `d` the class tables' monomials are formed from, so ray_bound's |d|^2 and Mono's u2 are one value, needed at once for
// rb.cull; under -ffp-contract=fast the compiler then fuses its products and sums, which it does not do in sq_query, and an
// RT_FLAG_FAST context would no longer return the streamed kernels' FP64 records bit for bit.  Here the bound is formed from an opaque
// copy of the direction (scr_ray_bound): the same number in the strict build, no shared subexpression in the contracted one.
// No new argument: every verdict is about the ray's whole half-line.  An occlusion query accepts EPS < t < t_max, a subset of what the
// half-line can meet, so t_max goes to the sweep alone.
// A ray nothing can be culled for (ray_bound's cull == false: |d|^2 not above EPS or not finite) answers "reaches" for every bound, as in
// sc_query_bounce: its wave stages every chunk.  Such lanes are left that way and not routed through rq_plain: a zero-direction ray that is
// `proven` has to return the class tables' answer bit for bit (the composers hold the kernels to it), and the tables are where it comes from.
// Nothing of the bounds goes to LDS, there is no workgroup barrier, and no lane leaves before the wave's last ballot.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_CULL_RAYS_HPP
#define RT_STREAM_CULL_RAYS_HPP

#include <hip/hip_runtime.h>

#include "rt_stream_cull_bounce.hpp" // ScBounceStats; rt_stream_cull.hpp's sweep and bound loads; rt_ray_bound.hpp

namespace RT_SYM(rtk) {

// rtm::ray_bound of (o, d) with the direction's components made opaque to the optimiser first: no instruction, the same bits
__device__ __forceinline__ RayBound scr_ray_bound(const D3 &o, const D3 &d)
{
    D3 dq = d;
    asm volatile("" : "+v"(dq.x), "+v"(dq.y), "+v"(dq.z));
    return ray_bound(o, dq);
}

// sq_query for the rays (o, d) of the lanes in `use`, nearest hit (t_max = MAX_T) or occlusion (roots below t_max).  Occlusion: a lane
// that is blocked asks about no further bound, and the wave leaves behind the chunk that decides its last lane (the other class tables
// are skipped then, as in sc_query_shadow).  Lanes whose ray is outside the tables' proof go through rq_plain over all objects.
// The work words are ScBounceStats' (rt_debug_stream_cull_rays): w[0] and w[2] count the chunks looked at before the early-out.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__device__ __forceinline__ void sc_query_ray(const RayQueryArgs &qa, const StreamCullArgs &ca, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane,
                                             const D3 &o, const D3 &d, bool use, double t_max, double &best_t, int &best, ScBounceStats &bs)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    const unsigned long long plain = __ballot(use && !proven);
    const bool usep = use && proven;
    const RayBound rb = scr_ray_bound(o, d);
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const bool quad = fabs(m.u2) > EPS;
    const double four_t2 = 4.0 * m.u2;
    uint32_t cullable = 0u;
    if (bs.on) {
        cullable = (uint32_t) __popcll(__ballot(usep && rb.cull));
        bs.w[4] += cullable == 0u ? 1u : 0u;
    }
    bool decided = OCCLUSION && __ballot(usep && best == 0) == 0ull; // (wave-uniform)
    for (uint32_t c = 0; !decided && c < ca.n_chunks; c++) {
        const UsEntry *src = ca.bounds + c; // (wave-uniform)
        const bool reaches = usep && ray_reaches(sc_entry(ScBound{src->kx, src->ky, src->kz, src->r, src->inv_r}), rb);
        const bool reach = reaches && !(OCCLUSION && best != 0);
        const unsigned long long lanes = __ballot(reach);
        if (bs.on) {
            bs.w[0] += 1u;
            bs.w[1] += lanes != 0ull ? 1u : 0u;
            bs.w[2] += cullable;
            bs.w[3] += (uint32_t) __popcll(__ballot(reaches && rb.cull));
        }
        if (lanes == 0ull) continue; // (wave-uniform) no undecided lane in use can meet a member
        const uint32_t base = c * SQ_CHUNK;
        const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
        (void) sq_stage_chunk(g_us, base, end, lane, slice);
        const unsigned long long it = end - base < SQ_CHUNK ? (1ull << (end - base)) - 1ull : ~0ull;
        sc_sweep<OCCLUSION>(s_us, it, m, quad, four_t2, reach, t_max, best_t, best);
        decided = OCCLUSION && __ballot(usep && best == 0) == 0ull;
    }
    if (!decided) {
        RayQueryArgs rest = qa; // the other class tables: sq_tables' own loops
        rest.n_us = 0u;
        sq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(rest, scene, slice, lane, m, usep, SqCone{false, D3{0.0, 0.0, 1.0}, 1.0}, t_max, best_t, best);
    }
    if (plain != 0ull) rq_plain<OCCLUSION>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, t_max, best_t, best);
}

// The query object (rt_ray_kernels.hpp) of a wave that culls for each of its rays: every query, a shadow ray's included, is sc_query_ray.
// It owns the wave's work words.  They count a query only if some lane is in use (wave-uniform): a wave of the grid-stride loop's last
// batch that holds no ray asks nothing and counts nothing.  The kernel adds them up at its end (sc_flush).
struct ScRayQuery {
    const RayQueryArgs &qa; // (the kernel's own arguments, by reference: held by value, ray_query_cull_kernel's loops came out at another
    const StreamCullArgs &ca; // place in the code and 3.6 % slower; DESIGN.md section 30, "Shapes")
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave
    ScBounceStats bs;

    template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
    __device__ __forceinline__ void query(uint32_t lane, const D3 &o, const D3 &d, bool use, double t_max, double &best_t, int &best)
    {
        bs.on = ca.stats != nullptr && __ballot(use) != 0ull;
        sc_query_ray<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, ca, scene, slice, lane, o, d, use, t_max, best_t, best, bs);
    }
};

} // namespace RT_SYM(rtk)

#endif
