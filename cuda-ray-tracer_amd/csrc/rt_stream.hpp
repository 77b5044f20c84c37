// rt_stream.hpp -- the object loops of the ray queries (rt_rayquery.hpp: rq_tables) for scenes whose class tables do not fit a
// workgroup's LDS: the tables stay in the scene blob in global memory and go through a wave-private LDS slice, 64 entries at a time.
// The chunks are the chunks rq_tables iterates over and a chunk's body is rq_tables' body, so a query returns what rq_tables returns
// for the same ray -- whatever the scene's size.  One ray per lane; the caller owns the whole wave (all 64 lanes call, `use` says which
// of them have a ray).  Nothing here is workgroup-wide: no barrier, no shared state between waves, so the waves of a workgroup may run
// any number of queries each.  Used by the streamed frame kernel (rt_stream.hip) and by the streamed query kernels
// (rt_stream_queries.hip), the latter through the query objects at the end: SqQuery for caller-supplied rays, SqPixels for pixels.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_STREAM_HPP
#define RT_STREAM_HPP

#include <hip/hip_runtime.h>

#include "rt_rayquery.hpp" // RayQueryArgs, rq_take, rq_tables_proven, rq_plain, rq_mono, SqCone and the block's cone

namespace RT_SYM(rtk) {

constexpr uint32_t SQ_CHUNK = 64;                                    // entries per chunk: one per lane
constexpr uint32_t SQ_SLICE_BYTES = SQ_CHUNK * (uint32_t) sizeof(GqEntry); // a wave's slice, sized for the largest entry kind
static_assert(sizeof(GqEntry) >= sizeof(UsEntry) && sizeof(GqEntry) >= sizeof(LinEntry) && sizeof(GqEntry) >= sizeof(uint32_t), "slice size");

// One chunk: lane j copies entry base + j of a table in global memory to the wave's slice (16-byte pieces; 4-byte ones for the index
// list) and keeps it; lanes beyond the table's end keep zeroes and store nothing.  Behind the stores the wave-level LDS idiom of
// rt_wavefront.hip: the slice is written and read by this wave only, LDS executes a wave's accesses in order, and the fences keep the
// compiler from moving the broadcast reads in front of the stores (or the next chunk's stores in front of this chunk's reads: the
// caller runs into the same idiom again before it writes).
template <typename T>
__device__ __forceinline__ T sq_stage_chunk(const T *__restrict__ table, uint32_t base, uint32_t end, uint32_t lane, unsigned char *slice)
{
    constexpr uint32_t PIECES = sizeof(T) / 16u;
    static_assert(sizeof(T) % 16u == 0u, "whole 16-byte pieces");
    union {
        T e;
        uint4 w[PIECES];
    } u;
#pragma unroll
    for (uint32_t i = 0; i < PIECES; i++) u.w[i] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    if (base + lane < end) {
        const uint4 *src = reinterpret_cast<const uint4 *>(table + base + lane);
        uint4 *dst = reinterpret_cast<uint4 *>(slice) + lane * PIECES;
#pragma unroll
        for (uint32_t i = 0; i < PIECES; i++) u.w[i] = src[i];
#pragma unroll
        for (uint32_t i = 0; i < PIECES; i++) dst[i] = u.w[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    return u.e;
}

__device__ __forceinline__ void sq_stage_indices(const uint32_t *__restrict__ table, uint32_t base, uint32_t end, uint32_t lane, unsigned char *slice)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    if (base + lane < end) reinterpret_cast<uint32_t *>(slice)[lane] = table[base + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// rq_tables with the tables streamed.  scene: the blob (DevObject records first, the tables from qa.off_us on); slice: SQ_SLICE_BYTES of
// LDS that belong to this wave.  All control flow around the staging is wave-uniform; `use` stays a predicate.  cone.on (primary rays
// of a block, wave-uniform): the lane that loaded a sphere tests it against the block's cone, and the wave sweeps only the survivors.
// HOST_CUB (rays from the frame's origin: the pixel family, as rq_tables' PRIMARY): the first RT_CUB_AT_MAX degree-3 objects
// take their data at the origin from the host's records in `frame` (cub_rec, cub_abs), indexed by the wave-uniform table position --
// kernel arguments, read by scalar loads, nothing in LDS.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION, bool HOST_CUB = false>
__device__ __forceinline__ void sq_tables(const RayQueryArgs &qa, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane, const Mono &m, bool use,
                                          const SqCone &cone, double t_max, double &best_t, int &best, const FrameArgs *frame = nullptr)
{
#define SQ_ALL_DECIDED() (OCCLUSION && __ballot(use && best == 0) == 0ull)
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const UsEntry *g_us = reinterpret_cast<const UsEntry *>(scene + qa.off_us);
    const GqEntry *g_gq = reinterpret_cast<const GqEntry *>(scene + qa.off_us + qa.off_gq);
    const LinEntry *g_lin = reinterpret_cast<const LinEntry *>(scene + qa.off_us + qa.off_lin);
    const uint32_t *g_cub = reinterpret_cast<const uint32_t *>(scene + qa.off_us + qa.off_cub);
    const UsEntry *s_us = reinterpret_cast<const UsEntry *>(slice);
    const GqEntry *s_gq = reinterpret_cast<const GqEntry *>(slice);
    const LinEntry *s_lin = reinterpret_cast<const LinEntry *>(slice);
    const uint32_t *s_cub = reinterpret_cast<const uint32_t *>(slice);

    const bool quad = fabs(m.u2) > EPS; // unit spheres share t2 = u2: one degree decision per ray
    const double four_t2 = 4.0 * m.u2;
    for (uint32_t base = 0; base < qa.n_us; base += SQ_CHUNK) {
        const uint32_t end = (base + SQ_CHUNK < qa.n_us) ? base + SQ_CHUNK : qa.n_us;
        const UsEntry mine = sq_stage_chunk(g_us, base, end, lane, slice);
        unsigned long long cand = 0;
        if (cone.on) {
            const bool rel = base + lane < end && sphere_in_cone(mine.kx, mine.ky, mine.kz, mine.r, mine.inv_r, m.o, cone.axis, cone.cos_t);
            unsigned long long it = __ballot(rel);
            while (it) { // wave-uniform loop over the spheres that reach into the block's cone
                const int b = __builtin_ctzll(it);
                it &= it - 1;
                const UsEntry e = s_us[b];
                const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
                cand |= need ? (1ull << b) : 0ull;
            }
        } else {
#pragma unroll 4
            for (uint32_t j = 0; j < end - base; j++) {
                const UsEntry e = s_us[j];
                const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
                cand |= need ? (1ull << j) : 0ull;
            }
        }
        if (!use) cand = 0;
        while (cand && !(OCCLUSION && best != 0)) { // per lane: the few spheres whose root must actually be computed
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const UsEntry e = s_us[b];
            rq_take<OCCLUSION>(solve_quadlin(m.u2, us_t1(e, m), us_t0(e, m)), (int) e.orig, t_max, best_t, best);
        }
        if (SQ_ALL_DECIDED()) return;
    }
    for (uint32_t base = 0; HAS_GQ && base < qa.n_gq; base += SQ_CHUNK) {
        const uint32_t end = (base + SQ_CHUNK < qa.n_gq) ? base + SQ_CHUNK : qa.n_gq;
        (void) sq_stage_chunk(g_gq, base, end, lane, slice);
        unsigned long long cand = 0;
#pragma unroll 2
        for (uint32_t j = 0; j < end - base; j++) {
            const GqEntry e = s_gq[j];
            cand |= needs_solve(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m)) ? (1ull << j) : 0ull;
        }
        if (!use) cand = 0;
        while (cand && !(OCCLUSION && best != 0)) {
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const GqEntry e = s_gq[b];
            rq_take<OCCLUSION>(solve_quadlin(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m)), (int) e.orig, t_max, best_t, best);
        }
        if (SQ_ALL_DECIDED()) return;
    }
    for (uint32_t base = 0; base < qa.n_lin; base += SQ_CHUNK) { // planes: every lane needs the one division, nothing to defer
        const uint32_t end = (base + SQ_CHUNK < qa.n_lin) ? base + SQ_CHUNK : qa.n_lin;
        (void) sq_stage_chunk(g_lin, base, end, lane, slice);
        for (uint32_t j = 0; j < end - base; j++) {
            const LinEntry e = s_lin[j];
            const double t1 = lin_t1(e, m);
            const double t0 = lin_t0(e, m);
            const double t = (fabs(t1) > EPS) ? -t0 / t1 : -1.0;
            if (use) rq_take<OCCLUSION>(t, (int) e.orig, t_max, best_t, best);
        }
        if (SQ_ALL_DECIDED()) return;
    }
    if (HAS_CUBIC) {
        if (SQ_ALL_DECIDED()) return;
        for (uint32_t base = 0; base < qa.n_cub; base += SQ_CHUNK) {
            const uint32_t end = (base + SQ_CHUNK < qa.n_cub) ? base + SQ_CHUNK : qa.n_cub;
            sq_stage_indices(g_cub, base, end, lane, slice);
            for (uint32_t j = 0; j < end - base; j++) {
                const uint32_t k = (uint32_t) __builtin_amdgcn_readfirstlane((int) s_cub[j]);
                if (use && !(OCCLUSION && best != 0)) {
                    // the guarded Taylor test with the surface's data at the lane's own origin, as the ray queries form it
                    CubicAt ca;
                    CubicAbs ab;
                    if (HOST_CUB && base + j < RT_CUB_AT_MAX) { // (wave-uniform)
                        const double *r = frame->cub_rec[base + j], *a = frame->cub_abs[base + j];
                        ca = CubicAt{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
                        ab = CubicAbs{a[0], a[1], a[2], a[3]};
                    } else {
                        ca = cubic_at(gobj[k].c, m.o);
                        ab = cubic_abs(gobj[k].c);
                    }
                    bool refused;
                    const double t = intersect_cubic_taylor<false>(gobj[k].c, ca, cubic_mag_origin(ab, m.o), m.o, m.d, OCCLUSION ? t_max : MAX_T, OCCLUSION, refused);
                    rq_take<OCCLUSION>(t, (int) k, t_max, best_t, best);
                }
                if (SQ_ALL_DECIDED()) return;
            }
        }
    }
#undef SQ_ALL_DECIDED
}

// One object loop for the ray (o, d) of every lane in `use` (RqStaged::query of rt_rayquery.hpp, with the tables streamed): through the streamed tables where
// rq_tables_proven says so, the plain path behind a ballot for the other lanes.  The cone is only used while every ray of the wave is
// proven: its lanes' directions define it.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__device__ __forceinline__ void sq_query(const RayQueryArgs &qa, const unsigned char *__restrict__ scene, unsigned char *slice, uint32_t lane, const D3 &o, const D3 &d,
                                         bool use, bool block_cone, double t_max, double &best_t, int &best)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    const Mono m = rq_mono<NEED_CROSS>(o, d);
    const unsigned long long plain = __ballot(use && !proven);
    SqCone cone{false, D3{0.0, 0.0, 1.0}, 1.0};
    if (block_cone && plain == 0ull) cone = sq_block_cone(d); // (wave-uniform)
    sq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, slice, lane, m, use && proven, cone, t_max, best_t, best);
    if (plain != 0ull) rq_plain<OCCLUSION>(qa, reinterpret_cast<const DevObject *>(scene), o, d, use && !proven, t_max, best_t, best);
}

// The query object (rt_ray_kernels.hpp) of a wave that streams the tables: sq_query for unrelated rays, never a cone (qa: the kernel's own
// argument)
struct SqQuery {
    const RayQueryArgs &qa;
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave

    template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
    __device__ __forceinline__ void query(uint32_t lane, const D3 &o, const D3 &d, bool use, double t_max, double &best_t, int &best) const
    {
        sq_query<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, slice, lane, o, d, use, false, t_max, best_t, best);
    }
};

// The query object of the pixel kernels (rt_pixel_kernels.hpp) of a wave that streams the tables (RqPixels of rt_rayquery.hpp, with
// the tables streamed): the nearest hit of the primary ray (m: from the frame's origin) of every lane in `live`, the cone as there, the
// host's degree-3 records from the kernel's own arguments.  The pixel family has no plain path: sq_tables directly, not sq_query.
struct SqPixels {
    const FrameArgs &fa; // (fa, qa: the kernel's own arguments)
    const RayQueryArgs &qa;
    const unsigned char *scene;
    unsigned char *slice; // SQ_SLICE_BYTES of LDS that belong to this wave

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t lane, const Mono &m, bool live, bool block, double &best_t, int &best) const
    {
        best = -1;
        best_t = INFINITY;
        sq_tables<HAS_GQ, HAS_CUBIC, false, true>(qa, scene, slice, lane, m, live, sq_pixel_cone(fa.cull != 0u, block, m.d), MAX_T, best_t, best, &fa);
    }
};

} // namespace RT_SYM(rtk)

#endif
