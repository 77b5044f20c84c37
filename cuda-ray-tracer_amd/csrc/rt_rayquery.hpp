// rt_rayquery.hpp -- what the kernels for caller-supplied rays share (rt_rays.hip: closest hit and occlusion; rt_shade_rays.hip: the
// reference's colour; rt_paths.hip: the bounces): the scene-layout argument words, the class tables in LDS, the object loops for one ray
// per lane -- through the tables where they are proven, through the dense expansion elsewhere; as a query object for the kernels' bodies
// (rt_ray_kernels.hpp): RqStaged -- and the 48-byte ray / record layouts of include/mi355rt.h.  The pixel queries (rt_gbuffer.hip; their
// bodies: rt_pixel_kernels.hpp) run the same object loop from the frame's origin, with the block's cone and the host's degree-3 records
// switched on (rq_tables<..., PRIMARY = true>); their query object over the tables in LDS is RqPixels.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_RAYQUERY_HPP
#define RT_RAYQUERY_HPP

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt_shade.hpp"          // RT_SYM and the variant's namespace
#include "rt_wavefront_math.hpp" // class-table coefficients, us_needs_solve, needs_solve, accept

namespace RT_SYM(rtk) {

// the scene-layout words of FrameArgs (all a ray query needs of it), the number of rays and what a NULL t_max array stands for
struct RayQueryArgs {
    uint32_t n_obj, n_us, n_gq, n_lin, n_cub;
    uint32_t off_gq, off_lin, off_cub; // byte offsets into the staged tables (i.e. relative to FrameArgs::off_us)
    uint32_t off_us, tab_bytes;        // the tables in the scene blob: [UsEntry][GqEntry][LinEntry][uint32 cubic indices], each padded to 16 bytes
    uint32_t n;
};

struct RqTables {
    const UsEntry *us;
    const GqEntry *gq;
    const LinEntry *lin;
    const uint32_t *cub;
};

// Above this magnitude a product of three components (times 3) can overflow, and a coefficient that is exactly zero then no longer
// contributes an exact zero to the reference's 20-term sums (0 * inf = NaN): the class tables, which leave those terms out, are only
// proven for rays below it.  NaN and +-inf components fail the comparison too.
constexpr double RQ_PLAIN_ABOVE = 1e100;

__device__ __forceinline__ bool rq_tables_proven(const D3 &o, const D3 &d)
{
    // (every component on its own: fmax would drop a NaN operand)
    return fabs(o.x) <= RQ_PLAIN_ABOVE && fabs(o.y) <= RQ_PLAIN_ABOVE && fabs(o.z) <= RQ_PLAIN_ABOVE && fabs(d.x) <= RQ_PLAIN_ABOVE &&
           fabs(d.y) <= RQ_PLAIN_ABOVE && fabs(d.z) <= RQ_PLAIN_ABOVE;
}

// The ray's monomials (rt_wavefront_math.hpp) for one object loop; NEED_CROSS: the scene holds a class that reads the cross terms
template <bool NEED_CROSS>
__device__ __forceinline__ Mono rq_mono(const D3 &o, const D3 &d)
{
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    return m;
}

// A wave's cone for the culling of primary rays against the unit spheres: on = false culls nothing.
struct SqCone {
    bool on;
    D3 axis;
    double cos_t;
};

__device__ __forceinline__ double sq_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// the cone of a wave whose lanes are the pixels of one 8 x 8 block, all from one origin: the axis from the central lane 36, the
// opening from the four corner lanes (the angle to the axis is quasi-convex on the image plane)
__device__ __forceinline__ SqCone sq_block_cone(const D3 &d)
{
    SqCone c;
    c.on = true;
    c.axis = D3{sq_readlane(d.x, 36), sq_readlane(d.y, 36), sq_readlane(d.z, 36)};
    const double ca = dot3(c.axis, d);
    const double c0 = sq_readlane(ca, 0), c1 = sq_readlane(ca, 7), c2 = sq_readlane(ca, 56), c3 = sq_readlane(ca, 63);
    const double m01 = c0 < c1 ? c0 : c1, m23 = c2 < c3 ? c2 : c3;
    c.cos_t = m01 < m23 ? m01 : m23;
    return c;
}

// The cone of a pixel query's wave (launch-uniform): the block's where the context culls and the lanes are the pixels of a block; for
// unrelated pixels (picking) a cone that culls nothing, through the same loop -- planes and picks share their kernel, so a picked pixel
// is the planes' entry in the FMA-contracted build too.  (sphere_in_cone: no cone wider than a half-space culls anything)
__device__ __forceinline__ SqCone sq_pixel_cone(bool cull, bool block, const D3 &d)
{
    SqCone cone{cull, D3{0.0, 0.0, 1.0}, block ? 1.0 : -1.0};
    if (cone.on && block) cone = sq_block_cone(d);
    return cone;
}

// One candidate's root against the query's acceptance rule.  Closest hit: rtm::accept (t >= EPS, t < MAX_T, nearest, lowest index on a
// tie).  Occlusion: t > EPS && t < t_max, both strict; a NaN on either side blocks nothing.
template <bool OCCLUSION>
__device__ __forceinline__ void rq_take(double t, int k, double t_max, double &best_t, int &best)
{
    if (OCCLUSION) {
        if (t > EPS && t < t_max) best = 1;
    } else {
        accept(t, k, best_t, best);
    }
}

// The object loops for one ray per lane, wave-uniform: the reference's loop (src/update-cpu.cpp:50-56) over the class tables, as phase A
// of the wavefront kernel runs it.  t1 / t0 and the sign of the discriminant first, the root and the division only in the lanes that
// need them (us_needs_solve / needs_solve say when the reference's solver returns nothing that `t >= EPS`, hence `t > EPS`, can
// accept); planes take their one division; degree 3 goes through the guarded Taylor test with the surface's data at the lane's own
// origin.  `use`: the lane has a ray whose answer comes from the tables.  OCCLUSION: best = 1 once something blocks; the wave leaves as
// soon as no lane is left undecided.
// PRIMARY (the pixel queries: every ray starts at the frame's origin; off for everyone else, who then passes none of the last three
// arguments): with cone.on the unit spheres are first culled against the wave's cone, one lane per sphere, and the wave sweeps only
// the survivors; the first RT_CUB_AT_MAX degree-3 objects take their data at the origin from the host's records (prim:
// FrameArgs::cub_rec, then FrameArgs::cub_abs), indexed by the wave-uniform table position.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION, bool PRIMARY = false>
__device__ __forceinline__ void rq_tables(const RayQueryArgs &qa, const RqTables &S, const DevObject *__restrict__ gobj, const Mono &m, bool use, double t_max,
                                          double &best_t, int &best, uint32_t lane = 0u, const SqCone &cone = SqCone{}, const double *prim = nullptr)
{
#define RQ_ALL_DECIDED() (OCCLUSION && __ballot(use && best == 0) == 0ull)
    const bool quad = fabs(m.u2) > EPS; // unit spheres share t2 = u2: one degree decision per ray
    const double four_t2 = 4.0 * m.u2;
    for (uint32_t base = 0; base < qa.n_us; base += 64) {
        const uint32_t end = (base + 64 < qa.n_us) ? base + 64 : qa.n_us;
        unsigned long long cand = 0;
        if (PRIMARY && cone.on) {
            bool rel = false;
            if (base + lane < end) {
                const UsEntry e = S.us[base + lane];
                rel = sphere_in_cone(e.kx, e.ky, e.kz, e.r, e.inv_r, m.o, cone.axis, cone.cos_t);
            }
            unsigned long long it = __ballot(rel);
            while (it) { // wave-uniform loop over the spheres that reach into the wave's cone
                const int b = __builtin_ctzll(it);
                it &= it - 1;
                const UsEntry e = S.us[base + b];
                const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
                cand |= need ? (1ull << b) : 0ull;
            }
        } else {
#pragma unroll 4
            for (uint32_t j = base; j < end; j++) {
                const UsEntry e = S.us[j];
                const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
                cand |= need ? (1ull << (j - base)) : 0ull;
            }
        }
        if (!use) cand = 0;
        while (cand && !(OCCLUSION && best != 0)) { // per lane: the few spheres whose root must actually be computed
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const UsEntry e = S.us[base + b];
            rq_take<OCCLUSION>(solve_quadlin(m.u2, us_t1(e, m), us_t0(e, m)), (int) e.orig, t_max, best_t, best);
        }
        if (RQ_ALL_DECIDED()) return;
    }
    for (uint32_t base = 0; HAS_GQ && base < qa.n_gq; base += 64) {
        const uint32_t end = (base + 64 < qa.n_gq) ? base + 64 : qa.n_gq;
        unsigned long long cand = 0;
#pragma unroll 2
        for (uint32_t j = base; j < end; j++) {
            const GqEntry e = S.gq[j];
            cand |= needs_solve(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m)) ? (1ull << (j - base)) : 0ull;
        }
        if (!use) cand = 0;
        while (cand && !(OCCLUSION && best != 0)) {
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const GqEntry e = S.gq[base + b];
            rq_take<OCCLUSION>(solve_quadlin(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m)), (int) e.orig, t_max, best_t, best);
        }
        if (RQ_ALL_DECIDED()) return;
    }
    for (uint32_t j = 0; j < qa.n_lin; j++) { // planes: every lane needs the one division, nothing to defer
        const LinEntry e = S.lin[j];
        const double t1 = lin_t1(e, m);
        const double t0 = lin_t0(e, m);
        const double t = (fabs(t1) > EPS) ? -t0 / t1 : -1.0;
        if (use) rq_take<OCCLUSION>(t, (int) e.orig, t_max, best_t, best);
    }
    if (HAS_CUBIC) {
        if (RQ_ALL_DECIDED()) return;
        for (uint32_t j = 0; j < qa.n_cub; j++) {
            const uint32_t k = (uint32_t) __builtin_amdgcn_readfirstlane((int) S.cub[j]);
            if (use && !(OCCLUSION && best != 0)) {
                // the guarded Taylor test of the render kernels (rt_math.hpp: cubic_guarded, dense expansion where it refuses); the surface's
                // data at the ray's origin is formed per lane: there is no host record for arbitrary origins
                CubicAt ca;
                CubicAbs ab;
                if (PRIMARY && j < RT_CUB_AT_MAX) { // ... but for the frame's, as in rt_render
                    const double *r = prim + j * RT_CUB_REC, *a = prim + RT_CUB_AT_MAX * RT_CUB_REC + j * 4u;
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
            if (RQ_ALL_DECIDED()) return;
        }
    }
#undef RQ_ALL_DECIDED
}

// The plain path: every object in index order through the reference's own expression, the dense 20-term expansion and its solver
// (rtm::intersect_cubic = intersect_ray, include/surface_impl.h:21-155, whatever the object's degree).  For rays the class tables are
// not proven for (rq_tables_proven): non-finite or astronomically large components.  Rare, so nothing here is tuned; the solver stays
// out of line (inlined, its expansion would set the register count of the whole kernel: 215 VGPRs instead of the callee's 152).
template <bool OCCLUSION>
__device__ __forceinline__ void rq_plain(const RayQueryArgs &qa, const DevObject *__restrict__ gobj, const D3 &o, const D3 &d, bool use, double t_max, double &best_t,
                                         int &best)
{
    for (uint32_t k = 0; k < qa.n_obj; k++) {
        if (use && !(OCCLUSION && best != 0)) {
            const double t = intersect_cubic(gobj[k].c, o.x, o.y, o.z, d.x, d.y, d.z);
            rq_take<OCCLUSION>(t, (int) k, t_max, best_t, best);
        }
    }
}

// The query object (rt_ray_kernels.hpp) of a workgroup that holds all class tables in LDS.  One object loop for the ray (o, d) of every
// lane in `use`: through the tables where rq_tables_proven says so, the plain path for the other lanes.  OCCLUSION: best = 1 once
// something blocks before t_max.
struct RqStaged {
    const RayQueryArgs qa; // (by value, as in ScShade: rt_stream_cull.hpp)
    const RqTables S;
    const DevObject *gobj;

    template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
    __device__ __forceinline__ void query(uint32_t, const D3 &o, const D3 &d, bool use, double t_max, double &best_t, int &best) const
    {
        constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
        const bool proven = rq_tables_proven(o, d);
        const Mono m = rq_mono<NEED_CROSS>(o, d);
        rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, use && proven, t_max, best_t, best);
        if (__ballot(use && !proven) != 0ull) rq_plain<OCCLUSION>(qa, gobj, o, d, use && !proven, t_max, best_t, best);
    }
};

// One rt_ray / rt_hit (include/mi355rt.h) as three 16-byte words
struct alignas(16) RqRay {
    double o[3], d[3];
};
struct alignas(16) RqRecord {
    double t, p[3];
    float n[3];
    int32_t object;
};
static_assert(sizeof(RqRay) == 48 && sizeof(RqRecord) == 48, "rt_ray / rt_hit layout");

// The class tables of the scene blob, copied to LDS by the whole 256-thread workgroup (ends with a barrier)
__device__ __forceinline__ RqTables rq_stage_tables(const RayQueryArgs &qa, const unsigned char *__restrict__ scene, unsigned char *smem)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(scene + qa.off_us);
    uint4 *dst = reinterpret_cast<uint4 *>(smem);
    for (uint32_t i = threadIdx.x; i < (qa.tab_bytes >> 4); i += 256u) dst[i] = src[i];
    __syncthreads();
    RqTables S;
    S.us = reinterpret_cast<const UsEntry *>(smem);
    S.gq = reinterpret_cast<const GqEntry *>(smem + qa.off_gq);
    S.lin = reinterpret_cast<const LinEntry *>(smem + qa.off_lin);
    S.cub = reinterpret_cast<const uint32_t *>(smem + qa.off_cub);
    return S;
}

// the scene-layout words of a context's FrameArgs for n rays
__host__ __device__ static inline RayQueryArgs rq_args(const FrameArgs *fa, uint32_t n)
{
    RayQueryArgs qa;
    qa.n_obj = fa->n_obj; qa.n_us = fa->n_us; qa.n_gq = fa->n_gq; qa.n_lin = fa->n_lin; qa.n_cub = fa->n_cub;
    qa.off_us = fa->off_us;
    qa.off_gq = fa->off_gq - fa->off_us; qa.off_lin = fa->off_lin - fa->off_us; qa.off_cub = fa->off_cub - fa->off_us;
    qa.tab_bytes = fa->off_mat - fa->off_us;
    qa.n = n;
    return qa;
}

// The query object of the pixel kernels (rt_pixel_kernels.hpp) of a workgroup that holds all class tables in LDS: the nearest hit of
// the primary ray (m: from the frame's origin) of every lane in `live`.  block: the wave's lanes are the pixels of one 8 x 8 block.
// The pixel family has no plain path: its rays are the camera's.
struct RqPixels {
    const bool cull; // FrameArgs::cull
    const RayQueryArgs qa;
    const RqTables S;
    const double *prim; // FrameArgs::cub_rec, then FrameArgs::cub_abs, in LDS
    const DevObject *gobj;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t lane, const Mono &m, bool live, bool block, double &best_t, int &best) const
    {
        best = -1;
        best_t = INFINITY;
        rq_tables<HAS_GQ, HAS_CUBIC, false, true>(qa, S, gobj, m, live, MAX_T, best_t, best, lane, sq_pixel_cone(cull, block, m.d), prim);
    }
};

// LDS bytes of the host's degree-3 records behind the staged tables (a multiple of 16)
constexpr uint32_t RQ_PRIM_BYTES = (uint32_t) sizeof(double) * (RT_CUB_REC + 4) * RT_CUB_AT_MAX;

// RqPixels for this workgroup: rq_stage_tables, and behind the tables the host's records of the first RT_CUB_AT_MAX degree-3 objects at
// the frame's origin (cub_rec[4][10], then cub_abs[4][4]: contiguous in FrameArgs).  Whatever else the caller wrote to LDS in front of
// this call is visible behind it: it ends with rq_stage_tables' barrier.
template <bool HAS_CUBIC>
__device__ __forceinline__ RqPixels rq_stage_pixels(const FrameArgs &fa, const unsigned char *__restrict__ scene, unsigned char *smem)
{
    const RayQueryArgs qa = rq_args(&fa, 0u);
    double *prim = reinterpret_cast<double *>(smem + qa.tab_bytes);
    if (HAS_CUBIC && threadIdx.x < (RT_CUB_REC + 4) * RT_CUB_AT_MAX) prim[threadIdx.x] = (&fa.cub_rec[0][0])[threadIdx.x];
    return RqPixels{fa.cull != 0u, qa, rq_stage_tables(qa, scene, smem), prim, reinterpret_cast<const DevObject *>(scene)};
}

// The launch ladder over the classes the scene of `fa` holds: calls launch(gq, cub) once, with std::true_type / std::false_type for
// <HAS_GQ, HAS_CUBIC> -- inside, decltype(gq)::value is the template argument of the kernel to launch.
template <typename Launch>
static inline void rq_for_classes(const FrameArgs *fa, Launch &&launch)
{
    if (fa->n_cub) {
        if (fa->n_gq) launch(std::true_type{}, std::true_type{});
        else launch(std::false_type{}, std::true_type{});
    } else {
        if (fa->n_gq) launch(std::true_type{}, std::false_type{});
        else launch(std::false_type{}, std::false_type{});
    }
}

// Launch `kernel` -- a parenthesised instantiation that names its first two template arguments GQ and CUB -- for the scene's classes
// (rq_for_classes), 256 threads per workgroup.  (A macro: a kernel template cannot be handed to a function.)
#define RK_LAUNCH(fa, kernel, g, lds, stream, ...)                                    \
    rq_for_classes(fa, [&](auto gq, auto cub) {                                       \
        constexpr bool GQ = decltype(gq)::value, CUB = decltype(cub)::value;          \
        hipLaunchKernelGGL(kernel, g, dim3(256), lds, stream, __VA_ARGS__);           \
    })

// the argument words of the colour kernels (rt_shade_rays.hip, rt_stream_queries.hip) and of the path kernels (rt_paths.hip, rt_stream_queries.hip)
struct ShadeRaysArgs {
    RayQueryArgs qa;
    uint32_t n_lights, max_refl;
    float bg[3];
};

struct PathArgs {
    RayQueryArgs qa;
    uint32_t max_refl, max_segments;
};

// One rt_path_end (include/mi355rt.h) as one 16-byte word
struct alignas(16) PathEnd {
    uint32_t segments, end;
    float ratio;
    int32_t object;
};
static_assert(sizeof(PathEnd) == 16, "rt_path_end layout");
enum : uint32_t { PATH_MISS = 0u, PATH_SURFACE = 1u, PATH_ESCAPED = 2u, PATH_CAP = 3u }; // RT_PATH_*

// the hit record of a ray (o, d) whose nearest hit is object `best` at best_t with normal nv at point p; a miss for best < 0
__device__ __forceinline__ void rq_store_record(RqRecord *__restrict__ dst_rec, int best, double best_t, const D3 &p, const D3 &nv)
{
    RqRecord r{INFINITY, {0.0, 0.0, 0.0}, {0.0f, 0.0f, 0.0f}, -1};
    if (best >= 0) {
        r.t = best_t;
        r.p[0] = p.x; r.p[1] = p.y; r.p[2] = p.z;
        r.n[0] = (float) nv.x; r.n[1] = (float) nv.y; r.n[2] = (float) nv.z;
        r.object = best;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(dst_rec); // three 16-byte stores
    const uint4 *srcw = reinterpret_cast<const uint4 *>(&r);
    dst[0] = srcw[0];
    dst[1] = srcw[1];
    dst[2] = srcw[2];
}

} // namespace RT_SYM(rtk)

#endif
