// rt_rays.hip -- ray queries for gfx950: closest hit and occlusion of caller-supplied rays (include/mi355rt.h, rt_trace_rays /
// rt_occluded_rays).
//
// What does THIS ray hit: the reference's nearest-hit loop (src/update-cpu.cpp:50-56) and its shadow loop (src/update-cpu.cpp:66-72) for
// rays the caller hands in, origin and direction per ray, the direction used exactly as given.  Compiled twice like rt_gbuffer.hip
// (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The arithmetic and the exact work removal come from
// the headers the render kernels use (rt_math.hpp, rt_wavefront_math.hpp); nothing of the render kernels' schedule applies: the rays
// of a wave are unrelated, so there is no cone, no chunk, no record per light.
// The kernel reads the scene blob and the caller's rays and writes the caller's records / flags: no camera tables, tile words,
// launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>

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

// The object loops for one ray per lane, wave-uniform as the non-cone branch of the G-buffer's nearest_hit: t1 / t0 and the sign of
// the discriminant first, the root and the division only in the lanes that need them (us_needs_solve / needs_solve say when the
// reference's solver returns nothing that `t >= EPS`, hence `t > EPS`, can accept); planes take their one division; degree 3 goes
// through the guarded Taylor test with the surface's data at the lane's own origin.  `use`: the lane has a ray whose answer comes from
// the tables.  OCCLUSION: best = 1 once something blocks; the wave leaves as soon as no lane is left undecided.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__device__ __forceinline__ void rq_tables(const RayQueryArgs &qa, const RqTables &S, const DevObject *__restrict__ gobj, const Mono &m, bool use, double t_max,
                                          double &best_t, int &best)
{
#define RQ_ALL_DECIDED() (OCCLUSION && __ballot(use && best == 0) == 0ull)
    const bool quad = fabs(m.u2) > EPS; // unit spheres share t2 = u2: one degree decision per ray
    const double four_t2 = 4.0 * m.u2;
    for (uint32_t base = 0; base < qa.n_us; base += 64) {
        const uint32_t end = (base + 64 < qa.n_us) ? base + 64 : qa.n_us;
        unsigned long long cand = 0;
#pragma unroll 4
        for (uint32_t j = base; j < end; j++) {
            const UsEntry e = S.us[j];
            const bool need = us_needs_solve(quad, four_t2, us_t1(e, m), us_t0(e, m));
            cand |= need ? (1ull << (j - base)) : 0ull;
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
                const CubicAt ca = cubic_at(gobj[k].c, m.o);
                const CubicAbs ab = cubic_abs(gobj[k].c);
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

// 256-thread workgroups, one ray per lane, a grid-stride loop over the rays (the grid is bounded by the launcher); the class tables go
// to LDS once per workgroup.  Closest hit: one rt_hit per ray.  OCCLUSION: one int32 per ray (t_max == NULL: MAX_T for every ray).
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_kernel(const RayQueryArgs qa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                        const double *__restrict__ t_max, RqRecord *__restrict__ out_rec, int32_t *__restrict__ out_blocked)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x;
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(scene + qa.off_us);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = tid; i < (qa.tab_bytes >> 4); i += 256u) dst[i] = src[i];
    }
    __syncthreads();
    RqTables S;
    S.us = reinterpret_cast<const UsEntry *>(smem);
    S.gq = reinterpret_cast<const GqEntry *>(smem + qa.off_gq);
    S.lin = reinterpret_cast<const LinEntry *>(smem + qa.off_lin);
    S.cub = reinterpret_cast<const uint32_t *>(smem + qa.off_cub);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (wave-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
        double tm = MAX_T;
        if (live) {
            const double2 *w = reinterpret_cast<const double2 *>(rays + i); // three 16-byte loads
            const double2 w0 = w[0], w1 = w[1], w2 = w[2];
            o = D3{w0.x, w0.y, w1.x};
            d = D3{w1.y, w2.x, w2.y};
            if (OCCLUSION && t_max) tm = t_max[i];
        }
        const bool proven = rq_tables_proven(o, d);
        Mono m;
        mono_set_o<NEED_CROSS>(m, o);
        mono_set_d<NEED_CROSS>(m, d);
        mono_set_od<NEED_CROSS>(m);
        double best_t = INFINITY;
        int best = OCCLUSION ? 0 : -1;
        rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, live && proven, tm, best_t, best);
        if (__ballot(live && !proven) != 0ull) rq_plain<OCCLUSION>(qa, gobj, o, d, live && !proven, tm, best_t, best);
        if (OCCLUSION) {
            if (live) out_blocked[i] = best;
        } else if (live) {
            RqRecord r{INFINITY, {0.0, 0.0, 0.0}, {0.0f, 0.0f, 0.0f}, -1};
            if (best >= 0) {
                const D3 p{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                // normal_vector in full for every class (per-lane index: a gather from global memory, per hit): the three-coefficient form
                // of a sphere differs in the sign of a zero component when the hit point has a negative-zero coordinate, which a caller's
                // origin can have
                const D3 nv = normal_vector(gobj[best].c, p);
                r.t = best_t;
                r.p[0] = p.x; r.p[1] = p.y; r.p[2] = p.z;
                r.n[0] = (float) nv.x; r.n[1] = (float) nv.y; r.n[2] = (float) nv.z;
                r.object = best;
            }
            uint4 *dst = reinterpret_cast<uint4 *>(out_rec + i); // three 16-byte stores
            const uint4 *srcw = reinterpret_cast<const uint4 *>(&r);
            dst[0] = srcw[0];
            dst[1] = srcw[1];
            dst[2] = srcw[2];
        }
    }
}

template <bool OCCLUSION>
static hipError_t launch(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    RayQueryArgs qa;
    qa.n_obj = fa->n_obj; qa.n_us = fa->n_us; qa.n_gq = fa->n_gq; qa.n_lin = fa->n_lin; qa.n_cub = fa->n_cub;
    qa.off_us = fa->off_us;
    qa.off_gq = fa->off_gq - fa->off_us; qa.off_lin = fa->off_lin - fa->off_us; qa.off_cub = fa->off_cub - fa->off_us;
    qa.tab_bytes = fa->off_mat - fa->off_us;
    qa.n = n;
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    const dim3 g(need < max_grid ? need : (max_grid ? max_grid : 1u)), block(256);
    const size_t lds = qa.tab_bytes;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    RqRecord *rec = OCCLUSION ? nullptr : reinterpret_cast<RqRecord *>(out);
    int32_t *blk = OCCLUSION ? reinterpret_cast<int32_t *>(out) : nullptr;
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((ray_query_kernel<true, true, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
        else hipLaunchKernelGGL((ray_query_kernel<false, true, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((ray_query_kernel<true, false, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
        else hipLaunchKernelGGL((ray_query_kernel<false, false, OCCLUSION>), g, block, lds, stream, qa, s, r, t_max, rec, blk);
    }
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// LDS bytes of one ray_query_kernel workgroup for this scene (the entry points refuse scenes beyond the device's limit)
extern "C" size_t RT_SYM(rt_rays_lds_bytes)(const FrameArgs *fa) { return (size_t) (fa->off_mat - fa->off_us); }

// rays = n rt_ray, out = n rt_hit, both in device memory and 16-byte aligned; at most max_grid workgroups
extern "C" hipError_t RT_SYM(rt_launch_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<false>(fa, scene, rays, nullptr, n, out, max_grid, stream);
}

// t_max = n doubles or NULL (MAX_T for every ray), out = n int32
extern "C" hipError_t RT_SYM(rt_launch_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                       uint32_t max_grid, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch<true>(fa, scene, rays, t_max, n, out, max_grid, stream);
}
