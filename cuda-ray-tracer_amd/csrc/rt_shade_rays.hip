// rt_shade_rays.hip -- the reference's colour for caller-supplied rays (include/mi355rt.h, rt_shade_rays).
//
// render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d of a ray the caller hands in, the direction used exactly as
// given: nearest hit, every light's shadow test and surface_color, the clamp, then the reflection loop with its blends -- the shading
// loop this kernel shares with the streamed kernels (rt_stream_shade.hpp: shade_loop), under the policy ShadeRaysStaged below.  Compiled
// twice like rt_rays.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The object loops are the ray
// queries' (rt_rayquery.hpp): the class tables where they are proven for the ray in hand -- decided anew for every shadow ray and every
// bounce, whose origins and directions the kernel forms itself -- and the dense expansion elsewhere.  None of the render kernels' work
// removal is used (facing-away skip, own-sphere rule, bounding-volume culling): their proofs lean on a pixel grid's rays, finite
// lights and colours, and a normalised direction.
// The kernel reads the scene blob, the lights and the caller's rays and writes the caller's pixels / records: no camera tables, tile
// words, launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_rayquery.hpp" // RayQueryArgs, the class tables in LDS, rq_tables / rq_plain, the ray and record layouts
#include "rt_stream_shade.hpp" // the shading loop

namespace RT_SYM(rtk) {

// One object loop for the ray (o, d) of every lane in `use`: through the tables where rq_tables_proven says so, the plain path for
// the other lanes.  OCCLUSION: best = 1 once something blocks before t_max.
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__device__ __forceinline__ void shade_query(const RayQueryArgs &qa, const RqTables &S, const DevObject *__restrict__ gobj, const D3 &o, const D3 &d, bool use, double t_max,
                                            double &best_t, int &best)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    const bool proven = rq_tables_proven(o, d);
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, d);
    mono_set_od<NEED_CROSS>(m);
    rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, use && proven, t_max, best_t, best);
    if (__ballot(use && !proven) != 0ull) rq_plain<OCCLUSION>(qa, gobj, o, d, use && !proven, t_max, best_t, best);
}

// The shading policy of a workgroup that holds all class tables in LDS: every query is shade_query; segment 0 stores the rt_hit of the
// lane's ray, as rt_trace_rays writes it (out_rec == NULL: nothing).
struct ShadeRaysStaged {
    using Segment = ShadeNoSegment;
    const RayQueryArgs qa; // (by value, as in ScShade: rt_stream_cull.hpp)
    const RqTables S;
    const DevObject *gobj;
    RqRecord *out_rec;
    uint64_t i;
    bool live;

    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void nearest(uint32_t, uint32_t, const D3 &o, const D3 &d, bool use, double &best_t, int &best) const
    {
        shade_query<HAS_GQ, HAS_CUBIC, false>(qa, S, gobj, o, d, use, MAX_T, best_t, best);
    }
    __device__ __forceinline__ Segment segment(bool, const D3 &) const { return Segment{}; }
    template <bool HAS_GQ, bool HAS_CUBIC>
    __device__ __forceinline__ void occluded(const Segment &, uint32_t, const DevLight &, const D3 &so, const D3 &sd, bool use, double max_t, int &blocked) const
    {
        double unused_t = INFINITY;
        shade_query<HAS_GQ, HAS_CUBIC, true>(qa, S, gobj, so, sd, use, max_t, unused_t, blocked);
    }
    __device__ __forceinline__ void first_hit(int best, double best_t, const D3 &sp, const D3 &sn) const
    {
        if (out_rec && live) rq_store_record(out_rec + i, best, best_t, sp, sn);
    }
};

// 256-thread workgroups, one ray per lane, the grid-stride loop of ray_query_kernel; the class tables go to LDS once per workgroup.
// Per ray one bounce loop for the whole wave: iteration k traces the k-th segment of every lane that is still bouncing (all such
// lanes have bounced exactly k times, so the reference's `cur_reflections` is the wave-uniform k).  out_rec != NULL: the rt_hit of
// segment 0, as rt_trace_rays writes it.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_kernel(const ShadeRaysArgs sa, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                                         const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba, RqRecord *__restrict__ out_rec)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const RayQueryArgs &qa = sa.qa;
    const uint32_t tid = threadIdx.x;
    const RqTables S = rq_stage_tables(qa, scene, smem);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (wave-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
        if (live) {
            const double2 *w = reinterpret_cast<const double2 *>(rays + i); // three 16-byte loads
            const double2 w0 = w[0], w1 = w[1], w2 = w[2];
            o = D3{w0.x, w0.y, w1.x};
            d = D3{w1.y, w2.x, w2.y};
        }
        ShadeRaysStaged pol{qa, S, gobj, out_rec, i, live};
        const F3 res = shade_loop<HAS_GQ, HAS_CUBIC>(sa, scene, lights, tid & 63u, pol, o, d, live);
        if (live) out_rgba[i] = float4{res.x, res.y, res.z, 1.0f}; // one 16-byte store
    }
}

} // namespace RT_SYM(rtk)

// rays = n rt_ray, rgba = n x 4 float32, hits = n rt_hit or NULL, all in device memory and 16-byte aligned; lights = the context's
// DevLight array; at most max_grid workgroups.  The scene must fit the LDS limit (rt_rays_lds_bytes).
extern "C" hipError_t RT_SYM(rt_launch_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba, void *hits,
                                                    uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    ShadeRaysArgs sa;
    sa.qa = rq_args(fa, n);
    sa.n_lights = fa->n_lights;
    sa.max_refl = fa->max_refl;
    sa.bg[0] = fa->bg[0]; sa.bg[1] = fa->bg[1]; sa.bg[2] = fa->bg[2];
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    const dim3 g(need < max_grid ? need : (max_grid ? max_grid : 1u)), block(256);
    const size_t lds = sa.qa.tab_bytes;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    float4 *px = reinterpret_cast<float4 *>(rgba);
    RqRecord *rec = reinterpret_cast<RqRecord *>(hits);
    rq_for_classes(fa, [&](auto gq, auto cub) { hipLaunchKernelGGL((shade_rays_kernel<decltype(gq)::value, decltype(cub)::value>), g, block, lds, stream, sa, s, lt, r, px, rec); });
    return hipGetLastError();
}
