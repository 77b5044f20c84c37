// rt_stream_queries.hip -- the streamed query kernels: the G-buffer, picking, object extents, the ray queries, their colour and their
// paths for scenes of any size (include/mi355rt.h, RT_FLAG_STREAM_QUERIES).
//
// Every kernel here is the twin of a kernel that copies all class tables into one workgroup's LDS (rt_gbuffer.hip, rt_rays.hip,
// rt_shade_rays.hip, rt_paths.hip) and differs from it in one thing: the object loops read the tables from the scene blob in global
// memory through a wave-private LDS slice, 64 entries at a time (rt_stream.hpp), as the streamed frame kernel does (rt_stream.hip).  The
// chunks are the staged loops' chunks and a chunk's body is theirs, so in a strict context a streamed kernel returns what its twin
// returns, bit for bit.  Rays, work geometry, loads, stores and launch bounds are the twin's: the twins share their bodies (rt_ray_kernels.hpp,
// DESIGN.md section 30; rt_pixel_kernels.hpp, section 32).
// Compiled twice like rt_stream.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file, and no lane leaves before its wave's last ballot, readlane or staged chunk: a
// lane without work stays with `use = false`.  Every kernel takes 4 * SQ_SLICE_BYTES = 24 KiB of LDS whatever the tables hold.
#include <hip/hip_runtime.h>
#include "rt_launch.h"   // the launchers below, as the host sees them
#include "rt_ray_kernels.hpp" // the ray, colour and path kernels' bodies; SqQuery, SqPixels and the streamed object loops (rt_stream.hpp); RayQueryArgs, the ray and record layouts (rt_rayquery.hpp)
#include "rt_pixel_kernels.hpp" // the pixel kernels' bodies; the extent record and its init kernel (rt_extents.hpp)

namespace RT_SYM(rtk) {

// ---- caller-supplied rays (rt_rays.hip, rt_shade_rays.hip, rt_paths.hip): the twins' bodies (rt_ray_kernels.hpp) over sq_query ---------------------
// (the slice: this wave's quarter of the workgroup's LDS, never another's)
template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>
__global__ __launch_bounds__(256) void ray_query_stream_kernel(const RayQueryArgs qa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                               const double *__restrict__ t_max, RqRecord *__restrict__ out_rec, int32_t *__restrict__ out_blocked)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    SqQuery q{qa, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES};
    rk_ray_query<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, rays, t_max, out_rec, out_blocked, q);
}

template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void shade_rays_stream_kernel(const ShadeRaysArgs sa, const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                                                const RqRay *__restrict__ rays, float4 *__restrict__ out_rgba, RqRecord *__restrict__ out_rec)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    SqQuery q{sa.qa, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES};
    rk_shade_rays<HAS_GQ, HAS_CUBIC>(sa, scene, lights, rays, out_rgba, out_rec, q);
}

// ---- paths (rt_paths.hip: path_query_kernel) -------------------------------------------------------------------------------------------------
// The one kernel of the nine that keeps its own text: rk_path_query's, line for line, with sq_query written in place of the query object
// (tests/test_stream_shade_host.py holds it to that).  Through the shared body its spheres-only instantiation has the same instructions in
// every loop, all of them 8 bytes earlier -- one compare hoisted in the entry block -- and took 4 to 5 % longer on every series measured
// (profiles/ray_kernel_bodies.txt); no shape of the body that was compiled moved them back.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void path_query_stream_kernel(const PathArgs pa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                                RqRecord *__restrict__ out_seg, RqRecord *__restrict__ out_last, PathEnd *__restrict__ out_end)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const RayQueryArgs &qa = pa.qa;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES;
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);

    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t first = (uint64_t) blockIdx.x * 256u; first < qa.n; first += stride) { // (workgroup-uniform trip count)
        const uint64_t i = first + tid;
        const bool live = i < qa.n;
        D3 o, d;
        rk_load_ray(rays, i, live, o, d);
        float cur_ratio = 1.0f;
        uint32_t segments = 0u, end = PATH_MISS;
        int last = -1; // the last hit: what out_last receives
        double last_t = INFINITY;
        D3 last_p{0.0, 0.0, 0.0}, last_n{0.0, 0.0, 0.0};
        bool bouncing = live;
        uint32_t k = 0;
        for (; __ballot(bouncing) != 0ull; k++) {
            // the nearest hit of segment k; from the first bounce on the ray is one the kernel formed, so sq_query decides for every segment
            double best_t = INFINITY;
            int best = -1;
            sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, bouncing, false, MAX_T, best_t, best);
            const bool hit = bouncing && best >= 0;
            const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
            D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
            if (hit) {
                sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                sn = normal_vector(bo->c, sp);
            }
            if (k < pa.max_segments && live) rq_store_record(out_seg + ((uint64_t) k * qa.n + i), hit ? best : -1, best_t, sp, sn);
            if (bouncing) {
                if (!hit) {
                    end = (k == 0u) ? PATH_MISS : PATH_ESCAPED;
                    bouncing = false;
                } else {
                    segments = k + 1u;
                    last = best;
                    last_t = best_t;
                    last_p = sp;
                    last_n = sn;
                    // the reflection loop, src/update-cpu.cpp:96-117
                    const float refl = bo->refl;
                    if (!((double) refl > EPS)) {
                        end = PATH_SURFACE;
                        bouncing = false;
                    } else {
                        cur_ratio *= refl;
                        if (k == pa.max_refl) {
                            end = PATH_CAP;
                            bouncing = false;
                        } else {
                            d = reflect_ray(d, sn); // of the direction as it is
                            o = D3{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
                        }
                    }
                }
            }
        }
        if (live) {
            const D3 zero{0.0, 0.0, 0.0};
            for (; k < pa.max_segments; k++) rq_store_record(out_seg + ((uint64_t) k * qa.n + i), -1, INFINITY, zero, zero); // planes no lane of the wave reached
            if (out_last) rq_store_record(out_last + i, last, last_t, last_p, last_n);
            out_end[i] = PathEnd{segments, end, cur_ratio, last}; // one 16-byte store
        }
    }
}

// ---- pixels: the G-buffer, picking, object extents (rt_gbuffer.hip) --------------------------------------------------------------------------
// The twins' bodies (rt_pixel_kernels.hpp) over SqPixels (rt_stream.hpp): sq_tables itself, without a plain path, as the staged family
// has none.  extents_stream_kernel has no accumulators in LDS: every wave merges into `out` itself.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void gbuffer_stream_kernel(const FrameArgs fa, const RayQueryArgs qa, const unsigned char *__restrict__ scene,
                                                             const double *__restrict__ camx, const double *__restrict__ camy, int32_t *__restrict__ out_object,
                                                             double *__restrict__ out_t, float4 *__restrict__ out_normal, const uint32_t *__restrict__ xy,
                                                             uint32_t n_query, RqRecord *__restrict__ out_rec)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    SqPixels q{fa, qa, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES};
    pk_gbuffer<HAS_GQ, HAS_CUBIC>(fa, scene, camx, camy, out_object, out_t, out_normal, xy, n_query, out_rec, q);
}

EXT_INIT_KERNEL(extents_init_stream_kernel)

template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void extents_stream_kernel(const FrameArgs fa, const RayQueryArgs qa, const ExtArgs ea, const unsigned char *__restrict__ scene,
                                                             const double *__restrict__ camx, const double *__restrict__ camy, ExtRecord *__restrict__ out)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    SqPixels q{fa, qa, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES};
    pk_extents<HAS_GQ, HAS_CUBIC>(fa, ea, camx, camy, out, nullptr, q);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
static hipError_t sqk_launch_pixels(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, uint32_t grid, int32_t *out_object, double *out_t,
                                    float *out_normal, const uint32_t *xy, uint32_t n, void *rec, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, 0u);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    float4 *nrm = reinterpret_cast<float4 *>(out_normal);
    RqRecord *r = reinterpret_cast<RqRecord *>(rec);
    RK_LAUNCH(fa, (gbuffer_stream_kernel<GQ, CUB>), dim3(grid), 0, stream, *fa, qa, s, camx, camy, out_object, out_t, nrm, xy, n, r);
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// The signatures are the staged launchers' (rt_gbuffer.hip, rt_rays.hip, rt_shade_rays.hip, rt_paths.hip), so an entry point picks one
// or the other by the context's one decision; a launch is the same number of graph nodes as its twin's.
extern "C" hipError_t RT_SYM(rt_launch_stream_gbuffer)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t,
                                                        float *out_normal, const ChunkTables *, hipStream_t stream)
{
    if (fa->n_tiles == 0u) return hipSuccess;
    return RT_SYM(rtk)::sqk_launch_pixels(fa, scene, camx, camy, fa->n_tiles, out_object, out_t, out_normal, nullptr, 0u, nullptr, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_stream_pick)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *xy, uint32_t n, void *out,
                                                     const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::sqk_launch_pixels(fa, scene, camx, camy, (n + 255u) / 256u, nullptr, nullptr, nullptr, xy, n, out, stream);
}

// Two nodes on `stream`, as rt_launch_object_extents: the identities, then -- when this rank owns a row of the rectangle -- the kernel.
extern "C" hipError_t RT_SYM(rt_launch_stream_object_extents)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *rect, void *out,
                                                               uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_obj == 0u) return hipSuccess;
    ExtRecord *rec = reinterpret_cast<ExtRecord *>(out);
    hipLaunchKernelGGL(extents_init_stream_kernel, dim3((fa->n_obj + 255u) / 256u), dim3(256), 0, stream, rec, fa->n_obj);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ExtArgs ea;
    if (!ext_args(fa, rect, ea)) return hipSuccess; // no row of the rectangle is this rank's: the identities stand
    const RayQueryArgs qa = rq_args(fa, 0u);
    const dim3 g(ea.n_tiles < max_grid ? ea.n_tiles : (max_grid ? max_grid : 1u));
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    RK_LAUNCH(fa, (extents_stream_kernel<GQ, CUB>), g, 0, stream, *fa, qa, ea, s, camx, camy, rec);
    return hipGetLastError();
}

namespace RT_SYM(rtk) {
template <bool OCCLUSION>
static hipError_t sqk_launch_rays(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, void *out, uint32_t max_grid, hipStream_t stream)
{
    const RayQueryArgs qa = rq_args(fa, n);
    RK_LAUNCH(fa, (ray_query_stream_kernel<GQ, CUB, OCCLUSION>), rk_ray_grid(n, max_grid), 0, stream, qa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), t_max, OCCLUSION ? nullptr : reinterpret_cast<RqRecord *>(out), OCCLUSION ? reinterpret_cast<int32_t *>(out) : nullptr);
    return hipGetLastError();
}
} // namespace RT_SYM(rtk)

extern "C" hipError_t RT_SYM(rt_launch_stream_trace_rays)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid,
                                                           const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::sqk_launch_rays<false>(fa, scene, rays, nullptr, n, out, max_grid, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_stream_occluded_rays)(const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out,
                                                              uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::sqk_launch_rays<true>(fa, scene, rays, t_max, n, out, max_grid, stream);
}

extern "C" hipError_t RT_SYM(rt_launch_stream_shade_rays)(const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba, void *hits,
                                                           uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    const ShadeRaysArgs sa = rk_shade_args(fa, n);
    RK_LAUNCH(fa, (shade_rays_stream_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), 0, stream, sa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const DevLight *>(lights), reinterpret_cast<const RqRay *>(rays), reinterpret_cast<float4 *>(rgba), reinterpret_cast<RqRecord *>(hits));
    return hipGetLastError();
}

extern "C" hipError_t RT_SYM(rt_launch_stream_trace_paths)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments,
                                                            void *last, void *ends, uint32_t max_grid, const ChunkTables *, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    const PathArgs pa = rk_path_args(fa, n, max_segments);
    RK_LAUNCH(fa, (path_query_stream_kernel<GQ, CUB>), rk_ray_grid(n, max_grid), 0, stream, pa, reinterpret_cast<const unsigned char *>(scene),
              reinterpret_cast<const RqRay *>(rays), reinterpret_cast<RqRecord *>(segments), reinterpret_cast<RqRecord *>(last), reinterpret_cast<PathEnd *>(ends));
    return hipGetLastError();
}
