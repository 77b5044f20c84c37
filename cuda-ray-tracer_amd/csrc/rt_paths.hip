// rt_paths.hip -- the hits along a ray's mirror bounces, and the context's own primary rays as explicit rays (include/mi355rt.h,
// rt_trace_paths / rt_primary_rays / rt_pick_paths).
//
// A path is the geometry of the reference's render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d of a ray the
// caller hands in, minus everything that concerns colour: nearest hit, normal_vector, the reflection-ratio test, reflect_ray and the
// bias step, until a hit is no mirror, a bounce leaves the scene or the scene's max_reflections is reached.  It is shade_rays_kernel
// (rt_shade_rays.hip) without its light loops, and it writes down what it met.  Compiled twice like rt_rays.hip (-DRT_VARIANT=strict
// -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).  The object loops are the ray queries' (rt_rayquery.hpp): the class
// tables where they are proven for the ray in hand -- decided anew for every bounce, whose origin and direction the kernel forms itself
// -- and the dense expansion elsewhere.
// The path kernel reads the scene blob and the caller's rays; the primary-ray kernel reads the camera-plane tables.  Neither touches
// tile words, launch-order generations, census, counters or frame tag -- both are invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_rayquery.hpp" // RayQueryArgs, the class tables in LDS, rq_tables / rq_plain, the ray and record layouts

namespace RT_SYM(rtk) {

// 256-thread workgroups, one ray per lane, the grid-stride loop of ray_query_kernel; the class tables go to LDS once per workgroup.
// Per ray one bounce loop for the whole wave: iteration k traces segment k of every lane that is still bouncing, and every lane with a
// ray -- done or not -- stores its record of plane k while k < max_segments (a lane that is done stores the miss record), so the wave's
// stores of one iteration are consecutive 48-byte records: out_seg is segment-major, record k * n + i.  max_segments only limits what
// is stored; the path is followed to its end.  out_last (may be NULL): the hit of the last segment.  out_end: one record per ray.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void path_query_kernel(const PathArgs pa, const unsigned char *__restrict__ scene, const RqRay *__restrict__ rays,
                                                         RqRecord *__restrict__ out_seg, RqRecord *__restrict__ out_last, PathEnd *__restrict__ out_end)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const RayQueryArgs &qa = pa.qa;
    const uint32_t tid = threadIdx.x;
    const RqTables S = rq_stage_tables(qa, scene, smem);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;

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
        float cur_ratio = 1.0f;
        uint32_t segments = 0u, end = PATH_MISS;
        int last = -1; // the last hit: what out_last receives
        double last_t = INFINITY;
        D3 last_p{0.0, 0.0, 0.0}, last_n{0.0, 0.0, 0.0};
        bool bouncing = live;
        uint32_t k = 0;
        for (; __ballot(bouncing) != 0ull; k++) {
            // the nearest hit of segment k (src/update-cpu.cpp:50-56).  From the first bounce on the ray is one the kernel formed: sp can lie
            // beyond the tables' proven range and sn can be NaN, so the decision is made for every segment
            const bool proven = rq_tables_proven(o, d);
            Mono m;
            mono_set_o<NEED_CROSS>(m, o);
            mono_set_d<NEED_CROSS>(m, d);
            mono_set_od<NEED_CROSS>(m);
            double best_t = INFINITY;
            int best = -1;
            rq_tables<HAS_GQ, HAS_CUBIC, false>(qa, S, gobj, m, bouncing && proven, MAX_T, best_t, best);
            if (__ballot(bouncing && !proven) != 0ull) rq_plain<false>(qa, gobj, o, d, bouncing && !proven, MAX_T, best_t, best);
            const bool hit = bouncing && best >= 0;
            const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
            D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
            if (hit) {
                sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
                sn = normal_vector(bo->c, sp); // all twenty coefficients, as rt_rays.hip; FP64, never flipped
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

// The context's own primary rays as rt_ray records: o = the frame's ray origin, d = primary_dir_tab of the pixel on the context's
// camera-plane tables -- the very function and tables of the render, G-buffer and pick kernels.  xy == NULL: the pixels of the rectangle
// x0 .. x0 + w - 1, y0 .. (GLOBAL rows), row-major from row y0; else n pixels by GLOBAL coordinates xy[2 * i], xy[2 * i + 1].
__global__ __launch_bounds__(256) void primary_rays_kernel(const FrameArgs fa, const double *__restrict__ camx, const double *__restrict__ camy,
                                                           const uint32_t *__restrict__ xy, uint32_t x0, uint32_t y0, uint32_t w, uint64_t n, RqRay *__restrict__ out)
{
    const uint64_t stride = (uint64_t) gridDim.x * 256u;
    for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        uint32_t col, row; // (validated by the host: col < width, row < height)
        if (xy) {
            col = xy[2u * i];
            row = xy[2u * i + 1u];
        } else {
            col = x0 + (uint32_t) (i % w);
            row = y0 + (uint32_t) (i / w);
        }
        const D3 dir = primary_dir_tab(fa, camx[col], camy[row]);
        double2 *dst = reinterpret_cast<double2 *>(out + i); // three 16-byte stores
        dst[0] = double2{fa.origin[0], fa.origin[1]};
        dst[1] = double2{fa.origin[2], dir.x};
        dst[2] = double2{dir.y, dir.z};
    }
}

} // namespace RT_SYM(rtk)

// rays = n rt_ray, segments = [max_segments][n] rt_hit (NULL iff max_segments == 0), last = n rt_hit or NULL, ends = n rt_path_end, all
// in device memory and 16-byte aligned; at most max_grid workgroups.  The scene must fit the LDS limit (rt_rays_lds_bytes).
extern "C" hipError_t RT_SYM(rt_launch_trace_paths)(const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments,
                                                     void *last, void *ends, uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (n == 0u) return hipSuccess;
    PathArgs pa;
    pa.qa = rq_args(fa, n);
    pa.max_refl = fa->max_refl;
    pa.max_segments = max_segments;
    const uint32_t need = (uint32_t) (((uint64_t) n + 255u) / 256u);
    const dim3 g(need < max_grid ? need : (max_grid ? max_grid : 1u)), block(256);
    const size_t lds = pa.qa.tab_bytes;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const RqRay *r = reinterpret_cast<const RqRay *>(rays);
    RqRecord *seg = reinterpret_cast<RqRecord *>(segments), *lst = reinterpret_cast<RqRecord *>(last);
    PathEnd *pe = reinterpret_cast<PathEnd *>(ends);
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((path_query_kernel<true, true>), g, block, lds, stream, pa, s, r, seg, lst, pe);
        else hipLaunchKernelGGL((path_query_kernel<false, true>), g, block, lds, stream, pa, s, r, seg, lst, pe);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((path_query_kernel<true, false>), g, block, lds, stream, pa, s, r, seg, lst, pe);
        else hipLaunchKernelGGL((path_query_kernel<false, false>), g, block, lds, stream, pa, s, r, seg, lst, pe);
    }
    return hipGetLastError();
}

// fa = the frame arguments with this call's camera and origin (rtf::frame_origin).  xy == NULL: rect = x0, y0, x1, y1 (inclusive, inside
// the image, validated by the caller) -> (y1 - y0 + 1) * (x1 - x0 + 1) rt_ray; else n_list pixels -> n_list rt_ray.  out in device
// memory, 16-byte aligned; at most max_grid workgroups.
extern "C" hipError_t RT_SYM(rt_launch_primary_rays)(const FrameArgs *fa, const double *camx, const double *camy, const uint32_t *rect, const uint32_t *xy,
                                                      uint32_t n_list, void *out, uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    const uint32_t w = xy ? 1u : rect[2] - rect[0] + 1u;
    const uint64_t n = xy ? (uint64_t) n_list : (uint64_t) w * (rect[3] - rect[1] + 1u);
    if (n == 0u) return hipSuccess;
    const uint64_t need = (n + 255u) / 256u;
    const dim3 g((uint32_t) (need < max_grid ? need : (max_grid ? max_grid : 1u))), block(256);
    hipLaunchKernelGGL(primary_rays_kernel, g, block, 0, stream, *fa, camx, camy, xy, xy ? 0u : rect[0], xy ? 0u : rect[1], w, n, reinterpret_cast<RqRay *>(out));
    return hipGetLastError();
}
