// rt_stream_cull_bounce.hip -- the culled streamed frame kernel with the bounce rays culled as well: rt_render of a context whose
// RT_FLAG_STREAM_CULL_BOUNCE decision is true (include/mi355rt.h, "Culled bounce rays").
//
// stream_cull_frame_kernel's launch shape (rt_stream_shell.hpp) and shading loop (rt_stream_cull.hip).  One line differs: the nearest-hit
// query of a segment k >= 1 is sc_query_bounce (rt_stream_cull_bounce.hpp) instead of sq_query's full sweep -- every lane asks
// rtm::ray_reaches about its own ray and each chunk bound, the wave stages a chunk only if some lane in use reaches it, and sweeps it for
// those lanes alone.  The primary and the shadow rays are culled as in the twin, and the twin's work words (rt_debug_stream_cull) count
// them exactly as the twin does; the bounce queries have five words of their own (rt_debug_stream_cull_bounce).  The frame is
// stream_frame_kernel's: the same arithmetic per tested object, and no dropped object's root could have been accepted.
// This kernel alone does not go through the shared loop (rt_stream_shade.hpp: shade_loop) but holds its text, ScShade's hooks written
// in place: through the shared loop the strict <true, true> instantiation needs 258 registers and loses its second wave per SIMD
// (profiles/stream_shared_loop.txt), whatever shape the policy takes.  A change to shade_loop has to be made here as well.
// All four instantiations of both builds meet the build rule (no VGPR spill, no private segment, two waves per SIMD): none keeps sq_query.
// Compiled twice like rt_stream_cull.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// There is no workgroup barrier anywhere in this file.  The work words are kept per wave in scalars behind a wave-uniform test and added
// with one vector atomic per word at the wave's end.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include "rt_stream_cull_bounce.hpp" // sc_query_bounce over rt_stream_cull.hpp's culled unit-sphere loops
#include "rt_stream_shell.hpp"       // a lane's pixel and the frame store

namespace RT_SYM(rtk) {

// stream_frame_kernel's shape: one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels;
// lanes outside the image trace a clamped pixel's whole path and store nothing.  ca: the chunk bounds and the twin's work words; bstats: the
// bounce work words (NULL exactly where ca.stats is).
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void stream_cull_bounce_frame_kernel(const FrameArgs fa, const RayQueryArgs qa, const StreamCullArgs ca, unsigned long long *bstats,
                                                                       const unsigned char *__restrict__ scene, const DevLight *__restrict__ lights,
                                                                       const double *__restrict__ camx, const double *__restrict__ camy, void *__restrict__ fb)
{
    __shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned char *slice = smem + wave * SQ_SLICE_BYTES; // this wave's, never another's
    ScStats st{ca.stats != nullptr, {0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    ScBounceStats bs{ca.stats != nullptr, {0u, 0u, 0u, 0u, 0u}};
    const SfPixel p = sf_pixel(fa, wave, lane);
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);
    const F3 bg{fa.bg[0], fa.bg[1], fa.bg[2]};
    D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    D3 d = primary_dir_tab(fa, camx[p.col], camy[p.row]);
    // shade_loop's text with ScShade's hooks in place (see the head of this file for why it is written out here)
    F3 res = bg; // a first-segment miss is the background colour
    float cur_ratio = 1.0f;
    bool bouncing = true;
    for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++) {
        // get_color_and_object, src/update-cpu.cpp:45-80: the nearest hit ...
        double best_t = INFINITY;
        int best = -1;
        if (k == 0u) sc_query_primary<HAS_GQ, HAS_CUBIC>(qa, ca, scene, slice, lane, o, d, bouncing, best_t, best, st); // (fa.cull != 0: the context's decision)
        else sc_query_bounce<HAS_GQ, HAS_CUBIC>(qa, ca, scene, slice, lane, o, d, bouncing, best_t, best, bs); // bounce rays: every lane its own ray
        const bool hit = bouncing && best >= 0;
        const DevObject *bo = &gobj[hit ? best : 0]; // per-lane index: gathers from global memory, per hit
        D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0};
        if (hit) {
            sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
            sn = normal_vector(bo->c, sp); // all twenty coefficients; FP64, never flipped
        }
        // ... every light in index order (wave-uniform: scalar loads), shadow_ray from sp + SHADOW_BIAS * sn; a ray the kernel formed, so
        // sq_query decides anew whether the tables are proven for it
        const D3 so{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
        F3 acc{0.0f, 0.0f, 0.0f};
        if (__ballot(hit) != 0ull) {
            const F3 albedo{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
            Ball ball;
            const bool cull_seg = wave_hit_ball(hit, sp, ball); // once per segment; false: a non-finite hit point, test everything
            for (uint32_t l = 0; l < fa.n_lights; l++) {
                const DevLight *lt = &lights[l];
                const bool spherical = lt->spherical != 0;
                double max_t;
                const D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
                double unused_t = INFINITY;
                int blocked = 0;
                if (cull_seg && (spherical || fabs(lt->u2) > EPS)) { // (wave-uniform)
                    if (spherical) sc_query_shadow<HAS_GQ, HAS_CUBIC, true>(qa, ca, scene, slice, lane, so, sd, hit, ball, *lt, max_t, blocked, st);
                    else sc_query_shadow<HAS_GQ, HAS_CUBIC, false>(qa, ca, scene, slice, lane, so, sd, hit, ball, *lt, max_t, blocked, st);
                } else {
                    sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, hit, false, max_t, unused_t, blocked);
                    if (st.on) st.w[6] += 1u;
                }
                if (hit && blocked == 0) {
                    const F3 c = surface_color(lt->p, lt->color, spherical, sp, sn, albedo);
                    acc.x += c.x;
                    acc.y += c.y;
                    acc.z += c.z;
                }
            }
        }
        if (bouncing) {
            if (!hit) {
                if (k != 0u) RT_SYM(rtk)::blend(res, cur_ratio, bg); // a bounce that leaves the scene picks up the background
                bouncing = false;
            } else {
                // glm::min(vec3(1.0f), acc)
                const F3 oc{(acc.x < 1.0f) ? acc.x : 1.0f, (acc.y < 1.0f) ? acc.y : 1.0f, (acc.z < 1.0f) ? acc.z : 1.0f};
                if (k == 0u) res = oc;
                else RT_SYM(rtk)::blend(res, cur_ratio, oc);
                // the reflection loop, src/update-cpu.cpp:96-117
                const float refl = bo->refl;
                if (!((double) refl > EPS)) {
                    bouncing = false;
                } else {
                    cur_ratio *= refl;
                    if (k == fa.max_refl) {
                        RT_SYM(rtk)::blend(res, cur_ratio, bg);
                        bouncing = false;
                    } else {
                        d = reflect_ray(d, sn); // of the direction as it is
                        o = so;
                    }
                }
            }
        }
    }
    if (st.on) {
        sc_flush(st.w, ca.stats, lane);
        sc_flush(bs.w, bstats, lane);
    }
    sf_store(fa, fb, p, res);
}

} // namespace RT_SYM(rtk)

// rt_launch_stream_cull's arguments, and: bounce_stats = 8 bounce work words to add to (the kernel writes the first five), NULL exactly where
// chunks->stats is NULL.
extern "C" hipError_t RT_SYM(rt_launch_stream_cull_bounce)(const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
                                                           const ChunkTables *chunks, unsigned long long *bounce_stats, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_tiles == 0u) return hipSuccess;
    const RayQueryArgs qa = rq_args(fa, 0u);
    StreamCullArgs ca;
    if (!sc_cull_args(fa, chunks, ca) || (ca.stats == nullptr) != (bounce_stats == nullptr)) return hipErrorInvalidValue;
    const dim3 g(fa->n_tiles), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    const DevLight *lt = reinterpret_cast<const DevLight *>(lights);
    rq_for_classes(fa, [&](auto gq, auto cub) {
        hipLaunchKernelGGL((stream_cull_bounce_frame_kernel<decltype(gq)::value, decltype(cub)::value>), g, block, 0, stream, *fa, qa, ca, bounce_stats, s, lt, camx, camy,
                           fb);
    });
    return hipGetLastError();
}
