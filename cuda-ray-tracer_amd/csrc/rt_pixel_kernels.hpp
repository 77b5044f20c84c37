// rt_pixel_kernels.hpp -- the kernels for the context's own pixels, once: what rt_render_gbuffer / rt_pick (and with them the G pass of
// an RT_FLAG_SSAA_GEOMETRY frame) and rt_object_extents do with a pixel is the same whichever way the context reads the class tables
// (DESIGN.md section 32).  The four kernels -- staged (rt_gbuffer.hip), streamed (rt_stream_queries.hip) -- take their LDS, build a
// query object and call one of the two bodies here.  A query object offers one call,
//   nearest<HAS_GQ, HAS_CUBIC>(lane, m, live, block, best_t, best)
// the nearest hit of the primary ray (m: its monomials, from the frame's origin) of every lane in `live` (block: the wave's lanes are
// the pixels of one 8 x 8 block, which may cull by the block's cone), and nothing else:
//   RqPixels  rt_rayquery.hpp  all class tables in the workgroup's LDS (rq_tables)
//   SqPixels  rt_stream.hpp    the tables through the wave's slice (sq_tables)
// The wave-level rules are rt_ray_kernels.hpp's: all 64 lanes call; `live` is a predicate; no lane leaves before the wave's last
// ballot, readlane or staged chunk; nothing here is workgroup-wide.  LDS and whatever fills it are the kernels' business.
// The bodies' pointer parameters carry no restrict: the kernels' own parameters do (rt_ray_kernels.hpp).
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_PIXEL_KERNELS_HPP
#define RT_PIXEL_KERNELS_HPP

#include <hip/hip_runtime.h>

#include "rt_rayquery.hpp" // rq_mono, the record layout
#include "rt_extents.hpp"  // the extent record and the wave reduction

namespace RT_SYM(rtk) {

// The pixel of a lane: one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels.
// (bx, blr): the block's first column and LOCAL row; (x, lr): the lane's.  A lane outside the image (live = false) traces a clamped
// pixel's ray, so that the block's corner lanes always span its cone.  (col, row): camera-table indices, row GLOBAL.
struct PkPixel {
    uint32_t bx, blr, x, lr, col, row;
    bool live;
};

__device__ __forceinline__ PkPixel pk_block_pixel(const FrameArgs &fa, uint32_t tile_x, uint32_t tile_y, uint32_t wave, uint32_t lane)
{
    PkPixel p;
    p.bx = tile_x * 16u + (wave & 1u) * 8u;
    p.blr = tile_y * 16u + (wave >> 1) * 8u;
    p.x = tile_x * 16u + (wave & 1u) * 8u + (lane & 7u);
    p.lr = tile_y * 16u + (wave >> 1) * 8u + (lane >> 3);
    p.live = p.x < fa.width && p.lr < fa.local_rows;
    p.col = p.x < fa.width ? p.x : fa.width - 1u;
    p.row = global_row(fa, p.lr < fa.local_rows ? p.lr : fa.local_rows - 1u);
    return p;
}

// ---- the G-buffer and picking ------------------------------------------------------------------------------------------------------------------
// What lies under one primary ray (include/mi355rt.h, "G-buffer"): object = -1, t = +inf, point = normal = 0 on a miss.
// Planes (xy == NULL): pk_block_pixel's geometry (a lane's row of eight consecutive pixels stores 32 / 64 / 128 contiguous bytes into
// the object / t / normal plane); a plane whose pointer is NULL is not written (launch-uniform); lanes outside the image store nothing.
// Picking (xy != NULL): one lane per query -- n_query pixels by GLOBAL coordinates, any row --, no cone, one rt_hit per lane.
// The planes and the picked records come from ONE kernel in two launch modes -- the same machine code, not merely the same source: in
// the FMA-contracted build the compiler is free to contract two inlined copies of one function differently, and a picked pixel must be
// bit-equal to the planes' entry there too.
template <bool HAS_GQ, bool HAS_CUBIC, typename Query>
__device__ __forceinline__ void pk_gbuffer(const FrameArgs &fa, const unsigned char *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t,
                                           float4 *out_normal, const uint32_t *xy, uint32_t n_query, RqRecord *out_rec, Query &q)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);

    const bool pick = xy != nullptr; // launch-uniform
    PkPixel px{};
    if (pick) {
        const uint32_t i = blockIdx.x * 256u + tid;
        px.live = i < n_query;
        px.col = px.live ? xy[2u * i] : 0u; // (validated by the host: col < width, row < height)
        px.row = px.live ? xy[2u * i + 1u] : 0u;
    } else {
        px = pk_block_pixel(fa, blockIdx.x % fa.tiles_x, blockIdx.x / fa.tiles_x, wave, lane);
    }
    const bool live = px.live;
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    const D3 dir = primary_dir_tab(fa, camx[px.col], camy[px.row]);
    const Mono m = rq_mono<HAS_GQ || HAS_CUBIC>(o, dir);
    double best_t;
    int best;
    q.template nearest<HAS_GQ, HAS_CUBIC>(lane, m, live, !pick, best_t, best);
    // (behind the last wave-wide operation)
    RqRecord r{INFINITY, {0.0, 0.0, 0.0}, {0.0f, 0.0f, 0.0f}, -1};
    if (live && best >= 0) {
        r.object = best;
        r.t = best_t;
        const D3 p{o.x + best_t * dir.x, o.y + best_t * dir.y, o.z + best_t * dir.z};
        r.p[0] = p.x; r.p[1] = p.y; r.p[2] = p.z;
        const DevObject *bo = &gobj[best]; // per-lane index: a gather from global memory, per hit
        D3 n;
        if (bo->cls & RT_CLS_UNITSQ) { // the pixel family's own normal: three coefficients instead of twenty (rt_wavefront_math.hpp: sphere_normal)
            UsEntry e{};
            e.kx = bo->c[K_X];
            e.ky = bo->c[K_Y];
            e.kz = bo->c[K_Z];
            n = sphere_normal(e, p);
        } else {
            n = normal_vector(bo->c, p);
        }
        r.n[0] = (float) n.x; r.n[1] = (float) n.y; r.n[2] = (float) n.z;
    }
    if (live && pick) {
        out_rec[blockIdx.x * 256u + tid] = r; // (16-byte words: RqRecord is alignas(16), and so is every buffer the host passes)
    } else if (live) {
        const size_t at = (size_t) px.lr * fa.width + px.x;
        if (out_object) out_object[at] = r.object;
        if (out_t) out_t[at] = r.t;
        if (out_normal) out_normal[at] = make_float4(r.n[0], r.n[1], r.n[2], 0.0f);
    }
}

// ---- object extents ------------------------------------------------------------------------------------------------------------------------------
// Per object: how many pixels of a rectangle show it, their bounding box and their range of t -- the planes' object and t entries
// reduced on the device, without the planes.  The rays, the work geometry and the query are pk_gbuffer's, so a record is the reduction
// of that body's planes bit for bit; the normal is not formed.  A few workgroups per CU, each striding over the tiles that meet the
// rectangle (workgroup-uniform trip count).  Lanes outside the rectangle (and outside the image) trace their ray for the block's cone
// and count nothing.  acc: ext_reduce_wave's.
template <bool HAS_GQ, bool HAS_CUBIC, typename Query>
__device__ __forceinline__ void pk_extents(const FrameArgs &fa, const ExtArgs &ea, const double *camx, const double *camy, ExtRecord *out, ExtRecord *acc, Query &q)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    for (uint32_t tile = blockIdx.x; tile < ea.n_tiles; tile += gridDim.x) {
        const PkPixel px = pk_block_pixel(fa, ea.tx0 + tile % ea.ntx, ea.ty0 + tile / ea.ntx, wave, lane);
        const D3 dir = primary_dir_tab(fa, camx[px.col], camy[px.row]);
        const Mono m = rq_mono<HAS_GQ || HAS_CUBIC>(o, dir);
        double best_t;
        int best;
        q.template nearest<HAS_GQ, HAS_CUBIC>(lane, m, px.live, true, best_t, best);
        const bool counted = px.live && best >= 0 && px.x >= ea.x0 && px.x <= ea.x1 && px.lr >= ea.lr0 && px.lr <= ea.lr1;
        ext_reduce_wave(fa, px.bx, px.blr, lane, counted, best, best_t, out, acc);
    }
}

} // namespace RT_SYM(rtk)

#endif
