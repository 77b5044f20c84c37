// rt_gbuffer.hip -- the primary-hit G-buffer (object, depth, normal planes) and pixel picking for gfx950 (include/mi355rt.h,
// rt_render_gbuffer / rt_pick), and the same rays reduced per object (rt_object_extents; section 18; at the end).
//
// What is under a pixel: the nearest hit of its primary ray -- phase A of the wavefront kernel (rt_wavefront.hip) without anything
// behind it.  Compiled twice like rt_adaptive.hip (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast).
// The planes and the picked records come from ONE kernel in two launch modes -- the same machine code, not merely the same source: in the
// FMA-contracted build the compiler is free to contract two inlined copies of one function differently, and a picked pixel must be
// bit-equal to the planes' entry there too.  The arithmetic and the exact work removal come from the headers the render kernels use
// (rt_math.hpp, rt_wavefront_math.hpp).
// The pass reads the scene blob and the camera-plane tables (both constant after rt_create) and writes the caller's planes: no tile
// words, launch-order generations, census, counters or frame tag -- it is invisible to rt_render.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_shade.hpp"          // RT_SYM and the variant's namespace
#include "rt_wavefront_math.hpp" // class-table coefficients, us_needs_solve, accept, sphere_in_cone, sphere_normal
#include "rt_extents.hpp"        // the extent record, its merge and the rectangle's tiles: shared with rt_stream_queries.hip

namespace RT_SYM(rtk) {

// the per-class tables (rt_scene_dev.h) and the degree-3 records of the frame's ray origin, staged in LDS
struct GbTables {
    const UsEntry *us;
    const GqEntry *gq;
    const LinEntry *lin;
    const uint32_t *cub;
    const double *prim; // FrameArgs::cub_rec, then FrameArgs::cub_abs
};

__device__ __forceinline__ double gb_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Nearest hit of one ray from the frame's origin: the reference's loop (src/update-cpu.cpp:50-56) over the class tables, as phase
// A of the wavefront kernel runs it.  block: the wave's lanes are the pixels of one 8 x 8 block (lanes 0, 7, 56, 63 its corners, lane
// 36 a central one), so unit spheres are first culled against the block's ray cone, one lane per sphere; otherwise (picking: lanes
// are unrelated pixels) the cone is the whole space and every sphere passes -- through the same loop.  Either way t1 / t0 and the sign
// of the discriminant come first and only the lanes that need a root compute it.  The loops are wave-uniform; a lane without a ray
// (live = false) accepts nothing.
template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ void nearest_hit(const FrameArgs &fa, const GbTables &S, const DevObject *__restrict__ gobj, const Mono &m, bool live, bool block,
                                            uint32_t lane, double &best_t, int &best)
{
    best = -1;
    best_t = INFINITY;
    const bool quad = fabs(m.u2) > EPS; // unit spheres share t2 = u2: one degree decision per ray
    const double four_t2 = 4.0 * m.u2;
    D3 axis{0.0, 0.0, 1.0};
    double cos_t = 1.0;
    const bool cone = fa.cull != 0u;
    if (cone && !block) cos_t = -1.0; // (sphere_in_cone: no cone wider than a half-space culls anything)
    if (cone && block) { // launch-uniform
        // the angle to the axis is quasi-convex on the image plane: over the block it peaks at one of the four corner pixels
        axis = D3{gb_readlane(m.d.x, 36), gb_readlane(m.d.y, 36), gb_readlane(m.d.z, 36)};
        const double ca = dot3(axis, m.d);
        const double c0 = gb_readlane(ca, 0), c1 = gb_readlane(ca, 7), c2 = gb_readlane(ca, 56), c3 = gb_readlane(ca, 63);
        const double m01 = c0 < c1 ? c0 : c1, m23 = c2 < c3 ? c2 : c3;
        cos_t = m01 < m23 ? m01 : m23;
    }
    for (uint32_t base = 0; base < fa.n_us; base += 64) {
        const uint32_t end = (base + 64 < fa.n_us) ? base + 64 : fa.n_us;
        unsigned long long cand = 0;
        if (cone) {
            bool rel = false;
            if (base + lane < end) {
                const UsEntry e = S.us[base + lane];
                rel = sphere_in_cone(e.kx, e.ky, e.kz, e.r, e.inv_r, m.o, axis, cos_t);
            }
            unsigned long long it = __ballot(rel);
            while (it) { // wave-uniform loop over the spheres that reach into this block's cone
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
        if (!live) cand = 0;
        while (cand) { // per lane: the few spheres whose root must actually be computed
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const UsEntry e = S.us[base + b];
            const double t = solve_quadlin(m.u2, us_t1(e, m), us_t0(e, m));
            accept(t, (int) e.orig, best_t, best);
        }
    }
    for (uint32_t base = 0; HAS_GQ && base < fa.n_gq; base += 64) {
        const uint32_t end = (base + 64 < fa.n_gq) ? base + 64 : fa.n_gq;
        unsigned long long cand = 0;
#pragma unroll 2
        for (uint32_t j = base; j < end; j++) {
            const GqEntry e = S.gq[j];
            cand |= needs_solve(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m)) ? (1ull << (j - base)) : 0ull;
        }
        if (!live) cand = 0;
        while (cand) {
            const int b = __builtin_ctzll(cand);
            cand &= cand - 1;
            const GqEntry e = S.gq[base + b];
            const double t = solve_quadlin(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m));
            accept(t, (int) e.orig, best_t, best);
        }
    }
    for (uint32_t j = 0; j < fa.n_lin; j++) { // planes: every lane needs the one division, nothing to defer
        const LinEntry e = S.lin[j];
        const double t1 = lin_t1(e, m);
        const double t0 = lin_t0(e, m);
        const double t = (fabs(t1) > EPS) ? -t0 / t1 : -1.0;
        if (live) accept(t, (int) e.orig, best_t, best);
    }
    if (HAS_CUBIC) {
        for (uint32_t j = 0; j < fa.n_cub; j++) {
            const uint32_t k = (uint32_t) __builtin_amdgcn_readfirstlane((int) S.cub[j]);
            if (live) {
                // the guarded Taylor test of the render kernels (rt_math.hpp: cubic_guarded, dense expansion where it refuses): the
                // surface's data at the frame's origin comes from the host for the first RT_CUB_AT_MAX objects, as in rt_render
                CubicAt ca;
                CubicAbs ab;
                if (j < RT_CUB_AT_MAX) {
                    const double *r = S.prim + j * RT_CUB_REC, *a = S.prim + RT_CUB_AT_MAX * RT_CUB_REC + j * 4u;
                    ca = CubicAt{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
                    ab = CubicAbs{a[0], a[1], a[2], a[3]};
                } else {
                    ca = cubic_at(gobj[k].c, m.o);
                    ab = cubic_abs(gobj[k].c);
                }
                bool refused;
                const double t = intersect_cubic_taylor<false>(gobj[k].c, ca, cubic_mag_origin(ab, m.o), m.o, m.d, MAX_T, false, refused);
                accept(t, (int) k, best_t, best);
            }
        }
    }
}

// What lies under one primary ray (include/mi355rt.h, "G-buffer"): object = -1, t = +inf, point = normal = 0 on a miss.
struct GbHit {
    int object;
    double t;
    D3 p;
    float nx, ny, nz;
};

template <bool HAS_GQ, bool HAS_CUBIC>
__device__ __forceinline__ GbHit primary_hit(const FrameArgs &fa, const GbTables &S, const DevObject *__restrict__ gobj, const D3 &o, const D3 &dir, bool live,
                                             bool block, uint32_t lane)
{
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;
    Mono m;
    mono_set_o<NEED_CROSS>(m, o);
    mono_set_d<NEED_CROSS>(m, dir);
    mono_set_od<NEED_CROSS>(m);
    GbHit h{-1, INFINITY, D3{0.0, 0.0, 0.0}, 0.0f, 0.0f, 0.0f};
    double best_t;
    int best;
    nearest_hit<HAS_GQ, HAS_CUBIC>(fa, S, gobj, m, live, block, lane, best_t, best);
    if (live && best >= 0) {
        h.object = best;
        h.t = best_t;
        h.p = D3{o.x + best_t * dir.x, o.y + best_t * dir.y, o.z + best_t * dir.z};
        const DevObject *bo = &gobj[best]; // per-lane index: a gather from global memory, per hit
        D3 n;
        if (bo->cls & RT_CLS_UNITSQ) { // three coefficients instead of twenty (rt_wavefront_math.hpp: sphere_normal)
            UsEntry e{};
            e.kx = bo->c[K_X];
            e.ky = bo->c[K_Y];
            e.kz = bo->c[K_Z];
            n = sphere_normal(e, h.p);
        } else {
            n = normal_vector(bo->c, h.p);
        }
        h.nx = (float) n.x;
        h.ny = (float) n.y;
        h.nz = (float) n.z;
    }
    return h;
}

// One rt_hit record (include/mi355rt.h): { double t; double point[3]; float normal[3]; int32 object } = 48 bytes.
struct GbRecord {
    double t, p[3];
    float n[3];
    int32_t object;
};
static_assert(sizeof(GbRecord) == 48, "rt_hit layout");

// Planes (xy == NULL): one 256-thread workgroup per 16 x 16 tile of this rank's rows, one wave per 8 x 8 block, lanes are pixels (a
// lane's row of eight consecutive pixels stores 32 / 64 / 128 contiguous bytes into the object / t / normal plane).  A plane whose
// pointer is NULL is not written (launch-uniform).  Lanes outside the image trace a clamped pixel's ray, so that the block's corner
// lanes always span its cone, and store nothing.
// Picking (xy != NULL): one lane per query -- n_query pixels by GLOBAL coordinates, any row --, no cone, one record per lane.
// The class tables go to LDS once per workgroup in both modes.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void gbuffer_kernel(const FrameArgs fa, const unsigned char *__restrict__ scene, const double *__restrict__ camx,
                                                      const double *__restrict__ camy, int32_t *__restrict__ out_object, double *__restrict__ out_t,
                                                      float4 *__restrict__ out_normal, const uint32_t *__restrict__ xy, uint32_t n_query,
                                                      GbRecord *__restrict__ out_rec)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tab_bytes = fa.off_mat - fa.off_us; // [UsEntry][GqEntry][LinEntry][uint32 cubic indices], each padded to 16 bytes
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(scene + fa.off_us);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = tid; i < (tab_bytes >> 4); i += 256u) dst[i] = src[i];
        if (HAS_CUBIC && tid < (RT_CUB_REC + 4) * RT_CUB_AT_MAX) // (cub_rec[4][10], then cub_abs[4][4]: contiguous in FrameArgs)
            reinterpret_cast<double *>(smem + tab_bytes)[tid] = (&fa.cub_rec[0][0])[tid];
    }
    __syncthreads();
    GbTables S;
    S.us = reinterpret_cast<const UsEntry *>(smem);
    S.gq = reinterpret_cast<const GqEntry *>(smem + (fa.off_gq - fa.off_us));
    S.lin = reinterpret_cast<const LinEntry *>(smem + (fa.off_lin - fa.off_us));
    S.cub = reinterpret_cast<const uint32_t *>(smem + (fa.off_cub - fa.off_us));
    S.prim = reinterpret_cast<const double *>(smem + tab_bytes);

    const bool pick = xy != nullptr; // launch-uniform
    uint32_t col, row, lr = 0, x = 0; // camera-table indices: pixel column, GLOBAL image row
    bool live;
    if (pick) {
        const uint32_t q = blockIdx.x * 256u + tid;
        live = q < n_query;
        col = live ? xy[2u * q] : 0u; // (validated by rt_pick: col < width, row < height)
        row = live ? xy[2u * q + 1u] : 0u;
    } else {
        const uint32_t tile_x = blockIdx.x % fa.tiles_x, tile_y = blockIdx.x / fa.tiles_x;
        x = tile_x * 16u + (wave & 1u) * 8u + (lane & 7u);
        lr = tile_y * 16u + (wave >> 1) * 8u + (lane >> 3);
        live = x < fa.width && lr < fa.local_rows;
        col = x < fa.width ? x : fa.width - 1u;
        row = global_row(fa, lr < fa.local_rows ? lr : fa.local_rows - 1u);
    }
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    const D3 dir = primary_dir_tab(fa, camx[col], camy[row]);
    const GbHit h = primary_hit<HAS_GQ, HAS_CUBIC>(fa, S, reinterpret_cast<const DevObject *>(scene), o, dir, live, !pick, lane);
    if (live && pick) {
        GbRecord r;
        r.t = h.t;
        r.p[0] = h.p.x; r.p[1] = h.p.y; r.p[2] = h.p.z;
        r.n[0] = h.nx; r.n[1] = h.ny; r.n[2] = h.nz;
        r.object = h.object;
        out_rec[blockIdx.x * 256u + tid] = r;
    } else if (live) {
        const size_t at = (size_t) lr * fa.width + x;
        if (out_object) out_object[at] = h.object;
        if (out_t) out_t[at] = h.t;
        if (out_normal) out_normal[at] = make_float4(h.nx, h.ny, h.nz, 0.0f);
    }
}

} // namespace RT_SYM(rtk)

// LDS bytes of one gbuffer_kernel workgroup for this scene (rt_render_gbuffer refuses scenes beyond the device's limit)
extern "C" size_t RT_SYM(rt_gbuffer_lds_bytes)(const FrameArgs *fa)
{
    return (size_t) (fa->off_mat - fa->off_us) + (fa->n_cub ? sizeof(double) * (RT_CUB_REC + 4) * RT_CUB_AT_MAX : 0u);
}

namespace RT_SYM(rtk) {
static hipError_t launch(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, uint32_t grid, int32_t *out_object, double *out_t, float *out_normal,
                         const uint32_t *xy, uint32_t n, void *rec, hipStream_t stream)
{
    const size_t lds = RT_SYM(rt_gbuffer_lds_bytes)(fa);
    const dim3 g(grid), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    float4 *nrm = reinterpret_cast<float4 *>(out_normal);
    GbRecord *r = reinterpret_cast<GbRecord *>(rec);
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((gbuffer_kernel<true, true>), g, block, lds, stream, *fa, s, camx, camy, out_object, out_t, nrm, xy, n, r);
        else hipLaunchKernelGGL((gbuffer_kernel<false, true>), g, block, lds, stream, *fa, s, camx, camy, out_object, out_t, nrm, xy, n, r);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((gbuffer_kernel<true, false>), g, block, lds, stream, *fa, s, camx, camy, out_object, out_t, nrm, xy, n, r);
        else hipLaunchKernelGGL((gbuffer_kernel<false, false>), g, block, lds, stream, *fa, s, camx, camy, out_object, out_t, nrm, xy, n, r);
    }
    return hipGetLastError();
}
} // namespace RT_SYM(rtk)

// planes = [local_rows][width] each; any of them may be NULL
extern "C" hipError_t RT_SYM(rt_launch_gbuffer)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t,
                                                 float *out_normal, hipStream_t stream)
{
    if (fa->n_tiles == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch(fa, scene, camx, camy, fa->n_tiles, out_object, out_t, out_normal, nullptr, 0u, nullptr, stream);
}

// xy = n coordinate pairs and out = n records, both in device memory: the planes' kernel in its picking mode
extern "C" hipError_t RT_SYM(rt_launch_pick)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *xy, uint32_t n, void *out,
                                              hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch(fa, scene, camx, camy, (n + 255u) / 256u, nullptr, nullptr, nullptr, xy, n, out, stream);
}

// RT_FLAG_SSAA_GEOMETRY (rt_adaptive.hip): the object and normal planes of this rank's rows (out_normal may be
// NULL) and, with several ranks, one record per pixel of the halo rows (halo_xy = n_halo global coordinate pairs) -- both from
// gbuffer_kernel itself, so the adaptive frame's edges are the ones rt_render_gbuffer / rt_pick report, in the FAST build too.
extern "C" hipError_t RT_SYM(rt_launch_gbuffer_edges)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object,
                                                       float *out_normal, const uint32_t *halo_xy, uint32_t n_halo, void *halo_rec, hipStream_t stream)
{
    if (fa->n_tiles != 0u) {
        const hipError_t e = RT_SYM(rtk)::launch(fa, scene, camx, camy, fa->n_tiles, out_object, nullptr, out_normal, nullptr, 0u, nullptr, stream);
        if (e != hipSuccess) return e;
    }
    if (n_halo == 0u) return hipSuccess;
    return RT_SYM(rtk)::launch(fa, scene, camx, camy, (n_halo + 255u) / 256u, nullptr, nullptr, nullptr, halo_xy, n_halo, halo_rec, stream);
}

// ---- object extents (include/mi355rt.h, "Object extents") ------------------------------------------------------
// Per object: how many pixels of a rectangle show it, their bounding box and their range of t -- the planes' object and t entries
// reduced on the device, without the planes.  The rays, the work geometry (16 x 16 tiles, 8 x 8 blocks, clamped lanes) and the
// per-lane function are gbuffer_kernel's, so a record is the reduction of that kernel's planes bit for bit; the normal is not formed.
namespace RT_SYM(rtk) {

__global__ __launch_bounds__(256) void extents_init_kernel(ExtRecord *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = ExtRecord{0ull, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, RT_EXT_INF_BITS, 0ull};
}

// A few workgroups per CU, each striding over the tiles that meet the rectangle.  Three levels: the wave reduces the lanes of each distinct
// object (count = popcount of their ballot, the box from the ballot's rows and columns, t by a butterfly), one lane merges that into the
// workgroup's LDS record of the object, and the workgroup adds the records it touched to `out` once, at its end.  Lanes outside the
// rectangle (and outside the image) trace their ray for the block's cone and count nothing.
template <bool HAS_GQ, bool HAS_CUBIC>
__global__ __launch_bounds__(256) void extents_kernel(const FrameArgs fa, const ExtArgs ea, const unsigned char *__restrict__ scene, const double *__restrict__ camx,
                                                      const double *__restrict__ camy, ExtRecord *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tab_bytes = fa.off_mat - fa.off_us;
    const uint32_t acc_off = tab_bytes + (HAS_CUBIC ? (uint32_t) sizeof(double) * (RT_CUB_REC + 4) * RT_CUB_AT_MAX : 0u); // (a multiple of 16)
    ExtRecord *acc = reinterpret_cast<ExtRecord *>(smem + acc_off);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(scene + fa.off_us);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = tid; i < (tab_bytes >> 4); i += 256u) dst[i] = src[i];
        if (HAS_CUBIC && tid < (RT_CUB_REC + 4) * RT_CUB_AT_MAX) reinterpret_cast<double *>(smem + tab_bytes)[tid] = (&fa.cub_rec[0][0])[tid];
        if (ea.lds_acc)
            for (uint32_t i = tid; i < fa.n_obj; i += 256u) acc[i] = ExtRecord{0ull, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, RT_EXT_INF_BITS, 0ull};
    }
    __syncthreads();
    GbTables S;
    S.us = reinterpret_cast<const UsEntry *>(smem);
    S.gq = reinterpret_cast<const GqEntry *>(smem + (fa.off_gq - fa.off_us));
    S.lin = reinterpret_cast<const LinEntry *>(smem + (fa.off_lin - fa.off_us));
    S.cub = reinterpret_cast<const uint32_t *>(smem + (fa.off_cub - fa.off_us));
    S.prim = reinterpret_cast<const double *>(smem + tab_bytes);
    const D3 o{fa.origin[0], fa.origin[1], fa.origin[2]};
    constexpr bool NEED_CROSS = HAS_GQ || HAS_CUBIC;

    for (uint32_t tile = blockIdx.x; tile < ea.n_tiles; tile += gridDim.x) { // workgroup-uniform
        const uint32_t tile_x = ea.tx0 + tile % ea.ntx, tile_y = ea.ty0 + tile / ea.ntx;
        const uint32_t bx = tile_x * 16u + (wave & 1u) * 8u, blr = tile_y * 16u + (wave >> 1) * 8u; // the block's first column and local row
        const uint32_t x = bx + (lane & 7u), lr = blr + (lane >> 3);
        const bool live = x < fa.width && lr < fa.local_rows;
        const uint32_t col = x < fa.width ? x : fa.width - 1u;
        const uint32_t row = global_row(fa, lr < fa.local_rows ? lr : fa.local_rows - 1u);
        const D3 dir = primary_dir_tab(fa, camx[col], camy[row]);
        Mono m;
        mono_set_o<NEED_CROSS>(m, o);
        mono_set_d<NEED_CROSS>(m, dir);
        mono_set_od<NEED_CROSS>(m);
        double best_t;
        int best;
        nearest_hit<HAS_GQ, HAS_CUBIC>(fa, S, reinterpret_cast<const DevObject *>(scene), m, live, true, lane, best_t, best);
        const bool counted = live && best >= 0 && x >= ea.x0 && x <= ea.x1 && lr >= ea.lr0 && lr <= ea.lr1;
        const unsigned long long tb = (unsigned long long) __double_as_longlong(best_t);
        unsigned long long todo = __ballot(counted);
        while (todo) { // wave-uniform: one turn per distinct object among the counted lanes (rt_extents.hpp: ext_reduce_wave, with the LDS records in front)
            const int id = __builtin_amdgcn_readlane(best, __builtin_ctzll(todo));
            const bool mine = counted && best == id;
            const unsigned long long mask = __ballot(mine); // bit 8 r + c: row r, column c of the block
            todo &= ~mask;
            unsigned long long lo = mine ? tb : RT_EXT_INF_BITS, hi = mine ? tb : 0ull;
#pragma unroll
            for (int s = 32; s; s >>= 1) {
                const unsigned long long l2 = __shfl_xor(lo, s), h2 = __shfl_xor(hi, s);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (lane == 0u) {
                uint32_t cols = (uint32_t) mask | (uint32_t) (mask >> 32);
                cols |= cols >> 16;
                cols = (cols | (cols >> 8)) & 0xFFu;
                const uint32_t x_min = bx + (uint32_t) __builtin_ctz(cols), x_max = bx + 31u - (uint32_t) __builtin_clz(cols);
                const uint32_t y_min = global_row(fa, blr + ((uint32_t) __builtin_ctzll(mask) >> 3)); // (global_row rises with the local row)
                const uint32_t y_max = global_row(fa, blr + ((63u - (uint32_t) __builtin_clzll(mask)) >> 3));
                const unsigned long long n = (unsigned long long) __builtin_popcountll(mask);
                if (ea.lds_acc) ext_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(acc + id, n, x_min, y_min, x_max, y_max, lo, hi);
                else ext_merge<__HIP_MEMORY_SCOPE_AGENT>(out + id, n, x_min, y_min, x_max, y_max, lo, hi);
            }
        }
    }
    if (ea.lds_acc) {
        __syncthreads();
        for (uint32_t i = tid; i < fa.n_obj; i += 256u) {
            const ExtRecord a = acc[i];
            if (a.pixels) ext_merge<__HIP_MEMORY_SCOPE_AGENT>(out + i, a.pixels, a.x_min, a.y_min, a.x_max, a.y_max, a.t_min, a.t_max);
        }
    }
}

} // namespace RT_SYM(rtk)

// Do the LDS accumulators (40 bytes per object) fit behind `table_bytes` of class tables in the 160 KiB a workgroup may take?  Otherwise
// the waves update the output records themselves.
extern "C" int RT_SYM(rt_extents_lds_accumulators)(size_t table_bytes, uint32_t n_obj)
{
    return table_bytes + sizeof(RT_SYM(rtk)::ExtRecord) * (size_t) n_obj <= 160u * 1024u;
}

// LDS bytes of one extents_kernel workgroup for this scene
extern "C" size_t RT_SYM(rt_extents_lds_bytes)(const FrameArgs *fa)
{
    const size_t tables = RT_SYM(rt_gbuffer_lds_bytes)(fa);
    return tables + (RT_SYM(rt_extents_lds_accumulators)(tables, fa->n_obj) ? sizeof(RT_SYM(rtk)::ExtRecord) * (size_t) fa->n_obj : 0u);
}

// rect = x0, y0, x1, y1 (inclusive, inside the image, GLOBAL rows); out = n_obj records in device memory.  Two nodes on `stream`: the
// identities, then -- when this rank owns a row of the rectangle -- the kernel, at most max_grid workgroups.
extern "C" hipError_t RT_SYM(rt_launch_object_extents)(const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *rect, void *out,
                                                        uint32_t max_grid, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (fa->n_obj == 0u) return hipSuccess;
    ExtRecord *rec = reinterpret_cast<ExtRecord *>(out);
    hipLaunchKernelGGL(extents_init_kernel, dim3((fa->n_obj + 255u) / 256u), dim3(256), 0, stream, rec, fa->n_obj);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ExtArgs ea;
    if (!ext_args(fa, rect, ea)) return hipSuccess; // no row of the rectangle is this rank's: the identities stand
    const size_t tables = RT_SYM(rt_gbuffer_lds_bytes)(fa);
    ea.lds_acc = RT_SYM(rt_extents_lds_accumulators)(tables, fa->n_obj) ? 1u : 0u;
    const size_t lds = RT_SYM(rt_extents_lds_bytes)(fa);
    const dim3 g(ea.n_tiles < max_grid ? ea.n_tiles : (max_grid ? max_grid : 1u)), block(256);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(scene);
    if (fa->n_cub) {
        if (fa->n_gq) hipLaunchKernelGGL((extents_kernel<true, true>), g, block, lds, stream, *fa, ea, s, camx, camy, rec);
        else hipLaunchKernelGGL((extents_kernel<false, true>), g, block, lds, stream, *fa, ea, s, camx, camy, rec);
    } else {
        if (fa->n_gq) hipLaunchKernelGGL((extents_kernel<true, false>), g, block, lds, stream, *fa, ea, s, camx, camy, rec);
        else hipLaunchKernelGGL((extents_kernel<false, false>), g, block, lds, stream, *fa, ea, s, camx, camy, rec);
    }
    return hipGetLastError();
}
