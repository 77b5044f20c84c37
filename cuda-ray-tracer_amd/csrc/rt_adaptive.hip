// rt_adaptive.hip -- edge-adaptive supersampling for gfx950 (include/mi355rt.h, RT_FLAG_SSAA_ADAPTIVE).
//
// A frame is: the plain pass P (the usual render kernels, one ray per pixel, RGBA32F), then with several ranks the halo rows
// (ray_list_kernel<1>: the centre rays of the rows just outside each band), then classify_kernel (which pixels see contrast in
// their 3x3 neighbourhood: those go to a device list, the others are written out at once), then ray_list_kernel<k> (k x k sample
// rays per listed pixel, reduced across lanes with the resolve's pairwise tree).  Compiled twice like rt_kernels.hip
// (-DRT_VARIANT=strict -ffp-contract=off / -DRT_VARIANT=fast -ffp-contract=fast): the ray kernel shares the simple kernel's
// shading (rt_shade.hpp).  The resolve's arithmetic -- the sums, 1/k^2 and the RGBA8 quantisation -- uses explicitly rounded
// operations, so it is the same in both builds and equal to rt_resolve.hip's.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_shade.hpp"
#include "rt_ray_list.hpp"       // the ray-list kernels' items, resolve and launch ladder
#include "rt_wave_ball.hpp"      // the ball around a wave's hit points
#include "rt_wavefront_math.hpp" // Ball, sphere_relevant: the wavefront kernel's conservative shadow culling

namespace RT_SYM(rtk) {

constexpr uint32_t WAVES = 4; // waves per workgroup of the ray kernel

// render_ray (rt_shade.hpp) for a wave whose lanes trace nearby rays, with the wavefront kernel's exact shadow culling: after each
// round of nearest hits the wave forms one ball around its lanes' hit points (wave_hit_ball, rt_wave_ball.hpp: box centre, half
// diagonal plus the 1e-2 shadow bias) and, per light, one wave-wide verdict per object (sphere_relevant, one object per lane); only
// objects that could block some lane's shadow ray are tested.  A culled object cannot block (that is the culling's contract), so
// every lane's in_shadow -- and with it every colour -- is what render_ray computes.  Lanes stay resident (a `live` flag instead of
// break) so that the reductions run on the whole wave.  scull[j] = object j's culling entry (r = +inf: always tested).
// COUNT builds count a shadow ray's tests as the reference does (rt_counters.tests): it stops at the first blocker and tests every
// object before it, culled or not -- the first blocker's index + 1, or n_obj when nothing blocks.  (The blocker the culled loop
// finds is that same object: a culled object cannot block.)
template <bool COUNT>
__device__ __forceinline__ F3 render_ray_culled(const FrameArgs &fa, const DevObject *__restrict__ gobj, const DevLight *__restrict__ glight,
                                                const DevObject *sobj, const UsEntry *scull, const D3 &origin, D3 dir, bool live, Cnt<COUNT> &cnt)
{
    const F3 bg{fa.bg[0], fa.bg[1], fa.bg[2]};
    const uint32_t lane = threadIdx.x & 63u;
    F3 res = bg;
    D3 o = origin;
    float cur_ratio = 1.0f;
    uint32_t n_refl = 0;
    bool first = true;
    while (__ballot(live)) { // wave-uniform
        // nearest hit: get_color_and_object, src/update-cpu.cpp:45-60 (the loop of trace(), rt_shade.hpp)
        int best = -1;
        double best_t = INFINITY;
        if (live) {
            Mono m;
            make_mono(m, o, dir);
            for (uint32_t k = 0; k < fa.n_obj; k++) {
                double t = intersect(gobj[k].c, gobj[k].cls, m, MAX_T, false);
                cnt.test();
                if (t >= EPS && t < MAX_T && t < best_t) {
                    best_t = t;
                    best = (int) k;
                }
            }
        }
        const bool hit = best >= 0;
        D3 sp{0.0, 0.0, 0.0}, sn{0.0, 0.0, 0.0}, so{0.0, 0.0, 0.0};
        F3 albedo{0.0f, 0.0f, 0.0f};
        if (hit) {
            cnt.hit();
            sp = D3{o.x + best_t * dir.x, o.y + best_t * dir.y, o.z + best_t * dir.z};
            const DevObject *bo = &sobj[best];
            sn = normal_vector(bo->c, sp);
            albedo = F3{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
            so = D3{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
        }
        F3 acc{0.0f, 0.0f, 0.0f};
        if (__ballot(hit)) { // wave-uniform
            bool cull = fa.cull != 0u;
            Ball ball{0.0, 0.0, 0.0, INFINITY};
            if (cull) cull = wave_hit_ball<true>(hit, sp, ball); // (false: a NaN / inf hit point, test everything)
            for (uint32_t l = 0; l < fa.n_lights; l++) {
                const DevLight *lt = &glight[l];
                const bool spherical = lt->spherical != 0;
                double max_t = 0.0;
                D3 sd{0.0, 0.0, 0.0};
                Mono sm;
                bool in_shadow = false;
                uint32_t blocker = fa.n_obj; // (COUNT builds)
                if (hit) {
                    sd = shadow_dir(lt->p, spherical, sp, max_t);
                    cnt.shadow();
                    make_mono(sm, so, sd);
                }
                for (uint32_t base = 0; base < fa.n_obj; base += 64u) {
                    unsigned long long mask;
                    if (cull && (spherical || fabs(lt->u2) > EPS)) { // (a directional light with |d|^2 <= EPS: the reference's linear branch, t = -t0 / t1, is not geometry -- test everything)
                        const uint32_t j = base + lane;
                        bool rel = false;
                        if (j < fa.n_obj) rel = spherical ? sphere_relevant<true>(scull[j], ball, *lt) : sphere_relevant<false>(scull[j], ball, *lt);
                        mask = __ballot(rel);
                    } else {
                        const uint32_t n = fa.n_obj - base;
                        mask = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
                    }
                    while (mask && __ballot(hit && !in_shadow)) { // wave-uniform
                        const uint32_t k = base + (uint32_t) __builtin_ctzll(mask);
                        mask &= mask - 1ull;
                        if (hit && !in_shadow) {
                            const double t = intersect(gobj[k].c, gobj[k].cls, sm, max_t, true);
                            if (t > EPS && t < max_t) {
                                in_shadow = true;
                                if (COUNT) blocker = k;
                            }
                        }
                    }
                }
                if (COUNT && hit) cnt.tests(in_shadow ? blocker + 1ull : (unsigned long long) fa.n_obj);
                if (hit && !in_shadow) {
                    const F3 c = surface_color(lt->p, lt->color, spherical, sp, sn, albedo);
                    acc.x += c.x;
                    acc.y += c.y;
                    acc.z += c.z;
                }
            }
        }
        if (live) { // the bounce decision of render_ray
            if (!hit) {
                if (!first) RT_SYM(rtk)::blend(res, cur_ratio, bg);
                live = false;
            } else {
                const F3 oc{(acc.x < 1.0f) ? acc.x : 1.0f, (acc.y < 1.0f) ? acc.y : 1.0f, (acc.z < 1.0f) ? acc.z : 1.0f};
                if (first) res = oc;
                else RT_SYM(rtk)::blend(res, cur_ratio, oc);
                first = false;
                const float refl = sobj[best].refl;
                if (!((double) refl > EPS)) {
                    live = false;
                } else {
                    cur_ratio *= refl;
                    if (n_refl == fa.max_refl) {
                        RT_SYM(rtk)::blend(res, cur_ratio, bg);
                        live = false;
                    } else {
                        n_refl++;
                        dir = reflect_ray(dir, sn);
                        cnt.reflect();
                        o = D3{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
                    }
                }
            }
        }
    }
    return res;
}

// One lane = one sample ray; a wave = 64 / K^2 pixels (K = 4: 4 pixels of 16 lanes; K = 2: 16 pixels of 4 lanes; K = 1: 64 pixels of the
// halo rows).  Workgroups of four waves stage the scene into LDS once and then take items by a grid-stride loop over the device-side
// count, so the grid size never depends on the frame.  The items, the resolve and the store are the streamed twins' (rt_ray_list.hpp:
// sl_item, sl_resolve_store); what is this kernel's own is the staging prologue, the counters and render_ray_culled.
template <int K, bool COUNT, bool RGBA8>
__global__ __launch_bounds__(256) void ray_list_kernel(const FrameArgs fa, const DevObject *__restrict__ gobj, const DevLight *__restrict__ glight,
                                                       const double *__restrict__ camx, const double *__restrict__ camy,
                                                       const uint32_t *__restrict__ list, const uint32_t *__restrict__ count_ptr, uint32_t n_items,
                                                       void *__restrict__ out, unsigned long long *__restrict__ counters)
{
    extern __shared__ __align__(16) unsigned char smem[];
    DevObject *sobj = reinterpret_cast<DevObject *>(smem);
    UsEntry *scull = reinterpret_cast<UsEntry *>(smem + (size_t) fa.n_obj * sizeof(DevObject));
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(gobj);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        const uint32_t n16 = fa.n_obj * (uint32_t) (sizeof(DevObject) / 16);
        for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
        for (uint32_t i = threadIdx.x; i < fa.n_obj; i += blockDim.x) { // culling entries (UsEntry layout; only kx, ky, kz, r, inv_r are read)
            const DevObject &g = gobj[i];
            UsEntry e{};
            e.kx = g.c[K_X];
            e.ky = g.c[K_Y];
            e.kz = g.c[K_Z];
            e.c = g.c[K_C];
            e.r = g.bs_radius;
            e.inv_r = (g.bs_radius < INFINITY) ? 1.0 / g.bs_radius : 0.0;
            e.orig = i;
            scull[i] = e;
        }
    }
    __syncthreads();

    constexpr uint32_t LANES = (uint32_t) (K * K), PPW = 64u / LANES; // lanes per pixel, pixels per wave
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t sub = lane % LANES, i = sub % (uint32_t) K, j = sub / (uint32_t) K;
    const uint32_t n = count_ptr ? *count_ptr : n_items;
    const D3 origin{fa.origin[0], fa.origin[1], fa.origin[2]};
    Cnt<COUNT> cnt;
    for (uint32_t base = (blockIdx.x * WAVES + wave) * PPW; base < n; base += gridDim.x * WAVES * PPW) { // wave-uniform
        const SlItem it = sl_item<K>(fa, camx, camy, list, base + lane / LANES, n, i, j);
        if (it.use) cnt.primary();
        const F3 c = render_ray_culled<COUNT>(fa, gobj, glight, sobj, scull, origin, it.dir, it.use, cnt);
        sl_resolve_store<K, RGBA8>(fa, out, it, sub, c);
    }
    cnt.flush(counters);
}

// One rt_hit record as gbuffer_kernel's coordinate-list mode writes it (rt_pixel_kernels.hpp: pk_gbuffer; rt_rayquery.hpp: RqRecord): the halo rows' object and normal
struct GeoHalo {
    double t, p[3];
    float n[3];
    int32_t object;
};
static_assert(sizeof(GeoHalo) == 48, "rt_hit layout");

// dotf of include/mi355rt.h (RT_FLAG_SSAA_GEOMETRY): float32, every operation rounded separately in every build
__device__ __forceinline__ float geo_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// The body of both classifiers.  One lane per output pixel, a wave per 8 x 8 block (a workgroup per 16 x 16 tile), so that the list keeps
// locality.  refine(x, y): tau < 0, or some 8-neighbour n inside the image and channel c with !(fabsf(P(x,y).c - P(n).c) <= tau); with
// GEOMETRY (RT_FLAG_SSAA_GEOMETRY) also when that neighbour has another primary-hit object, or the same object (>= 0) and
// !(dotf(N(x, y), N(n)) >= min_cos).  obj / nrm: this rank's planes ([local_rows][width], gbuffer_kernel's plane mode; nrm = NULL: ids
// only, launch-uniform), ghalo: [2 * bands][width] records of the halo rows (world > 1; the slots of `halo`); none of the three is read
// without GEOMETRY.  Every neighbour is read where it lies: a neighbour row is local row r of P and the planes (the same band) or halo
// slot r (a row of another rank) -- with bands of any height per lane, so there is no rectangular apron to stage.
// Unrefined pixels are written to `out` in the context's format (nothing to write when out is P itself); refined ones are appended to
// the list, one atomicAdd per wave.
template <bool RGBA8, bool GEOMETRY>
__device__ __forceinline__ void classify_body(const float4 *__restrict__ p, const float4 *__restrict__ halo, const int32_t *__restrict__ obj,
                                              const float4 *__restrict__ nrm, const GeoHalo *__restrict__ ghalo, uint32_t width, uint32_t height,
                                              uint32_t local_rows, uint32_t tiles_x, uint32_t band_rows, uint32_t world, uint32_t rank, float tau,
                                              float min_cos, void *out, uint32_t *__restrict__ list, uint32_t *__restrict__ count)
{
    const uint32_t tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = tile_x * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t lr = tile_y * 16u + (wave >> 1) * 8u + (lane >> 3);
    const bool in = x < width && lr < local_rows;
    const bool normals = GEOMETRY && nrm != nullptr; // launch-uniform
    bool refine = false;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (in) {
        const size_t at = (size_t) lr * width + x;
        c = p[at];
        refine = tau < 0.0f;
        int32_t id = -1;
        float4 n0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (GEOMETRY) {
            id = obj[at];
            if (normals && id >= 0) n0 = nrm[at];
        }
        const uint32_t b = lr / band_rows, t = lr - b * band_rows;
        const int64_t gy = ((int64_t) b * world + rank) * band_rows + t;
        for (int dy = -1; dy <= 1 && !refine; dy++) {
            const int64_t ny = gy + dy;
            if (ny < 0 || ny >= (int64_t) height) continue;
            // the neighbour row: local row r of P and the planes, or halo slot r
            bool from_halo = false;
            uint32_t r = lr;
            if (dy != 0) {
                if (world == 1u) r = lr + dy;
                else if (dy < 0) { from_halo = t == 0u; r = from_halo ? 2u * b : lr - 1u; }
                else { from_halo = !(t + 1u < band_rows && lr + 1u < local_rows); r = from_halo ? 2u * b + 1u : lr + 1u; }
            }
            const size_t row = (size_t) r * width;
            for (int dx = -1; dx <= 1; dx++) {
                const int64_t nx = (int64_t) x + dx;
                if ((dx == 0 && dy == 0) || nx < 0 || nx >= (int64_t) width) continue;
                const float4 v = from_halo ? halo[row + nx] : p[row + nx];
                if (!(fabsf(c.x - v.x) <= tau) || !(fabsf(c.y - v.y) <= tau) || !(fabsf(c.z - v.z) <= tau)) refine = true;
                if constexpr (GEOMETRY) {
                    const int32_t idn = from_halo ? ghalo[row + nx].object : obj[row + nx];
                    if (idn != id) {
                        refine = true;
                    } else if (normals && id >= 0) {
                        float bx, by, bz;
                        if (from_halo) {
                            const GeoHalo *g = &ghalo[row + nx];
                            bx = g->n[0]; by = g->n[1]; bz = g->n[2];
                        } else {
                            const float4 n1 = nrm[row + nx];
                            bx = n1.x; by = n1.y; bz = n1.z;
                        }
                        if (!(geo_dot(n0.x, n0.y, n0.z, bx, by, bz) >= min_cos)) refine = true;
                    }
                }
            }
        }
    }
    const unsigned long long m = __ballot(refine);
    if (in && !refine) {
        const size_t o = (size_t) lr * width + x;
        if (RGBA8) reinterpret_cast<uchar4 *>(out)[o] = quantise(c.x, c.y, c.z);
        else if (out != (const void *) p) reinterpret_cast<float4 *>(out)[o] = make_float4(c.x, c.y, c.z, 1.0f);
    }
    if (m == 0ull) return; // wave-uniform
    uint32_t base = 0;
    if (lane == 0u) base = atomicAdd(count, (uint32_t) __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (refine) list[base + (uint32_t) __popcll(m & ((1ull << lane) - 1ull))] = (lr << 16) | x;
}

// The classifier of the colour term alone: classify_body with everything geometric compiled out.
template <bool RGBA8>
__global__ __launch_bounds__(256) void classify_kernel(const float4 *__restrict__ p, const float4 *__restrict__ halo, uint32_t width, uint32_t height,
                                                       uint32_t local_rows, uint32_t tiles_x, uint32_t band_rows, uint32_t world, uint32_t rank, float tau,
                                                       void *out, uint32_t *__restrict__ list, uint32_t *__restrict__ count)
{
    classify_body<RGBA8, false>(p, halo, nullptr, nullptr, nullptr, width, height, local_rows, tiles_x, band_rows, world, rank, tau, 0.0f, out, list, count);
}

// ... and with the geometric term of RT_FLAG_SSAA_GEOMETRY.
template <bool RGBA8>
__global__ __launch_bounds__(256) void classify_geometry_kernel(const float4 *__restrict__ p, const float4 *__restrict__ halo, const int32_t *__restrict__ obj,
                                                                const float4 *__restrict__ nrm, const GeoHalo *__restrict__ ghalo, uint32_t width,
                                                                uint32_t height, uint32_t local_rows, uint32_t tiles_x, uint32_t band_rows, uint32_t world,
                                                                uint32_t rank, float tau, float min_cos, void *out, uint32_t *__restrict__ list,
                                                                uint32_t *__restrict__ count)
{
    classify_body<RGBA8, true>(p, halo, obj, nrm, ghalo, width, height, local_rows, tiles_x, band_rows, world, rank, tau, min_cos, out, list, count);
}

template <int K, bool COUNT, bool RGBA8>
static hipError_t launch_rays(const FrameArgs *fa, const DevObject *gobj, const DevLight *glight, const double *camx, const double *camy, const uint32_t *list,
                              const uint32_t *count_ptr, uint32_t n_items, uint32_t grid, void *out, unsigned long long *counters, hipStream_t stream)
{
    const size_t lds = (size_t) fa->n_obj * (sizeof(DevObject) + sizeof(UsEntry));
    hipLaunchKernelGGL((ray_list_kernel<K, COUNT, RGBA8>), dim3(grid), dim3(256), lds, stream, *fa, gobj, glight, camx, camy, list, count_ptr, n_items, out, counters);
    return hipGetLastError();
}

} // namespace RT_SYM(rtk)

// k = 2 / 4: sample rays of the listed pixels (count_ptr = the device-side list length) into `out` (rgba8: uchar4, else float4);
// k = 1: the halo rows' centre rays, n_items = 2 * bands * width slots, into `out` = [2 * bands][width] float4.  `grid` workgroups
// of 256 lanes, fixed per context.
extern "C" hipError_t RT_SYM(rt_launch_ray_list)(const FrameArgs *fa, const DevObject *gobj, const DevLight *glight, const double *camx, const double *camy,
                                                  const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out,
                                                  int rgba8, int count, unsigned long long *counters, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    if (grid == 0u) return hipSuccess;
    return sl_for_shapes(k, rgba8, [&](auto kk, auto r8) {
        constexpr int K = decltype(kk)::value;
        constexpr bool RGBA8 = decltype(r8)::value;
        return count ? launch_rays<K, true, RGBA8>(fa, gobj, glight, camx, camy, list, count_ptr, n_items, grid, out, counters, stream)
                     : launch_rays<K, false, RGBA8>(fa, gobj, glight, camx, camy, list, count_ptr, n_items, grid, out, counters, stream);
    });
}

// p = [local_rows][width] RGBA32F plain frame, halo = [2 * bands][width] (world > 1), out = [local_rows][width] pixels (may be p
// itself for RGBA32F), list = [local_rows * width] words, count = the list length (cleared by the caller on the stream).
extern "C" hipError_t RT_SYM(rt_launch_classify)(const void *p, const void *halo, uint32_t width, uint32_t height, uint32_t local_rows, uint32_t band_rows,
                                                  uint32_t world, uint32_t rank, float tau, void *out, int rgba8, uint32_t *list, uint32_t *count,
                                                  hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    const uint32_t tiles_x = (width + 15u) / 16u, tiles = tiles_x * ((local_rows + 15u) / 16u);
    if (tiles == 0u) return hipSuccess;
    if (rgba8)
        hipLaunchKernelGGL((classify_kernel<true>), dim3(tiles), dim3(256), 0, stream, (const float4 *) p, (const float4 *) halo, width, height, local_rows,
                           tiles_x, band_rows, world, rank, tau, out, list, count);
    else
        hipLaunchKernelGGL((classify_kernel<false>), dim3(tiles), dim3(256), 0, stream, (const float4 *) p, (const float4 *) halo, width, height, local_rows,
                           tiles_x, band_rows, world, rank, tau, out, list, count);
    return hipGetLastError();
}

// The same with the geometric term (RT_FLAG_SSAA_GEOMETRY): obj / nrm = this rank's id and normal planes (nrm = NULL: ids only),
// ghalo = [2 * bands][width] rt_hit records of the halo rows (world > 1).
extern "C" hipError_t RT_SYM(rt_launch_classify_geometry)(const void *p, const void *halo, const int32_t *obj, const float *nrm, const void *ghalo, uint32_t width,
                                                           uint32_t height, uint32_t local_rows, uint32_t band_rows, uint32_t world, uint32_t rank, float tau,
                                                           float min_cos, void *out, int rgba8, uint32_t *list, uint32_t *count, hipStream_t stream)
{
    using namespace RT_SYM(rtk);
    const uint32_t tiles_x = (width + 15u) / 16u, tiles = tiles_x * ((local_rows + 15u) / 16u);
    if (tiles == 0u) return hipSuccess;
    if (rgba8)
        hipLaunchKernelGGL((classify_geometry_kernel<true>), dim3(tiles), dim3(256), 0, stream, (const float4 *) p, (const float4 *) halo, obj, (const float4 *) nrm,
                           (const GeoHalo *) ghalo, width, height, local_rows, tiles_x, band_rows, world, rank, tau, min_cos, out, list, count);
    else
        hipLaunchKernelGGL((classify_geometry_kernel<false>), dim3(tiles), dim3(256), 0, stream, (const float4 *) p, (const float4 *) halo, obj, (const float4 *) nrm,
                           (const GeoHalo *) ghalo, width, height, local_rows, tiles_x, band_rows, world, rank, tau, min_cos, out, list, count);
    return hipGetLastError();
}
