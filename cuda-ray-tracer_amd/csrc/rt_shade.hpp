// rt_shade.hpp -- the per-lane shading of one camera ray (the reference's render_pixel), shared by the simple kernel
// (rt_kernels.hip) and the adaptive supersampling kernels (rt_adaptive.hip).  Included by files that are compiled once per
// variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_SHADE_HPP
#define RT_SHADE_HPP

#include <hip/hip_runtime.h>

#include "rt_launch.h" // RT_SYM
#include "rt_math.hpp"
#include "rt_scene_dev.h"

#ifndef RT_VARIANT
#error "define RT_VARIANT=strict|fast"
#endif

namespace RT_SYM(rtk) {

using namespace rtm;

// Per-lane work counters (RT_FLAG_COUNT builds only).
template <bool COUNT>
struct Cnt {
    __device__ __forceinline__ void primary() {}
    __device__ __forceinline__ void shadow() {}
    __device__ __forceinline__ void reflect() {}
    __device__ __forceinline__ void test() {}
    __device__ __forceinline__ void tests(unsigned long long) {}
    __device__ __forceinline__ void hit() {}
    __device__ __forceinline__ void solve() {}
    __device__ __forceinline__ void flush(unsigned long long *) {}
};
template <>
struct Cnt<true> {
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void primary() { v[0]++; }
    __device__ __forceinline__ void shadow() { v[1]++; }
    __device__ __forceinline__ void reflect() { v[2]++; }
    __device__ __forceinline__ void test() { v[3]++; }
    __device__ __forceinline__ void tests(unsigned long long n) { v[3] += n; }
    __device__ __forceinline__ void hit() { v[4]++; }
    __device__ __forceinline__ void solve() { v[5]++; }
    __device__ __forceinline__ void flush(unsigned long long *g)
    {
        for (int i = 0; i < 6; i++)
            if (v[i]) atomicAdd(&g[i], v[i]);
    }
};

// Nearest hit + direct lighting for one ray: get_color_and_object, src/update-cpu.cpp:45-80
// (SURVEY.md Q7, Q12).  gobj/glight are the scene in global memory, indexed wave-uniformly (the compiler
// turns those reads into scalar loads: operands arrive in SGPRs, no VGPR or LDS bandwidth spent on
// them); sobj is the same scene staged in LDS for the reads whose index differs per lane.
template <bool COUNT>
__device__ __forceinline__ int trace(const FrameArgs &fa, const DevObject *__restrict__ gobj,
                                     const DevLight *__restrict__ glight, const DevObject *sobj, const D3 &o,
                                     const D3 &d, F3 &color, D3 &sp, D3 &sn, Cnt<COUNT> &cnt)
{
    Mono m;
    make_mono(m, o, d);
    int best = -1;
    double best_t = INFINITY;
    for (uint32_t k = 0; k < fa.n_obj; k++) {
        double t = intersect(gobj[k].c, gobj[k].cls, m, MAX_T, false);
        cnt.test();
        if (t >= EPS && t < MAX_T && t < best_t) {
            best_t = t;
            best = (int) k;
        }
    }
    if (best < 0) return -1;

    cnt.hit();
    sp = D3{o.x + best_t * d.x, o.y + best_t * d.y, o.z + best_t * d.z};
    const DevObject *bo = &sobj[best]; // per-lane index: LDS gather
    sn = normal_vector(bo->c, sp);
    const F3 albedo{bo->albedo[0], bo->albedo[1], bo->albedo[2]};
    const D3 so{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
    F3 acc{0.0f, 0.0f, 0.0f};
    for (uint32_t l = 0; l < fa.n_lights; l++) {
        const DevLight *lt = &glight[l];
        const bool spherical = lt->spherical != 0;
        double max_t;
        D3 sd = shadow_dir(lt->p, spherical, sp, max_t);
        cnt.shadow();
        Mono sm;
        make_mono(sm, so, sd);
        bool in_shadow = false;
        for (uint32_t k = 0; k < fa.n_obj; k++) {
            double t = intersect(gobj[k].c, gobj[k].cls, sm, max_t, true);
            cnt.test();
            if (t > EPS && t < max_t) {
                in_shadow = true;
                break;
            }
        }
        if (!in_shadow) {
            F3 c = surface_color(lt->p, lt->color, spherical, sp, sn, albedo);
            acc.x += c.x;
            acc.y += c.y;
            acc.z += c.z;
        }
    }
    // glm::min(vec3(1.0f), acc)
    color.x = (acc.x < 1.0f) ? acc.x : 1.0f;
    color.y = (acc.y < 1.0f) ? acc.y : 1.0f;
    color.z = (acc.z < 1.0f) ? acc.z : 1.0f;
    return best;
}

__device__ __forceinline__ void blend(F3 &res, float ratio, const F3 &c)
{
    // UPDATE_COLOR, src/update-cpu.cpp:100
    res.x = (1.0f - ratio) * res.x + ratio * c.x;
    res.y = (1.0f - ratio) * res.y + ratio * c.y;
    res.z = (1.0f - ratio) * res.z + ratio * c.z;
}

// render_pixel, src/update-cpu.cpp:82-119, for a primary ray from `origin` along `dir`: the colour the pixel stores (before
// quantisation).  sobj = the scene's object records staged in LDS.
template <bool COUNT>
__device__ __forceinline__ F3 render_ray(const FrameArgs &fa, const DevObject *__restrict__ gobj, const DevLight *__restrict__ glight,
                                         const DevObject *sobj, const D3 &origin, D3 dir, Cnt<COUNT> &cnt)
{
    // render_pixel, src/update-cpu.cpp:82-119, written as ONE bounce loop so that the
    // trace code exists once: iteration 0 is the primary ray, iteration k the k-th mirror bounce.  The loop
    // ends for the wave when no lane is still bouncing (exec mask empty).
    const F3 bg{fa.bg[0], fa.bg[1], fa.bg[2]};
    F3 res = bg;
    D3 o = origin;
    float cur_ratio = 1.0f;
    uint32_t n_refl = 0;
    bool first = true;
    for (;;) {
        F3 oc;
        D3 sp, sn;
        const int idx = trace<COUNT>(fa, gobj, glight, sobj, o, dir, oc, sp, sn, cnt);
        if (idx < 0) {
            if (!first) blend(res, cur_ratio, bg); // a bounce that leaves the scene picks up the background
            break;
        }
        if (first) res = oc;
        else blend(res, cur_ratio, oc);
        first = false;
        const float refl = sobj[idx].refl;
        if (!((double) refl > EPS)) break;
        cur_ratio *= refl;
        if (n_refl == fa.max_refl) {
            blend(res, cur_ratio, bg);
            break;
        }
        n_refl++;
        dir = reflect_ray(dir, sn);
        cnt.reflect();
        o = D3{sp.x + SHADOW_BIAS * sn.x, sp.y + SHADOW_BIAS * sn.y, sp.z + SHADOW_BIAS * sn.z};
    }

    return res;
}

// the RGBA8 store of the render kernels, (unsigned char)(int)(v * 255.0f + 0.5f), with both operations rounded separately in
// every build (the strict kernels' and rt_resolve.hip's value): what the ray-list kernels store (rt_adaptive.hip, rt_stream_shell.hpp)
__device__ __forceinline__ uchar4 quantise(float x, float y, float z)
{
    uchar4 px;
    px.x = (unsigned char) (int) __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
    px.y = (unsigned char) (int) __fadd_rn(__fmul_rn(y, 255.0f), 0.5f);
    px.z = (unsigned char) (int) __fadd_rn(__fmul_rn(z, 255.0f), 0.5f);
    px.w = 255;
    return px;
}

// pairwise float32 sum over the lanes `m` apart (the resolve's tree, one level)
__device__ __forceinline__ F3 xor_add(const F3 &v, int m)
{
    return F3{__fadd_rn(v.x, __shfl_xor(v.x, m)), __fadd_rn(v.y, __shfl_xor(v.y, m)), __fadd_rn(v.z, __shfl_xor(v.z, m))};
}

} // namespace RT_SYM(rtk)

#endif
