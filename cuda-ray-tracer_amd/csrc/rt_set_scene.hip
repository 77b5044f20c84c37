// rt_set_scene.hip -- rewrite a context's scene in stream order: rt_set_scene (include/mi355rt.h).
//
// One launch of ONE workgroup reads the caller's raw descriptor arrays (rt_scene_desc layout; a NULL array = the raw values the
// context's own DevObject / DevLight records hold), rebuilds every derived record with the functions rt_create itself packs with
// (rt_scene_pack.hpp) and rewrites the blob and both light tables in place -- or, when the new scene would not have the layout the
// host-side state of the context was chosen for, writes nothing at all and says why.
//
//   phase 1  derive + validate, objects: every thread derives the DevObject of its objects (i = thread, thread + 256, ...) in registers
//            and holds it against the record the context holds: same table, same cullability, degree 3: the same 20
//            coefficients bit for bit.  It also reduces "every albedo is finite" (the lights' backface_exact / LightK::flags 2 and 8)
//            and "some object is a mirror" (FrameArgs::has_mirror must stay what it is).
//   phase 2  derive + validate, lights: DevLight and LightK of every light; LightK::flags must be the ones the context holds.
//   phase 3  commit, all or nothing: nothing offended -> DevObject and MatEntry of every object, barrier, the table entries (slot by
//            slot, from the new DevObject of the slot's `orig`, exactly as rt_create forms them from its object array), DevLight and
//            LightK, then (contexts with chunk bounds, RT_FLAG_STREAM_CULL) barrier and the bound of every 64-entry chunk of the
//            unit-sphere table from its rebuilt entries, then status.applied += 1.  Otherwise status.rejected += 1 with the reason and the index of the first offender.
//
// A record is 224 bytes and rt_create accepts about 2 500 objects (160 KiB of class tables), so the derived records of phase 1 cannot
// wait in LDS for the verdict (560 KB); phase 3 derives them again from the same inputs -- a few dozen FP64 operations per object --
// and the only things that cross the barriers are the verdict and three reduction words in LDS.  The inputs must not change while the kernel runs.
//
// The status block is written by thread 0 with ordinary (vector) stores.
//
// Built ONCE, without FMA contraction, and used by strict and RT_FLAG_FAST contexts alike (as rt_resolve.hip is): rt_create packs on the
// host without contraction whatever the context's flags, and -ffp-contract=fast lets the back end fuse across rt_scene_pack.hpp's own
// contraction pragma (seen: cx * cx + cy * cy + cz * cz became two v_fmac_f64), so a "fast" build of this kernel would not reproduce
// rt_create's bytes.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include <stdint.h>

#include "rt_scene_dev.h"
#include "rt_scene_pack.hpp"
#include "rt_set_scene.h"

namespace rtk_set_scene {

#define SS_THREADS 256
#define SS_OK 0xFFFFFFFFu

// raw values of object i: the caller's arrays where given, else what the context's record holds
__device__ inline void raw_object(const SetSceneArgs &a, const DevObject *objs, uint32_t i, double *c, float *albedo, float &refl)
{
    const DevObject &old = objs[i];
    for (int k = 0; k < 20; k++) c[k] = a.coefs ? a.coefs[(size_t) i * 20u + k] : old.c[k];
    for (int k = 0; k < 3; k++) albedo[k] = a.albedo ? a.albedo[(size_t) i * 3u + k] : old.albedo[k];
    refl = a.reflection ? a.reflection[i] : old.refl;
}

__device__ inline bool pack_light_of(const SetSceneArgs &a, const DevLight *lights, uint32_t l, bool albedos_finite, DevLight &dl)
{
    const DevLight &old = lights[l];
    double p[3];
    float col[3];
    for (int k = 0; k < 3; k++) {
        p[k] = a.light_p ? a.light_p[(size_t) l * 3u + k] : old.p[k];
        col[k] = a.light_color ? a.light_color[(size_t) l * 3u + k] : old.color[k];
    }
    return rtp::pack_light(dl, p, col, old.spherical, albedos_finite); // (the kind is fixed)
}

// the verdict: (index << 4 | reason) of the first offender, objects before lights, lowest index first
__device__ inline void offend(uint32_t *verdict, uint32_t index, uint32_t reason) { atomicMin(verdict, (index << 4) | reason); }

__global__ void __launch_bounds__(SS_THREADS) set_scene_kernel(SetSceneArgs a)
{
    __shared__ uint32_t s_verdict, s_nonfinite, s_any_mirror, s_lost_mirror;
    const uint32_t tid = threadIdx.x;
    DevObject *objs = reinterpret_cast<DevObject *>(a.blob);
    DevLight *lights = a.lights;
    LightK *lightk = reinterpret_cast<LightK *>(a.lights + a.n_lights);
    if (tid == 0) {
        s_verdict = SS_OK;
        s_nonfinite = 0u;
        s_any_mirror = 0u;
        s_lost_mirror = SS_OK;
    }
    __syncthreads();

    // ---- phase 1: objects ---------------------------------------------------------------------------------------------------
    for (uint32_t i = tid; i < a.n_obj; i += SS_THREADS) {
        double c[20];
        float albedo[3], refl;
        raw_object(a, objs, i, c, albedo, refl);
        DevObject o;
        rtp::pack_object(o, c, albedo, refl);
        const DevObject &old = objs[i];
        if (!rtp::albedo_finite(o.albedo)) atomicOr(&s_nonfinite, 1u);
        uint32_t reason = 0u;
        if (rtp::table_of(o.cls) != rtp::table_of(old.cls)) reason = RT_SCENE_REJECT_CLASS;
        else if (rtp::cullable(o) != rtp::cullable(old)) reason = RT_SCENE_REJECT_BOUND;
        else if (rtp::is_mirror(o.refl) && !a.has_mirror) reason = RT_SCENE_REJECT_MIRROR; // the scene would gain its first mirror
        else if (o.cls & RT_CLS_CUBIC) {
            bool same = true;
            for (int k = 0; k < 20; k++) same = same && (__double_as_longlong(o.c[k]) == __double_as_longlong(old.c[k]));
            if (!same) reason = RT_SCENE_REJECT_CUBIC;
        }
        if (reason) offend(&s_verdict, i, reason);
        if (rtp::is_mirror(o.refl)) atomicOr(&s_any_mirror, 1u);
        else if (rtp::is_mirror(old.refl)) atomicMin(&s_lost_mirror, i);
    }
    __syncthreads();
    const bool albedos_finite = s_nonfinite == 0u;
    if (tid == 0 && a.has_mirror && !s_any_mirror) offend(&s_verdict, s_lost_mirror, RT_SCENE_REJECT_MIRROR); // ... or lose its last one

    // ---- phase 2: lights ----------------------------------------------------------------------------------------------------
    for (uint32_t l = tid; l < a.n_lights; l += SS_THREADS) {
        DevLight dl;
        LightK k;
        const bool term_finite = pack_light_of(a, lights, l, albedos_finite, dl);
        rtp::pack_lightk(k, dl, term_finite);
        if (k.flags != lightk[l].flags) offend(&s_verdict, a.n_obj + l, RT_SCENE_REJECT_LIGHT);
    }
    __syncthreads();
    const uint32_t verdict = s_verdict;

    // ---- phase 3: commit, all or nothing --------------------------------------------------------------------------------------
    if (verdict == SS_OK) {
        MatEntry *mat = reinterpret_cast<MatEntry *>(a.blob + a.off_mat);
        for (uint32_t i = tid; i < a.n_obj; i += SS_THREADS) {
            double c[20];
            float albedo[3], refl;
            raw_object(a, objs, i, c, albedo, refl);
            DevObject o;
            rtp::pack_object(o, c, albedo, refl);
            MatEntry m;
            rtp::pack_mat(m, o);
            objs[i] = o;
            mat[i] = m;
        }
        for (uint32_t l = tid; l < a.n_lights; l += SS_THREADS) {
            DevLight dl;
            LightK k;
            const bool term_finite = pack_light_of(a, lights, l, albedos_finite, dl);
            rtp::pack_lightk(k, dl, term_finite);
            lights[l] = dl;
            lightk[l] = k;
        }
        __syncthreads(); // the table entries are formed from the new object records, as rt_create forms them
        UsEntry *us = reinterpret_cast<UsEntry *>(a.blob + a.off_us);
        for (uint32_t s = tid; s < a.n_us; s += SS_THREADS) {
            const uint32_t orig = us[s].orig;
            UsEntry e;
            rtp::pack_us(e, objs[orig], orig);
            us[s] = e;
        }
        GqEntry *gq = reinterpret_cast<GqEntry *>(a.blob + a.off_gq);
        for (uint32_t s = tid; s < a.n_gq; s += SS_THREADS) {
            const uint32_t orig = gq[s].orig;
            GqEntry e;
            rtp::pack_gq(e, objs[orig], orig);
            gq[s] = e;
        }
        LinEntry *lin = reinterpret_cast<LinEntry *>(a.blob + a.off_lin);
        for (uint32_t s = tid; s < a.n_lin; s += SS_THREADS) {
            const uint32_t orig = lin[s].orig;
            LinEntry e;
            rtp::pack_lin(e, objs[orig], orig);
            lin[s] = e;
        }
        // (degree 3: the table is the objects' indices, which stay; their coefficients were held equal above)
        if (a.n_chunks) { // (launch-uniform) RT_FLAG_STREAM_CULL: the chunk bounds from the rebuilt entries, as rt_create forms them (rt_scene_image.hpp)
            __syncthreads();
            for (uint32_t c = tid; c < a.n_chunks; c += SS_THREADS) {
                const uint32_t first = 64u * c, n = a.n_us - first < 64u ? a.n_us - first : 64u;
                UsEntry b;
                rtp::pack_chunk_bound(b, us + first, n, c);
                a.bounds[c] = b;
            }
        }
    }
    if (tid == 0) {
        SetSceneStatus *st = a.status;
        if (verdict == SS_OK) {
            st->applied = st->applied + 1ull;
            st->last = 1u;
        } else {
            const uint32_t idx = verdict >> 4;
            st->rejected = st->rejected + 1ull;
            st->reason = verdict & 15u;
            st->index = idx >= a.n_obj ? idx - a.n_obj : idx; // (a light's own index)
            st->last = 2u;
        }
    }
}

} // namespace rtk_set_scene

extern "C" hipError_t rt_launch_set_scene(const SetSceneArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(rtk_set_scene::set_scene_kernel, dim3(1), dim3(SS_THREADS), 0, stream, *args);
    return hipGetLastError();
}
