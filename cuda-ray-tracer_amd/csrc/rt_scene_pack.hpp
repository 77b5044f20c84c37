// rt_scene_pack.hpp -- the derived scene data, one record at a time: what rt_create packs on the host (rt_scene_image.hpp, scene_image) and
// what rt_set_scene rebuilds on the device (rt_set_scene.hip).  Both call these functions, so the two cannot drift apart.
//
// Every function is a pure function of the raw descriptor values (rt_scene_desc semantics: 20 coefficients, reflection, albedo; a
// light's p, colour and kind) and fills EVERY byte of its record, pads included -- none of the records has implicit padding
// (rt_scene_dev.h, static_asserts) -- so a record formed here is bit for bit the record of a fresh context.
//
// Arithmetic: FP64 / FP32 exactly as written, one rounding per operation; sqrt and division are the correctly rounded ones on both
// sides.  Every translation unit that includes this is built with -ffp-contract=off (the Makefile's host flags and the rule of
// rt_set_scene.hip); the pragma below covers a compiler default that honours pragmas, but NOT -ffp-contract=fast, under which the back
// end fuses whatever it finds -- so there is no RT_FLAG_FAST build of these functions.
#ifndef RT_SCENE_PACK_HPP
#define RT_SCENE_PACK_HPP

#include <math.h>
#include <stdint.h>

#include "rt_scene_dev.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_PACK_FN __host__ __device__ inline
#else
#define RT_PACK_FN inline
#endif
#if defined(__clang__)
#define RT_PACK_STRICT _Pragma("clang fp contract(off)")
#else
#define RT_PACK_STRICT /* (the host compiler gets -ffp-contract=off from the build) */
#endif

namespace rtp {

// isfinite / isinf as comparisons (NaN compares false): the same truth values as <cmath>'s, available to every compiler that reads this
RT_PACK_FN bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }
RT_PACK_FN bool finite32(float x) { return fabsf(x) <= 3.402823466e38f; }

// the table an object of class `cls` lives in: 0 unit spheres (UsEntry), 1 other quadrics (GqEntry), 2 planes (LinEntry), 3 degree 3
RT_PACK_FN uint32_t table_of(uint32_t cls)
{
    if (cls & RT_CLS_CUBIC) return 3u;
    if (cls & RT_CLS_UNITSQ) return 0u;
    if (cls & (RT_CLS_SQUARE | RT_CLS_CROSS)) return 1u;
    return 2u;
}

RT_PACK_FN uint32_t classify(const double *c)
{
    uint32_t cls = 0;
    for (int i = K_X3; i <= K_XYZ; i++)
        if (c[i] != 0.0) cls |= RT_CLS_CUBIC;
    if (cls & RT_CLS_CUBIC) return RT_CLS_CUBIC; // dense path handles everything
    if (c[K_X2] != 0.0 || c[K_Y2] != 0.0 || c[K_Z2] != 0.0) cls |= RT_CLS_SQUARE;
    if (c[K_XY] != 0.0 || c[K_XZ] != 0.0 || c[K_YZ] != 0.0) cls |= RT_CLS_CROSS;
    if (!(cls & RT_CLS_CROSS) && c[K_X2] == 1.0 && c[K_Y2] == 1.0 && c[K_Z2] == 1.0) cls |= RT_CLS_UNITSQ;
    return cls;
}

// EPS of the reflection loop, src/update-cpu.cpp:101: this object makes the scene one "with a mirror" (FrameArgs::has_mirror)
RT_PACK_FN bool is_mirror(float reflection) { return (double) reflection > 1e-7; }

// DevObject from Object (coefs[20], albedo[3], reflection).  Cullable (counted for FrameArgs::cull / all_cullable) = bs_radius finite.
RT_PACK_FN void pack_object(DevObject &o, const double *coefs, const float *albedo, float reflection)
{
    RT_PACK_STRICT
    for (int k = 0; k < 20; k++) o.c[k] = coefs[k];
    o.albedo[0] = albedo[0];
    o.albedo[1] = albedo[1];
    o.albedo[2] = albedo[2];
    o.refl = reflection;
    o.cls = classify(o.c);
    o.pad[0] = o.pad[1] = o.pad[2] = 0u;
    // bounding sphere of a sphere: centre -k/2, r^2 = |centre|^2 - c (src/surface.cpp:4-15 inverted)
    o.bs_center[0] = o.bs_center[1] = o.bs_center[2] = 0.0;
    o.bs_radius = INFINITY;
    if (o.cls & RT_CLS_UNITSQ) {
        const double cx = -0.5 * o.c[K_X], cy = -0.5 * o.c[K_Y], cz = -0.5 * o.c[K_Z];
        const double r2 = cx * cx + cy * cy + cz * cz - o.c[K_C];
        if (r2 > 0.0 && finite64(r2)) {
            o.bs_center[0] = cx;
            o.bs_center[1] = cy;
            o.bs_center[2] = cz;
            o.bs_radius = sqrt(r2);
        }
    }
}

RT_PACK_FN bool cullable(const DevObject &o) { return o.bs_radius < INFINITY; }

RT_PACK_FN void pack_us(UsEntry &e, const DevObject &o, uint32_t orig)
{
    RT_PACK_STRICT
    e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
    e.r = o.bs_radius;
    e.inv_r = (o.bs_radius < INFINITY) ? 1.0 / o.bs_radius : 0.0;
    e.orig = orig;
    e.pad = 0u;
    // window of the reference's own t0 inside which a shadow ray leaving this sphere towards a directional light in front of the
    // surface cannot be blocked by this sphere (rt_wavefront.hip, own_sphere_skippable): (1e-10 (r^2 + 1) + 1e-20 S^2, (r + 1)^2),
    // S = 2 |centre|_1 + 3 r + 3; rounded inwards to FP32.  No window (+inf, 0) for spheres without a real radius.
    e.own_lo = INFINITY;
    e.own_hi = 0.0f;
    if (o.bs_radius < INFINITY && o.bs_radius > 0.0) {
        const double r = o.bs_radius, S = 2.0 * (fabs(o.bs_center[0]) + fabs(o.bs_center[1]) + fabs(o.bs_center[2])) + 3.0 * r + 3.0;
        const double lo = 1e-10 * (r * r + 1.0) + 1e-20 * S * S, hi = (r + 1.0) * (r + 1.0);
        float flo = (float) lo, fhi = (float) hi;
        if (!((double) flo > lo)) flo = nextafterf(flo, INFINITY);
        if (!((double) fhi < hi)) fhi = nextafterf(fhi, -INFINITY);
        if (finite64(lo) && finite64(hi) && (double) flo > lo && (double) fhi < hi && flo < fhi) {
            e.own_lo = flo;
            e.own_hi = fhi;
        }
    }
}

// The bound of one 64-entry chunk of the unit-sphere table (RT_FLAG_STREAM_CULL): a sphere entry that the culling
// predicates of rt_wavefront_math.hpp (sphere_in_cone, sphere_relevant) are asked about INSTEAD of the chunk's members, so that a
// "skip" for the bound skips the whole chunk.  members: the chunk's n entries (1 .. 64) as pack_us wrote them; chunk: its index.
//
//   centre C   the middle of the box of the members' centres (a member's centre is -k / 2, exactly)
//   inv_r      the largest of the members' inv_r
//   r          max_i (|c_i - C| + r_i) + pad, pad = 2e-6 D + 1e-12 inv_r D (2 |C|_1 + D) + 1e-14 (|C|_1 + D + r_max), D = max_i |c_i - C|,
//              the sum then rounded outwards by a factor 1 + 1e-12
//   kx .. kz   -2 C;  c = |C|^2 - r^2 (a genuine sphere);  orig = chunk;  no own-sphere window
//
// Why a verdict about the bound covers every member.  Both predicates skip a sphere (centre c, radius r, 1 / r = q) when a distance of
// its centre from the rays' cone / axis / segment exceeds  lim(c, r, q) = r + [R] + 1e-6 (|c - p|_1 + r + ...) + 1e-12 (|c|^2 + s + 1) q,
// p and s being the same for every sphere of the call.  For a member i, with d_i = |c_i - C| <= D:
//   * its distance is at least the bound's distance minus d_i (triangle inequality; the "entirely behind" half of the directional test
//     moves by at most d_i |sdir| < d_i len_u);
//   * lim(c_i, r_i, q_i) - lim(C, r, inv_r) <= (r_i - r) + 1e-6 (|c_i - C|_1 + r_i - r) + 1e-12 (|c_i|^2 - |C|^2) inv_r, since inv_r >= q_i;
//     |c_i - C|_1 <= sqrt(3) d_i and |c_i|^2 - |C|^2 <= d_i (2 |C| + d_i), so the difference is at most (r_i - r) + (pad - 1e-14 (...)).
// Hence r >= d_i + r_i + pad makes "bound skipped" imply "member i skipped by its own predicate in exact arithmetic", whose margins
// (1e-6 relative) dwarf the rounding of either evaluation; the 1e-14 term covers the rounding of c_i - C itself when the centres are
// far from the origin, the factor that of the sums here.  A chunk with a member without a bounding radius (r = +inf) gets r = +inf,
// inv_r = 0 and a zero centre: every predicate answers "test it".  So does one whose r overflows.
// Only + - * / sqrt fabs and comparisons; writes every byte; called by rt_create on the host and by rt_set_scene on the device.
RT_PACK_FN void pack_chunk_bound(UsEntry &out, const UsEntry *members, uint32_t n, uint32_t chunk)
{
    RT_PACK_STRICT
    out.orig = chunk;
    out.pad = 0u;
    out.own_lo = INFINITY;
    out.own_hi = 0.0f;
    bool bounded = n > 0u;
    double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY, q = 0.0, rmax = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        const UsEntry &e = members[i];
        if (!(e.r < INFINITY)) {
            bounded = false;
            continue;
        }
        const double cx = -0.5 * e.kx, cy = -0.5 * e.ky, cz = -0.5 * e.kz;
        lx = cx < lx ? cx : lx; ly = cy < ly ? cy : ly; lz = cz < lz ? cz : lz;
        hx = cx > hx ? cx : hx; hy = cy > hy ? cy : hy; hz = cz > hz ? cz : hz;
        q = e.inv_r > q ? e.inv_r : q;
        rmax = e.r > rmax ? e.r : rmax;
    }
    double Cx = 0.0, Cy = 0.0, Cz = 0.0, r = INFINITY;
    if (bounded) {
        Cx = 0.5 * lx + 0.5 * hx; // (halves first: no overflow)
        Cy = 0.5 * ly + 0.5 * hy;
        Cz = 0.5 * lz + 0.5 * hz;
        double reach = 0.0, D = 0.0;
        for (uint32_t i = 0; i < n; i++) {
            const UsEntry &e = members[i];
            const double wx = -0.5 * e.kx - Cx, wy = -0.5 * e.ky - Cy, wz = -0.5 * e.kz - Cz;
            const double d = sqrt(wx * wx + wy * wy + wz * wz);
            D = d > D ? d : D;
            reach = d + e.r > reach ? d + e.r : reach;
        }
        const double C1 = fabs(Cx) + fabs(Cy) + fabs(Cz);
        const double pad = 2e-6 * D + 1e-12 * q * D * (2.0 * C1 + D) + 1e-14 * (C1 + D + rmax);
        r = (reach + pad) * (1.0 + 1e-12);
        if (!(r < INFINITY)) bounded = false; // (overflow, or a NaN: never culled)
    }
    if (!bounded) {
        Cx = Cy = Cz = 0.0;
        r = INFINITY;
        q = 0.0;
    }
    out.kx = -2.0 * Cx;
    out.ky = -2.0 * Cy;
    out.kz = -2.0 * Cz;
    out.r = r;
    out.inv_r = q;
    out.c = bounded ? ((Cx * Cx + Cy * Cy) + Cz * Cz) - r * r : 0.0;
}

// The key the unit-sphere table of a culling context is ordered by (RT_FLAG_STREAM_CULL; rt_scene_image.hpp, stream_cull_image, on the host and
// rt_reorder_scene.hip on the device): entries ascend by (key, orig).  lo / hi: the box of the centres (-k / 2) of the entries with a
// bounding radius.  Per axis q = (uint64) ((c - lo) / (hi - lo) * 2097151.0), clamped to 0 .. 2097151 (21 bits) and 0 where the span is
// not a positive finite number; bit 3 b + 2 of the key is bit b of q_x, 3 b + 1 that of q_y, 3 b that of q_z: 63 bits.  An entry
// without a bounding radius gets ~0 and so stands behind every bounded one.
// The sign of a zero in lo / hi does not reach the key: c - lo differs between lo = +0 and lo = -0 only where c is a zero too, and then
// it is a zero of either sign, whose quotient and product are zeros that the clamp (f > 0.0) sends to +0; hi - lo differs only where
// both are zeros, and a zero span of either sign fails span > 0.0.  So a box reduced in another order than the host's (the device's
// integer minimum / maximum puts -0 below +0, the host's sequential < / > keeps whichever came first) gives the same keys.
RT_PACK_FN uint64_t stream_cull_key(const UsEntry &e, const double *lo, const double *hi)
{
    RT_PACK_STRICT
    if (!(e.r < INFINITY)) return ~(uint64_t) 0;
    const double c[3] = {-0.5 * e.kx, -0.5 * e.ky, -0.5 * e.kz};
    uint64_t m = 0;
    for (int k = 0; k < 3; k++) {
        const double span = hi[k] - lo[k];
        double f = (span > 0.0 && finite64(span)) ? (c[k] - lo[k]) / span * 2097151.0 : 0.0;
        f = f > 0.0 ? (f < 2097151.0 ? f : 2097151.0) : 0.0;
        const uint64_t q = (uint64_t) f;
        for (int b = 0; b < 21; b++) m |= ((q >> b) & 1u) << (3 * b + (2 - k));
    }
    return m;
}

RT_PACK_FN void pack_gq(GqEntry &e, const DevObject &o, uint32_t orig)
{
    e.x2 = o.c[K_X2]; e.y2 = o.c[K_Y2]; e.z2 = o.c[K_Z2];
    e.xy = o.c[K_XY]; e.xz = o.c[K_XZ]; e.yz = o.c[K_YZ];
    e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
    e.orig = orig;
    e.pad[0] = e.pad[1] = e.pad[2] = 0u;
}

RT_PACK_FN void pack_lin(LinEntry &e, const DevObject &o, uint32_t orig)
{
    e.kx = o.c[K_X]; e.ky = o.c[K_Y]; e.kz = o.c[K_Z]; e.c = o.c[K_C];
    e.orig = orig;
    e.pad[0] = e.pad[1] = e.pad[2] = 0u;
}

RT_PACK_FN void pack_mat(MatEntry &m, const DevObject &o)
{
    m.albedo[0] = o.albedo[0];
    m.albedo[1] = o.albedo[1];
    m.albedo[2] = o.albedo[2];
    m.refl = o.refl;
}

RT_PACK_FN bool albedo_finite(const float *albedo) { return finite32(albedo[0]) && finite32(albedo[1]) && finite32(albedo[2]); }

// DevLight from LightSource (p[3], colour[3], kind).  albedos_finite: every albedo of the scene is finite.  Returns "this light's colour
// and every albedo are finite" (a factor max(0, n.l) = 0 makes its term exactly +0), which pack_lightk wants too.
RT_PACK_FN bool pack_light(DevLight &l, const double *p, const float *color, uint32_t spherical, bool albedos_finite)
{
    RT_PACK_STRICT
    for (int k = 0; k < 3; k++) {
        l.p[k] = p[k];
        l.color[k] = color[k];
    }
    l.spherical = spherical ? 1u : 0u;
    for (int k = 0; k < 3; k++) l.sdir[k] = (double) (float) l.p[k];
    l.dxx = l.sdir[0] * l.sdir[0];
    l.dyy = l.sdir[1] * l.sdir[1];
    l.dzz = l.sdir[2] * l.sdir[2];
    l.dxy = l.sdir[0] * l.sdir[1];
    l.dxz = l.sdir[0] * l.sdir[2];
    l.dyz = l.sdir[1] * l.sdir[2];
    l.u2 = (l.dxx + l.dyy) + l.dzz;
    l.inv_uu = l.u2 > 0.0 ? 1.0 / l.u2 : 0.0;
    l.len_u = 1.001 * sqrt(l.u2);
    const bool finite = finite32(l.color[0]) && finite32(l.color[1]) && finite32(l.color[2]) && albedos_finite;
    l.backface_exact = (!l.spherical && finite) ? 1u : 0u;
    l.pad_ = 0u;
    return finite;
}

// the same light as the lean path reads it
RT_PACK_FN void pack_lightk(LightK &k, const DevLight &l, bool term_finite)
{
    RT_PACK_STRICT
    for (int c = 0; c < 3; c++) { k.p[c] = l.p[c]; k.sdir[c] = l.sdir[c]; k.color[c] = l.color[c]; }
    k.u2 = l.u2; k.inv_uu = l.inv_uu; k.len_u = l.len_u;
    k.four_u2 = 4.0 * l.u2;
    k.s_yz = fabs(l.sdir[1]) + fabs(l.sdir[2]);
    k.s_xz = fabs(l.sdir[0]) + fabs(l.sdir[2]);
    k.s_xy = fabs(l.sdir[0]) + fabs(l.sdir[1]);
    k.flags = (l.spherical ? 1u : 0u) | (l.backface_exact ? 2u : 0u) | (fabs(l.u2) > 1e-7 ? 4u : 0u) | // EPS of include/surface_impl.h:16,138
              ((l.spherical && term_finite) ? 8u : 0u);
    k.pad[0] = k.pad[1] = 0u;
}

} // namespace rtp

#endif
