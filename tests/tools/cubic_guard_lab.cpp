// cubic_guard_lab.cpp -- CPU experiment behind rt_math.hpp's cubic_guarded (test infrastructure: it links the oracle).
// For every primary ray of a scene and every shadow ray of its hits it compares, per degree-3 object,
//   the oracle's intersect_ray (dense expansion + the reference's solver, oracle/rt_oracle.c)      -- the truth
//   with cubic_guarded on the Taylor coefficients (the kernel's own header, compiled for the host) -- the candidate,
// and counts: tests, tests the guard passes on to the dense path, and among the ones it answers itself the decisions that differ
// (t >= EPS for primary rays, EPS < t < max_t for shadow rays) and the accepted roots that differ by more than 1e-7 relative.
// Built and driven by tests/tools/cubic_guard_lab.py.  lab_enumerate / lab_oracle hand the same tests to the device lab (tests/tools/cubic_device_lab.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>

#define RT_CUB_LAB 1
#include "rt_math.hpp"
#include "../../oracle/rt_oracle.h"
#include "cubic_lab_rays.h"

using namespace rtm;

struct LabStats {
    uint64_t tests[2], fallback[2], decision_diff[2], value_diff[2]; // [0] primary, [1] shadow
    double worst_rel[2];
    uint64_t fb_reason[8];
    uint64_t blocks[2], blocks_refusing[2]; // 8 x 8 pixel blocks (x light, for shadow rays) with a test / with a refused test
};

static bool is_cubic(const double *c)
{
    for (int k = 0; k < 10; k++)
        if (c[k] != 0.0) return true;
    return false;
}

static bool one(const double *c, const CubicAbs &ab, const CubicAt &ca, const CubicMag &mo, const double o[3], const double d[3], double max_t, int kind, bool strict_gt,
                LabStats *st, int verbose)
{
    const double t_ref = orc_intersect_ray(c, o, d);
    double t3, t2, t1, t0;
    cubic_coefs(c, ca, D3{d[0], d[1], d[2]}, t3, t2, t1, t0);
    const double dmax = fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2]));
    const CubicMag mg = cubic_mag_dir(mo, dmax);
    double t = 0.0;
    st->tests[kind]++;
    if (!cubic_guarded(t3, t2, t1, t0, mg, max_t, strict_gt, t)) {
        st->fallback[kind]++;
        st->fb_reason[g_cub_why & 7]++;
        return true;
    }
    const bool acc_ref = strict_gt ? (t_ref > EPS && t_ref < max_t) : (t_ref >= EPS && t_ref < max_t);
    const bool acc = strict_gt ? (t > EPS && t < max_t) : (t >= EPS && t < max_t);
    if (acc != acc_ref) {
        st->decision_diff[kind]++;
        if (verbose) {
            double tc[4];
            int br;
            orc_intersect_ray_ex(c, o, d, tc, &br);
            fprintf(stderr, "decision differs (%s): ref %.17g (branch %d) ours %.17g  dense t3..t0 %.17g %.17g %.17g %.17g  taylor %.17g %.17g %.17g %.17g\n", kind ? "shadow" : "primary", t_ref,
                    br, t, tc[3], tc[2], tc[1], tc[0], t3, t2, t1, t0);
        }
        return false;
    }
    if (acc && !strict_gt) { // (shadow rays are asked for the decision only)
        const double rel = fabs(t - t_ref) / fabs(t_ref);
        if (rel > st->worst_rel[kind]) st->worst_rel[kind] = rel;
        if (rel > 1e-7) {
            st->value_diff[kind]++;
            if (verbose) fprintf(stderr, "value differs (%s): ref %.17g ours %.17g rel %.3g\n", kind ? "shadow" : "primary", t_ref, t, rel);
        }
    }
    (void) ab;
    return false;
}

// Every degree-3 test of a frame, as the oracle's frame loop makes it (src/update-cpu.cpp:45-119): the primary ray of every pixel against
// every degree-3 object, the shadow ray of its nearest hit towards every light (direction and max_t from the surface point, the ray
// starting at the biased point, :62-66), and -- with `bounce` -- the first reflected ray of a mirror hit (:96-117).  Nearest hits are the
// oracle's (whatever libm it runs under).  emit(const LabRay &, const LabWhere &) is called for each test.
template <class Emit>
static void enumerate_rays(const orc_scene *scene, const double cam[16], bool bounce, Emit &&emit)
{
    const double org[3] = {cam[12], cam[13], cam[14]};
    for (uint32_t y = 0; y < scene->px_height; y++) {
        for (uint32_t x = 0; x < scene->px_width; x++) {
            LabRay r;
            double d[3];
            orc_primary_dir(scene, cam, (int) x, (int) y, d);
            int best = -1;
            double best_t = INFINITY;
            for (uint32_t k = 0; k < scene->n_objects; k++) {
                const double *c = scene->objects[k].c;
                const double t = orc_intersect_ray(c, org, d);
                if (t >= EPS && t < 1e6 && t < best_t) {
                    best_t = t;
                    best = (int) k;
                }
                if (is_cubic(c)) {
                    const CubicAt ca = cubic_at(c, D3{org[0], org[1], org[2]});
                    const double rec[10] = {ca.f, ca.gx, ca.gy, ca.gz, ca.hxx, ca.hyy, ca.hzz, ca.hxy, ca.hxz, ca.hyz};
                    memcpy(r.o, org, sizeof(r.o));
                    memcpy(r.d, d, sizeof(r.d));
                    memcpy(r.rec, rec, sizeof(r.rec));
                    r.max_t = 1e6;
                    r.obj = (int32_t) k;
                    r.flags = LAB_HAS_REC;
                    emit(r, LabWhere{0, (int32_t) x, (int32_t) y, -1});
                }
            }
            if (best < 0) continue;
            double p[3], n[3], so[3];
            for (int i = 0; i < 3; i++) p[i] = org[i] + best_t * d[i];
            orc_normal_vector(scene->objects[best].c, p, n);
            for (int i = 0; i < 3; i++) so[i] = p[i] + SHADOW_BIAS * n[i];
            memset(r.rec, 0, sizeof(r.rec));
            memcpy(r.o, so, sizeof(r.o));
            for (uint32_t l = 0; l < scene->n_lights; l++) {
                float fd[3];
                double max_t;
                orc_shadow_ray(&scene->lights[l], p, fd, &max_t);
                for (int i = 0; i < 3; i++) r.d[i] = (double) fd[i];
                r.max_t = max_t;
                r.flags = LAB_DECIDE;
                for (uint32_t k = 0; k < scene->n_objects; k++) {
                    if (!is_cubic(scene->objects[k].c)) continue;
                    r.obj = (int32_t) k;
                    emit(r, LabWhere{1, (int32_t) x, (int32_t) y, (int32_t) l});
                }
            }
            if (bounce && scene->objects[best].reflection_ratio > EPS && scene->max_reflections > 0) {
                orc_reflect_ray(d, n, r.d);
                r.max_t = 1e6;
                r.flags = 0;
                for (uint32_t k = 0; k < scene->n_objects; k++) {
                    if (!is_cubic(scene->objects[k].c)) continue;
                    r.obj = (int32_t) k;
                    emit(r, LabWhere{2, (int32_t) x, (int32_t) y, -1});
                }
            }
        }
    }
}

extern "C" void lab_run(const orc_scene *scene, const double cam[16], LabStats *st, int verbose)
{
    const uint32_t bw = (scene->px_width + 7) / 8, bh = (scene->px_height + 7) / 8, nl = scene->n_lights + 1;
    unsigned char *blk = (unsigned char *) calloc((size_t) bw * bh * nl, 1); // bit 0: tested, bit 1: refused; slot 0 primary, 1 + l shadow of light l
    enumerate_rays(scene, cam, false, [&](const LabRay &r, const LabWhere &w) {
        const double *c = scene->objects[r.obj].c;
        const CubicAbs ab = cubic_abs(c);
        const D3 o{r.o[0], r.o[1], r.o[2]};
        const CubicAt ca = (r.flags & LAB_HAS_REC) ? CubicAt{r.rec[0], r.rec[1], r.rec[2], r.rec[3], r.rec[4], r.rec[5], r.rec[6], r.rec[7], r.rec[8], r.rec[9]} : cubic_at(c, o);
        const CubicMag mo = cubic_mag_origin(ab, o);
        const int kind = w.kind == 1 ? 1 : 0;
        unsigned char *b = blk + ((size_t) (w.y / 8) * bw + w.x / 8) * nl + (w.kind == 1 ? 1 + w.light : 0);
        *b |= 1 | (one(c, ab, ca, mo, r.o, r.d, r.max_t, kind, kind == 1, st, verbose) ? 2 : 0);
    });
    for (size_t i = 0; i < (size_t) bw * bh; i++)
        for (uint32_t l = 0; l < nl; l++) {
            const unsigned char v = blk[i * nl + l];
            if (v & 1) st->blocks[l ? 1 : 0]++;
            if (v & 2) st->blocks_refusing[l ? 1 : 0]++;
        }
    free(blk);
}

// The records of enumerate_rays (with the first bounce of mirror hits): returns how many there are, writes the first `cap`.
extern "C" uint64_t lab_enumerate(const orc_scene *scene, const double cam[16], LabRay *rays, LabWhere *where, uint64_t cap)
{
    uint64_t n = 0;
    enumerate_rays(scene, cam, true, [&](const LabRay &r, const LabWhere &w) {
        if (n < cap) {
            rays[n] = r;
            where[n] = w;
        }
        n++;
    });
    return n;
}

// The oracle's intersect_ray on each record (orc_intersect_ray_ex: root, dense t3..t0 and branch), under whatever libm it runs.
extern "C" void lab_oracle(const orc_scene *scene, const LabRay *rays, uint64_t n, double *t, double *tc, int32_t *branch)
{
    for (uint64_t i = 0; i < n; i++) {
        int br = 0;
        double c4[4];
        t[i] = orc_intersect_ray_ex(scene->objects[rays[i].obj].c, rays[i].o, rays[i].d, c4, &br);
        for (int k = 0; k < 4; k++) tc[4 * i + k] = c4[3 - k]; // t3 .. t0
        branch[i] = br;
    }
}

// cubic_guarded itself, for unit tests: returns 1 (answered; *t = the root the callers compare) or 0 (refused).  m[4] = the uncertainties m3 .. m0.
extern "C" int lab_guard(double t3, double t2, double t1, double t0, const double m[4], double max_t, int decide, double *t)
{
    double r = 0.0;
    const bool ok = cubic_guarded(t3, t2, t1, t0, CubicMag{m[0], m[1], m[2], m[3]}, max_t, decide != 0, r);
    *t = r;
    return ok ? 1 : 0;
}
// the reference's solver on the same coefficients (rt_math.hpp: solve_cubic / solve_quadlin, as intersect_cubic chains them)
extern "C" double lab_reference(double t3, double t2, double t1, double t0)
{
    return fabs(t3) > EPS ? solve_cubic(t3, t2, t1, t0) : solve_quadlin(t2, t1, t0);
}
