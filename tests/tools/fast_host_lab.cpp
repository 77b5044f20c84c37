// fast_host_lab.cpp -- the kernels' own per-ray arithmetic (csrc/rt_math.hpp, rt_wavefront_math.hpp) compiled for the HOST with
// -mfma -ffp-contract=fast -DRT_FAST=1, the way tests/tools/cubic_guard_lab.cpp compiles it strict: what the contracted build computes
// for degree <= 2, without a GPU.  Test infrastructure of tests/test_fast_ref_host.py (tests/tools/fast_ref.py judges the results).
//   form 0: the dense form -- make_mono, quadric_poly on the 20 coefficients, solve_quadlin, every object in index order;
//   form 1: the class tables' forms as the query kernels walk them (csrc/rt_rayquery.hpp: rq_tables) -- us_t1 / us_t0 on the shared
//           u2, gq_t2 / gq_t1 / gq_t0, lin_t1 / lin_t0, the root only where us_needs_solve / needs_solve ask for it.
// The hit point is o + t d and the normal normal_vector there, stored as float, as csrc/rt_rays.hip does.
#include <cmath>
#include <cstdint>

#include "rt_wavefront_math.hpp"
#include "rt_scene_pack.hpp"

using namespace rtm;

static double root_of(const double *c, const Mono &m, int form)
{
    const uint32_t cls = rtp::classify(c);
    if (cls & RT_CLS_CUBIC) return NAN; // out of scope: nothing accepts a NaN
    if (form == 0) {
        double t2, t1, t0;
        quadric_poly(c, cls, m, t2, t1, t0);
        return solve_quadlin(t2, t1, t0);
    }
    if (cls & RT_CLS_UNITSQ) {
        UsEntry e{};
        e.kx = c[K_X]; e.ky = c[K_Y]; e.kz = c[K_Z]; e.c = c[K_C];
        if (!us_needs_solve(fabs(m.u2) > EPS, 4.0 * m.u2, us_t1(e, m), us_t0(e, m))) return -1.0;
        return solve_quadlin(m.u2, us_t1(e, m), us_t0(e, m));
    }
    if (cls & (RT_CLS_SQUARE | RT_CLS_CROSS)) {
        GqEntry e{};
        e.x2 = c[K_X2]; e.y2 = c[K_Y2]; e.z2 = c[K_Z2]; e.xy = c[K_XY]; e.xz = c[K_XZ]; e.yz = c[K_YZ];
        e.kx = c[K_X]; e.ky = c[K_Y]; e.kz = c[K_Z]; e.c = c[K_C];
        if (!needs_solve(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m))) return -1.0;
        return solve_quadlin(gq_t2(e, m), gq_t1(e, m), gq_t0(e, m));
    }
    LinEntry e{};
    e.kx = c[K_X]; e.ky = c[K_Y]; e.kz = c[K_Z]; e.c = c[K_C];
    const double t1 = lin_t1(e, m), t0 = lin_t0(e, m);
    return (fabs(t1) > EPS) ? -t0 / t1 : -1.0;
}

static void mono_of(Mono &m, const double *ray, int form)
{
    const D3 o{ray[0], ray[1], ray[2]}, d{ray[3], ray[4], ray[5]};
    if (form == 0) {
        make_mono(m, o, d);
    } else {
        mono_set_o<true>(m, o);
        mono_set_d<true>(m, d);
        mono_set_od<true>(m);
    }
}

extern "C" {

// rays: n x (o, d); coefs: m x 20.  Per ray: object or -1, t (+inf for a miss), point, normal (0 for a miss).
void lab_closest(const double *coefs, int m_obj, const double *rays, int n, int form, int32_t *object, double *t, double *point, float *normal)
{
    for (int i = 0; i < n; i++) {
        Mono m;
        mono_of(m, rays + 6 * i, form);
        double best_t = INFINITY;
        int best = -1;
        for (int k = 0; k < m_obj; k++) accept(root_of(coefs + 20 * k, m, form), k, best_t, best);
        object[i] = best;
        t[i] = best_t;
        for (int a = 0; a < 3; a++) point[3 * i + a] = 0.0, normal[3 * i + a] = 0.0f;
        if (best >= 0) {
            const D3 p{m.o.x + best_t * m.d.x, m.o.y + best_t * m.d.y, m.o.z + best_t * m.d.z};
            const D3 nv = normal_vector(coefs + 20 * best, p);
            point[3 * i] = p.x; point[3 * i + 1] = p.y; point[3 * i + 2] = p.z;
            normal[3 * i] = (float) nv.x; normal[3 * i + 1] = (float) nv.y; normal[3 * i + 2] = (float) nv.z;
        }
    }
}

// t_max: one value per ray.  blocked: 1 where some object gives EPS < t < t_max.
void lab_occluded(const double *coefs, int m_obj, const double *rays, const double *t_max, int n, int form, int32_t *blocked)
{
    for (int i = 0; i < n; i++) {
        Mono m;
        mono_of(m, rays + 6 * i, form);
        int hit = 0;
        for (int k = 0; k < m_obj && !hit; k++) {
            const double t = root_of(coefs + 20 * k, m, form);
            if (t > EPS && t < t_max[i]) hit = 1;
        }
        blocked[i] = hit;
    }
}

// the bare root of one pair, to see that this build is in fact contracted (it differs from the strict oracle somewhere)
double lab_root(const double *coef, const double *ray, int form)
{
    Mono m;
    mono_of(m, ray, form);
    return root_of(coef, m, form);
}
}
