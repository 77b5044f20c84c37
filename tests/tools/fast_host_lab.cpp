// fast_host_lab.cpp -- the kernels' own per-ray arithmetic (csrc/rt_math.hpp, rt_wavefront_math.hpp) compiled for the HOST with
// -mfma -ffp-contract=fast -DRT_FAST=1, the way tests/tools/cubic_guard_lab.cpp compiles it strict: what the contracted build computes,
// without a GPU.  Test infrastructure of tests/test_fast_ref_host.py (tests/tools/fast_ref.py judges the results); built a second time
// with -ffp-contract=off to show that the first build is in fact contracted.
//   form 0: the dense form -- make_mono, quadric_poly on the 20 coefficients, solve_quadlin, every object in index order;
//   form 1: the class tables' forms as the query kernels walk them (csrc/rt_rayquery.hpp: rq_tables) -- us_t1 / us_t0 on the shared
//           u2, gq_t2 / gq_t1 / gq_t0, lin_t1 / lin_t0, the root only where us_needs_solve / needs_solve ask for it.
// Degree 3 -- form 0: the dense form, cubic_poly + solve_cubic (intersect_cubic_inl); form 1: the guarded form as both kernels use it
// (intersect_cubic_taylor: cubic_at, cubic_coefs, cubic_mag_*, cubic_guarded, the dense form where the guard refuses), which reports
// the refusals.
// The hit point is o + t d and the normal normal_vector there, stored as float, as csrc/rt_rays.hip does.
#include <cmath>
#include <cstdint>

#include "rt_wavefront_math.hpp"
#include "rt_scene_pack.hpp"

using namespace rtm;

static double root_of(const double *c, const Mono &m, int form, double max_t, bool decide, bool &refused)
{
    const uint32_t cls = rtp::classify(c);
    refused = false;
    if (cls & RT_CLS_CUBIC) {
        if (form == 0) return intersect_cubic_inl(c, m.o.x, m.o.y, m.o.z, m.d.x, m.d.y, m.d.z);
        return intersect_cubic_taylor<true>(c, cubic_at(c, m.o), cubic_mag_origin(cubic_abs(c), m.o), m.o, m.d, max_t, decide, refused);
    }
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

// rays: n x (o, d); coefs: m x 20.  Per ray: object or -1, t (+inf for a miss), point, normal (0 for a miss), guarded (1: the winner is
// of degree 3 and cubic_guarded answered for it), branch (the solver branch of a degree-3 winner's dense form -- 0 Cardano, 1
// trigonometric, 2 quadratic, 3 linear / constant -- else -1).  Returns the number of tests the guard refused.
int64_t lab_closest(const double *coefs, int m_obj, const double *rays, int n, int form, int32_t *object, double *t, double *point, float *normal, int32_t *guarded,
                    int32_t *branch)
{
    int64_t n_refused = 0;
    for (int i = 0; i < n; i++) {
        Mono m;
        mono_of(m, rays + 6 * i, form);
        double best_t = INFINITY;
        int best = -1;
        bool best_refused = false;
        for (int k = 0; k < m_obj; k++) {
            bool refused;
            const int before = best;
            accept(root_of(coefs + 20 * k, m, form, MAX_T, false, refused), k, best_t, best);
            n_refused += refused;
            if (best != before) best_refused = refused;
        }
        object[i] = best;
        t[i] = best_t;
        guarded[i] = 0;
        branch[i] = -1;
        if (best >= 0 && (rtp::classify(coefs + 20 * best) & RT_CLS_CUBIC)) {
            int br;
            intersect_cubic_branch(coefs + 20 * best, m.o.x, m.o.y, m.o.z, m.d.x, m.d.y, m.d.z, br);
            branch[i] = br;
            guarded[i] = (form == 1 && !best_refused) ? 1 : 0;
        }
        for (int a = 0; a < 3; a++) point[3 * i + a] = 0.0, normal[3 * i + a] = 0.0f;
        if (best >= 0) {
            const D3 p{m.o.x + best_t * m.d.x, m.o.y + best_t * m.d.y, m.o.z + best_t * m.d.z};
            const D3 nv = normal_vector(coefs + 20 * best, p);
            point[3 * i] = p.x; point[3 * i + 1] = p.y; point[3 * i + 2] = p.z;
            normal[3 * i] = (float) nv.x; normal[3 * i + 1] = (float) nv.y; normal[3 * i + 2] = (float) nv.z;
        }
    }
    return n_refused;
}

// Every ray against every object alone, as a nearest-hit search asks (max_t = MAX_T, the root itself): t and refused, n x m each.
void lab_pairs(const double *coefs, int m_obj, const double *rays, int n, int form, double *t, int32_t *refused_out)
{
    for (int i = 0; i < n; i++) {
        Mono m;
        mono_of(m, rays + 6 * i, form);
        for (int k = 0; k < m_obj; k++) {
            bool refused;
            t[(size_t) i * m_obj + k] = root_of(coefs + 20 * k, m, form, MAX_T, false, refused);
            refused_out[(size_t) i * m_obj + k] = refused;
        }
    }
}

// t_max: one value per ray.  blocked: 1 where some object gives EPS < t < t_max (degree 3, form 1: the guard is asked for the decision
// only, as the kernels' shadow loops ask it).  Returns the number of tests the guard refused.
int64_t lab_occluded(const double *coefs, int m_obj, const double *rays, const double *t_max, int n, int form, int32_t *blocked)
{
    int64_t n_refused = 0;
    for (int i = 0; i < n; i++) {
        Mono m;
        mono_of(m, rays + 6 * i, form);
        int hit = 0;
        for (int k = 0; k < m_obj && !hit; k++) {
            bool refused;
            const double t = root_of(coefs + 20 * k, m, form, t_max[i], true, refused);
            n_refused += refused;
            if (t > EPS && t < t_max[i]) hit = 1;
        }
        blocked[i] = hit;
    }
    return n_refused;
}

// the bare root of one pair, to see that this build is in fact contracted (it differs from the strict oracle somewhere)
double lab_root(const double *coef, const double *ray, int form)
{
    Mono m;
    mono_of(m, ray, form);
    bool refused;
    return root_of(coef, m, form, MAX_T, false, refused);
}
}
