// ray_cull_lab.cpp -- host lab behind RT_FLAG_STREAM_CULL_RAYS (test infrastructure: it links the oracle).
// The predicate is bounce_cull_lab.cpp's -- rtm::ray_reaches (csrc/rt_ray_bound.hpp) about a bound packed by rtp::pack_chunk_bound -- and so
// is the construction (lab_bounce, included as text); the Python side (ray_cull_lab.py) supplies the rays a CALLER can hand in.  What this
// file adds is the truth of an occlusion query: the kernel passes t_max to the sweep only and asks ray_reaches about the whole half-line,
// so a skipped bound must have no member with a root EPS < t < t_max (rq_take<true>'s rule) for ANY t_max.
// Built and driven by tests/tools/ray_cull_lab.py.
#include "bounce_cull_lab.cpp"

// lab_bounce's cases (par, comp) with one t_max factor per case.  t_max = factor x the grazed sphere's root where the oracle gives it one
// (t >= EPS), else factor x the tangent point's parameter |s|; NaN and +inf factors are passed on as they are.  Out: t_max as used,
// verdict = ray_reaches about the bound (it never sees t_max), truth = the oracle gives some member a root with t > EPS && t < t_max.
extern "C" void lab_ray_occluded(uint64_t n, const double *par, int m, const double *comp, const double *factor, double *t_max_out, int32_t *verdict, int32_t *truth)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * BR_W;
        const double o[3] = {q[0], q[1], q[2]}, d[3] = {q[3], q[4], q[5]};
        const double r = q[6], delta = q[7], s = q[8], phi = q[9], f = q[10];
        const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double a[3] = {fabs(d[0]) < 0.5 * dn ? 1.0 : 0.0, fabs(d[0]) < 0.5 * dn ? 0.0 : 1.0, 0.0};
        double u[3] = {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]};
        const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        for (int k = 0; k < 3; k++) u[k] /= un;
        const double v[3] = {(d[1] * u[2] - d[2] * u[1]) / dn, (d[2] * u[0] - d[0] * u[2]) / dn, (d[0] * u[1] - d[1] * u[0]) / dn};
        double centre[3];
        for (int k = 0; k < 3; k++) centre[k] = o[k] + s * d[k] + f * r * (1.0 + delta) * (cos(phi) * u[k] + sin(phi) * v[k]);
        std::vector<std::vector<double>> coefs;
        const std::vector<UsEntry> us = pack_members(centre, r, m, comp + i * 4 * (uint64_t) m, coefs);
        const double t0 = orc_intersect_ray(coefs[0].data(), o, d);
        const double t_max = factor[i] * (t0 >= EPS && t0 < MAX_T ? t0 : fabs(s));
        int any = 0;
        for (size_t k = 0; k < us.size(); k++) {
            const double t = orc_intersect_ray(coefs[k].data(), o, d);
            if (t > EPS && t < t_max) any = 1;
        }
        UsEntry b;
        memset(&b, 0xA5, sizeof(b));
        rtp::pack_chunk_bound(b, us.data(), (uint32_t) us.size(), 0u);
        t_max_out[i] = t_max;
        verdict[i] = rtm::ray_reaches(b, D3{o[0], o[1], o[2]}, D3{d[0], d[1], d[2]}) ? 1 : 0;
        truth[i] = any;
    }
}
