// bounce_cull_lab.cpp -- host lab behind RT_FLAG_STREAM_CULL_BOUNCE (test infrastructure: it links the oracle).
// rtm::ray_reaches (csrc/rt_ray_bound.hpp, compiled here as the kernel compiles it) asked about the BOUND of a chunk -- packed by the
// library's own rtp::pack_chunk_bound -- whose members are one sphere grazed by a single ray and companions placed by the caller.  The
// truth is the oracle's verdict for EVERY member under the reference's acceptance rule: orc_intersect_ray gives a root with
// t >= EPS && t < MAX_T.
// The grazing construction is cull_lab.cpp's (lab_graze_shadow: a tangent point along the ray, an angle around it, a relative clearance),
// with the ray given outright -- its own origin, its own double-precision direction of any length -- instead of derived from a light.
// stream_cull_lab.cpp (and through it cull_lab.cpp) is included as text for the packing helpers and the record layout.
// Built and driven by tests/tools/bounce_cull_lab.py.
#include "stream_cull_lab.cpp"

#include "rt_ray_bound.hpp"

// One case = BR_W doubles: o[3], d[3], radius r of the grazed sphere, relative clearance delta, position s of the tangent point along the
// ray in units of d, angle phi around the ray, factor f on the centre's distance from the ray's line (1: the sphere grazes the line at
// clearance delta; < 1 with s < 0: a sphere behind the origin), one spare.
// Per case out: rec[REC_SH] in cull_lab's shadow-record layout (the bound, ball = the origin with R = 0, sdir = d, inv_uu, len_u), verdict
// = ray_reaches about the bound, truth = the oracle accepts some member, g_truth = it accepts the grazed sphere, alone = ray_reaches about
// the grazed sphere's own entry, members_out as in stream_cull_lab.cpp.
constexpr int BR_W = 12;

extern "C" void lab_bounce(uint64_t n, const double *par, int m, const double *comp, double *rec, int32_t *verdict, int32_t *truth, int32_t *g_truth, int32_t *alone,
                           double *members_out)
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
        int any = 0, g = 0;
        for (size_t k = 0; k < us.size(); k++) {
            const double t = orc_intersect_ray(coefs[k].data(), o, d);
            if (t >= EPS && t < MAX_T) {
                any = 1;
                if (k == 0) g = 1;
            }
        }
        UsEntry b;
        memset(&b, 0xA5, sizeof(b));
        rtp::pack_chunk_bound(b, us.data(), (uint32_t) us.size(), 0u);
        const D3 oo{o[0], o[1], o[2]}, dd{d[0], d[1], d[2]};
        const rtm::RayBound rb = rtm::ray_bound(oo, dd);
        double *rr = rec + i * REC_SH;
        memset(rr, 0, sizeof(double) * REC_SH);
        rr[0] = b.kx; rr[1] = b.ky; rr[2] = b.kz; rr[3] = b.c; rr[4] = b.r; rr[5] = b.inv_r;
        rr[6] = rb.ball.cx; rr[7] = rb.ball.cy; rr[8] = rb.ball.cz; rr[9] = rb.ball.R;
        for (int k = 0; k < 3; k++) rr[16 + k] = rb.dir.sdir[k];
        rr[19] = rb.dir.inv_uu; rr[20] = rb.dir.len_u;
        rr[25] = rb.cull ? 1.0 : 0.0;
        verdict[i] = rtm::ray_reaches(b, oo, dd) ? 1 : 0;
        alone[i] = rtm::ray_reaches(us[0], oo, dd) ? 1 : 0;
        truth[i] = any;
        g_truth[i] = g;
        for (size_t k = 0; k < us.size(); k++) {
            double *mo = members_out + (i * (uint64_t) (m + 1) + k) * 5;
            mo[0] = -0.5 * us[k].kx; mo[1] = -0.5 * us[k].ky; mo[2] = -0.5 * us[k].kz; mo[3] = us[k].r; mo[4] = us[k].inv_r;
        }
    }
}

// ray_reaches about one given bound (kx ky kz r inv_r) for n rays (o[3], d[3]): the rays nothing is culled for
extern "C" void lab_bounce_verdicts(uint64_t n, const double *bound, const double *rays, int32_t *verdict)
{
    UsEntry b{};
    b.kx = bound[0]; b.ky = bound[1]; b.kz = bound[2]; b.r = bound[3]; b.inv_r = bound[4];
    for (uint64_t i = 0; i < n; i++) {
        const double *q = rays + 6 * i;
        verdict[i] = rtm::ray_reaches(b, D3{q[0], q[1], q[2]}, D3{q[3], q[4], q[5]}) ? 1 : 0;
    }
}

// ray_reaches about every record's own bound and ray (rec[REC_SH] as lab_bounce writes them).  The Python side builds this file a second
// time with -mfma -ffp-contract=fast -DRT_FAST=1 and calls ONLY this function of that build: the predicate as the FAST kernel build
// compiles it, about bounds packed and truths formed by the strict build.
extern "C" void lab_bounce_eval(uint64_t n, const double *rec, int32_t *verdict)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *r = rec + i * REC_SH;
        UsEntry b{};
        b.kx = r[0]; b.ky = r[1]; b.kz = r[2]; b.c = r[3]; b.r = r[4]; b.inv_r = r[5];
        verdict[i] = rtm::ray_reaches(b, D3{r[6], r[7], r[8]}, D3{r[16], r[17], r[18]}) ? 1 : 0;
    }
}
