// group_cull_lab.cpp -- host lab behind RT_FLAG_STREAM_CULL_GROUPS (test infrastructure: it links the oracle).
//   * the group bounds of a chunk-bound table by the library's own host function (csrc/rt_scene_image.hpp: stream_group_image over
//     rtp::pack_chunk_bound);
//   * the predicate lab: sphere_in_cone, sphere_relevant<false / true> and rtm::ray_reaches asked about the bound of a GROUP of two chunks
//     -- chunk A holds a sphere of cull_lab's grazing generator and companions, chunk B companions further out --, about both chunk bounds
//     and about every member's own entry, with the oracle's verdict for every member beside them.  A group verdict of "skip" may stand
//     beside no "test it" of a chunk bound or a member, and beside no member the oracle accepts.
// The generators, record layouts and packing helpers are the earlier labs' (included as text: their helpers have internal linkage).
// Built and driven by tests/tools/group_cull_lab.py.
#include "bounce_cull_lab.cpp"

// groups: ceil(n_chunks / 64) records, every byte preset to `fill` before the pack function writes it
extern "C" void lab_group_image(const unsigned char *bounds, uint32_t n_chunks, uint32_t fill, unsigned char *groups)
{
    std::vector<UsEntry> b(n_chunks);
    if (n_chunks) memcpy(b.data(), bounds, sizeof(UsEntry) * n_chunks);
    const std::vector<UsEntry> g = rtp::stream_group_image(b, (unsigned char) fill);
    if (!g.empty()) memcpy(groups, g.data(), sizeof(UsEntry) * g.size());
}

namespace {

constexpr int GL_OUT = 8; // per case: group verdict, chunk A's, chunk B's, "some member's own verdict is test-it", oracle accepts a member,
                          // not enclosed, inv_r short, chunk bounds kept among the skipped group's (always 0 or the case is unsound)

// chunk B: m spheres (centre, radius), none of them the grazing one; orig continues behind chunk A's
std::vector<UsEntry> pack_far(int first, int m, const double *comp, std::vector<std::vector<double>> &coefs)
{
    std::vector<UsEntry> us;
    for (int k = 0; k < m; k++) {
        std::vector<double> coef(ORC_NCOEF);
        orc_surface_sphere(comp + 4 * k, comp[4 * k + 3], coef.data());
        const float albedo[3] = {1.0f, 1.0f, 1.0f};
        DevObject o;
        rtp::pack_object(o, coef.data(), albedo, 0.0f);
        UsEntry e;
        rtp::pack_us(e, o, (uint32_t) (first + k));
        us.push_back(e);
        coefs.push_back(coef);
    }
    return us;
}

struct Level {
    UsEntry chunk[2], group;
};

Level pack_levels(const std::vector<UsEntry> &a, const std::vector<UsEntry> &b)
{
    Level l;
    memset(&l, 0xA5, sizeof(l));
    rtp::pack_chunk_bound(l.chunk[0], a.data(), (uint32_t) a.size(), 0u);
    rtp::pack_chunk_bound(l.chunk[1], b.data(), (uint32_t) b.size(), 1u);
    rtp::pack_chunk_bound(l.group, l.chunk, 2u, 0u);
    return l;
}

// the enclosure and inv_r claims in double (the 50-digit ones are made on the scenes' tables): out[5], out[6]
void enclosure(const Level &l, const std::vector<UsEntry> &a, const std::vector<UsEntry> &b, int32_t *out)
{
    out[5] = out[6] = 0;
    if (!(l.group.r < INFINITY)) return;
    const double C[3] = {-0.5 * l.group.kx, -0.5 * l.group.ky, -0.5 * l.group.kz};
    auto one = [&](const UsEntry &e) {
        const double w[3] = {-0.5 * e.kx - C[0], -0.5 * e.ky - C[1], -0.5 * e.kz - C[2]};
        if (sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + e.r > l.group.r) out[5] = 1;
        if (e.inv_r > l.group.inv_r) out[6] = 1;
    };
    one(l.chunk[0]);
    one(l.chunk[1]);
    for (const UsEntry &e : a) one(e);
    for (const UsEntry &e : b) one(e);
}

} // namespace

// Primary rays.  par: cull_lab's GP_W doubles per case (mode 0); comp_a / comp_b: per case m companions of four doubles (centre, radius)
// for chunk A (behind the grazing sphere) and chunk B.  out: GL_OUT words per case.
extern "C" void lab_group_primary(uint64_t n, const double *par, int m, const double *comp_a, const double *comp_b, int32_t *out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GP_W;
        double one_rec[REC_CONE], one_pyr[REC_PYR], centre[3];
        int32_t t_cone = 0, t_pyr = 0;
        LabOut lo;
        memset(&lo, 0, sizeof(lo));
        lo.cone = Out{one_rec, &t_cone, 1, 0};
        lo.pyr = Out{one_pyr, &t_pyr, 1, 0};
        lab_graze_primary(1, q, &lo, centre);
        orc_scene sc;
        memset(&sc, 0, sizeof(sc));
        sc.px_width = (uint32_t) q[0];
        sc.px_height = (uint32_t) q[1];
        sc.vertical_fov = q[2];
        FrameArgs fa;
        make_frame(fa, &sc, q + 3);
        double d[64][3];
        block_dirs(&sc, q + 3, (int) q[19], (int) q[20], d);
        std::vector<std::vector<double>> coefs;
        const std::vector<UsEntry> a = pack_members(centre, q[23], m, comp_a + i * 4 * (uint64_t) m, coefs);
        const std::vector<UsEntry> b = pack_far(m + 1, m, comp_b + i * 4 * (uint64_t) m, coefs);
        const Level l = pack_levels(a, b);
        int32_t *o = out + i * GL_OUT;
        auto ask = [&](const UsEntry &e) {
            double r[REC_CONE];
            memcpy(r, one_rec, sizeof(one_rec)); // org, axis, cos_t of the block
            r[0] = e.kx; r[1] = e.ky; r[2] = e.kz; r[3] = e.r; r[4] = e.inv_r;
            return eval_cone(r);
        };
        o[0] = ask(l.group); o[1] = ask(l.chunk[0]); o[2] = ask(l.chunk[1]);
        o[3] = o[4] = 0;
        for (const UsEntry &e : a) o[3] |= ask(e) ? 1 : 0;
        for (const UsEntry &e : b) o[3] |= ask(e) ? 1 : 0;
        for (size_t k = 0; k < coefs.size(); k++)
            for (int ln = 0; ln < 64; ln++) {
                const double t = orc_intersect_ray(coefs[k].data(), fa.origin, d[ln]);
                if (t >= EPS && t < MAX_T) o[4] = 1;
            }
        enclosure(l, a, b, o);
        o[7] = o[0] ? 0 : (o[1] != 0) + (o[2] != 0);
    }
}

// Shadow rays.  par: cull_lab's GS_W doubles per case; a case the generator drops (a directional light with |d|^2 <= EPS) gets out[0] = -1.
extern "C" void lab_group_shadow(uint64_t n, const double *par, int m, const double *comp_a, const double *comp_b, int32_t *out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GS_W;
        double one_rec[REC_SH], centre[3];
        int32_t t_sh = 0;
        LabOut lo;
        memset(&lo, 0, sizeof(lo));
        lo.sh = Out{one_rec, &t_sh, 1, 0};
        lab_graze_shadow(1, q, &lo, centre);
        int32_t *o = out + i * GL_OUT;
        memset(o, 0, sizeof(int32_t) * GL_OUT);
        o[0] = -1;
        if (lo.sh.n != 1) continue;
        orc_light light;
        memset(&light, 0, sizeof(light));
        light.is_spherical = q[0] != 0.0 ? 1 : 0;
        for (int k = 0; k < 3; k++) { light.p[k] = q[1 + k]; light.color[k] = 1.0f; }
        const int nh = (int) q[9];
        double pts[64 * 3], sos[64 * 3];
        for (int h = 0; h < nh; h++) {
            const double *hp = q + 10 + 6 * h;
            const double nn = sqrt(hp[3] * hp[3] + hp[4] * hp[4] + hp[5] * hp[5]);
            for (int k = 0; k < 3; k++) {
                pts[3 * h + k] = hp[k];
                sos[3 * h + k] = hp[k] + SHADOW_BIAS * (hp[3 + k] / nn);
            }
        }
        std::vector<std::vector<double>> coefs;
        const std::vector<UsEntry> a = pack_members(centre, q[4], m, comp_a + i * 4 * (uint64_t) m, coefs);
        const std::vector<UsEntry> b = pack_far(m + 1, m, comp_b + i * 4 * (uint64_t) m, coefs);
        const Level l = pack_levels(a, b);
        auto ask = [&](const UsEntry &e) {
            double r[REC_SH], crec[6];
            memcpy(r, one_rec, sizeof(one_rec)); // ball, box, light
            r[0] = e.kx; r[1] = e.ky; r[2] = e.kz; r[3] = e.c; r[4] = e.r; r[5] = e.inv_r;
            return eval_sh(r, crec) & 1;
        };
        o[0] = ask(l.group); o[1] = ask(l.chunk[0]); o[2] = ask(l.chunk[1]);
        for (const UsEntry &e : a) o[3] |= ask(e) ? 1 : 0;
        for (const UsEntry &e : b) o[3] |= ask(e) ? 1 : 0;
        for (size_t k = 0; k < coefs.size(); k++)
            for (int h = 0; h < nh; h++)
                if (shadow_blocks(coefs[k].data(), &light, pts + 3 * h, sos + 3 * h)) o[4] = 1;
        enclosure(l, a, b, o);
        o[7] = o[0] ? 0 : (o[1] != 0) + (o[2] != 0);
    }
}

// One ray per case.  par: bounce_cull_lab's BR_W doubles per case (the grazing construction is lab_bounce's).
extern "C" void lab_group_ray(uint64_t n, const double *par, int m, const double *comp_a, const double *comp_b, int32_t *out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * BR_W;
        const double o3[3] = {q[0], q[1], q[2]}, d[3] = {q[3], q[4], q[5]};
        const double r = q[6], delta = q[7], s = q[8], phi = q[9], f = q[10];
        const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double ax[3] = {fabs(d[0]) < 0.5 * dn ? 1.0 : 0.0, fabs(d[0]) < 0.5 * dn ? 0.0 : 1.0, 0.0};
        double u[3] = {d[1] * ax[2] - d[2] * ax[1], d[2] * ax[0] - d[0] * ax[2], d[0] * ax[1] - d[1] * ax[0]};
        const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        for (int k = 0; k < 3; k++) u[k] /= un;
        const double v[3] = {(d[1] * u[2] - d[2] * u[1]) / dn, (d[2] * u[0] - d[0] * u[2]) / dn, (d[0] * u[1] - d[1] * u[0]) / dn};
        double centre[3];
        for (int k = 0; k < 3; k++) centre[k] = o3[k] + s * d[k] + f * r * (1.0 + delta) * (cos(phi) * u[k] + sin(phi) * v[k]);
        std::vector<std::vector<double>> coefs;
        const std::vector<UsEntry> a = pack_members(centre, r, m, comp_a + i * 4 * (uint64_t) m, coefs);
        const std::vector<UsEntry> b = pack_far(m + 1, m, comp_b + i * 4 * (uint64_t) m, coefs);
        const Level l = pack_levels(a, b);
        const D3 oo{o3[0], o3[1], o3[2]}, dd{d[0], d[1], d[2]};
        auto ask = [&](const UsEntry &e) { return rtm::ray_reaches(e, oo, dd) ? 1 : 0; };
        int32_t *o = out + i * GL_OUT;
        o[0] = ask(l.group); o[1] = ask(l.chunk[0]); o[2] = ask(l.chunk[1]);
        o[3] = o[4] = 0;
        for (const UsEntry &e : a) o[3] |= ask(e);
        for (const UsEntry &e : b) o[3] |= ask(e);
        for (size_t k = 0; k < coefs.size(); k++) {
            const double t = orc_intersect_ray(coefs[k].data(), o3, d);
            if (t >= EPS && t < MAX_T) o[4] = 1;
        }
        enclosure(l, a, b, o);
        o[7] = o[0] ? 0 : (o[1] != 0) + (o[2] != 0);
    }
}
