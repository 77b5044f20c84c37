// stream_cull_lab.cpp -- host lab behind RT_FLAG_STREAM_CULL (test infrastructure: it links the oracle).
//   * the scene image of a context whose decision is true, by the library's own host functions (csrc/rt_scene_image.hpp: scene_image,
//     stream_cull_image over rtp::pack_chunk_bound): the blob with its ordered unit-sphere table, and the chunk bounds;
//   * the predicate lab: the culling predicates of rt_wavefront_math.hpp asked about the BOUND of a chunk whose members are a sphere of
//     cull_lab's grazing generator and companions placed by the caller; the truth is the oracle's verdict for EVERY member under the
//     reference's acceptance rules, on the ray set the generator used.
// The generators, the record layouts and the formation code are cull_lab.cpp's own (included as text: its helpers have internal linkage).
// Built and driven by tests/tools/stream_cull_lab.py.
#include "cull_lab.cpp"

#include "rt_scene_image.hpp"

struct LabDesc { // the arrays of rt_scene_desc, as tests/tools/scene_pack_lab.h passes them (that header's LabLight clashes with cull_lab.cpp's)
    uint32_t n_objects, n_lights;
    const double *coefs;
    const float *reflection, *albedo;
    const uint8_t *light_is_spherical;
    const double *light_p;
    const float *light_color;
};

static rt_scene_desc lab_desc(const LabDesc *sd)
{
    rt_scene_desc d{};
    d.n_objects = sd->n_objects; d.n_lights = sd->n_lights;
    d.coefs = sd->coefs; d.reflection = sd->reflection; d.albedo = sd->albedo;
    d.light_is_spherical = sd->light_is_spherical; d.light_p = sd->light_p; d.light_color = sd->light_color;
    return d;
}

// ---- the scene image -----------------------------------------------------------------------------------------------------------------
// words: n_us, off_us, n_chunks, fa.cull, scene_bytes.  slot_orig: NULL = the order of rt_create, else the object of every table slot.
// ordered = 0: the blob of a context without the flag (no bounds).  Returns the blob's size; fills what fits.
extern "C" uint64_t lab_stream_cull_image(const LabDesc *sd, uint32_t flags, uint32_t fill, int ordered, const uint32_t *slot_orig, unsigned char *blob, uint64_t blob_cap,
                                          unsigned char *bounds, uint64_t bounds_cap, uint32_t *words)
{
    FrameArgs fa{};
    rtp::SceneImage im = rtp::scene_image(lab_desc(sd), flags, fa, (unsigned char) fill);
    std::vector<UsEntry> b;
    if (ordered) b = rtp::stream_cull_image(im, fa, (unsigned char) fill, slot_orig);
    words[0] = fa.n_us; words[1] = fa.off_us; words[2] = (uint32_t) b.size(); words[3] = fa.cull; words[4] = fa.scene_bytes;
    if (blob && blob_cap >= im.blob.size()) memcpy(blob, im.blob.data(), im.blob.size());
    if (bounds && bounds_cap >= b.size() * sizeof(UsEntry) && !b.empty()) memcpy(bounds, b.data(), b.size() * sizeof(UsEntry));
    return im.blob.size();
}

// ---- the predicate lab ---------------------------------------------------------------------------------------------------------------
namespace {

// the chunk's members as rt_create packs them: the grazing sphere first, then the companions (centre, radius)
std::vector<UsEntry> pack_members(const double g_centre[3], double g_r, int m, const double *comp, std::vector<std::vector<double>> &coefs)
{
    std::vector<UsEntry> us;
    for (int k = 0; k <= m; k++) {
        const double *c = k == 0 ? g_centre : comp + 4 * (k - 1);
        const double r = k == 0 ? g_r : comp[4 * (k - 1) + 3];
        std::vector<double> coef(ORC_NCOEF);
        orc_surface_sphere(c, r, coef.data());
        const float albedo[3] = {1.0f, 1.0f, 1.0f};
        DevObject o;
        rtp::pack_object(o, coef.data(), albedo, 0.0f);
        UsEntry e;
        rtp::pack_us(e, o, (uint32_t) k);
        us.push_back(e);
        coefs.push_back(coef);
    }
    return us;
}

} // namespace

// Primary rays.  par: cull_lab's GP_W doubles per case (mode 0).  comp: per case m companions of four doubles (centre, radius).
// Per case out: rec[REC_CONE] = the cone record of the BOUND, verdict = sphere_in_cone about it, truth = the oracle accepts some member
// for some ray of the block, g_truth = it accepts the grazing sphere, bound[8] = kx ky kz c r inv_r of the bound and max_i(|c_i - C| + r_i)
// is left to the caller (members_out: (m + 1) x (centre, r, inv_r) as packed).
extern "C" void lab_bound_primary(uint64_t n, const double *par, int m, const double *comp, double *rec, int32_t *verdict, int32_t *truth, int32_t *g_truth,
                                  double *members_out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GP_W;
        double one_rec[REC_CONE], one_pyr[REC_PYR], centre[3];
        int32_t t_cone = 0, t_pyr = 0;
        LabOut out;
        memset(&out, 0, sizeof(out));
        out.cone = Out{one_rec, &t_cone, 1, 0};
        out.pyr = Out{one_pyr, &t_pyr, 1, 0};
        lab_graze_primary(1, q, &out, centre);
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
        const std::vector<UsEntry> us = pack_members(centre, q[23], m, comp + i * 4 * (uint64_t) m, coefs);
        int any = 0, g = 0;
        for (size_t k = 0; k < us.size(); k++)
            for (int l = 0; l < 64; l++) {
                const double t = orc_intersect_ray(coefs[k].data(), fa.origin, d[l]);
                if (t >= EPS && t < MAX_T) {
                    any = 1;
                    if (k == 0) g = 1;
                }
            }
        UsEntry b;
        memset(&b, 0xA5, sizeof(b));
        rtp::pack_chunk_bound(b, us.data(), (uint32_t) us.size(), 0u);
        double *r = rec + i * REC_CONE;
        memcpy(r, one_rec, sizeof(one_rec)); // org, axis, cos_t of the block
        r[0] = b.kx; r[1] = b.ky; r[2] = b.kz; r[3] = b.r; r[4] = b.inv_r;
        verdict[i] = eval_cone(r);
        truth[i] = any;
        g_truth[i] = g;
        for (size_t k = 0; k < us.size(); k++) {
            double *mo = members_out + (i * (uint64_t) (m + 1) + k) * 5;
            mo[0] = -0.5 * us[k].kx; mo[1] = -0.5 * us[k].ky; mo[2] = -0.5 * us[k].kz; mo[3] = us[k].r; mo[4] = us[k].inv_r;
        }
    }
}

// Shadow rays.  par: cull_lab's GS_W doubles per case; the rest as above with rec[REC_SH] (bit 0 of the verdict: sphere_relevant<kind>).
// A case the generator drops (a directional light with |d|^2 <= EPS) gets verdict -1.
extern "C" void lab_bound_shadow(uint64_t n, const double *par, int m, const double *comp, double *rec, int32_t *verdict, int32_t *truth, int32_t *g_truth,
                                 double *members_out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GS_W;
        double one_rec[REC_SH], centre[3];
        int32_t t_sh = 0;
        LabOut out;
        memset(&out, 0, sizeof(out));
        out.sh = Out{one_rec, &t_sh, 1, 0};
        lab_graze_shadow(1, q, &out, centre);
        verdict[i] = -1;
        if (out.sh.n != 1) continue;
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
        const std::vector<UsEntry> us = pack_members(centre, q[4], m, comp + i * 4 * (uint64_t) m, coefs);
        int any = 0, g = 0;
        for (size_t k = 0; k < us.size(); k++)
            for (int h = 0; h < nh; h++)
                if (shadow_blocks(coefs[k].data(), &light, pts + 3 * h, sos + 3 * h)) {
                    any = 1;
                    if (k == 0) g = 1;
                }
        UsEntry b;
        memset(&b, 0xA5, sizeof(b));
        rtp::pack_chunk_bound(b, us.data(), (uint32_t) us.size(), 0u);
        double *r = rec + i * REC_SH;
        memcpy(r, one_rec, sizeof(one_rec)); // ball, box, light
        r[0] = b.kx; r[1] = b.ky; r[2] = b.kz; r[3] = b.c; r[4] = b.r; r[5] = b.inv_r;
        double crec[6];
        verdict[i] = eval_sh(r, crec) & 1;
        truth[i] = any;
        g_truth[i] = g;
        for (size_t k = 0; k < us.size(); k++) {
            double *mo = members_out + (i * (uint64_t) (m + 1) + k) * 5;
            mo[0] = -0.5 * us[k].kx; mo[1] = -0.5 * us[k].ky; mo[2] = -0.5 * us[k].kz; mo[3] = us[k].r; mo[4] = us[k].inv_r;
        }
    }
}
