// cull_lab.cpp -- CPU lab behind the work-removal predicates of rt_wavefront_math.hpp (test infrastructure: it links the oracle).
// The kernels' own header is compiled for the host (as tools/count_flops.cpp does) and every predicate is called through it:
//   us_needs_solve, needs_solve, sphere_in_cone, tile_planes + sphere_in_pyramid, sphere_relevant<false|true>,
//   cull_record + crec_relevant, both crec_in_box_shadow overloads, the own-sphere window and the two "light behind the surface" skips.
// The truth is always the oracle (orc_intersect_ray, orc_primary_dir, orc_shadow_ray, orc_normal_vector, orc_surface_color) under the
// reference's acceptance rules: nearest hit t >= EPS && t < MAX_T, shadow t > EPS && t < max_t.
//
// Two halves:
//   * generators turn a frame (lab_frame) or a list of grazing parameters (lab_graze_primary, lab_graze_shadow) into RECORDS -- the
//     predicate's own inputs, formed as the callers form them -- and the oracle's verdict for each ("does any ray of the set accept");
//   * evaluators (lab_eval_*) run the predicates on records.  tests/tools/cull_device_lab.hip evaluates the same records on the device.
// Built and driven by tests/tools/cull_lab.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_frame_host.hpp"
#include "rt_wavefront_math.hpp"
#include "../../oracle/rt_oracle.h"
#include "cull_lab_records.h"

using namespace rtm;

namespace {

struct Out { // records of one kind, and the oracle's verdict for each
    double *rec;
    int32_t *truth;
    uint64_t cap, n;
    void push(const double *r, int width, int t)
    {
        if (n < cap) {
            memcpy(rec + n * (uint64_t) width, r, sizeof(double) * (size_t) width);
            truth[n] = t;
        }
        n++;
    }
};

} // namespace

extern "C" {
struct LabOut {
    Out cone, pyr, sh, us, gq;
    uint64_t corner_n, corner_bad; // the corner claim: dot(axis, d) >= cos_t (1 - 1e-9) over all 64 lanes
    double corner_worst;           // smallest dot(axis, d) / cos_t seen
    uint64_t own_n, own_skip, own_bad; // own-sphere window: evaluated, inside the window, inside and the oracle's test blocks
    uint64_t bf_n, bf_skip, bf_bad;    // backface skips: evaluated, skipped, skipped although adding the oracle's term to an accumulator would change its bits
    uint64_t bf_negzero;               // skipped terms with a channel that is -0 (a negative colour times zero), which no accumulator notices: x + -0 == x
};
}

namespace {

// ---- formation code: the frame from the library's own function; the records restated from rt_scene_pack.hpp, cited line by line -----
bool is_unitsq(const double *c)
{
    for (int i = 0; i < 10; i++)
        if (c[i] != 0.0) return false;
    return c[ORC_XY] == 0.0 && c[ORC_XZ] == 0.0 && c[ORC_YZ] == 0.0 && c[ORC_X2] == 1.0 && c[ORC_Y2] == 1.0 && c[ORC_Z2] == 1.0;
}
bool is_cubic(const double *c)
{
    for (int i = 0; i < 10; i++)
        if (c[i] != 0.0) return true;
    return false;
}
bool has_deg2(const double *c)
{
    for (int i = ORC_X2; i <= ORC_YZ; i++)
        if (c[i] != 0.0) return true;
    return false;
}

UsEntry make_us(const double *c, uint32_t orig) // pack_object + pack_us: bounding sphere, table entry and own-sphere window
{
    UsEntry e{};
    e.kx = c[ORC_X]; e.ky = c[ORC_Y]; e.kz = c[ORC_Z]; e.c = c[ORC_C];
    double radius = INFINITY, bc[3] = {0, 0, 0};
    const double cx = -0.5 * c[ORC_X], cy = -0.5 * c[ORC_Y], cz = -0.5 * c[ORC_Z];
    const double r2 = cx * cx + cy * cy + cz * cz - c[ORC_C];
    if (r2 > 0.0 && std::isfinite(r2)) {
        bc[0] = cx; bc[1] = cy; bc[2] = cz;
        radius = std::sqrt(r2);
    }
    e.r = radius;
    e.inv_r = (radius < INFINITY) ? 1.0 / radius : 0.0;
    e.orig = orig;
    e.own_lo = INFINITY;
    e.own_hi = 0.0f;
    if (radius < INFINITY && radius > 0.0) {
        const double r = radius, S = 2.0 * (std::fabs(bc[0]) + std::fabs(bc[1]) + std::fabs(bc[2])) + 3.0 * r + 3.0;
        const double lo = 1e-10 * (r * r + 1.0) + 1e-20 * S * S, hi = (r + 1.0) * (r + 1.0);
        float flo = (float) lo, fhi = (float) hi;
        if (!((double) flo > lo)) flo = std::nextafterf(flo, INFINITY);
        if (!((double) fhi < hi)) fhi = std::nextafterf(fhi, -INFINITY);
        if (std::isfinite(lo) && std::isfinite(hi) && (double) flo > lo && (double) fhi < hi && flo < fhi) {
            e.own_lo = flo;
            e.own_hi = fhi;
        }
    }
    return e;
}

struct LabLight {
    DevLight l;
    LightK k;
};
LabLight make_light(const orc_light &src, bool colours_finite) // pack_light + pack_lightk: DevLight and LightK of one light
{
    LabLight o;
    memset(&o, 0, sizeof(o));
    DevLight &l = o.l;
    for (int k = 0; k < 3; k++) {
        l.p[k] = src.p[k];
        l.color[k] = src.color[k];
    }
    l.spherical = src.is_spherical ? 1u : 0u;
    for (int k = 0; k < 3; k++) l.sdir[k] = (double) (float) l.p[k];
    l.dxx = l.sdir[0] * l.sdir[0];
    l.dyy = l.sdir[1] * l.sdir[1];
    l.dzz = l.sdir[2] * l.sdir[2];
    l.u2 = (l.dxx + l.dyy) + l.dzz;
    l.inv_uu = l.u2 > 0.0 ? 1.0 / l.u2 : 0.0;
    l.len_u = 1.001 * std::sqrt(l.u2);
    const bool finite = colours_finite && std::isfinite(l.color[0]) && std::isfinite(l.color[1]) && std::isfinite(l.color[2]);
    l.backface_exact = (!l.spherical && finite) ? 1u : 0u;
    LightK &k = o.k;
    for (int c = 0; c < 3; c++) { k.p[c] = l.p[c]; k.sdir[c] = l.sdir[c]; k.color[c] = l.color[c]; }
    k.u2 = l.u2; k.inv_uu = l.inv_uu; k.len_u = l.len_u;
    k.four_u2 = 4.0 * l.u2;
    k.s_yz = std::fabs(l.sdir[1]) + std::fabs(l.sdir[2]);
    k.s_xz = std::fabs(l.sdir[0]) + std::fabs(l.sdir[2]);
    k.s_xy = std::fabs(l.sdir[0]) + std::fabs(l.sdir[1]);
    k.flags = (l.spherical ? 1u : 0u) | (l.backface_exact ? 2u : 0u) | (std::fabs(l.u2) > 1e-7 ? 4u : 0u) | ((l.spherical && finite) ? 8u : 0u);
    return o;
}

// rt_render: the frame constants behind tile_planes, formed by the library's own function (csrc/rt_frame_host.hpp) for the oracle's scene
void make_frame(FrameArgs &fa, const orc_scene *sc, const double cam[16])
{
    memset(&fa, 0, sizeof(fa));
    fa.width = sc->px_width;
    fa.height = sc->px_height;
    fa.aspect = (double) sc->px_width / sc->px_height;
    fa.tan_half_fov = std::tan(0.5 * sc->vertical_fov);
    rtf::frame_camera(fa, cam, {});
}

// ---- formation code restated from the kernels ---------------------------------------------------------------------------------
float f_rd(double v) // __double2float_rd
{
    float f = (float) v;
    if ((double) f > v) f = std::nextafterf(f, -INFINITY);
    return f;
}
float f_ru(double v) // __double2float_ru
{
    float f = (float) v;
    if ((double) f < v) f = std::nextafterf(f, INFINITY);
    return f;
}
// phase A' of the general path, the lean block and rt_adaptive.hip: the chunk's box in FP32 with outward rounding, its ball in FP64
void form_ball_box(const double *p, int n, Ball &b, BoxH &h)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], f_rd(p[3 * i + k]));
            hi[k] = fmaxf(hi[k], f_ru(p[3 * i + k]));
        }
    const double dx = (double) hi[0] - (double) lo[0], dy = (double) hi[1] - (double) lo[1], dz = (double) hi[2] - (double) lo[2];
    b.cx = 0.5 * ((double) lo[0] + (double) hi[0]);
    b.cy = 0.5 * ((double) lo[1] + (double) hi[1]);
    b.cz = 0.5 * ((double) lo[2] + (double) hi[2]);
    b.R = 0.5 * sqrt(dx * dx + dy * dy + dz * dz) * (1.0 + 1e-9) + 1.01e-2;
    h = BoxH{0.5 * dx * (1.0 + 1e-9) + 1.01e-2, 0.5 * dy * (1.0 + 1e-9) + 1.01e-2, 0.5 * dz * (1.0 + 1e-9) + 1.01e-2, 0.0};
}

// nearest(): axis = lane 36's direction, cos_t = the minimum over lanes 0, 7, 56, 63
void form_cone(const double d[64][3], D3 &axis, double &cos_t)
{
    axis = D3{d[36][0], d[36][1], d[36][2]};
    auto ca = [&](int l) { return dot3(axis, D3{d[l][0], d[l][1], d[l][2]}); };
    const double c0 = ca(0), c1 = ca(7), c2 = ca(56), c3 = ca(63);
    const double m01 = c0 < c1 ? c0 : c1, m23 = c2 < c3 ? c2 : c3;
    cos_t = m01 < m23 ? m01 : m23;
}

void corner_claim(LabOut *out, const double d[64][3], const D3 &axis, double cos_t)
{
    if (!(cos_t > 0.2)) return; // (sphere_in_cone culls nothing then)
    for (int l = 0; l < 64; l++) {
        const double c = dot3(axis, D3{d[l][0], d[l][1], d[l][2]});
        out->corner_n++;
        if (!(c >= cos_t * (1.0 - 1e-9))) out->corner_bad++;
        if (c / cos_t < out->corner_worst) out->corner_worst = c / cos_t;
    }
}

// the directions of an 8 x 8 block: lane = 8 * row + column; lanes outside the image take the last column / row (rt_wavefront.hip: xc, lrc)
void block_dirs(const orc_scene *sc, const double cam[16], int bx, int by, double d[64][3])
{
    for (int l = 0; l < 64; l++) {
        int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
        if (x >= (int) sc->px_width) x = (int) sc->px_width - 1;
        if (y >= (int) sc->px_height) y = (int) sc->px_height - 1;
        orc_primary_dir(sc, cam, x, y, d[l]);
    }
}

void cone_record(double *r, const UsEntry &e, const double org[3], const D3 &axis, double cos_t)
{
    r[0] = e.kx; r[1] = e.ky; r[2] = e.kz; r[3] = e.r; r[4] = e.inv_r;
    r[5] = org[0]; r[6] = org[1]; r[7] = org[2];
    r[8] = axis.x; r[9] = axis.y; r[10] = axis.z; r[11] = cos_t;
}

// classify_tiles / the tile-level test of the tile's own workgroup: the tile's camera-plane window
void tile_window(const FrameArgs &fa, int tx, int ty, double w[4])
{
    const uint32_t x0 = (uint32_t) tx * RT_TILE, y0 = (uint32_t) ty * RT_TILE;
    const uint32_t x1 = x0 + RT_TILE - 1 < fa.width ? x0 + RT_TILE - 1 : fa.width - 1;
    const uint32_t y1 = y0 + RT_TILE - 1 < fa.height ? y0 + RT_TILE - 1 : fa.height - 1;
    w[0] = fa.cx_a * ((double) x0 - 0.5) + fa.cx_b;
    w[1] = fa.cx_a * ((double) x1 + 0.5) + fa.cx_b;
    w[2] = fa.cy_a * ((double) y0 - 0.5) + fa.cy_b;
    w[3] = fa.cy_a * ((double) y1 + 0.5) + fa.cy_b;
}
void pyr_record(double *r, const UsEntry &e, const FrameArgs &fa, const double w[4])
{
    r[0] = e.kx; r[1] = e.ky; r[2] = e.kz; r[3] = e.r; r[4] = e.inv_r;
    r[5] = fa.origin[0]; r[6] = fa.origin[1]; r[7] = fa.origin[2];
    for (int k = 0; k < 9; k++) r[8 + k] = fa.tile_nt[k];
    for (int k = 0; k < 4; k++) r[17 + k] = w[k];
}

void sh_record(double *r, const UsEntry &e, const Ball &b, const BoxH &h, const LabLight &lt)
{
    r[0] = e.kx; r[1] = e.ky; r[2] = e.kz; r[3] = e.c; r[4] = e.r; r[5] = e.inv_r;
    r[6] = b.cx; r[7] = b.cy; r[8] = b.cz; r[9] = b.R;
    r[10] = h.hx; r[11] = h.hy; r[12] = h.hz;
    for (int k = 0; k < 3; k++) { r[13 + k] = lt.l.p[k]; r[16 + k] = lt.l.sdir[k]; }
    r[19] = lt.l.inv_uu; r[20] = lt.l.len_u;
    r[21] = lt.k.s_yz; r[22] = lt.k.s_xz; r[23] = lt.k.s_xy;
    r[24] = lt.l.spherical ? 1.0 : 0.0;
    r[25] = 0.0;
}

bool shadow_blocks(const double *coef, const orc_light *light, const double p[3], const double so[3])
{
    float fd[3];
    double max_t;
    orc_shadow_ray(light, p, fd, &max_t);
    const double d[3] = {(double) fd[0], (double) fd[1], (double) fd[2]};
    const double t = orc_intersect_ray(coef, so, d);
    return t > EPS && t < max_t;
}

// One chunk of hits (surface points p, biased ray origins so) against every light and every unit sphere: one shadow record each.
void chunk_records(LabOut *out, const double *p, const double *so, int n, const std::vector<LabLight> &lights, const orc_light *olights,
                   const std::vector<UsEntry> &us, const std::vector<const double *> &us_coef)
{
    Ball b;
    BoxH h;
    form_ball_box(p, n, b, h);
    for (size_t l = 0; l < lights.size(); l++) {
        if (!lights[l].l.spherical && !(lights[l].k.flags & 4u)) continue; // |d|^2 <= EPS: every sphere is a candidate in the kernels
        for (size_t j = 0; j < us.size(); j++) {
            int truth = 0;
            for (int i = 0; i < n && !truth; i++) truth = shadow_blocks(us_coef[j], &olights[l], p + 3 * i, so + 3 * i) ? 1 : 0;
            double r[REC_SH];
            sh_record(r, us[j], b, h, lights[l]);
            out->sh.push(r, REC_SH, truth);
        }
    }
}

void us_record(LabOut *out, const UsEntry &e, const Mono &m, double t_ref)
{
    const double r[REC_US] = {fabs(m.u2) > EPS ? 1.0 : 0.0, 4.0 * m.u2, us_t1(e, m), us_t0(e, m), t_ref};
    out->us.push(r, REC_US, (t_ref >= EPS || t_ref > EPS) ? 1 : 0);
}

} // namespace

// Every block, tile and chunk of one frame.  `stride` thins the per-ray solve records (every stride-th pixel); blocks, tiles and chunks are all taken.
extern "C" void lab_frame(const orc_scene *sc, const double cam[16], LabOut *out, int stride)
{
    const int W = (int) sc->px_width, H = (int) sc->px_height, NO = (int) sc->n_objects;
    FrameArgs fa;
    make_frame(fa, sc, cam);
    const double *org = fa.origin;
    std::vector<UsEntry> us;
    std::vector<const double *> us_coef;
    std::vector<int> us_of(NO, -1);
    bool finite = true;
    for (int k = 0; k < NO; k++) {
        const double *c = sc->objects[k].c;
        if (is_unitsq(c)) {
            us_of[k] = (int) us.size();
            us.push_back(make_us(c, (uint32_t) k));
            us_coef.push_back(c);
        }
        for (int i = 0; i < 3; i++) finite = finite && std::isfinite(sc->objects[k].color[i]);
    }
    std::vector<LabLight> lights;
    for (uint32_t l = 0; l < sc->n_lights; l++) lights.push_back(make_light(sc->lights[l], finite));

    // the oracle's root of every (pixel, object), its nearest hit, surface point, normal and shadow-ray origin
    std::vector<double> T((size_t) W * H * (NO ? NO : 1)), P((size_t) W * H * 3), SO((size_t) W * H * 3), N((size_t) W * H * 3);
    std::vector<int> best((size_t) W * H, -1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t px = (size_t) y * W + x;
            double d[3];
            orc_primary_dir(sc, cam, x, y, d);
            Mono m;
            mono_set_o<true>(m, D3{org[0], org[1], org[2]});
            mono_set_d<true>(m, D3{d[0], d[1], d[2]});
            mono_set_od<true>(m);
            double best_t = INFINITY;
            const bool sample = ((x + 3 * y) % stride) == 0;
            for (int k = 0; k < NO; k++) {
                const double *c = sc->objects[k].c;
                const double t = orc_intersect_ray(c, org, d);
                T[px * NO + k] = t;
                if (t >= EPS && t < MAX_T && t < best_t) {
                    best_t = t;
                    best[px] = k;
                }
                if (!sample) continue;
                if (us_of[k] >= 0) us_record(out, us[us_of[k]], m, t);
                else if (!is_cubic(c) && has_deg2(c)) {
                    GqEntry e{};
                    e.x2 = c[ORC_X2]; e.y2 = c[ORC_Y2]; e.z2 = c[ORC_Z2]; e.xy = c[ORC_XY]; e.xz = c[ORC_XZ]; e.yz = c[ORC_YZ];
                    e.kx = c[ORC_X]; e.ky = c[ORC_Y]; e.kz = c[ORC_Z]; e.c = c[ORC_C];
                    const double r[REC_GQ] = {gq_t2(e, m), gq_t1(e, m), gq_t0(e, m), t};
                    out->gq.push(r, REC_GQ, t == -1.0 ? 0 : 1);
                }
            }
            if (best[px] < 0) continue;
            const int bk = best[px];
            double *p = &P[px * 3], *so = &SO[px * 3], *n = &N[px * 3];
            for (int i = 0; i < 3; i++) p[i] = org[i] + best_t * d[i];
            orc_normal_vector(sc->objects[bk].c, p, n);
            for (int i = 0; i < 3; i++) so[i] = p[i] + SHADOW_BIAS * n[i];
            // the shadow rays' own solve skipping, the own-sphere window and the backface skips
            Mono sm;
            mono_set_o<true>(sm, D3{so[0], so[1], so[2]});
            for (uint32_t l = 0; l < sc->n_lights; l++) {
                const LabLight &lt = lights[l];
                float fd[3];
                double max_t;
                orc_shadow_ray(&sc->lights[l], p, fd, &max_t);
                const double dd[3] = {(double) fd[0], (double) fd[1], (double) fd[2]};
                mono_set_d<true>(sm, D3{dd[0], dd[1], dd[2]});
                mono_set_od<true>(sm);
                if (sample)
                    for (size_t j = 0; j < us.size(); j++) us_record(out, us[j], sm, orc_intersect_ray(us_coef[j], so, dd));
                float col[3];
                orc_surface_color(&sc->lights[l], p, n, sc->objects[bk].color, col);
                uint32_t bits[3];
                memcpy(bits, col, sizeof(bits));
                const bool plus_zero = bits[0] == 0u && bits[1] == 0u && bits[2] == 0u;
                bool inert = true; // what the skips rely on: accumulating the term changes no bit (src/update-cpu.cpp:74; the sum starts at +0 and is never -0)
                for (int ch = 0; ch < 3; ch++)
                    for (float acc : {0.0f, 1.17549435e-38f, 0.25f, 1.0f}) {
                        const float sum = acc + col[ch];
                        inert = inert && memcmp(&sum, &acc, sizeof(float)) == 0;
                    }
                const D3 sn = us_of[bk] >= 0 ? sphere_normal(us[us_of[bk]], D3{p[0], p[1], p[2]}) : D3{n[0], n[1], n[2]};
                out->bf_n++;
                if (!lt.l.spherical) {
                    const float lam = (float) dot3(sn, D3{lt.k.p[0], lt.k.p[1], lt.k.p[2]});
                    if ((lt.k.flags & 2u) && !(0.0f < lam)) { // backface_exact
                        out->bf_skip++;
                        if (!inert) out->bf_bad++;
                        else if (!plus_zero) out->bf_negzero++;
                    }
                    if (us_of[bk] >= 0 && (lt.k.flags & 4u) && 0.0f < lam) { // own_sphere_skippable
                        const UsEntry &eo = us[us_of[bk]];
                        Mono so_m;
                        mono_set_o<false>(so_m, D3{p[0] + SHADOW_BIAS * sn.x, p[1] + SHADOW_BIAS * sn.y, p[2] + SHADOW_BIAS * sn.z});
                        const double t0_own = us_t0(eo, so_m);
                        out->own_n++;
                        if (t0_own > (double) eo.own_lo && t0_own < (double) eo.own_hi) {
                            out->own_skip++;
                            if (shadow_blocks(us_coef[us_of[bk]], &sc->lights[l], p, so)) out->own_bad++;
                        }
                    }
                } else {
                    const double dx = lt.k.p[0] - p[0], dy = lt.k.p[1] - p[1], dz = lt.k.p[2] - p[2];
                    const double q = dot3(sn, D3{dx, dy, dz});
                    const double mag = fabs(sn.x * dx) + fabs(sn.y * dy) + fabs(sn.z * dz);
                    if ((lt.k.flags & 8u) != 0u && q < -1e-9 * mag) {
                        out->bf_skip++;
                        if (!inert) out->bf_bad++;
                        else if (!plus_zero) out->bf_negzero++;
                    }
                }
            }
        }

    auto accepts = [&](int x, int y, int k) {
        const double t = T[((size_t) y * W + x) * NO + k];
        return t >= EPS && t < MAX_T;
    };
    // 8 x 8 blocks: the primary cone, and the block's hits as one chunk (the lean path's)
    for (int by = 0; by * 8 < H; by++)
        for (int bx = 0; bx * 8 < W; bx++) {
            double d[64][3];
            block_dirs(sc, cam, bx, by, d);
            D3 axis;
            double cos_t;
            form_cone(d, axis, cos_t);
            corner_claim(out, d, axis, cos_t);
            double pts[64 * 3], sos[64 * 3];
            int n = 0;
            for (int l = 0; l < 64; l++) {
                const int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
                if (x >= W || y >= H || best[(size_t) y * W + x] < 0) continue;
                memcpy(pts + 3 * n, &P[((size_t) y * W + x) * 3], 24);
                memcpy(sos + 3 * n, &SO[((size_t) y * W + x) * 3], 24);
                n++;
            }
            for (size_t j = 0; j < us.size(); j++) {
                int truth = 0;
                for (int l = 0; l < 64 && !truth; l++) {
                    const int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
                    truth = accepts(x < W ? x : W - 1, y < H ? y : H - 1, (int) us[j].orig) ? 1 : 0;
                }
                double r[REC_CONE];
                cone_record(r, us[j], org, axis, cos_t);
                out->cone.push(r, REC_CONE, truth);
            }
            if (n) chunk_records(out, pts, sos, n, lights, sc->lights, us, us_coef);
        }
    // 16 x 16 tiles: the pyramid, and the tile's hits in chunks of 64 (the general path's queue; rt_adaptive.hip's chunks are subsets of a tile too)
    for (int ty = 0; ty * RT_TILE < H; ty++)
        for (int tx = 0; tx * RT_TILE < W; tx++) {
            std::vector<double> pts, sos;
            for (int yy = ty * RT_TILE; yy < (ty + 1) * RT_TILE && yy < H; yy++)
                for (int xx = tx * RT_TILE; xx < (tx + 1) * RT_TILE && xx < W; xx++) {
                    const size_t px = (size_t) yy * W + xx;
                    if (best[px] < 0) continue;
                    pts.insert(pts.end(), &P[px * 3], &P[px * 3] + 3);
                    sos.insert(sos.end(), &SO[px * 3], &SO[px * 3] + 3);
                }
            for (size_t first = 0; first * 3 < pts.size(); first += 64) {
                const int n = (int) (pts.size() / 3 - first < 64 ? pts.size() / 3 - first : 64);
                chunk_records(out, pts.data() + 3 * first, sos.data() + 3 * first, n, lights, sc->lights, us, us_coef);
            }
            if (!fa.tile_planes_ok) continue;
            double w[4];
            tile_window(fa, tx, ty, w);
            for (size_t j = 0; j < us.size(); j++) {
                int truth = 0;
                for (int yy = ty * RT_TILE; yy < (ty + 1) * RT_TILE && yy < H && !truth; yy++)
                    for (int xx = tx * RT_TILE; xx < (tx + 1) * RT_TILE && xx < W && !truth; xx++) truth = accepts(xx, yy, (int) us[j].orig) ? 1 : 0;
                double r[REC_PYR];
                pyr_record(r, us[j], fa, w);
                out->pyr.push(r, REC_PYR, truth);
            }
        }
}

// ---- the grazing generator ----------------------------------------------------------------------------------------------------
// Primary rays.  One case = GP_W doubles: width, height, vertical fov (radians), cam[16], block column, block row (8 x 8 blocks), lane,
// distance of the tangent point along that lane's ray, radius, relative clearance (negative: the ray cuts the sphere), mode
// (0: tangent to a ray of the block, on the side away from the block's axis -- one cone record; 1: the same for an edge ray of the 16 x 16
// tile the block lies in, away from the tile's centre -- one pyramid record).  centre_out[3 n] receives the sphere's centre.
extern "C" void lab_graze_primary(uint64_t n, const double *par, LabOut *out, double *centre_out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GP_W;
        orc_scene sc;
        memset(&sc, 0, sizeof(sc));
        sc.px_width = (uint32_t) q[0];
        sc.px_height = (uint32_t) q[1];
        sc.vertical_fov = q[2];
        const double *cam = q + 3;
        const int bx = (int) q[19], by = (int) q[20], lane = (int) q[21], mode = (int) q[25];
        const double s = q[22], r = q[23], delta = q[24];
        FrameArgs fa;
        make_frame(fa, &sc, cam);
        const double *org = fa.origin;
        const int W = (int) sc.px_width, H = (int) sc.px_height;
        double d[64][3];
        // the rays of the set, and the one the sphere is placed against
        std::vector<double> rays;
        double dj[3], ctr_dir[3];
        if (mode == 0) {
            block_dirs(&sc, cam, bx, by, d);
            for (int l = 0; l < 64; l++) rays.insert(rays.end(), d[l], d[l] + 3);
            memcpy(dj, d[lane], 24);
            memcpy(ctr_dir, d[36], 24);
        } else {
            const int tx = bx / 2, ty = by / 2;
            const int x0 = tx * RT_TILE, y0 = ty * RT_TILE, x1 = x0 + RT_TILE - 1 < W ? x0 + RT_TILE - 1 : W - 1, y1 = y0 + RT_TILE - 1 < H ? y0 + RT_TILE - 1 : H - 1;
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) {
                    double dd[3];
                    orc_primary_dir(&sc, cam, x, y, dd);
                    rays.insert(rays.end(), dd, dd + 3);
                }
            // `lane` walks the tile's perimeter
            const int side = lane & 3, k = lane >> 2, nx = x1 - x0, ny = y1 - y0;
            int x = x0, y = y0;
            if (side == 0) { x = x0 + (nx ? k % (nx + 1) : 0); y = y0; }
            if (side == 1) { x = x0 + (nx ? k % (nx + 1) : 0); y = y1; }
            if (side == 2) { y = y0 + (ny ? k % (ny + 1) : 0); x = x0; }
            if (side == 3) { y = y0 + (ny ? k % (ny + 1) : 0); x = x1; }
            orc_primary_dir(&sc, cam, x, y, dj);
            orc_primary_dir(&sc, cam, (x0 + x1) / 2, (y0 + y1) / 2, ctr_dir);
        }
        // unit vector perpendicular to dj, pointing away from the centre of the ray set
        double u[3];
        const double dc = dj[0] * ctr_dir[0] + dj[1] * ctr_dir[1] + dj[2] * ctr_dir[2];
        for (int k = 0; k < 3; k++) u[k] = dj[k] * dc - ctr_dir[k];
        double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (!(un > 1e-12)) { // the central ray itself: any perpendicular
            const double a[3] = {fabs(dj[0]) < 0.5 ? 1.0 : 0.0, fabs(dj[0]) < 0.5 ? 0.0 : 1.0, 0.0};
            u[0] = dj[1] * a[2] - dj[2] * a[1]; u[1] = dj[2] * a[0] - dj[0] * a[2]; u[2] = dj[0] * a[1] - dj[1] * a[0];
            un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        }
        double centre[3], coef[ORC_NCOEF];
        for (int k = 0; k < 3; k++) centre[k] = org[k] + s * dj[k] + r * (1.0 + delta) * (u[k] / un);
        if (centre_out) memcpy(centre_out + 3 * i, centre, 24);
        orc_surface_sphere(centre, r, coef);
        const UsEntry e = make_us(coef, 0);
        int truth = 0;
        for (size_t k = 0; k < rays.size() && !truth; k += 3) {
            const double t = orc_intersect_ray(coef, org, &rays[k]);
            truth = (t >= EPS && t < MAX_T) ? 1 : 0;
        }
        if (mode == 0) {
            D3 axis;
            double cos_t;
            form_cone(d, axis, cos_t);
            corner_claim(out, d, axis, cos_t);
            double rec[REC_CONE];
            cone_record(rec, e, org, axis, cos_t);
            out->cone.push(rec, REC_CONE, truth);
        } else if (fa.tile_planes_ok) {
            double w[4], rec[REC_PYR];
            tile_window(fa, bx / 2, by / 2, w);
            pyr_record(rec, e, fa, w);
            out->pyr.push(rec, REC_PYR, truth);
        }
    }
}

// Shadow rays.  One case = GS_W doubles: light kind (1 point), light p[3] (direction as stored / position), blocker radius, relative clearance,
// distance of the tangent point along the chosen hit's ray (in units of the ray's direction vector: 0 = its origin, 1 = the light for a point
// light), angle of the tangent point around that ray, index of the chosen hit, number of hits m (<= 64), then m hits of six doubles: surface
// point and (unnormalised) normal.  The chunk's ball and box are formed from the surface points as the kernels form them; every hit's ray is
// the oracle's (orc_shadow_ray from the surface point, origin = point + 1e-2 * unit normal).  One shadow record per case.
extern "C" void lab_graze_shadow(uint64_t n, const double *par, LabOut *out, double *centre_out)
{
    for (uint64_t i = 0; i < n; i++) {
        const double *q = par + i * GS_W;
        orc_light light;
        memset(&light, 0, sizeof(light));
        light.is_spherical = q[0] != 0.0 ? 1 : 0;
        for (int k = 0; k < 3; k++) { light.p[k] = q[1 + k]; light.color[k] = 1.0f; }
        const double r = q[4], delta = q[5], s = q[6], phi = q[7];
        const int j = (int) q[8], m = (int) q[9];
        double pts[64 * 3], sos[64 * 3];
        for (int h = 0; h < m; h++) {
            const double *hp = q + 10 + 6 * h;
            const double nn = sqrt(hp[3] * hp[3] + hp[4] * hp[4] + hp[5] * hp[5]);
            for (int k = 0; k < 3; k++) {
                pts[3 * h + k] = hp[k];
                sos[3 * h + k] = hp[k] + SHADOW_BIAS * (hp[3 + k] / nn);
            }
        }
        const LabLight lt = make_light(light, true);
        if (!lt.l.spherical && !(lt.k.flags & 4u)) continue;
        float fd[3];
        double max_t;
        orc_shadow_ray(&light, pts + 3 * j, fd, &max_t);
        const double d[3] = {(double) fd[0], (double) fd[1], (double) fd[2]};
        const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double a[3] = {fabs(d[0]) < 0.5 * dn ? 1.0 : 0.0, fabs(d[0]) < 0.5 * dn ? 0.0 : 1.0, 0.0};
        double u[3] = {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]};
        double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        for (int k = 0; k < 3; k++) u[k] /= un;
        double v[3] = {(d[1] * u[2] - d[2] * u[1]) / dn, (d[2] * u[0] - d[0] * u[2]) / dn, (d[0] * u[1] - d[1] * u[0]) / dn};
        double centre[3], coef[ORC_NCOEF];
        for (int k = 0; k < 3; k++) centre[k] = sos[3 * j + k] + s * d[k] + r * (1.0 + delta) * (cos(phi) * u[k] + sin(phi) * v[k]);
        if (centre_out) memcpy(centre_out + 3 * i, centre, 24);
        orc_surface_sphere(centre, r, coef);
        const UsEntry e = make_us(coef, 0);
        int truth = 0;
        for (int h = 0; h < m && !truth; h++) truth = shadow_blocks(coef, &light, pts + 3 * h, sos + 3 * h) ? 1 : 0;
        Ball b;
        BoxH bh;
        form_ball_box(pts, m, b, bh);
        double rec[REC_SH];
        sh_record(rec, e, b, bh, lt);
        out->sh.push(rec, REC_SH, truth);
    }
}

// ---- the evaluators: the predicates themselves, on records ----------------------------------------------------------------------
extern "C" void lab_eval_cone(uint64_t n, const double *rec, int32_t *verdict)
{
    for (uint64_t i = 0; i < n; i++) verdict[i] = eval_cone(rec + i * REC_CONE);
}
extern "C" void lab_eval_pyr(uint64_t n, const double *rec, int32_t *verdict)
{
    for (uint64_t i = 0; i < n; i++) verdict[i] = eval_pyr(rec + i * REC_PYR);
}
// verdict: bit 0 sphere_relevant<kind>, 1 crec_relevant(cull_record) (directional), 2 / 3 the two crec_in_box_shadow overloads (directional);
// crec[6 n]: the fields of cull_record
extern "C" void lab_eval_sh(uint64_t n, const double *rec, int32_t *verdict, double *crec)
{
    for (uint64_t i = 0; i < n; i++) verdict[i] = eval_sh(rec + i * REC_SH, crec + 6 * i);
}
// verdict: us_needs_solve(quad, four_t2, t1, t0)
extern "C" void lab_eval_us(uint64_t n, const double *rec, int32_t *verdict)
{
    for (uint64_t i = 0; i < n; i++) verdict[i] = eval_us(rec + i * REC_US);
}
// verdict: needs_solve(t2, t1, t0)
extern "C" void lab_eval_gq(uint64_t n, const double *rec, int32_t *verdict)
{
    for (uint64_t i = 0; i < n; i++) verdict[i] = eval_gq(rec + i * REC_GQ);
}
// the oracle's root for a ray against 20 coefficients (hand-made cases)
extern "C" double lab_oracle_root(const double *coef, const double *o, const double *d)
{
    return orc_intersect_ray(coef, o, d);
}
