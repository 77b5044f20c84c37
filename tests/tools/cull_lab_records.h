// cull_lab_records.h -- the records of tests/tools/cull_lab.cpp and how a predicate of rt_wavefront_math.hpp is called on one.
// Shared by the host lab and tests/tools/cull_device_lab.hip, so that both run the same call on the same bits.
// Include after rt_wavefront_math.hpp.
#pragma once

// doubles per record
#define REC_CONE 12 // kx ky kz r inv_r | org[3] | axis[3] | cos_t
#define REC_PYR 21  // kx ky kz r inv_r | org[3] | tile_nt[9] | cx0 cx1 cy0 cy1
#define REC_SH 26   // kx ky kz c r inv_r | ball c[3] R | box h[3] | p[3] | sdir[3] | inv_uu len_u | s_yz s_xz s_xy | spherical | pad
#define REC_US 5    // quad | four_t2 | t1 | t0 | the oracle's root
#define REC_GQ 4    // t2 | t1 | t0 | the oracle's root
// doubles per case of the grazing generator
#define GP_W 26
#define GS_W (10 + 6 * 64)

namespace rtm {

__device__ __forceinline__ int eval_cone(const double *r)
{
    return sphere_in_cone(r[0], r[1], r[2], r[3], r[4], D3{r[5], r[6], r[7]}, D3{r[8], r[9], r[10]}, r[11]) ? 1 : 0;
}

__device__ __forceinline__ int eval_pyr(const double *r)
{
    FrameArgs fa{}; // (tile_planes reads tile_nt only)
    for (int k = 0; k < 9; k++) fa.tile_nt[k] = r[8 + k];
    const TilePlanes P = tile_planes(fa, r[17], r[18], r[19], r[20]);
    return sphere_in_pyramid(r[0], r[1], r[2], r[3], r[4], D3{r[5], r[6], r[7]}, P) ? 1 : 0;
}

__device__ __forceinline__ int eval_sh(const double *r, double *crec_out)
{
    UsEntry e{};
    e.kx = r[0]; e.ky = r[1]; e.kz = r[2]; e.c = r[3]; e.r = r[4]; e.inv_r = r[5];
    const Ball b{r[6], r[7], r[8], r[9]};
    const BoxH h{r[10], r[11], r[12], 0.0};
    DevLight lt{};
    for (int k = 0; k < 3; k++) { lt.p[k] = r[13 + k]; lt.sdir[k] = r[16 + k]; }
    lt.inv_uu = r[19];
    lt.len_u = r[20];
    const D3 sdir{r[16], r[17], r[18]};
    const CullRec c = cull_record(e, b);
    crec_out[0] = c.wx; crec_out[1] = c.wy; crec_out[2] = c.wz; crec_out[3] = c.ww; crec_out[4] = c.lim; crec_out[5] = c.limr;
    int v = 0;
    if (r[24] != 0.0) {
        v = sphere_relevant<true>(e, b, lt) ? 1 : 0;
    } else {
        v = sphere_relevant<false>(e, b, lt) ? 1 : 0;
        v |= crec_relevant(c, sdir, r[19], r[20]) ? 2 : 0;
        v |= crec_in_box_shadow(c, h, sdir, r[21], r[22], r[23]) ? 4 : 0;
        v |= crec_in_box_shadow(c, h, sdir) ? 8 : 0;
    }
    return v;
}

__device__ __forceinline__ int eval_us(const double *r)
{
    return us_needs_solve(r[0] != 0.0, r[1], r[2], r[3]) ? 1 : 0;
}

__device__ __forceinline__ int eval_gq(const double *r)
{
    return needs_solve(r[0], r[1], r[2]) ? 1 : 0;
}

} // namespace rtm
