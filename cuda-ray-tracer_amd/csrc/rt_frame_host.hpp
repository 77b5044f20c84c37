// rt_frame_host.hpp -- the frame constants the host forms for the kernels: the camera-plane tables of a context, the per-frame camera words
// of FrameArgs, and the global row of a halo slot.  rt_capi.cpp calls these; so do the test tools (tests/tools/cull_lab.cpp), which is why
// they are free of HIP calls and compile with a plain C++ compiler (rt_math.hpp over a stand-in <hip/hip_runtime.h>).
//
// Parity-critical: the values feed the kernels' FP64 arithmetic, so every translation unit that includes this is built with
// -ffp-contract=off (one rounding per operation, as written).
#ifndef RT_FRAME_HOST_HPP
#define RT_FRAME_HOST_HPP

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_math.hpp" // (rtm::cubic_at, host side: the Taylor data of degree-3 objects at the frame's ray origin)
#include "rt_scene_dev.h"

namespace rtf {

// camera-plane coordinates of every pixel column / row of an nx x ny frame: render_pixel's camera_x / camera_y
// (src/update-cpu.cpp:84-87) depend only on the pixel index and the scene, so they are evaluated once,
// with the same IEEE operations in the same order
inline void camera_tables(uint32_t nx, uint32_t ny, double aspect, double tan_half_fov, std::vector<double> &cx, std::vector<double> &cy)
{
    cx.resize(nx);
    cy.resize(ny);
    for (uint32_t x = 0; x < nx; x++) {
        const double ndc_x = ((int) x + 0.5) / (int) nx;
        cx[x] = (2.0 * ndc_x - 1.0) * aspect * tan_half_fov;
    }
    for (uint32_t y = 0; y < ny; y++) {
        const double ndc_y = ((int) y + 0.5) / (int) ny;
        cy[y] = (2.0 * ndc_y - 1.0) * tan_half_fov;
    }
}

// the camera, the ray origin of its frame and the degree-3 objects' records at that origin: all a G-buffer pass or a pick needs
inline void frame_origin(FrameArgs &fa, const double cam[16], const std::vector<double> &cub_coefs)
{
    std::memcpy(fa.cam, cam, sizeof(double) * 16);
    // g_ray_origin = camera_matrix * (0,0,0,1), src/update-cpu.cpp:123 -- glm order (m0*x + m1*y) + (m2*z + m3*w)
    for (int r = 0; r < 3; r++) fa.origin[r] = (cam[0 + r] * 0.0 + cam[4 + r] * 0.0) + (cam[8 + r] * 0.0 + cam[12 + r] * 1.0);
    for (size_t j = 0; j * 20 < cub_coefs.size(); j++) { // degree-3 objects: F, grad F, half Hessian at the frame's ray origin (rt_math.hpp, cubic_at)
        const rtm::CubicAt a = rtm::cubic_at(cub_coefs.data() + j * 20, rtm::D3{fa.origin[0], fa.origin[1], fa.origin[2]});
        const rtm::CubicAbs ab = rtm::cubic_abs(cub_coefs.data() + j * 20); // what cubic_guarded's error bounds follow from (same function as on the device)
        const double v[RT_CUB_REC] = {a.f, a.gx, a.gy, a.gz, a.hxx, a.hyy, a.hzz, a.hxy, a.hxz, a.hyz};
        const double va[4] = {ab.a3, ab.a2, ab.a1, ab.a0};
        std::memcpy(fa.cub_rec[j], v, sizeof(v));
        std::memcpy(fa.cub_abs[j], va, sizeof(va));
    }
}

// ... and what a rendered frame needs besides: the tile pyramids of the early-out test (FrameArgs::tile_nt, the inverse transpose of the
// camera's 3x3 part) and the linear form of the camera-plane coordinates.  Reads fa.width, height, aspect, tan_half_fov.
inline void frame_camera(FrameArgs &fa, const double cam[16], const std::vector<double> &cub_coefs)
{
    frame_origin(fa, cam, cub_coefs);
    const double a = cam[0], b = cam[4], c = cam[8], d = cam[1], e = cam[5], f = cam[9], g = cam[2], h = cam[6], i = cam[10];
    const double co00 = e * i - f * h, co01 = -(d * i - f * g), co02 = d * h - e * g;
    const double co10 = -(b * i - c * h), co11 = a * i - c * g, co12 = -(a * h - b * g);
    const double co20 = b * f - c * e, co21 = -(a * f - c * d), co22 = a * e - b * d;
    const double det = a * co00 + b * co01 + c * co02;
    const double amax = std::fabs(a) + std::fabs(b) + std::fabs(c) + std::fabs(d) + std::fabs(e) + std::fabs(f) + std::fabs(g) + std::fabs(h) + std::fabs(i);
    fa.tile_planes_ok = (std::isfinite(det) && std::isfinite(amax) && std::fabs(det) > 1e-9 * amax * amax * amax) ? 1u : 0u;
    if (fa.tile_planes_ok) { // (M^-1)^T = cofactor matrix / det; stored column-major: element (row r, col k) at [3 * k + r]
        const double inv = 1.0 / det;
        const double nt[9] = {co00 * inv, co10 * inv, co20 * inv, co01 * inv, co11 * inv, co21 * inv, co02 * inv, co12 * inv, co22 * inv};
        for (int k = 0; k < 9; k++) fa.tile_nt[k] = nt[k];
    }
    fa.cx_a = 2.0 * fa.aspect * fa.tan_half_fov / (double) fa.width;
    fa.cx_b = (1.0 / (double) fa.width - 1.0) * fa.aspect * fa.tan_half_fov;
    fa.cy_a = 2.0 * fa.tan_half_fov / (double) fa.height;
    fa.cy_b = (1.0 / (double) fa.height - 1.0) * fa.tan_half_fov;
    if (!(fa.cx_a > 0.0) || !(fa.cy_a > 0.0) || !std::isfinite(fa.cx_a) || !std::isfinite(fa.cy_a)) fa.tile_planes_ok = 0;
}

// Adaptive supersampling on several ranks: halo slot 2b / 2b + 1 holds the global row just below / above this rank's local band b (the
// ray-list kernel's own rule, rt_adaptive.hip).  -1 or the image's height: the slot lies outside the image.
inline int64_t halo_global_row(uint32_t h, uint32_t band_rows, uint32_t world, uint32_t rank, uint32_t local_rows)
{
    const uint32_t b = h >> 1, rows = std::min(band_rows, local_rows - b * band_rows);
    const int64_t g0 = ((int64_t) b * world + rank) * band_rows;
    return (h & 1u) ? g0 + rows : g0 - 1;
}

} // namespace rtf

#endif
