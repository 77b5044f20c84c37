// rt_wave_box.hip -- rt_debug_wave_box (include/mi355rt.h): the box helper of the render kernel's two schedules (rt_wave_box.hpp) run alone,
// one wave per entry, so that a test can hold its lane patterns and its directed roundings to numpy value by value.
//
// Compiled ONCE, with -ffp-contract=off, like rt_resolve.hip: the helper converts, selects and takes minima and maxima -- there is no
// arithmetic in it that a contraction could change.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include "rt_wave_box.hpp"
#include <cstdint>

namespace {

// pts = [n_waves][64][3] doubles, use_masks = [n_waves] (bit l: lane l's point counts), out = [n_waves][6]: lox, hix, loy, hiy, loz, hiz.
// One wave per workgroup, all 64 lanes active throughout (the helper's precondition); lane 0 stores the wave-uniform result.
__global__ __launch_bounds__(64) void wave_box_kernel(const double *__restrict__ pts, const unsigned long long *__restrict__ use_masks, uint32_t n_waves,
                                                      float *__restrict__ out)
{
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    if (w >= n_waves) return; // (wave-uniform; the grid is n_waves workgroups)
    const double *p = pts + ((size_t) w * 64u + lane) * 3u;
    const bool use = (use_masks[w] >> lane) & 1ull;
    float lo[3], hi[3];
    wave_box_f32(use, p[0], p[1], p[2], lo, hi);
    if (lane == 0u) {
        float *o = out + (size_t) w * 6u;
        o[0] = lo[0]; o[1] = hi[0]; o[2] = lo[1]; o[3] = hi[1]; o[4] = lo[2]; o[5] = hi[2];
    }
}

} // namespace

extern "C" hipError_t rt_launch_wave_box(const double *pts, const unsigned long long *use_masks, uint32_t n_waves, float *out, hipStream_t stream)
{
    if (n_waves == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wave_box_kernel, dim3(n_waves), dim3(64), 0, stream, pts, use_masks, n_waves, out);
    return hipGetLastError();
}
