// rt_wave_cone.hpp -- the cone of a wave whose lanes are NOT the pixels of one 8 x 8 block: the sample rays of listed pixels and the
// centre rays of halo rows (ray_list_cull_kernel, rt_stream_cull_adaptive.hip).  All rays leave one origin.
//   axis  = the direction of one lane in use, bit for bit (so it is unit to rounding, as sphere_in_cone's proof assumes): the lane whose
//           direction lies nearest the mean of the used directions -- a tightness choice, any used lane is sound;
//   cos_t = the minimum of dot3(axis, d) over ALL lanes in use.  No corner shortcut: the pixels of a list wave are not convex on the
//           image plane.  Lanes with use == false contribute nothing.
// The lanes' own parts are the functions below; between them the wave reduces (sum, max, readlane, min): wc_wave_cone in the kernel's
// file, and tests/tools/wave_cone_lab.cpp on the host, which compiles this header as cull_lab.cpp compiles rt_wavefront_math.hpp.
#ifndef RT_WAVE_CONE_HPP
#define RT_WAVE_CONE_HPP

#include <hip/hip_runtime.h>

#include "rt_math.hpp"

namespace rtm {

// what a lane adds to the sum of the used directions
__device__ __forceinline__ D3 wc_term(const D3 &d, bool use)
{
    return use ? d : D3{0.0, 0.0, 0.0};
}
// how near a lane's direction is to the mean (the sum: its length does not matter); the wave's maximum picks the axis lane
__device__ __forceinline__ double wc_score(const D3 &sum, const D3 &d, bool use)
{
    return use ? dot3(sum, d) : -INFINITY;
}
// is this lane a candidate for the axis?  (NaN scores compare false: a wave without a candidate takes its first used lane)
__device__ __forceinline__ bool wc_is_pick(double score, double best, bool use)
{
    return use && score == best;
}
// what a lane offers to the minimum that is cos_t
__device__ __forceinline__ double wc_cos(const D3 &axis, const D3 &d, bool use)
{
    return use ? dot3(axis, d) : INFINITY;
}

} // namespace rtm

#endif
