// rt_wave_ball.hpp -- the ball around a wave's hit points, once, for every kernel that culls a segment's shadow rays by it: ray_list_kernel
// (rt_adaptive.hip: render_ray_culled) and the streamed cull kernels (rt_stream_cull.hpp and what includes it).  The wavefront kernel forms
// its own at its two sites (rt_wavefront.hip: the hot path, with the box beside the ball).
// The ball only decides which objects a conservative test (sphere_relevant, rt_wavefront_math.hpp) may skip: a skipped object cannot
// block, so no colour and no RT_FLAG_COUNT counter depends on it, nor on the order or the form of the reductions below.
// Cross-lane builtins, hence not part of rt_wavefront_math.hpp, which promises tools/count_flops.cpp to hold none.
// Included by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_WAVE_BALL_HPP
#define RT_WAVE_BALL_HPP

#include <hip/hip_runtime.h>

#include "rt_shade.hpp"          // RT_SYM and the variant's namespace
#include "rt_wavefront_math.hpp" // Ball

namespace RT_SYM(rtk) {

// Every lane ends with the wave's minimum / maximum (no NaN where it matters: wave_hit_ball's callers drop the ball then).  LIBM: the
// steps are fmin / fmax instead of a compare and a select -- the same value up to the sign of a zero; wave_hit_ball says who asks and why.
template <bool LIBM>
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = LIBM ? fmin(v, o) : (o < v ? o : v);
    }
    return v;
}
template <bool LIBM>
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = LIBM ? fmax(v, o) : (o > v ? o : v);
    }
    return v;
}

// The ball around the hit points sp of the wave's lanes with `hit`: the centre of their box, half its diagonal (rounded up) plus the 1e-2
// shadow bias of the ray origins, as the wavefront kernel forms it.  All 64 lanes call.  Returns false -- cull nothing in this segment
// -- when a hit point is not finite.
// LIBM = false is the streamed cull kernels' form, LIBM = true ray_list_kernel's: that kernel runs one wave per SIMD, nothing hides the
// six reductions' latency, and with the compare form its K = 4 passes on 20spheres took 1 to 3 % longer (the compiler waits for every
// shuffle on its own; profiles/adaptive_passes.txt part 3).  Each kernel therefore keeps the machine code it had.  For every wave whose
// hit points are finite the two forms give the same box up to the sign of a zero in a corner.
template <bool LIBM = false>
__device__ __forceinline__ bool wave_hit_ball(bool hit, const D3 &sp, Ball &ball)
{
    const bool finite = !hit || (isfinite(sp.x) && isfinite(sp.y) && isfinite(sp.z));
    const double lx = wave_min<LIBM>(hit ? sp.x : INFINITY), ly = wave_min<LIBM>(hit ? sp.y : INFINITY), lz = wave_min<LIBM>(hit ? sp.z : INFINITY);
    const double hx = wave_max<LIBM>(hit ? sp.x : -INFINITY), hy = wave_max<LIBM>(hit ? sp.y : -INFINITY), hz = wave_max<LIBM>(hit ? sp.z : -INFINITY);
    const double dx = hx - lx, dy = hy - ly, dz = hz - lz;
    ball.cx = 0.5 * (lx + hx);
    ball.cy = 0.5 * (ly + hy);
    ball.cz = 0.5 * (lz + hz);
    ball.R = 0.5 * sqrt(dx * dx + dy * dy + dz * dz) * (1.0 + 1e-9) + 1.01e-2;
    return __ballot(!finite) == 0ull;
}

} // namespace RT_SYM(rtk)

#endif
