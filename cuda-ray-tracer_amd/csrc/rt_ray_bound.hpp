// rt_ray_bound.hpp -- can ONE ray meet anything inside a chunk bound?  The per-ray culling predicate of the bounce rays of streamed frames
// (RT_FLAG_STREAM_CULL_BOUNCE: sc_query_bounce, rt_stream_cull_bounce.hpp).
// Nothing new is decided here: sphere_relevant<false> (rt_wavefront_math.hpp) answers whether a sphere can be met by a half-line that
// starts inside a ball and runs along one direction, roots above EPS only.  A bounce ray (o, d) is that half-line with the ball shrunk to
// its own origin (R = 0) and the direction its own d, in double precision and unrounded:
//     ray_reaches(bound, o, d) = sphere_relevant<false>(bound, Ball{o, 0}, RayDir{d, 1 / |d|^2, 1.001 |d|}),
// inv_uu and len_u by the formulas rtp::pack_light uses for a directional light.  rtp::pack_chunk_bound's argument covers sphere_relevant
// for ANY ball and direction held fixed over the call, so "the bound is skipped" implies "every member is skipped by its own predicate",
// and a member skipped by its own predicate has no root the reference's acceptance rule (t >= EPS, t < MAX_T) could take.
// The answer is "test it" -- nothing is culled for this ray -- when
//   * |d|^2 is not finite or not above EPS: the reference's solver then takes its linear branch, which is not geometry;
//   * a component of o or d is beyond the magnitude the class tables are proven for (rq_tables_proven, rt_rayquery.hpp), NaN included;
//   * the bound has r = +inf (a member without a radius): sphere_relevant itself says so.
// Host and device, like rt_wave_cone.hpp: tests/tools/bounce_cull_lab.cpp compiles this header and holds it to the oracle.
#ifndef RT_RAY_BOUND_HPP
#define RT_RAY_BOUND_HPP

#include <hip/hip_runtime.h>

#include "rt_wavefront_math.hpp" // UsEntry, Ball, sphere_relevant

namespace rtm {

constexpr double RB_PLAIN_ABOVE = 1e100; // rq_tables_proven's bound (rt_stream_cull_bounce.hpp asserts that the two are one number)

// what sphere_relevant<false> reads of a light (p: the point-light half reads it and has to compile; never formed, never read here)
struct RayDir {
    double sdir[3];
    double inv_uu, len_u;
    double p[3];
};

// a ray as the predicate wants it, formed once per query: the ray's own part of every verdict
struct RayBound {
    Ball ball;  // the origin, R = 0
    RayDir dir; // d, 1 / |d|^2, 1.001 |d|
    bool cull;  // false: every bound is answered "test it"
};

__device__ __forceinline__ RayBound ray_bound(const D3 &o, const D3 &d)
{
    const double dd = (d.x * d.x + d.y * d.y) + d.z * d.z;
    // (every component on its own: a NaN fails its comparison)
    const bool small = fabs(o.x) <= RB_PLAIN_ABOVE && fabs(o.y) <= RB_PLAIN_ABOVE && fabs(o.z) <= RB_PLAIN_ABOVE && fabs(d.x) <= RB_PLAIN_ABOVE &&
                       fabs(d.y) <= RB_PLAIN_ABOVE && fabs(d.z) <= RB_PLAIN_ABOVE;
    RayBound rb;
    rb.cull = small && dd > EPS && dd < INFINITY;
    rb.ball = Ball{o.x, o.y, o.z, 0.0};
    rb.dir.sdir[0] = d.x;
    rb.dir.sdir[1] = d.y;
    rb.dir.sdir[2] = d.z;
    rb.dir.inv_uu = dd > 0.0 ? 1.0 / dd : 0.0;
    rb.dir.len_u = 1.001 * sqrt(dd);
    rb.dir.p[0] = rb.dir.p[1] = rb.dir.p[2] = 0.0;
    return rb;
}

__device__ __forceinline__ bool ray_reaches(const UsEntry &bound, const RayBound &rb)
{
    return !rb.cull || sphere_relevant<false>(bound, rb.ball, rb.dir);
}

__device__ __forceinline__ bool ray_reaches(const UsEntry &bound, const D3 &o, const D3 &d)
{
    return ray_reaches(bound, ray_bound(o, d));
}

} // namespace rtm

#endif
