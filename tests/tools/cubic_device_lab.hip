// cubic_device_lab.hip -- the degree-3 path of rt_math.hpp on gfx950, one ray at a time (test infrastructure).
// The kernels' own header, compiled with the strict variant's flags (cuda-ray-tracer_amd/Makefile: DEVFLAGS -ffp-contract=off), in a
// plain kernel per entry point.  Each entry point allocates, copies, launches, synchronises and frees by itself and returns the HIP
// status (0: success).  Built and driven by tests/tools/cubic_device_lab.py; the ray records come from the oracle
// (tests/tools/cubic_guard_lab.cpp, lab_enumerate).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mi355rt.h"
#include "rt_math.hpp"
#include "cubic_lab_rays.h"

using namespace rtm;

struct LabOut {
    double t;          // intersect_cubic_taylor: what both kernels use
    double t_dense;    // intersect_cubic_branch: the dense expansion and the reference's solver
    double t_guard;    // cubic_guarded by itself (meaningful where guard_ok)
    double tc[4];      // the Taylor coefficients t3 .. t0 the guard saw
    int32_t refused;   // intersect_cubic_taylor took the dense path
    int32_t branch;    // of the dense path: 0 Cardano, 1 trigonometric, 2 quadratic, 3 linear / constant
    int32_t guard_ok;
    int32_t pad;
};
static_assert(sizeof(LabOut) == 72, "layout restated in cubic_device_lab.py");

__global__ void k_libm(int fn, const double *x, uint32_t n, double *y)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    y[i] = fn == 0 ? cbrt(v) : fn == 1 ? acos(v) : cos(v); // (solve_cubic's calls)
}

__global__ void k_rays(const double *coefs, const LabRay *rays, uint32_t n, LabOut *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LabRay &r = rays[i];
    const double *c = coefs + (size_t) r.obj * RT_NCOEF;
    const D3 o{r.o[0], r.o[1], r.o[2]}, d{r.d[0], r.d[1], r.d[2]};
    const bool decide = (r.flags & LAB_DECIDE) != 0;
    const CubicAt ca = (r.flags & LAB_HAS_REC) ? CubicAt{r.rec[0], r.rec[1], r.rec[2], r.rec[3], r.rec[4], r.rec[5], r.rec[6], r.rec[7], r.rec[8], r.rec[9]}
                                               : cubic_at(c, o);
    const CubicMag mo = cubic_mag_origin(cubic_abs(c), o);
    LabOut q;
    bool refused = false;
    q.t = intersect_cubic_taylor(c, ca, mo, o, d, r.max_t, decide, refused);
    q.refused = refused ? 1 : 0;
    int branch = -1;
    q.t_dense = intersect_cubic_branch(c, o.x, o.y, o.z, d.x, d.y, d.z, branch);
    q.branch = branch;
    double t3, t2, t1, t0, tg = 0.0;
    cubic_coefs(c, ca, d, t3, t2, t1, t0);
    q.guard_ok = cubic_guarded(t3, t2, t1, t0, cubic_mag_dir(mo, fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z))), r.max_t, decide, tg) ? 1 : 0;
    q.t_guard = tg;
    q.tc[0] = t3;
    q.tc[1] = t2;
    q.tc[2] = t1;
    q.tc[3] = t0;
    q.pad = 0;
    out[i] = q;
}

// case: t3, t2, t1, t0, m3, m2, m1, m0, max_t, decide (10 doubles) -> ok, t
__global__ void k_guard(const double *cases, uint32_t n, double *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *a = cases + (size_t) i * 10;
    double t = 0.0;
    const bool ok = cubic_guarded(a[0], a[1], a[2], a[3], CubicMag{a[4], a[5], a[6], a[7]}, a[8], a[9] != 0.0, t);
    out[2 * (size_t) i] = ok ? 1.0 : 0.0;
    out[2 * (size_t) i + 1] = t;
}

namespace {
struct Buffers { // device buffers of one call, freed on every way out
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Buffers()
    {
        for (void *q : p)
            if (q) (void) hipFree(q);
    }
};
#define LAB_TRY(x)                                                                                                                    \
    do {                                                                                                                              \
        const hipError_t e_ = (x);                                                                                                    \
        if (e_ != hipSuccess) return (int) e_;                                                                                        \
    } while (0)

int finish_launch()
{
    LAB_TRY(hipGetLastError());
    LAB_TRY(hipDeviceSynchronize());
    return 0;
}
constexpr uint32_t BLOCK = 256;
} // namespace

extern "C" int lab_libm(int fn, const double *x, uint64_t n, double *y)
{
    if (fn < 0 || fn > 2 || n >= (1ull << 31)) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    Buffers b;
    LAB_TRY(hipMalloc(&b.p[0], n * sizeof(double)));
    LAB_TRY(hipMalloc(&b.p[1], n * sizeof(double)));
    LAB_TRY(hipMemcpy(b.p[0], x, n * sizeof(double), hipMemcpyHostToDevice));
    k_libm<<<(uint32_t) ((n + BLOCK - 1) / BLOCK), BLOCK>>>(fn, (const double *) b.p[0], (uint32_t) n, (double *) b.p[1]);
    if (int e = finish_launch()) return e;
    LAB_TRY(hipMemcpy(y, b.p[1], n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lab_rays(const double *coefs, uint32_t n_obj, const LabRay *rays, uint64_t n, LabOut *out)
{
    if (n >= (1ull << 31) || n_obj == 0) return (int) hipErrorInvalidValue;
    for (uint64_t i = 0; i < n; i++) // (every record names an object that exists)
        if (rays[i].obj < 0 || (uint32_t) rays[i].obj >= n_obj) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    Buffers b;
    LAB_TRY(hipMalloc(&b.p[0], (size_t) n_obj * RT_NCOEF * sizeof(double)));
    LAB_TRY(hipMalloc(&b.p[1], n * sizeof(LabRay)));
    LAB_TRY(hipMalloc(&b.p[2], n * sizeof(LabOut)));
    LAB_TRY(hipMemcpy(b.p[0], coefs, (size_t) n_obj * RT_NCOEF * sizeof(double), hipMemcpyHostToDevice));
    LAB_TRY(hipMemcpy(b.p[1], rays, n * sizeof(LabRay), hipMemcpyHostToDevice));
    k_rays<<<(uint32_t) ((n + BLOCK - 1) / BLOCK), BLOCK>>>((const double *) b.p[0], (const LabRay *) b.p[1], (uint32_t) n, (LabOut *) b.p[2]);
    if (int e = finish_launch()) return e;
    LAB_TRY(hipMemcpy(out, b.p[2], n * sizeof(LabOut), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lab_guard(const double *cases, uint64_t n, double *out)
{
    if (n >= (1ull << 31)) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    Buffers b;
    LAB_TRY(hipMalloc(&b.p[0], n * 10 * sizeof(double)));
    LAB_TRY(hipMalloc(&b.p[1], n * 2 * sizeof(double)));
    LAB_TRY(hipMemcpy(b.p[0], cases, n * 10 * sizeof(double), hipMemcpyHostToDevice));
    k_guard<<<(uint32_t) ((n + BLOCK - 1) / BLOCK), BLOCK>>>((const double *) b.p[0], (uint32_t) n, (double *) b.p[1]);
    if (int e = finish_launch()) return e;
    LAB_TRY(hipMemcpy(out, b.p[1], n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
