// cull_device_lab.hip -- the predicates of rt_wavefront_math.hpp on the device, over the records of tests/tools/cull_lab.cpp (test infrastructure).
// One record per lane, plain loads and stores; the calls are those of tests/tools/cull_lab_records.h, the same the host lab makes, so a
// verdict or a cull_record field that differs from the host's shows a device sqrt, a contraction or a reordering that the host build lacks.
// Built at test time by tests/tools/cull_device_lab.py with the kernels' own flags; CULL_LAB_SUFFIX names the variant's entry points.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rt_wavefront_math.hpp"
#include "cull_lab_records.h"

using namespace rtm;

// kind: 0 cone, 1 pyramid, 2 shadow (crec [6 n] too), 3 us_needs_solve, 4 needs_solve
template <int KIND>
__global__ __launch_bounds__(256) void eval_kernel(const double *__restrict__ rec, uint64_t n, int32_t *__restrict__ verdict, double *__restrict__ crec)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int W = KIND == 0 ? REC_CONE : KIND == 1 ? REC_PYR : KIND == 2 ? REC_SH : KIND == 3 ? REC_US : REC_GQ;
    double r[W];
    for (int k = 0; k < W; k++) r[k] = rec[i * W + k];
    int v;
    if (KIND == 0) v = eval_cone(r);
    else if (KIND == 1) v = eval_pyr(r);
    else if (KIND == 2) {
        double c[6];
        v = eval_sh(r, c);
        for (int k = 0; k < 6; k++) crec[i * 6 + k] = c[k];
    } else if (KIND == 3) v = eval_us(r);
    else v = eval_gq(r);
    verdict[i] = v;
}

#define LAB_TRY(x)                          \
    do {                                    \
        hipError_t e_ = (x);                \
        if (e_ != hipSuccess) {             \
            status = (int) e_;              \
            goto done;                      \
        }                                   \
    } while (0)

// One launch over n records of one kind.  Returns 0 or the HIP error.
extern "C" int lab_device_eval(int kind, const double *rec, uint64_t n, int32_t *verdict, double *crec)
{
    static const int width[5] = {REC_CONE, REC_PYR, REC_SH, REC_US, REC_GQ};
    if (kind < 0 || kind > 4) return -1;
    if (n == 0) return 0;
    int status = 0;
    double *d_rec = nullptr, *d_crec = nullptr;
    int32_t *d_v = nullptr;
    const unsigned blocks = (unsigned) ((n + 255) / 256);
    LAB_TRY(hipMalloc(&d_rec, n * width[kind] * sizeof(double)));
    LAB_TRY(hipMalloc(&d_v, n * sizeof(int32_t)));
    LAB_TRY(hipMalloc(&d_crec, n * 6 * sizeof(double)));
    LAB_TRY(hipMemcpy(d_rec, rec, n * width[kind] * sizeof(double), hipMemcpyHostToDevice));
    LAB_TRY(hipMemset(d_crec, 0, n * 6 * sizeof(double)));
    switch (kind) {
    case 0: eval_kernel<0><<<blocks, 256>>>(d_rec, n, d_v, d_crec); break;
    case 1: eval_kernel<1><<<blocks, 256>>>(d_rec, n, d_v, d_crec); break;
    case 2: eval_kernel<2><<<blocks, 256>>>(d_rec, n, d_v, d_crec); break;
    case 3: eval_kernel<3><<<blocks, 256>>>(d_rec, n, d_v, d_crec); break;
    default: eval_kernel<4><<<blocks, 256>>>(d_rec, n, d_v, d_crec); break;
    }
    LAB_TRY(hipGetLastError());
    LAB_TRY(hipDeviceSynchronize());
    LAB_TRY(hipMemcpy(verdict, d_v, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (crec) LAB_TRY(hipMemcpy(crec, d_crec, n * 6 * sizeof(double), hipMemcpyDeviceToHost));
done:
    (void) hipFree(d_rec);
    (void) hipFree(d_v);
    (void) hipFree(d_crec);
    return status;
}
