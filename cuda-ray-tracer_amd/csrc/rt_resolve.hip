// rt_resolve.hip -- supersampling resolve for gfx950: box filter of the internal k-times finer RGBA32F frame into the output
// frame (include/mi355rt.h, RT_FLAG_SSAA2 / RT_FLAG_SSAA4).
//
// Compiled ONCE, with -ffp-contract=off: the resolve is part of the image's definition (a pairwise float32 tree per sub-row, the
// same tree over the sub-rows, one multiplication by 1/k^2, then the render kernels' quantisation), so a FAST context resolves
// exactly as a strict one does.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include <cstdint>

namespace {

// One sample, one global_load_dwordx4.  Alpha is not resolved (the output's is 1.0f / 255), so the compiler would narrow the load to
// dwordx3; the empty asm makes the w lane live and keeps the access 16 bytes wide and 16-byte aligned.
template <bool NT>
__device__ __forceinline__ float4 load16(const float4 *p)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f *q = reinterpret_cast<const v4f *>(p);
    v4f v;
    if constexpr (NT) v = __builtin_nontemporal_load(q);
    else v = *q;
    float w = v.w;
    asm volatile("" : "+v"(w));
    return make_float4(v.x, v.y, v.z, w);
}

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// pairwise tree over the k samples of one sub-row: k = 2: s0 + s1; k = 4: (s0 + s1) + (s2 + s3)
template <int K, bool NT>
__device__ __forceinline__ float4 row_sum(const float4 *p)
{
    if constexpr (K == 2) {
        return add4(load16<NT>(p), load16<NT>(p + 1));
    } else {
        const float4 s0 = load16<NT>(p), s1 = load16<NT>(p + 1), s2 = load16<NT>(p + 2), s3 = load16<NT>(p + 3);
        return add4(add4(s0, s1), add4(s2, s3));
    }
}

// One lane per output pixel; a block covers 256 consecutive pixels of one output row (blockIdx.y = local output row).  A lane reads
// its k contiguous 16-byte samples from each of the k internal rows k*lr .. k*lr + k - 1 of this rank's local rows (internal local
// row k*lr + j is internal global row k*y + j: internal bands are k times as tall), so a wave reads 64 * k * 16 contiguous bytes
// per sub-row; every pixel is written once, as one float4 or uchar4.
template <int K, bool RGBA8, bool NT>
__global__ __launch_bounds__(256) void resolve_kernel(const float4 *__restrict__ in, void *__restrict__ out, uint32_t width)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, lr = blockIdx.y;
    if (x >= width) return;
    const size_t in_w = (size_t) K * width;
    const float4 *p = in + ((size_t) K * lr) * in_w + (size_t) K * x;
    float4 r[K];
#pragma unroll
    for (int j = 0; j < K; j++) r[j] = row_sum<K, NT>(p + (size_t) j * in_w);
    const float4 s = K == 2 ? add4(r[0], r[1]) : add4(add4(r[0], r[1]), add4(r[2], r[3]));
    constexpr float inv = 1.0f / (float) (K * K); // 0.25f / 0.0625f, exact
    const float vx = s.x * inv, vy = s.y * inv, vz = s.z * inv;
    const size_t o = (size_t) lr * width + x;
    if constexpr (RGBA8) {
        uchar4 px;
        px.x = (unsigned char) (int) (vx * 255.0f + 0.5f);
        px.y = (unsigned char) (int) (vy * 255.0f + 0.5f);
        px.z = (unsigned char) (int) (vz * 255.0f + 0.5f);
        px.w = 255;
        reinterpret_cast<uchar4 *>(out)[o] = px;
    } else {
        reinterpret_cast<float4 *>(out)[o] = make_float4(vx, vy, vz, 1.0f);
    }
}

template <int K, bool NT>
void launch(const float4 *in, void *out, uint32_t width, uint32_t rows, int rgba8, hipStream_t stream)
{
    const dim3 grid((width + 255u) / 256u, rows), block(256);
    if (rgba8)
        hipLaunchKernelGGL((resolve_kernel<K, true, NT>), grid, block, 0, stream, in, out, width);
    else
        hipLaunchKernelGGL((resolve_kernel<K, false, NT>), grid, block, 0, stream, in, out, width);
}

} // namespace

// in = [k * rows][k * width] float4 (a context's internal local rows), out = [rows][width] pixels (rgba8: uchar4, else float4).
// nt: read the internal frame with non-temporal loads.
extern "C" hipError_t rt_launch_resolve(const void *in, void *out, uint32_t width, uint32_t rows, uint32_t k, int rgba8, int nt, hipStream_t stream)
{
    if (width == 0u || rows == 0u) return hipSuccess;
    if (rows > 65535u || (k != 2u && k != 4u)) return hipErrorInvalidValue;
    const float4 *src = (const float4 *) in;
    if (k == 2u) {
        if (nt) launch<2, true>(src, out, width, rows, rgba8, stream);
        else launch<2, false>(src, out, width, rows, rgba8, stream);
    } else {
        if (nt) launch<4, true>(src, out, width, rows, rgba8, stream);
        else launch<4, false>(src, out, width, rows, rgba8, stream);
    }
    return hipGetLastError();
}
