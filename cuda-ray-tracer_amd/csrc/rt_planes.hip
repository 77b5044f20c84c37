// rt_planes.hip -- root-side helpers of the multi-GPU layer for data that is not a frame (include/mi355rt.h, rt_assemble_planes and
// rt_merge_object_extents): the reassembly of a gathered plane of 4-, 8- or 16-byte elements into row order (the G-buffer's object, t
// and normal planes; rt_assemble only knows the two pixel formats) and the merge of several ranks' object-extent records.
//
// Compiled ONCE, with -ffp-contract=off, like rt_resolve.hip: there is no floating-point arithmetic in this file at all -- elements are
// moved as integers of their size, and t_min / t_max are compared as the unsigned integers of their bits, as the reduction kernel
// does (t is in [1e-7, 1e6), +inf and +0.0 are the identities: the bits order as the doubles do).  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include <cstdint>

namespace {

// Element i = (y, x) of the full plane comes from rank r = band % world, local row lr: the mapping of assemble_kernel (rt_kernels.hip)
// and of rt_row_map.  One element per lane and step -- a 4-, 8- or 16-byte vector load and store --, consecutive lanes on consecutive
// elements of a row; grid-stride over the plane.  slot_stride counts elements.
template <typename E>
__global__ __launch_bounds__(256) void assemble_planes_kernel(const E *__restrict__ gathered, size_t slot_stride, E *__restrict__ full, uint32_t width, uint32_t height,
                                                              uint32_t world, uint32_t band_rows)
{
    const size_t n = (size_t) width * height;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t) (i / width), x = (uint32_t) (i - (size_t) y * width);
        const uint32_t band = y / band_rows, r = band % world;
        const uint32_t lr = (band / world) * band_rows + (y - band * band_rows);
        full[i] = gathered[(size_t) r * slot_stride + (size_t) lr * width + x];
    }
}

// rt_object_extent as five 8-byte words: pixels | x_min, y_min | x_max, y_max | bits of t_min | bits of t_max
constexpr uint32_t REC_WORDS = 5u;

__device__ __forceinline__ uint32_t lo32(uint64_t v) { return (uint32_t) v; }
__device__ __forceinline__ uint32_t hi32(uint64_t v) { return (uint32_t) (v >> 32); }
__device__ __forceinline__ uint64_t pack32(uint32_t lo, uint32_t hi) { return (uint64_t) lo | ((uint64_t) hi << 32); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// One lane per object, grid-stride over the objects; the parts are read one after another, each record as five 8-byte loads.  The
// accumulators start from the reduction identities, so all-identity input gives the identity record bit for bit.
__global__ __launch_bounds__(256) void merge_extents_kernel(const uint64_t *__restrict__ parts, uint32_t n_parts, uint32_t n_obj, uint64_t *__restrict__ out)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_obj; i += (size_t) gridDim.x * blockDim.x) {
        uint64_t pixels = 0u;
        uint32_t x_min = 0xFFFFFFFFu, y_min = 0xFFFFFFFFu, x_max = 0u, y_max = 0u;
        uint64_t t_min = 0x7FF0000000000000ull, t_max = 0u; // +inf, +0.0
        for (uint32_t p = 0; p < n_parts; p++) {
            const uint64_t *rec = parts + ((size_t) p * n_obj + i) * REC_WORDS;
            const uint64_t w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4];
            pixels += w0;
            x_min = umin(x_min, lo32(w1));
            y_min = umin(y_min, hi32(w1));
            x_max = umax(x_max, lo32(w2));
            y_max = umax(y_max, hi32(w2));
            t_min = w3 < t_min ? w3 : t_min;
            t_max = w4 > t_max ? w4 : t_max;
        }
        uint64_t *dst = out + i * REC_WORDS;
        dst[0] = pixels;
        dst[1] = pack32(x_min, y_min);
        dst[2] = pack32(x_max, y_max);
        dst[3] = t_min;
        dst[4] = t_max;
    }
}

uint32_t blocks_for(size_t n) { return (uint32_t) ((n + 255u) / 256u < 4096u ? (n + 255u) / 256u : 4096u); }

} // namespace

// gathered + r * slot_stride elements = rank r's [max_local_rows][width] elements; full = [height][width] elements (elem_bytes = 4, 8, 16)
extern "C" hipError_t rt_launch_assemble_planes(const void *gathered, size_t slot_stride, void *full, uint32_t width, uint32_t height, uint32_t world, uint32_t band_rows,
                                                uint32_t elem_bytes, hipStream_t stream)
{
    const size_t n = (size_t) width * height;
    if (n == 0u) return hipSuccess;
    if (world == 0u || band_rows == 0u) return hipErrorInvalidValue;
    const dim3 grid(blocks_for(n)), block(256);
    if (elem_bytes == 4u)
        hipLaunchKernelGGL(assemble_planes_kernel<uint32_t>, grid, block, 0, stream, (const uint32_t *) gathered, slot_stride, (uint32_t *) full, width, height, world, band_rows);
    else if (elem_bytes == 8u)
        hipLaunchKernelGGL(assemble_planes_kernel<uint2>, grid, block, 0, stream, (const uint2 *) gathered, slot_stride, (uint2 *) full, width, height, world, band_rows);
    else if (elem_bytes == 16u)
        hipLaunchKernelGGL(assemble_planes_kernel<uint4>, grid, block, 0, stream, (const uint4 *) gathered, slot_stride, (uint4 *) full, width, height, world, band_rows);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// parts = [n_parts][n_obj] records of 40 bytes, out = [n_obj] records
extern "C" hipError_t rt_launch_merge_extents(const void *parts, uint32_t n_parts, uint32_t n_obj, void *out, hipStream_t stream)
{
    if (n_obj == 0u) return hipSuccess;
    if (n_parts == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_extents_kernel, dim3(blocks_for(n_obj)), dim3(256), 0, stream, (const uint64_t *) parts, n_parts, n_obj, (uint64_t *) out);
    return hipGetLastError();
}
