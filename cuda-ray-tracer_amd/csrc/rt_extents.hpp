// rt_extents.hpp -- what the two object-extents kernels share (rt_gbuffer.hip: extents_kernel, the class tables staged in LDS;
// rt_stream_queries.hip: extents_stream_kernel, the tables streamed) besides their body (rt_pixel_kernels.hpp: pk_extents): the record
// as the kernels update it, its identity and the kernel that writes it, the merge, the reduction of a wave's 8 x 8 block into the
// accumulators or the output records, and what a launcher derives from the caller's rectangle.  Included behind rt_shade.hpp
// (global_row) by files that are compiled once per variant (-DRT_VARIANT=strict|fast); everything lives in that variant's namespace.
#ifndef RT_EXTENTS_HPP
#define RT_EXTENTS_HPP

#include <hip/hip_runtime.h>

#include "rt_shade.hpp" // RT_SYM and the variant's namespace, global_row

namespace RT_SYM(rtk) {

// One rt_object_extent as the kernels update it: t_min / t_max as the bits of the double (t is in [1e-7, 1e6), so the bits order as
// unsigned integers and +inf / +0.0 are the identities of min / max).
struct ExtRecord {
    unsigned long long pixels;
    uint32_t x_min, y_min, x_max, y_max;
    unsigned long long t_min, t_max;
};
static_assert(sizeof(ExtRecord) == 40, "rt_object_extent layout");
#define RT_EXT_INF_BITS 0x7FF0000000000000ull

// the record of an object no pixel shows: the identity of ext_merge
__device__ __forceinline__ ExtRecord ext_identity() { return ExtRecord{0ull, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, RT_EXT_INF_BITS, 0ull}; }

// The kernel that sets the n output records to the identity, one record per thread, 256-thread workgroups.  Written once; each of the
// two files defines it under the name its launcher and the build's resource report use.
#define EXT_INIT_KERNEL(name)                                                                      \
    __global__ __launch_bounds__(256) void name(ExtRecord *__restrict__ out, uint32_t n)           \
    {                                                                                              \
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;                                        \
        if (i < n) out[i] = ext_identity();                                                        \
    }

// what the launcher derives from the rectangle: its columns, this rank's LOCAL rows inside it, and the tiles that meet both
struct ExtArgs {
    uint32_t x0, x1, lr0, lr1; // inclusive
    uint32_t tx0, ty0, ntx;    // first tile column / tile row, tile columns
    uint32_t n_tiles;          // tiles to trace
    uint32_t lds_acc;          // 1: one ExtRecord per object in LDS behind the tables, flushed once per workgroup; 0: every wave updates `out`
};

// merge one partial record into r: seven atomics whose result does not depend on their order
template <int SCOPE>
__device__ __forceinline__ void ext_merge(ExtRecord *r, unsigned long long n, uint32_t x_min, uint32_t y_min, uint32_t x_max, uint32_t y_max, unsigned long long t_min,
                                          unsigned long long t_max)
{
    __hip_atomic_fetch_add(&r->pixels, n, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_min(&r->x_min, x_min, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_min(&r->y_min, y_min, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_max(&r->x_max, x_max, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_max(&r->y_max, y_max, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_min(&r->t_min, t_min, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_fetch_max(&r->t_max, t_max, __ATOMIC_RELAXED, SCOPE);
}

// One wave, one 8 x 8 block whose first column is bx and first local row blr: the lanes in `counted` hit object `best` at best_t.  One
// turn per distinct object among them (wave-uniform): count = popcount of their ballot, the box from the ballot's rows and columns, t by
// a butterfly; lane 0 merges that into the workgroup's accumulators in LDS (acc != NULL, launch-uniform: one record per object, which
// the workgroup adds to `out` at its end) or into `out` itself.  Every lane of the wave must call.
__device__ __forceinline__ void ext_reduce_wave(const FrameArgs &fa, uint32_t bx, uint32_t blr, uint32_t lane, bool counted, int best, double best_t,
                                                ExtRecord *__restrict__ out, ExtRecord *acc)
{
    const unsigned long long tb = (unsigned long long) __double_as_longlong(best_t);
    unsigned long long todo = __ballot(counted);
    while (todo) { // wave-uniform: one turn per distinct object among the counted lanes
        const int id = __builtin_amdgcn_readlane(best, __builtin_ctzll(todo));
        const bool mine = counted && best == id;
        const unsigned long long mask = __ballot(mine); // bit 8 r + c: row r, column c of the block
        todo &= ~mask;
        unsigned long long lo = mine ? tb : RT_EXT_INF_BITS, hi = mine ? tb : 0ull;
#pragma unroll
        for (int s = 32; s; s >>= 1) {
            const unsigned long long l2 = __shfl_xor(lo, s), h2 = __shfl_xor(hi, s);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0u) {
            uint32_t cols = (uint32_t) mask | (uint32_t) (mask >> 32);
            cols |= cols >> 16;
            cols = (cols | (cols >> 8)) & 0xFFu;
            const uint32_t x_min = bx + (uint32_t) __builtin_ctz(cols), x_max = bx + 31u - (uint32_t) __builtin_clz(cols);
            const uint32_t y_min = global_row(fa, blr + ((uint32_t) __builtin_ctzll(mask) >> 3)); // (global_row rises with the local row)
            const uint32_t y_max = global_row(fa, blr + ((63u - (uint32_t) __builtin_clzll(mask)) >> 3));
            const unsigned long long n = (unsigned long long) __builtin_popcountll(mask);
            if (acc) ext_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(acc + id, n, x_min, y_min, x_max, y_max, lo, hi);
            else ext_merge<__HIP_MEMORY_SCOPE_AGENT>(out + id, n, x_min, y_min, x_max, y_max, lo, hi);
        }
    }
}

// rect = x0, y0, x1, y1 (inclusive, inside the image, GLOBAL rows) -> the columns, this rank's local rows inside it and the tiles that
// meet both; false when no row of the rectangle is this rank's.  lds_acc is left to the launcher.
static inline bool ext_args(const FrameArgs *fa, const uint32_t *rect, ExtArgs &ea)
{
    // this rank's local rows inside [y0, y1]: the global row rises with the local one
    const auto grow = [&](uint32_t lr) { const uint32_t b = lr / fa->band_rows; return (uint64_t) (b * (uint64_t) fa->world + fa->rank) * fa->band_rows + (lr - b * fa->band_rows); };
    const auto first_at_least = [&](uint64_t y) { // the first local row whose global row is >= y (local_rows if none)
        uint32_t lo = 0, hi = fa->local_rows;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (grow(mid) >= y) hi = mid;
            else lo = mid + 1u;
        }
        return lo;
    };
    const uint32_t lr_lo = first_at_least(rect[1]), lr_end = first_at_least((uint64_t) rect[3] + 1u);
    if (lr_lo >= lr_end) return false;
    ea.x0 = rect[0];
    ea.x1 = rect[2];
    ea.lr0 = lr_lo;
    ea.lr1 = lr_end - 1u;
    ea.tx0 = ea.x0 / 16u;
    ea.ty0 = ea.lr0 / 16u;
    ea.ntx = ea.x1 / 16u - ea.tx0 + 1u;
    ea.n_tiles = ea.ntx * (ea.lr1 / 16u - ea.ty0 + 1u);
    ea.lds_acc = 0u;
    return true;
}

} // namespace RT_SYM(rtk)

#endif
