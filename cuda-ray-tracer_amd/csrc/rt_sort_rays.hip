// rt_sort_rays.hip -- rt_sort_rays and rt_permute (include/mi355rt.h, "Sorting rays"): caller-supplied rays ordered on
// the device by rtm::ray_sort_key (rt_ray_sort_key.hpp), so that the 64 consecutive rays a wave of the culled ray kernels
// (RT_FLAG_STREAM_CULL_RAYS) takes reach the same few chunk bounds; and the gathers and scatters that carry t_max into that order and
// hits, flags, colours and path records back into the caller's.
//
// Compiled ONCE, with -ffp-contract=off, like rt_planes.hip: the key is part of the result's definition (the order), not of a variant,
// and the host reproduces it (tests/tools/ray_sort_lab.cpp).  No scene state, no allocation, no host read-back: every launch below is
// decided by n alone, so a captured graph stays valid for any rays of the same count.
//
// Stages (the work space's layout is sort_layout's):
//   box      init_box_kernel sets the six box words to the reduction identities; box_kernel reduces the class-0 origins of a workgroup's
//            rays and merges them with 64-bit integer minimum / maximum atomics on the order-preserving image of the doubles' bits
//            (rsk_image): minimum and maximum do not depend on the order of arrival.
//   keys     keys_kernel: one lane per ray, key[i] and idx[i] = i.
//   sort     a stable LSD radix sort of the (key, idx) pairs, four passes of 8-bit digits.  Per pass: histogram_kernel counts a tile's
//            digits into table[digit][tile]; the exclusive scan of that digit-major table (reduce_chunks_kernel up the levels, scan_chunks_kernel
//            down them) turns the counts into the first place of every (digit, tile); scatter_kernel ranks a tile's pairs in input
//            order -- a round of 256 consecutive pairs after the other, inside a round wave after wave (their counts ordered through
//            LDS), inside a wave by a match of the digit over ballots -- and stores them.  The only atomics are the histogram's integer
//            adds in LDS, whose sum does not depend on their order.  A place is table + counts of pairs that exist, so it is below n by
//            construction: the histogram and the scatter read the same pairs.
//   gather   gather_rays_kernel: sorted[i] = rays[perm[i]], three 16-byte loads and stores per lane.
// rt_permute's kernel moves planes x n records of 16-byte vectors, or of 4-byte words, either way round.
//
// Grids: one workgroup per 256 rays, per tile or per scan chunk, at most max_grid of them, each looping with a workgroup-uniform trip
// count (the rule of rt_ray_kernels.hpp).  Indices are size_t throughout: n goes up to 2^32 - 1.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launchers below, as the host sees them
#include "rt_ray_sort_key.hpp"
#include <cstdint>

using namespace rtm;

namespace {

uint32_t grid_for(size_t items, uint32_t max_grid) { return (uint32_t) (items < max_grid ? items : (max_grid ? max_grid : 1u)); }

// ---- rays ---------------------------------------------------------------------------------------------------------------------------------
// a ray is three 16-byte vectors here as in the gather; the six doubles are their halves
__device__ __forceinline__ void load_ray(const uint4 *__restrict__ rays, size_t i, D3 &o, D3 &d)
{
    const uint4 *v = rays + 3u * i;
    const uint4 a = v[0], b = v[1], c = v[2];
    o = D3{__hiloint2double((int) a.y, (int) a.x), __hiloint2double((int) a.w, (int) a.z), __hiloint2double((int) b.y, (int) b.x)};
    d = D3{__hiloint2double((int) b.w, (int) b.z), __hiloint2double((int) c.y, (int) c.x), __hiloint2double((int) c.w, (int) c.z)};
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ---- box ----------------------------------------------------------------------------------------------------------------------------------
// box words: [0..2] the images of lo, [3..5] the images of hi
__global__ __launch_bounds__(64) void init_box_kernel(unsigned long long *__restrict__ box)
{
    if (threadIdx.x < 6u) box[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFFFFFFFFFull : 0ull;
}

__global__ __launch_bounds__(RS_THREADS) void box_kernel(const uint4 *__restrict__ rays, size_t n, unsigned long long *__restrict__ box)
{
    __shared__ uint64_t part[RS_WAVES][6];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t acc[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    for (size_t first = (size_t) blockIdx.x * RS_THREADS; first < n; first += (size_t) gridDim.x * RS_THREADS) {
        const size_t i = first + tid;
        if (i < n) {
            D3 o, d;
            load_ray(rays, i, o, d);
            if (ray_sort_class0(o, d)) {
                const double oc[3] = {o.x + 0.0, o.y + 0.0, o.z + 0.0};
                for (int a = 0; a < 3; a++) {
                    const uint64_t img = rsk_image((uint64_t) __double_as_longlong(oc[a]));
                    acc[a] = umin64(acc[a], img);
                    acc[3 + a] = umax64(acc[3 + a], img);
                }
            }
        }
    }
    for (int a = 0; a < 6; a++) {
        uint64_t v = acc[a];
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t other = (uint64_t) __shfl_xor((unsigned long long) v, off, 64);
            v = a < 3 ? umin64(v, other) : umax64(v, other);
        }
        if (lane == 0u) part[wave][a] = v;
    }
    __syncthreads();
    if (tid < 6u) {
        uint64_t v = part[0][tid];
        for (uint32_t w = 1; w < RS_WAVES; w++) v = tid < 3u ? umin64(v, part[w][tid]) : umax64(v, part[w][tid]);
        if (tid < 3u)
            atomicMin(box + tid, (unsigned long long) v);
        else
            atomicMax(box + tid, (unsigned long long) v);
    }
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void keys_kernel(const uint4 *__restrict__ rays, size_t n, const unsigned long long *__restrict__ box_words,
                                                          uint32_t *__restrict__ keys, uint32_t *__restrict__ idx)
{
    RayKeyBox box;
    for (int a = 0; a < 3; a++) {
        box.lo[a] = __longlong_as_double((long long) rsk_unimage(box_words[a]));
        box.hi[a] = __longlong_as_double((long long) rsk_unimage(box_words[3 + a]));
    }
    for (size_t i = (size_t) blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += (size_t) gridDim.x * RS_THREADS) {
        D3 o, d;
        load_ray(rays, i, o, d);
        keys[i] = ray_sort_key(o, d, box);
        idx[i] = (uint32_t) i;
    }
}

// ---- one pass of the sort -------------------------------------------------------------------------------------------------------------------
// table[digit * tiles + tile] = how many of the tile's keys have that digit
__global__ __launch_bounds__(RS_THREADS) void histogram_kernel(const uint32_t *__restrict__ keys, size_t n, size_t tiles, uint32_t shift, uint32_t *__restrict__ table)
{
    __shared__ uint32_t hist[RS_DIGITS];
    const uint32_t tid = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        hist[tid] = 0u;
        __syncthreads();
        const size_t base = tile * RS_TILE;
        for (uint32_t j = 0; j < RS_ITEMS; j++) {
            const size_t i = base + (size_t) j * RS_THREADS + tid;
            if (i < n) atomicAdd(&hist[(keys[i] >> shift) & (RS_DIGITS - 1u)], 1u); // (an integer sum: the order of arrival does not show)
        }
        __syncthreads();
        table[(size_t) tid * tiles + tile] = hist[tid];
        __syncthreads();
    }
}

// the exclusive scan of one value per lane over the workgroup; total: the sum of all 256
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t) off) incl += up;
    }
    if (lane == 63u) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
    for (uint32_t w = 0; w < RS_WAVES; w++) {
        const uint32_t s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads(); // (wave_sums is free again)
    return before + incl - v;
}

// sums[chunk] = the sum of the chunk's entries of data[0 .. len)
__global__ __launch_bounds__(RS_THREADS) void reduce_chunks_kernel(const uint32_t *__restrict__ data, size_t len, size_t chunks, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wave_sums[RS_WAVES];
    const uint32_t tid = threadIdx.x;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const size_t at = chunk * RS_SCAN_CHUNK + (size_t) tid * RS_SCAN_ITEMS;
        uint32_t s = 0u;
        for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++)
            if (at + k < len) s += data[at + k];
        uint32_t total;
        block_exclusive_scan(s, wave_sums, total);
        if (tid == 0u) sums[chunk] = total;
    }
}

// data[0 .. len) becomes its exclusive scan: chunk by chunk, each from offs[chunk] (the scanned level above; NULL: one chunk, from 0)
__global__ __launch_bounds__(RS_THREADS) void scan_chunks_kernel(uint32_t *__restrict__ data, size_t len, size_t chunks, const uint32_t *__restrict__ offs)
{
    __shared__ uint32_t wave_sums[RS_WAVES];
    const uint32_t tid = threadIdx.x;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const size_t at = chunk * RS_SCAN_CHUNK + (size_t) tid * RS_SCAN_ITEMS;
        uint32_t v[RS_SCAN_ITEMS], s = 0u;
        for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++) {
            v[k] = at + k < len ? data[at + k] : 0u;
            s += v[k];
        }
        uint32_t total;
        uint32_t run = block_exclusive_scan(s, wave_sums, total) + (offs ? offs[chunk] : 0u);
        for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++) {
            if (at + k < len) data[at + k] = run;
            run += v[k];
        }
    }
}

// The tile's pairs to their places.  Round j takes the pairs base + j * 256 + tid; sub-block (j, wave) is 64 consecutive pairs.  count[j * 4
// + wave][digit] first holds how many pairs of the sub-block have the digit (written by the lowest lane that has it), then -- one lane per
// digit running over the sub-blocks in input order from table[digit][tile] -- the place of the sub-block's first such pair.
__global__ __launch_bounds__(RS_THREADS) void scatter_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ idx_in, size_t n, size_t tiles, uint32_t shift,
                                                             const uint32_t *__restrict__ table, uint32_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out)
{
    __shared__ uint32_t count[RS_ITEMS * RS_WAVES][RS_DIGITS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (uint32_t s = 0; s < RS_ITEMS * RS_WAVES; s++) count[s][tid] = 0u;
        __syncthreads();
        const size_t base = tile * RS_TILE;
        uint32_t key[RS_ITEMS], idx[RS_ITEMS], rank[RS_ITEMS];
        for (uint32_t j = 0; j < RS_ITEMS; j++) {
            const size_t i = base + (size_t) j * RS_THREADS + tid;
            const bool live = i < n;
            key[j] = live ? keys_in[i] : 0u;
            idx[j] = live ? idx_in[i] : 0u;
            const uint32_t dg = (key[j] >> shift) & (RS_DIGITS - 1u);
            uint64_t same = __ballot(live); // the lanes of this wave that hold a pair with this lane's digit
            for (uint32_t b = 0; b < RS_DIGIT_BITS; b++) {
                const bool bit = (dg >> b) & 1u;
                const uint64_t set = __ballot(bit);
                same &= bit ? set : ~set;
            }
            rank[j] = (uint32_t) __popcll(same & below);
            if (live && rank[j] == 0u) count[j * RS_WAVES + wave][dg] = (uint32_t) __popcll(same);
        }
        __syncthreads();
        uint32_t run = table[(size_t) tid * tiles + tile];
        for (uint32_t s = 0; s < RS_ITEMS * RS_WAVES; s++) {
            const uint32_t c = count[s][tid];
            count[s][tid] = run;
            run += c;
        }
        __syncthreads();
        for (uint32_t j = 0; j < RS_ITEMS; j++) {
            const size_t i = base + (size_t) j * RS_THREADS + tid;
            if (i < n) {
                const size_t at = (size_t) count[j * RS_WAVES + wave][(key[j] >> shift) & (RS_DIGITS - 1u)] + rank[j];
                keys_out[at] = key[j];
                idx_out[at] = idx[j];
            }
        }
        __syncthreads();
    }
}

// ---- gather and permute ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void gather_rays_kernel(const uint4 *__restrict__ rays, const uint32_t *__restrict__ perm, size_t n, uint4 *__restrict__ sorted)
{
    for (size_t i = (size_t) blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += (size_t) gridDim.x * RS_THREADS) {
        const uint4 *src = rays + 3u * (size_t) perm[i];
        const uint4 w0 = src[0], w1 = src[1], w2 = src[2];
        uint4 *dst = sorted + 3u * i;
        dst[0] = w0, dst[1] = w1, dst[2] = w2;
    }
}

// planes x n records of `per` elements E each, one element per lane and step, consecutive lanes on consecutive elements of the record
// stream that is read (gather) or written (scatter) in order
template <typename E, bool SCATTER>
__global__ __launch_bounds__(RS_THREADS) void permute_kernel(const uint32_t *__restrict__ perm, size_t n, const E *__restrict__ src, E *__restrict__ dst, uint32_t per, uint32_t planes)
{
    const size_t per_plane = n * per;
    for (size_t j = (size_t) blockIdx.x * RS_THREADS + threadIdx.x; j < per_plane; j += (size_t) gridDim.x * RS_THREADS) {
        const size_t i = j / per;
        const size_t other = (size_t) perm[i] * per + (j - i * per);
        for (uint32_t p = 0; p < planes; p++) {
            const size_t plane = (size_t) p * per_plane;
            if (SCATTER)
                dst[plane + other] = src[plane + j];
            else
                dst[plane + j] = src[plane + other];
        }
    }
}

template <typename E>
void permute_launch(const uint32_t *perm, size_t n, const void *src, void *dst, uint32_t per, uint32_t planes, int scatter, uint32_t max_grid, hipStream_t stream)
{
    const dim3 grid(grid_for((n * per + RS_THREADS - 1u) / RS_THREADS, max_grid)), block(RS_THREADS);
    if (scatter)
        hipLaunchKernelGGL((permute_kernel<E, true>), grid, block, 0, stream, perm, n, (const E *) src, (E *) dst, per, planes);
    else
        hipLaunchKernelGGL((permute_kernel<E, false>), grid, block, 0, stream, perm, n, (const E *) src, (E *) dst, per, planes);
}

} // namespace

extern "C" size_t rt_sort_rays_work_size(uint32_t n) { return n ? sort_layout(n).bytes : 0u; }

// rays: n rt_ray; sorted, keys_out: may be NULL; work: at least rt_sort_rays_work_size(n) bytes (the caller checked); n > 0
extern "C" hipError_t rt_launch_sort_rays(const void *rays_, uint32_t n_, void *sorted, uint32_t *perm, uint32_t *keys_out, void *work, uint32_t max_grid,
                                          hipStream_t stream)
{
    const size_t n = n_;
    if (n == 0u) return hipErrorInvalidValue;
    const SortLayout l = sort_layout(n_);
    unsigned char *base = (unsigned char *) (((uintptr_t) work + RS_ALIGN - 1u) / RS_ALIGN * RS_ALIGN);
    const uint4 *rays = (const uint4 *) rays_;
    unsigned long long *box = (unsigned long long *) base;
    uint32_t *keys_a = (uint32_t *) (base + l.keys_a), *idx_a = (uint32_t *) (base + l.idx_a);
    uint32_t *keys_b = (uint32_t *) (base + l.keys_b), *idx_b = (uint32_t *) (base + l.idx_b);
    uint32_t *level[RS_MAX_LEVELS];
    size_t chunks[RS_MAX_LEVELS];
    for (uint32_t k = 0; k < l.levels; k++) {
        level[k] = (uint32_t *) (base + l.level_off[k]);
        chunks[k] = (l.level_len[k] + RS_SCAN_CHUNK - 1u) / RS_SCAN_CHUNK;
    }
    const dim3 block(RS_THREADS), per_ray(grid_for((n + RS_THREADS - 1u) / RS_THREADS, max_grid)), per_tile(grid_for(l.tiles, max_grid));

    hipLaunchKernelGGL(init_box_kernel, dim3(1), dim3(64), 0, stream, box);
    hipLaunchKernelGGL(box_kernel, per_ray, block, 0, stream, rays, n, box);
    hipLaunchKernelGGL(keys_kernel, per_ray, block, 0, stream, rays, n, box, keys_b, idx_b);
    // B -> A -> B -> A -> (keys_out or B's keys, perm)
    const uint32_t *kin = keys_b, *iin = idx_b;
    for (uint32_t pass = 0; pass < RS_PASSES; pass++) {
        const bool last = pass + 1u == RS_PASSES;
        uint32_t *kout = last ? (keys_out ? keys_out : keys_b) : ((pass & 1u) ? keys_b : keys_a);
        uint32_t *iout = last ? perm : ((pass & 1u) ? idx_b : idx_a);
        const uint32_t shift = pass * RS_DIGIT_BITS;
        hipLaunchKernelGGL(histogram_kernel, per_tile, block, 0, stream, kin, n, l.tiles, shift, level[0]);
        for (uint32_t k = 0; k + 1u < l.levels; k++)
            hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_for(chunks[k], max_grid)), block, 0, stream, level[k], l.level_len[k], chunks[k], level[k + 1u]);
        for (uint32_t k = l.levels; k-- > 0u;)
            hipLaunchKernelGGL(scan_chunks_kernel, dim3(grid_for(chunks[k], max_grid)), block, 0, stream, level[k], l.level_len[k], chunks[k],
                               k + 1u < l.levels ? level[k + 1u] : nullptr);
        hipLaunchKernelGGL(scatter_kernel, per_tile, block, 0, stream, kin, iin, n, l.tiles, shift, level[0], kout, iout);
        kin = kout, iin = iout;
    }
    if (sorted) hipLaunchKernelGGL(gather_rays_kernel, per_ray, block, 0, stream, rays, perm, n, (uint4 *) sorted);
    return hipGetLastError();
}

// planes x n records of elem_bytes (a multiple of 4, at most 256; the caller checked), plane stride n * elem_bytes
extern "C" hipError_t rt_launch_permute(const uint32_t *perm, uint32_t n, const void *src, void *dst, uint32_t elem_bytes, uint32_t planes, int scatter, uint32_t max_grid,
                                        hipStream_t stream)
{
    if (n == 0u || planes == 0u || elem_bytes == 0u || (elem_bytes & 3u)) return hipErrorInvalidValue;
    if (elem_bytes % 16u == 0u && (((uintptr_t) src | (uintptr_t) dst) & 15u) == 0u)
        permute_launch<uint4>(perm, n, src, dst, elem_bytes / 16u, planes, scatter, max_grid, stream);
    else
        permute_launch<uint32_t>(perm, n, src, dst, elem_bytes / 4u, planes, scatter, max_grid, stream);
    return hipGetLastError();
}
